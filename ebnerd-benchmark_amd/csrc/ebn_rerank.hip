// Greedy Maximal-Marginal-Relevance re-ranking of a relevance pool (the trade of relevance against IntralistDiversity in the
// beyond-accuracy workflow, examples/beyond_accuracy/make_beyond_accuracy.ipynb, cell "Your Model").
//
// Per user: a pool of P <= 64 entries (relevance rel[i], row row[i] of the UNIT table `unit` [n_rows, D]).
//   d(i, j) = fminf(fmaxf(1 - u_i . u_j, 0), 2)                  the distance of IntralistDiversity (ebn_beyond.hip)
//   round 0: the present entry with the largest rel;  round t >= 1: the present, unpicked entry with the largest
//   obj_i = lam rel[i] + (1 - lam) min over picked j of d(i, j);   larger obj first, equal obj to the smaller pool index.
//
// A 256-thread workgroup owns 64 image rows: one user when P > 32, two users (rows 0..31 and 32..63) when P <= 32.  The unit rows are
// gathered in 32-deep k slabs through registers into LDS, as two 16-deep XOR-swizzled float4 images of ebn_gemm.hip / ebn_topk.hip
// (S4[row][kq ^ ((row >> 2) & 3)], one conflict-free ds_read_b128 per four MFMA steps), two buffers, one barrier per slab.  Wave w forms
// the 32x32 Gram tile (w >> 1, w & 1) with v_mfma_f32_32x32x2_f32: every element is ONE fma chain over D in a fixed k order, the same
// chain whichever user, launch or workgroup it is computed in, and u_i . u_j has the bits of u_j . u_i (the same products in the same
// order) -- so tile (1, 0) is never formed: the wave of tile (0, 1) writes each distance to both places, and a quarter of the MFMA
// work is saved.  With two users per workgroup only the two diagonal tiles are formed.  The distances then overwrite the operand
// images (64 rows of 65 floats: the odd stride keeps the transposed stores off one bank), and one wave per user runs the k greedy
// rounds: lane i owns entry i (rel, running min d, picked bit), a round is a wave-wide argmax under the total order above followed
// by one LDS row read.  An absent entry's row is never turned into an address: its image row is zeros.
#include <math.h>

#include "ebn_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RR_ROWS = 64, RR_BK = 32, RR_THREADS = 256;
constexpr int RR_MAX_P = 64, RR_MAX_K = 64, RR_MAX_D = 8192;
constexpr int RR_SUB_FLOATS = RR_ROWS * 16;         // one 16-deep swizzled image
constexpr int RR_BUF_FLOATS = 2 * RR_SUB_FLOATS;    // one slab: two of them
constexpr int RR_DIST_LD = RR_ROWS + 1;             // row stride of the distance matrix
constexpr int RR_NONE = INT32_MAX;                  // index of "no entry" in the argmax (sorts after every real entry)
static_assert(RR_ROWS * RR_DIST_LD <= 2 * RR_BUF_FLOATS + RR_ROWS, "the distances fit the operand images and their tail");

struct RerankArgs {
  const float* unit;
  const int32_t* pool_rows;
  const float* pool_rel;
  int32_t* out_sel;
  float* out_obj;
  int32_t* flags;
  int64_t U, n_rows;
  int32_t D, P, k, upw;  // upw: users per workgroup (1 or 2)
  float lam;
};

__global__ __launch_bounds__(RR_THREADS) void mmr_rerank_kernel(RerankArgs a) {
  __shared__ __attribute__((aligned(16))) float img[2 * RR_BUF_FLOATS + RR_ROWS];  // operand slabs, then the 64 x 65 distances
  __shared__ int srow[RR_ROWS];                                          // table row of an image row, -1: absent
  __shared__ float srel[RR_ROWS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = lane >> 5, il = lane & 31;
  const int P = a.P, D = a.D, upw = a.upw;

  // ---- the pool: image row e is entry e of the user (upw == 1) or entry e & 31 of user e >> 5 (upw == 2)
  if (tid < RR_ROWS) {
    const int g = upw == 2 ? tid >> 5 : 0;
    const int i = upw == 2 ? tid & 31 : tid;
    const int64_t u = static_cast<int64_t>(blockIdx.x) * upw + g;
    int row = -1;
    float rel = -INFINITY;
    if (u < a.U && i < P) {
      const int64_t r = a.pool_rows[u * P + i];
      const float x = a.pool_rel[u * P + i];
      const bool row_ok = r >= 0 && r < a.n_rows;
      const bool rel_ok = fabsf(x) < INFINITY;  // false for NaN
      if (!row_ok && r != -1) a.flags[0] = 1;
      if (!rel_ok && !(x == -INFINITY)) a.flags[1] = 1;
      if (row_ok && rel_ok) {
        row = static_cast<int>(r);
        rel = x;
      }
    }
    srow[tid] = row;
    srel[tid] = rel;
  }
  __syncthreads();

  // ---- gather + Gram.  This thread's two float4 of a slab: item v = tid + 256 i -> image row v / 8, k quad v % 8
  const float* src[2];
  int sdst[2];
  bool have[2];
  const int q8 = tid & 7;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (tid >> 3) + 32 * i;
    const int r = srow[row];
    have[i] = r >= 0;
    src[i] = a.unit + static_cast<int64_t>(have[i] ? r : 0) * D + q8 * 4;  // formed, never read when absent
    sdst[i] = (q8 >> 2) * RR_SUB_FLOATS + (row * 4 + ((q8 & 3) ^ ((row >> 2) & 3))) * 4;
  }
  const int ti = wave >> 1, tj = wave & 1;
  const bool active = upw == 1 ? ti <= tj : ti == tj;  // wave-uniform; tile (1, 0) is the transpose of tile (0, 1)

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  float4 reg[2];
  // D % 4 == 0: a float4 is all inside the row or all outside
  auto fetch = [&](int kt) {
    const bool in = kt * RR_BK + q8 * 4 < D;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      reg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (have[i] && in) reg[i] = *reinterpret_cast<const float4*>(src[i] + kt * RR_BK);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(&img[buf * RR_BUF_FLOATS + sdst[i]]) = reg[i];
  };
  // contraction index of MFMA step w of quad pair j8 of sub-image s, lane half kl: k = 16 s + 8 j8 + 4 kl + w, for both operands
  auto mma = [&](int buf) {
    if (!active) return;
    const int sw = (il >> 2) & 3;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float* as = img + buf * RR_BUF_FLOATS + s * RR_SUB_FLOATS + (ti * 32 + il) * 16;
      const float* bs = img + buf * RR_BUF_FLOATS + s * RR_SUB_FLOATS + (tj * 32 + il) * 16;
#pragma unroll
      for (int j8 = 0; j8 < 2; ++j8) {
        const int q = ((2 * j8 + kl) ^ sw) * 4;
        const float4 av = *reinterpret_cast<const float4*>(as + q);
        const float4 bv = *reinterpret_cast<const float4*>(bs + q);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
      }
    }
  };

  const int nk = (D + RR_BK - 1) / RR_BK;
  fetch(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) fetch(kt + 1);
    mma(buf);
    if (kt + 1 < nk) store(buf ^ 1);
    __syncthreads();  // the next slab is in place, and every wave is done with this one
  }

  // ---- distances into LDS, over the images.  C/D map of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* dist = img;
  if (active) {
    const int j = tj * 32 + il;
    const bool pj = srow[j] >= 0;
    bool saw_nan = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
      const float dot = acc[r];
      const bool nan = dot != dot;
      saw_nan |= nan && pj && i != j && srow[i] >= 0;
      const float d = nan ? 0.0f : fminf(fmaxf(1.0f - dot, 0.0f), 2.0f);  // (fmaxf alone already turns a NaN into 0)
      dist[i * RR_DIST_LD + j] = d;
      if (ti != tj) dist[j * RR_DIST_LD + i] = d;
    }
    if (saw_nan) a.flags[1] = 1;
  }
  __syncthreads();

  // ---- greedy selection: wave g runs the user g of the workgroup, lane i owns entry i
  if (wave >= upw) return;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * upw + wave;
  if (u >= a.U) return;
  const int base = upw == 2 ? wave * 32 : 0;
  const bool mine = lane < P;
  const float rel = mine ? srel[base + lane] : -INFINITY;
  const bool present = mine && srow[base + lane] >= 0;
  const float lam = a.lam, oml = 1.0f - a.lam;
  const int k = a.k;
  bool picked = false;
  float mind = INFINITY;
  int my_sel = -1;         // lane t keeps the pick of round t
  float my_obj = -INFINITY;
  for (int t = 0; t < k; ++t) {
    const bool cand = present && !picked;
    const float obj = t == 0 ? rel : lam * rel + oml * mind;
    float bo = cand ? obj : -INFINITY;
    int bi = cand ? lane : RR_NONE;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float oo = __shfl_xor(bo, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (oo > bo || (oo == bo && oi < bi)) {
        bo = oo;
        bi = oi;
      }
    }
    if (bi == RR_NONE) break;  // nothing left: the list stays short (wave-uniform)
    if (lane == t) {
      my_sel = bi;
      my_obj = bo;
    }
    picked |= lane == bi;
    if (mine) mind = fminf(mind, dist[(base + bi) * RR_DIST_LD + base + lane]);
  }
  if (lane < k) {
    a.out_sel[u * k + lane] = my_sel;
    if (a.out_obj != nullptr) a.out_obj[u * k + lane] = my_obj;
  }
}

}  // namespace

extern "C" int ebn_mmr_rerank_f32(const float* unit, int64_t n_rows, int32_t D, const int32_t* pool_rows, const float* pool_rel,
                                  int32_t P, int32_t k, float lam, int32_t* out_sel, float* out_obj, int32_t* flags, int64_t U,
                                  ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(U, n_rows) && D >= 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(lam >= 0.0f && lam <= 1.0f, EBN_ERR_BAD_ARG);  // false for NaN
  EBN_REQUIRE(P >= 1 && P <= RR_MAX_P && k >= 1 && k <= RR_MAX_K && D >= 4 && D % 4 == 0 && D <= RR_MAX_D, EBN_ERR_UNSUPPORTED);
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(pool_rows != nullptr && pool_rel != nullptr && out_sel != nullptr && flags != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(unit != nullptr || n_rows == 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_aligned16(unit), EBN_ERR_ALIGN);
  RerankArgs a;
  a.unit = unit;
  a.pool_rows = pool_rows;
  a.pool_rel = pool_rel;
  a.out_sel = out_sel;
  a.out_obj = out_obj;
  a.flags = flags;
  a.U = U;
  a.n_rows = n_rows;
  a.D = D;
  a.P = P;
  a.k = k;
  a.upw = P <= 32 ? 2 : 1;
  a.lam = lam;
  const int64_t blocks = ebn_ceil_div(U, a.upw);  // U <= 2^31 - 1: fits the grid's 32 bits
  EBN_LAUNCH(mmr_rerank_kernel, dim3(static_cast<unsigned>(blocks)), dim3(RR_THREADS), 0, ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
