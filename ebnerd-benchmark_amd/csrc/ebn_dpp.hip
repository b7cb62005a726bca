// Greedy determinantal-point-process (DPP) re-ranking of a relevance pool: fast greedy MAP inference (Chen, Zhang, Zhou, "Fast Greedy
// MAP Inference for Determinantal Point Process to Improve Recommendation Diversity", NeurIPS 2018) over the similarity that belongs
// to the distance of IntralistDiversity.  Where MMR (ebn_rerank.hip) scores a pick against its NEAREST earlier pick, DPP scores the
// whole list through log det of its similarity matrix: a candidate inside the span of three earlier picks is penalised even when it
// is close to none of them.
//
// Per user: a pool of P <= 64 entries (relevance rel[i], row row[i] of the UNIT table `unit` [n_rows, D]).
//   d(i, j) = fminf(fmaxf(1 - u_i . u_j, 0), 2)                  the distance of IntralistDiversity (ebn_beyond.hip)
//   S(i, j) = 1 - d(i, j) / 2                                    (1 + cos) / 2 for unit rows: PSD, in [0, 1], monotone in the cosine;
//                                                                the diagonal AS COMPUTED (1 up to rounding, 1/2 for a zero row)
//   state per entry: d2_i, the conditional variance of i given the picks (initially S(i, i)), and a Cholesky row c_i[0..t);  EPS = 1e-4f
//   round t = 0, 1, ...: among the present entries not yet picked, the largest
//   obj_i = lam rel[i] + (1 - lam) logf(fmaxf(d2_i, EPS));       larger obj first, equal obj to the smaller pool index.
//   lam rel_i is the marginal gain of lam sum rel + (1 - lam) log det S_Y, so lam = 1 is the relevance order of the pool.
//   after picking j: d2_j <= EPS -- the pick is degenerate (already spanned): c_i[t] = 0, nothing else changes; otherwise, for every i,
//   e_i = (S(j, i) - sum_{s<t} c_j[s] c_i[s]) / sqrtf(d2_j),  c_i[t] = e_i,  d2_i -= e_i e_i      the sum over s ascending, ONE fma chain.
//   The rounds end after k picks or when nothing is left; a pool whose rank is below k still fills its list: spanned entries are
//   clamped at EPS, not dropped, and then order by relevance.
//
// The Gram stage is that of mmr_rerank_kernel, restated here so that ebn_rerank.hip and its bits stay as they are: a 256-thread
// workgroup owns 64 image rows -- one user when P > 32, two users (rows 0..31 and 32..63) when P <= 32; the unit rows are gathered in
// 32-deep k slabs through registers into two 16-deep XOR-swizzled float4 images (S4[row][kq ^ ((row >> 2) & 3)]), two buffers, one
// barrier per slab; wave w forms the 32x32 tile (w >> 1, w & 1) with v_mfma_f32_32x32x2_f32, every element ONE fma chain over D in a
// fixed k order, tile (1, 0) never formed (the wave of tile (0, 1) writes each distance to both places).  The distances overwrite
// the operand images (64 rows of 65 floats).  An absent entry's row is never turned into an address: its image row is zeros.
//
// Greedy stage: one wave per user, lane i owns entry i (rel, d2, picked bit in registers).  The Cholesky rows live in LDS slot-major,
// c_e[s] = chol[64 s + e]: lane i reads word 64 s + i -- bank i, no conflict, no padding -- and c_j[s] is one broadcast read; that
// part of the LDS is dynamic, k - 1 slots rounded up to whole chunks of four (the last pick stores nothing), zeroed at the start so
// that a sum runs in whole chunks: sum + 0 * 0 for the slots from t on.  A round is: logf; the wave-wide maximum of obj by four
// data-parallel-primitive steps and four v_readlane (no LDS round trips: the rounds are a latency chain, and __shfl_xor's twelve
// ds_bpermute per round were most of it), a ballot of the lanes that hold it, whose lowest set bit is the pick; v_readlane of d2_j;
// 2 t LDS reads and t fmas for the sum; one LDS read of S(j, i); one division.  LDS per workgroup: 4160 floats of images /
// distances + 512 B of pool = 17 152 B static, plus 256 B per slot: 20 224 B at k = 10 (eight workgroups per CU, as MMR), 33 536 B at
// k = 64 (four).  No atomics: a user's bits depend neither on U nor on the users that share its launch or workgroup.
#include <math.h>

#include "ebn_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int DP_ROWS = 64, DP_BK = 32, DP_THREADS = 256;
constexpr int DP_MAX_P = 64, DP_MAX_K = 64, DP_MAX_D = 8192;
constexpr int DP_SUB_FLOATS = DP_ROWS * 16;         // one 16-deep swizzled image
constexpr int DP_BUF_FLOATS = 2 * DP_SUB_FLOATS;    // one slab: two of them
constexpr int DP_DIST_LD = DP_ROWS + 1;             // row stride of the distance matrix
constexpr float DP_EPS = 1e-4f;
constexpr int DP_CHUNK = 4;                         // slots read together in a Cholesky sum
static_assert(DP_ROWS * DP_DIST_LD <= 2 * DP_BUF_FLOATS + DP_ROWS, "the distances fit the operand images and their tail");

struct DppArgs {
  const float* unit;
  const int32_t* pool_rows;
  const float* pool_rel;
  int32_t* out_sel;
  float* out_obj;
  int32_t* flags;
  int64_t U, n_rows;
  int32_t D, P, k, upw;  // upw: users per workgroup (1 or 2)
  int32_t slots;         // Cholesky slots in the dynamic LDS
  float lam;
};

// The largest value of a full wave, in every lane: four data-parallel-primitive steps (lane ^ 1, lane ^ 2, the mirror of each 8,
// the mirror of each 16) leave every row of 16 lanes with its maximum, the four rows meet through scalar registers.  No LDS, unlike
// __shfl_xor: a round of the greedy stage waits on this, so its latency is what counts.  The values must not be NaN.
__device__ inline float wave_max(float v) {
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)));   // quad_perm [1, 0, 3, 2]
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)));   // quad_perm [2, 3, 0, 1]
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false)));  // row_half_mirror
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false)));  // row_mirror
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

__global__ __launch_bounds__(DP_THREADS) void dpp_rerank_kernel(DppArgs a) {
  __shared__ __attribute__((aligned(16))) float img[2 * DP_BUF_FLOATS + DP_ROWS];  // operand slabs, then the 64 x 65 distances
  extern __shared__ float chol[];                                        // Cholesky rows, slot-major: c_e[s] = chol[s * 64 + e]
  __shared__ int srow[DP_ROWS];                                          // table row of an image row, -1: absent
  __shared__ float srel[DP_ROWS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = lane >> 5, il = lane & 31;
  const int P = a.P, D = a.D, upw = a.upw;

  for (int i = tid; i < a.slots * DP_ROWS; i += DP_THREADS) chol[i] = 0.0f;  // a slot is zero until its round (ordered by the barriers below)

  // ---- the pool: image row e is entry e of the user (upw == 1) or entry e & 31 of user e >> 5 (upw == 2)
  if (tid < DP_ROWS) {
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
    sdst[i] = (q8 >> 2) * DP_SUB_FLOATS + (row * 4 + ((q8 & 3) ^ ((row >> 2) & 3))) * 4;
  }
  const int ti = wave >> 1, tj = wave & 1;
  const bool active = upw == 1 ? ti <= tj : ti == tj;  // wave-uniform; tile (1, 0) is the transpose of tile (0, 1)

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  float4 reg[2];
  // D % 4 == 0: a float4 is all inside the row or all outside
  auto fetch = [&](int kt) {
    const bool in = kt * DP_BK + q8 * 4 < D;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      reg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (have[i] && in) reg[i] = *reinterpret_cast<const float4*>(src[i] + kt * DP_BK);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(&img[buf * DP_BUF_FLOATS + sdst[i]]) = reg[i];
  };
  // contraction index of MFMA step w of quad pair j8 of sub-image s, lane half kl: k = 16 s + 8 j8 + 4 kl + w, for both operands
  auto mma = [&](int buf) {
    if (!active) return;
    const int sw = (il >> 2) & 3;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float* as = img + buf * DP_BUF_FLOATS + s * DP_SUB_FLOATS + (ti * 32 + il) * 16;
      const float* bs = img + buf * DP_BUF_FLOATS + s * DP_SUB_FLOATS + (tj * 32 + il) * 16;
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

  const int nk = (D + DP_BK - 1) / DP_BK;
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
  // The diagonal is kept as computed and, unlike MMR's, is used (d2_i starts from it): a NaN there is flagged like any other.
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
      saw_nan |= nan && pj && srow[i] >= 0;
      const float d = nan ? 0.0f : fminf(fmaxf(1.0f - dot, 0.0f), 2.0f);  // (fmaxf alone already turns a NaN into 0)
      dist[i * DP_DIST_LD + j] = d;
      if (ti != tj) dist[j * DP_DIST_LD + i] = d;
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
  const float lrel = lam * rel;
  const int k = a.k;
  const int me = mine ? base + lane : base;  // a lane outside the pool computes on entry 0's words and stores nothing
  bool picked = false;
  float d2 = fmaf(-0.5f, dist[me * DP_DIST_LD + me], 1.0f);  // S(i, i)
  int my_sel = -1;         // lane t keeps the pick of round t
  float my_obj = -INFINITY;
  for (int t = 0; t < k; ++t) {
    const bool cand = present && !picked;
    const float obj = fmaf(oml, logf(fmaxf(d2, DP_EPS)), lrel);  // lam = 1: exactly rel
    // the total order: the largest obj, and of the lanes that hold it the lowest
    const float bo = wave_max(cand ? obj : -INFINITY);
    const unsigned long long best = __ballot(cand && obj == bo);
    if (best == 0ull) break;  // nothing left: the list stays short
    const int j = __builtin_amdgcn_readfirstlane(__ffsll(best) - 1);
    if (lane == t) {
      my_sel = j;
      my_obj = bo;
    }
    picked |= lane == j;
    if (t + 1 == k) break;  // the last pick needs no update
    const float d2j = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d2), j));
    float e = 0.0f;
    if (d2j > DP_EPS) {  // wave-uniform; otherwise the pick is degenerate: the round only consumes slot t
      const float* cj = chol + base + j;
      const float* ci = chol + me;
      float sum = 0.0f;
      for (int s = 0; s < t; s += DP_CHUNK) {  // ascending s, one chain; the slots from t on still hold their zeros: sum + 0 * 0
        float cjs[DP_CHUNK], cis[DP_CHUNK];
#pragma unroll
        for (int w = 0; w < DP_CHUNK; ++w) {
          cjs[w] = cj[(s + w) * DP_ROWS];
          cis[w] = ci[(s + w) * DP_ROWS];
        }
#pragma unroll
        for (int w = 0; w < DP_CHUNK; ++w) sum = fmaf(cjs[w], cis[w], sum);
      }
      const float sji = fmaf(-0.5f, dist[(base + j) * DP_DIST_LD + me], 1.0f);
      e = (sji - sum) / sqrtf(d2j);
      d2 = fmaf(-e, e, d2);
    }
    if (mine) chol[t * DP_ROWS + me] = e;
    // lanes read each other's words in later rounds: keep the store ahead of them (one wave, so ordering is all that is needed)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (lane < k) {
    a.out_sel[u * k + lane] = my_sel;
    if (a.out_obj != nullptr) a.out_obj[u * k + lane] = my_obj;
  }
}

}  // namespace

extern "C" int ebn_dpp_rerank_f32(const float* unit, int64_t n_rows, int32_t D, const int32_t* pool_rows, const float* pool_rel,
                                  int32_t P, int32_t k, float lam, int32_t* out_sel, float* out_obj, int32_t* flags, int64_t U,
                                  ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(U, n_rows) && D >= 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(lam >= 0.0f && lam <= 1.0f, EBN_ERR_BAD_ARG);  // false for NaN
  EBN_REQUIRE(P >= 1 && P <= DP_MAX_P && k >= 1 && k <= DP_MAX_K && D >= 4 && D % 4 == 0 && D <= DP_MAX_D, EBN_ERR_UNSUPPORTED);
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(pool_rows != nullptr && pool_rel != nullptr && out_sel != nullptr && flags != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(unit != nullptr || n_rows == 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_aligned16(unit), EBN_ERR_ALIGN);
  DppArgs a;
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
  a.slots = (k - 1 + DP_CHUNK - 1) / DP_CHUNK * DP_CHUNK;  // the last pick stores nothing; whole chunks, so the sums need no tail
  const size_t chol_bytes = static_cast<size_t>(a.slots) * DP_ROWS * sizeof(float);
  EBN_LAUNCH(dpp_rerank_kernel, dim3(static_cast<unsigned>(blocks)), dim3(DP_THREADS), chol_bytes, ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
