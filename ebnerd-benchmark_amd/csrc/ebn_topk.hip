// Top-k recommendation from an encoded catalogue: score a tile of users against streamed candidates and keep each user's best k
// (examples/beyond_accuracy/make_beyond_accuracy.ipynb, cell "Your Model": the model's top-N out of one shared candidate list).
//
//   score[u, c] = users[u, :] . news_all[cand_rows[c], :]      (exact fp32: v_mfma_f32_32x32x2_f32, an fma chain over F in k order)
//
// The scores are never written out.  A 256-thread workgroup owns 128 users and walks its range of 128-candidate tiles; the four
// waves are stacked along the users (wave w: rows 32w .. 32w + 31, all 128 columns -- 4 MFMA tiles, 64 accumulator registers), so a
// user's list is only ever touched by ONE wave and the selection needs no workgroup barrier and no atomics.  Both operands are
// k-contiguous and go through registers into the XOR-swizzled float4 image of ebn_gemm.hip (S4[mn][kq ^ ((mn >> 2) & 3)], one
// conflict-free ds_read_b128 per four MFMA steps), 16-deep slabs, two LDS buffers, one barrier per slab.
//
// Selection epilogue, per tile and wave:
//   1. one compare per element against the user's current k-th best, thr[row] (LDS, -inf while the list is short):
//      survivor = !(score < thr) -- NaN survives on purpose, it has to reach the flag.  No survivor in the wave: next tile.
//   2. the survivors of one accumulator index (2 rows x 128 columns, at most 256) are compacted into a per-wave LDS queue by
//      ballot + lane-prefix, then drained 64 at a time: each lane checks ITS entry (user / candidate in range, NaN, the current thr,
//      the user's exclusion list), and what is left is inserted by the whole wave, one entry at a time: lane t holds slot t of the
//      sorted list, the rank of the newcomer is a ballot popcount, the tail moves down by one lane.
// The order is total -- score descending, then candidate position ascending -- so the list does not depend on the order in which
// survivors arrive, nor on how the candidates are split over workgroups: every element's dot product is the same fma chain whatever
// the split, partial lists are merged in the same order by a second launch.  Bit-identical for every n_splits and from run to run.
// Ranking is on the raw dot product; the sigmoid is applied to the k kept values when they are written.
#include <math.h>

#include "ebn_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TK_BM = 128, TK_BN = 128, TK_BK = 16, TK_THREADS = 256;
constexpr int TK_TN = TK_BN / 32;      // MFMA tiles of a wave along the candidates
constexpr int TK_QCAP = 2 * TK_BN;     // survivors of one accumulator index: 2 rows x 128 columns
constexpr int TK_MAX_K = 64, TK_MAX_X = 256, TK_MAX_F = 8192, TK_MAX_SPLITS = 64;
constexpr int TK_EMPTY = INT32_MAX;    // position of an empty slot inside the kernels (sorts after every real candidate)
constexpr int TK_TILE_FLOATS = TK_BM * TK_BK;  // one operand slab image

struct TopkArgs {
  const float* users;
  const float* news;
  const int32_t* cand_rows;
  const int32_t* exclude;
  int32_t* out_pos;
  float* out_score;
  int32_t* flags;
  int32_t* part_pos;   // [n_splits, U, k] (n_splits > 1)
  float* part_score;
  int64_t U, M, n_rows;
  int32_t F, X, k, mode, n_splits, tiles_per_split;
};

__device__ __forceinline__ float topk_act(float s, int mode) { return mode == 1 ? 1.0f / (1.0f + expf(-s)) : s; }

// (s0, p0) ranks strictly before (s1, p1)
__device__ __forceinline__ bool topk_before(float s0, int p0, float s1, int p1) { return s0 > s1 || (s0 == s1 && p0 < p1); }

// dynamic LDS layout (floats): operand images | thr[128] | candrow[128] | queue score[4][256] | queue rowcol[4][256] | list score
// [128][k] | list pos [128][k]
__global__ __launch_bounds__(TK_THREADS, 2) void topk_score_kernel(TopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                           // 2 buffers
  float* Bs = smem + 2 * TK_TILE_FLOATS;      // 2 buffers
  volatile float* thr = smem + 4 * TK_TILE_FLOATS;
  volatile int* candrow = reinterpret_cast<volatile int*>(smem + 4 * TK_TILE_FLOATS + TK_BM);
  volatile float* qs_all = smem + 4 * TK_TILE_FLOATS + TK_BM + TK_BN;
  volatile int* qrc_all = reinterpret_cast<volatile int*>(smem + 4 * TK_TILE_FLOATS + TK_BM + TK_BN + 4 * TK_QCAP);
  volatile float* lsc = smem + 4 * TK_TILE_FLOATS + TK_BM + TK_BN + 8 * TK_QCAP;
  volatile int* lps = reinterpret_cast<volatile int*>(smem + 4 * TK_TILE_FLOATS + TK_BM + TK_BN + 8 * TK_QCAP + TK_BM * a.k);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = lane >> 5, il = lane & 31;
  const int k = a.k, F = a.F, X = a.X;
  const int64_t u0 = static_cast<int64_t>(blockIdx.x) * TK_BM;
  const int split = blockIdx.y;
  volatile float* qs = qs_all + wave * TK_QCAP;
  volatile int* qrc = qrc_all + wave * TK_QCAP;

  for (int i = tid; i < TK_BM * k; i += TK_THREADS) {
    lsc[i] = -INFINITY;
    lps[i] = TK_EMPTY;
  }
  if (tid < TK_BM) thr[tid] = -INFINITY;
  __syncthreads();  // a range without tiles (more splits than tiles divide into) still writes its empty lists out

  // this thread's two float4 of an operand slab: item v = tid + 256 i -> tile row v / 4, k quarter v % 4
  const float* pa[2];
  int sdst[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int v = tid + i * TK_THREADS, mn = v >> 2, kq = v & 3;
    int64_t u = u0 + mn;
    u = u < a.U ? u : a.U - 1;  // rows past the last user repeat it; their lists are never written out
    pa[i] = a.users + u * F + kq * 4;
    sdst[i] = (mn * 4 + (kq ^ ((mn >> 2) & 3))) * 4;
  }
  const int kq4 = (tid & 3) * 4;
  bool saw_nan = false;

  const int64_t n_tiles = (a.M + TK_BN - 1) / TK_BN;
  const int64_t t_beg = static_cast<int64_t>(split) * a.tiles_per_split;
  int64_t t_end = t_beg + a.tiles_per_split;
  t_end = t_end < n_tiles ? t_end : n_tiles;
  const int nk = (F + TK_BK - 1) / TK_BK;

  for (int64_t t = t_beg; t < t_end; ++t) {
    const int64_t n0 = t * TK_BN;
    __syncthreads();  // every wave is done with the previous tile's candrow (and the lists are initialised)
    if (tid < TK_BN) {
      const int64_t c = n0 + tid;
      int row = -2;  // past the last candidate
      if (c < a.M) {
        const int64_t r = a.cand_rows != nullptr ? static_cast<int64_t>(a.cand_rows[c]) : c;
        if (r < 0 || r >= a.n_rows) {
          row = -1;  // never turned into an address
          a.flags[0] = 1;
        } else {
          row = static_cast<int>(r);
        }
      }
      candrow[tid] = row;
    }
    __syncthreads();
    const float* pb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int mn = (tid + i * TK_THREADS) >> 2;
      const int r = candrow[mn];
      pb[i] = a.news + static_cast<int64_t>(r > 0 ? r : 0) * F + kq4;
    }

    f32x16 acc[TK_TN];
#pragma unroll
    for (int j = 0; j < TK_TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    float4 ra[2], rb[2];
    // F % 4 == 0: a float4 is all inside the row or all outside; an outside piece reads the row's first bytes and is zeroed
    auto fetch = [&](int kt) {
      const int kk = kt * TK_BK;
      const bool ok = kk + kq4 < F;
      const int off = ok ? kk : -kq4;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float4 x = *reinterpret_cast<const float4*>(pa[i] + off);
        const float4 y = *reinterpret_cast<const float4*>(pb[i] + off);
        ra[i] = make_float4(ok ? x.x : 0.f, ok ? x.y : 0.f, ok ? x.z : 0.f, ok ? x.w : 0.f);
        rb[i] = make_float4(ok ? y.x : 0.f, ok ? y.y : 0.f, ok ? y.z : 0.f, ok ? y.w : 0.f);
      }
    };
    auto store = [&](int buf) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        *reinterpret_cast<float4*>(&As[buf * TK_TILE_FLOATS + sdst[i]]) = ra[i];
        *reinterpret_cast<float4*>(&Bs[buf * TK_TILE_FLOATS + sdst[i]]) = rb[i];
      }
    };
    // contraction index of MFMA step 4 j8' + w of lane half kl: k = 8 j8 + 4 kl + w, the same for both operands
    auto mma = [&](int buf) {
      const float* as = As + buf * TK_TILE_FLOATS + (wave * 32 + il) * 16;
      const float* bs = Bs + buf * TK_TILE_FLOATS + il * 16;
      const int sw = (il >> 2) & 3;
#pragma unroll
      for (int j8 = 0; j8 < TK_BK / 8; ++j8) {
        const int q = ((2 * j8 + kl) ^ sw) * 4;
        float av[4], bv[TK_TN][4];
#pragma unroll
        for (int w = 0; w < 4; ++w) av[w] = as[q + w];
#pragma unroll
        for (int j = 0; j < TK_TN; ++j)
#pragma unroll
          for (int w = 0; w < 4; ++w) bv[j][w] = bs[j * 32 * 16 + q + w];
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
          for (int j = 0; j < TK_TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[w], bv[j][w], acc[j], 0, 0, 0);
      }
    };

    fetch(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
      if (kt + 1 < nk) fetch(kt + 1);
      mma(0);
      if (kt + 1 < nk) store(1);
      __syncthreads();
      if (kt + 1 < nk) {
        if (kt + 2 < nk) fetch(kt + 2);
        mma(1);
        if (kt + 2 < nk) store(0);
        __syncthreads();
      }
    }

    // ---- selection.  C/D map of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int rbase = wave * 32 + 4 * kl;
    bool any = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float th = thr[rbase + (r & 3) + 8 * (r >> 2)];
#pragma unroll
      for (int j = 0; j < TK_TN; ++j) any |= !(acc[j][r] < th);
    }
    if (__ballot(any) == 0ull) continue;

#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = rbase + (r & 3) + 8 * (r >> 2);
      const float th = thr[rl];
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < TK_TN; ++j) {
        const bool pass = !(acc[j][r] < th);
        const unsigned long long m = __ballot(pass);
        if (pass) {
          const int slot = cnt + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
          qs[slot] = acc[j][r];
          qrc[slot] = (rl << 8) | (j * 32 + il);
        }
        cnt += __popcll(m);
      }
      for (int base = 0; base < cnt; base += 64) {
        const int idx = base + lane;
        bool ok = idx < cnt;
        const float s = ok ? qs[idx] : 0.f;
        const int rc = ok ? qrc[idx] : 0;
        const int erl = rc >> 8, ecol = rc & 255;
        const int64_t u = u0 + erl, c = n0 + ecol;
        const int crow = candrow[ecol];
        ok = ok && u < a.U && crow >= 0;
        if (ok && s != s) {
          saw_nan = true;
          ok = false;
        }
        ok = ok && !(s < thr[erl]);
        if (ok && X > 0) {
          const int32_t* ex = a.exclude + u * X;
          bool hit = false;
          for (int x = 0; x < X; ++x) hit |= ex[x] == crow;
          ok = !hit;
        }
        unsigned long long m = __ballot(ok);
        while (m != 0ull) {
          const int l = __builtin_ctzll(m);
          m &= m - 1ull;
          const float ns = __shfl(s, l, 64);
          const int nrl = __shfl(erl, l, 64);
          const int np = static_cast<int>(__shfl(static_cast<int>(c), l, 64));
          // the whole wave inserts (ns, np) into the list of row nrl: lane t holds slot t
          const bool in = lane < k;
          const float es = in ? lsc[nrl * k + lane] : 0.f;
          const int ep = in ? lps[nrl * k + lane] : 0;
          const int rank = __popcll(__ballot(in && topk_before(es, ep, ns, np)));
          const float us = __shfl_up(es, 1, 64);
          const int up = __shfl_up(ep, 1, 64);
          if (rank < k) {
            if (in && lane >= rank) {
              const float ws = lane == rank ? ns : us;
              lsc[nrl * k + lane] = ws;
              lps[nrl * k + lane] = lane == rank ? np : up;
              if (lane == k - 1) thr[nrl] = ws;
            }
          }
        }
      }
    }
  }

  if (saw_nan) a.flags[1] = 1;
  // a wave writes the lists of its own 32 rows: lane t slot t
  const bool direct = a.n_splits == 1;
  for (int rr = 0; rr < 32; ++rr) {
    const int rl = wave * 32 + rr;
    const int64_t u = u0 + rl;
    if (u >= a.U || lane >= k) continue;
    const float es = lsc[rl * k + lane];
    const int ep = lps[rl * k + lane];
    if (direct) {
      const bool empty = ep == TK_EMPTY;
      a.out_pos[u * k + lane] = empty ? -1 : ep;
      a.out_score[u * k + lane] = empty ? -INFINITY : topk_act(es, a.mode);
    } else {
      const int64_t o = (static_cast<int64_t>(split) * a.U + u) * k + lane;
      a.part_pos[o] = ep;
      a.part_score[o] = es;
    }
  }
}

// Merge of the n_splits (<= 64) sorted partial lists of a user: one wave per user, lane s holds the head of split s, k rounds of a
// wave-wide "first in the total order".  Positions of real candidates are distinct, so the winner is unique.
__global__ __launch_bounds__(256) void topk_merge_kernel(TopkArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (u >= a.U) return;
  const int k = a.k;
  const bool has = lane < a.n_splits;
  const int64_t base = (static_cast<int64_t>(has ? lane : 0) * a.U + u) * k;
  int head = 0;
  for (int t = 0; t < k; ++t) {
    const bool live = has && head < k;
    const float s = live ? a.part_score[base + head] : -INFINITY;
    const int p = live ? a.part_pos[base + head] : TK_EMPTY;
    float bs = s;
    int bp = p;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float os = __shfl_xor(bs, off, 64);
      const int op = __shfl_xor(bp, off, 64);
      if (topk_before(os, op, bs, bp)) {
        bs = os;
        bp = op;
      }
    }
    const bool empty = bp == TK_EMPTY;
    if (!empty && live && p == bp) ++head;
    if (lane == 0) {
      a.out_pos[u * k + t] = empty ? -1 : bp;
      a.out_score[u * k + t] = empty ? -INFINITY : topk_act(bs, a.mode);
    }
  }
}

__global__ __launch_bounds__(256) void topk_fill_empty_kernel(int32_t* __restrict__ out_pos, float* __restrict__ out_score, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
    out_pos[i] = -1;
    out_score[i] = -INFINITY;
  }
}

int64_t topk_lds_bytes(int k) {
  return static_cast<int64_t>(4 * TK_TILE_FLOATS + TK_BM + TK_BN + 8 * TK_QCAP + 2 * TK_BM * k) * 4;
}

int topk_resolve_splits(int64_t U, int64_t M, int32_t n_splits) {
  const int64_t tiles = ebn_ceil_div(M, TK_BN);
  int64_t s = n_splits > 0 ? n_splits : ebn_topk_auto_splits(U, M);
  if (s > tiles) s = tiles;
  if (s > TK_MAX_SPLITS) s = TK_MAX_SPLITS;
  return static_cast<int>(s < 1 ? 1 : s);
}

}  // namespace

extern "C" int ebn_topk_auto_splits(int64_t n_users, int64_t n_cand) {
  if (!ebn_dim_ok(n_users, n_cand) || n_users == 0 || n_cand == 0) return 1;
  // a few hundred workgroups (two per CU) when the users alone do not give them; never finer than one candidate tile
  const int64_t user_tiles = ebn_ceil_div(n_users, TK_BM), tiles = ebn_ceil_div(n_cand, TK_BN);
  int64_t s = ebn_ceil_div(512, user_tiles);
  if (s > tiles) s = tiles;
  if (s > TK_MAX_SPLITS) s = TK_MAX_SPLITS;
  return static_cast<int>(s < 1 ? 1 : s);
}

extern "C" int64_t ebn_topk_workspace_bytes(int64_t n_users, int32_t k, int32_t n_splits) {
  if (!ebn_dim_ok(n_users) || k < 1 || k > TK_MAX_K || n_splits < 1) return 0;
  if (n_splits == 1 || n_users == 0) return 16;  // one split writes the outputs directly
  const int64_t s = n_splits > TK_MAX_SPLITS ? TK_MAX_SPLITS : n_splits;
  return ebn_sat_add(ebn_sat_mul(ebn_sat_mul(ebn_sat_mul(s, n_users), k), 8), 16);
}

extern "C" int ebn_topk_score_f32(const float* users, const float* news_all, int64_t n_rows, const int32_t* cand_rows, int64_t M,
                                  const int32_t* exclude, int32_t X, int32_t k, int32_t mode, int32_t n_splits, int32_t* out_pos,
                                  float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U, int32_t F,
                                  ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(U, M, n_rows) && F >= 0 && X >= 0 && n_splits >= 0 && workspace_bytes >= 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(mode == 0 || mode == 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(k >= 1 && k <= TK_MAX_K && X <= TK_MAX_X && F >= 4 && F % 4 == 0 && F <= TK_MAX_F, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(cand_rows != nullptr || M == n_rows, EBN_ERR_BAD_ARG);
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(out_pos != nullptr && out_score != nullptr && flags != nullptr, EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (M == 0) {
    const int64_t n = U * k;
    const int64_t blocks = ebn_ceil_div(n, 256);
    EBN_LAUNCH(topk_fill_empty_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, out_pos, out_score, n);
    EBN_CHECK_LAUNCH();
    return EBN_OK;
  }
  EBN_REQUIRE(users != nullptr && news_all != nullptr && n_rows >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_aligned16(users) && ebn_aligned16(news_all), EBN_ERR_ALIGN);
  if (exclude == nullptr) X = 0;
  const int splits = topk_resolve_splits(U, M, n_splits);
  const int64_t user_tiles = ebn_ceil_div(U, TK_BM);
  EBN_REQUIRE(user_tiles <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  TopkArgs a;
  a.users = users;
  a.news = news_all;
  a.cand_rows = cand_rows;
  a.exclude = exclude;
  a.out_pos = out_pos;
  a.out_score = out_score;
  a.flags = flags;
  a.part_pos = nullptr;
  a.part_score = nullptr;
  a.U = U;
  a.M = M;
  a.n_rows = n_rows;
  a.F = F;
  a.X = X;
  a.k = k;
  a.mode = mode;
  a.n_splits = splits;
  a.tiles_per_split = static_cast<int32_t>(ebn_ceil_div(ebn_ceil_div(M, TK_BN), splits));
  if (splits > 1) {
    const int64_t need = ebn_topk_workspace_bytes(U, k, splits);
    EBN_REQUIRE(workspace != nullptr && workspace_bytes >= need, EBN_ERR_BAD_ARG);
    EBN_REQUIRE(ebn_aligned16(workspace), EBN_ERR_ALIGN);
    const int64_t n = static_cast<int64_t>(splits) * U * k;
    a.part_pos = static_cast<int32_t*>(workspace);
    a.part_score = reinterpret_cast<float*>(a.part_pos + n);
  }
  const int64_t lds = topk_lds_bytes(k);
  // above the 64 KB a kernel may use without asking (k > 44); set per call: the attribute belongs to the current device
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(topk_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(topk_lds_bytes(TK_MAX_K))) != hipSuccess) {
    (void)hipGetLastError();
    return EBN_ERR_UNSUPPORTED;
  }
  EBN_LAUNCH(topk_score_kernel, dim3(static_cast<unsigned>(user_tiles), static_cast<unsigned>(splits)), dim3(TK_THREADS),
             static_cast<size_t>(lds), s, a);
  EBN_CHECK_LAUNCH();
  if (splits > 1) {
    EBN_LAUNCH(topk_merge_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(U, 4))), dim3(256), 0, s, a);
    EBN_CHECK_LAUNCH();
  }
  return EBN_OK;
}
