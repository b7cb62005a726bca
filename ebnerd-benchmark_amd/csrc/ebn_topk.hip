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
// The list code (LDS plan, drain and insert, write-out, merge and fill launches) is ebn_topk_list.h, shared with ebn_npa_topk.hip.
//
// Windowed form (ebn_topk_score_window_f32, the WINDOWED instantiation): user u may only receive the candidate positions of
// window[u] = [lo, hi), clamped to [0, M).  The workgroup keeps its 128 users' clamped ranges in LDS behind the list plan (1 KB),
// reduces them to their union [wlo, whi) and walks only the candidate tiles that meet it, dealt evenly over the n_splits ranges of
// ITS OWN tile span -- with the candidates sorted by what the windows are about (publish time) and the users of a launch sorted
// alike, the cost follows the window, not the catalogue.  A wave whose 32 users' union misses a visited tile only takes the
// barriers; an accumulator element is a survivor only when its column also lies in its row's window (a tile inside every window of
// the wave takes the plain compare), so nothing outside a window reaches the queue, the NaN flag or the lists.  A pair's dot
// product is the same fma chain as in the plain form: the same bits, whatever the windows, the split and the other users are.
#include "ebn_topk_list.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TK_TN = TK_BN / 32;      // MFMA tiles of a wave along the candidates
constexpr int TK_MAX_F = 8192;
static_assert(TK_QCAP >= 2 * TK_BN, "the survivors of one accumulator index: 2 rows x 128 columns");

struct TopkArgs : TopkList {
  const float* users;
  const float* news;
  const int32_t* cand_rows;
  int64_t M, n_rows;
  int32_t F, tiles_per_split;
  const int32_t* window;  // [U, 2] (lo, hi) candidate positions; the WINDOWED instantiation only
};

constexpr int TK_WINDOW_LDS_BYTES = 2 * TK_BM * 4;  // lo[128] | hi[128] behind the plan of ebn_topk_list.h

// dynamic LDS layout: ebn_topk_list.h (WINDOWED: + lo[128] | hi[128])
template <bool WINDOWED>
__global__ __launch_bounds__(TK_THREADS, 2) void topk_score_kernel(TopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = lane >> 5, il = lane & 31;
  const int k = a.k, F = a.F;
  const int64_t u0 = static_cast<int64_t>(blockIdx.x) * TK_BM;
  const int split = blockIdx.y;
  const TopkLds lds = topk_lds(smem, wave, k);
  float *As = lds.As, *Bs = lds.Bs;
  volatile float* thr = lds.thr;
  volatile int* candrow = lds.candrow;
  volatile float* qs = lds.qs;
  volatile int* qrc = lds.qrc;

  topk_list_init(lds, k, tid);
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
  int64_t t_beg = static_cast<int64_t>(split) * a.tiles_per_split;
  int64_t t_end = t_beg + a.tiles_per_split;
  t_end = t_end < n_tiles ? t_end : n_tiles;
  const int nk = (F + TK_BK - 1) / TK_BK;

  // WINDOWED: the users' clamped ranges (an empty one, and a row past the last user, is [0, 0): no column passes), the union of
  // the workgroup [wlo, whi) and of this wave [vlo, vhi) over the non-empty ones, the intersection of this wave [ilo, ihi) over
  // its users below U.  All of them are wave-uniform.
  volatile int* win_lo = lds.lps + TK_BM * k;  // the end of the plan: topk_lds_bytes(k)
  volatile int* win_hi = win_lo + TK_BM;
  int wlo = 0, whi = 0, vlo = 0, vhi = 0, ilo = 0, ihi = 0;
  if constexpr (WINDOWED) {
    if (tid < TK_BM) {
      const int64_t u = u0 + tid;
      int lo = 0, hi = 0;
      if (u < a.U) {
        lo = a.window[2 * u];
        hi = a.window[2 * u + 1];
        lo = lo > 0 ? lo : 0;
        hi = static_cast<int64_t>(hi) < a.M ? hi : static_cast<int>(a.M);  // M <= INT32_MAX
        if (lo >= hi) lo = hi = 0;
      }
      win_lo[tid] = lo;
      win_hi[tid] = hi;
    }
    __syncthreads();
    // lane l: rows l and l + 64 for the workgroup, row 32 wave + (l & 31) for the wave
    int ulo = INT32_MAX, uhi = 0, xlo = INT32_MAX, xhi = 0, nlo = 0, nhi = INT32_MAX;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int lo = win_lo[lane + 64 * i], hi = win_hi[lane + 64 * i];
      if (lo < hi) {
        ulo = lo < ulo ? lo : ulo;
        uhi = hi > uhi ? hi : uhi;
      }
    }
    {
      const int row = wave * 32 + il;
      const int lo = win_lo[row], hi = win_hi[row];
      if (lo < hi) {
        xlo = lo;
        xhi = hi;
      }
      if (u0 + row < a.U) {
        nlo = lo;
        nhi = hi;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o0 = __shfl_xor(ulo, off, 64), o1 = __shfl_xor(uhi, off, 64), o2 = __shfl_xor(xlo, off, 64);
      const int o3 = __shfl_xor(xhi, off, 64), o4 = __shfl_xor(nlo, off, 64), o5 = __shfl_xor(nhi, off, 64);
      ulo = o0 < ulo ? o0 : ulo;
      uhi = o1 > uhi ? o1 : uhi;
      xlo = o2 < xlo ? o2 : xlo;
      xhi = o3 > xhi ? o3 : xhi;
      nlo = o4 > nlo ? o4 : nlo;
      nhi = o5 < nhi ? o5 : nhi;
    }
    wlo = __builtin_amdgcn_readfirstlane(ulo);
    whi = __builtin_amdgcn_readfirstlane(uhi);
    vlo = __builtin_amdgcn_readfirstlane(xlo);
    vhi = __builtin_amdgcn_readfirstlane(xhi);
    ilo = __builtin_amdgcn_readfirstlane(nlo);
    ihi = __builtin_amdgcn_readfirstlane(nhi);
    // the tiles that meet the union (none: wlo = INT32_MAX, whi = 0), dealt evenly over the splits
    const int64_t w_beg = wlo / TK_BN, w_end = wlo < whi ? (static_cast<int64_t>(whi) + TK_BN - 1) / TK_BN : w_beg;
    const int64_t w_n = w_end - w_beg;
    t_beg = w_beg + w_n * split / a.n_splits;
    t_end = w_beg + w_n * (split + 1) / a.n_splits;
  }

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
          if (!WINDOWED || (c >= wlo && c < whi)) a.flags[0] = 1;  // a visited tile also has columns outside the union
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

    // WINDOWED: a wave none of whose users' windows meets the tile fills the operand images and takes the barriers, nothing else
    const bool wave_on = !WINDOWED || (n0 < vhi && n0 + TK_BN > vlo);
    fetch(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
      if (kt + 1 < nk) fetch(kt + 1);
      if (wave_on) mma(0);
      if (kt + 1 < nk) store(1);
      __syncthreads();
      if (kt + 1 < nk) {
        if (kt + 2 < nk) fetch(kt + 2);
        if (wave_on) mma(1);
        if (kt + 2 < nk) store(0);
        __syncthreads();
      }
    }
    if (!wave_on) continue;

    // ---- selection.  C/D map of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int rbase = wave * 32 + 4 * kl;
    // WINDOWED: the column must lie in the row's window as well -- unless the tile is inside every window of this wave's users
    const bool gated = WINDOWED && !(n0 >= ilo && n0 + TK_BN <= ihi);
    const int c0 = static_cast<int>(n0) + il;  // this lane's column of MFMA tile 0
    bool any = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = rbase + (r & 3) + 8 * (r >> 2);
      const float th = thr[rl];
      // lo <= c < hi as ONE unsigned compare: (c - lo) < (hi - lo); 0 <= lo <= hi <= M and c < 2^31, nothing wraps
      int d = 0;
      unsigned w = UINT32_MAX;
      if constexpr (WINDOWED) {
        if (gated) {
          const int lo = win_lo[rl];
          d = c0 - lo;
          w = static_cast<unsigned>(win_hi[rl] - lo);
        }
      }
#pragma unroll
      for (int j = 0; j < TK_TN; ++j) any |= !(acc[j][r] < th) && (!WINDOWED || static_cast<unsigned>(d + 32 * j) < w);
    }
    if (__ballot(any) == 0ull) continue;

#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = rbase + (r & 3) + 8 * (r >> 2);
      const float th = thr[rl];
      int d = 0;
      unsigned w = UINT32_MAX;
      if constexpr (WINDOWED) {
        if (gated) {
          const int lo = win_lo[rl];
          d = c0 - lo;
          w = static_cast<unsigned>(win_hi[rl] - lo);
        }
      }
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < TK_TN; ++j) {
        const bool pass = !(acc[j][r] < th) && (!WINDOWED || static_cast<unsigned>(d + 32 * j) < w);
        const unsigned long long m = __ballot(pass);
        if (pass) {
          const int slot = cnt + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
          qs[slot] = acc[j][r];
          qrc[slot] = (rl << 8) | (j * 32 + il);
        }
        cnt += __popcll(m);
      }
      topk_list_drain(a, lds, cnt, u0, n0, lane, saw_nan);
    }
  }

  if (saw_nan) a.flags[1] = 1;
  topk_list_write(a, lds, u0, split, wave, lane);
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

namespace {

// both entry points: the checks, the plan and the launches; WINDOWED adds the window argument and 1 KB of LDS
template <bool WINDOWED>
int topk_score(const float* users, const float* news_all, int64_t n_rows, const int32_t* cand_rows, int64_t M, const int32_t* window,
               const int32_t* exclude, int32_t X, int32_t k, int32_t mode, int32_t n_splits, int32_t* out_pos, float* out_score,
               int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U, int32_t F, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(U, M, n_rows) && F >= 0 && X >= 0 && n_splits >= 0 && workspace_bytes >= 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(mode == 0 || mode == 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(k >= 1 && k <= TK_MAX_K && X <= TK_MAX_X && F >= 4 && F % 4 == 0 && F <= TK_MAX_F, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(cand_rows != nullptr || M == n_rows, EBN_ERR_BAD_ARG);
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(out_pos != nullptr && out_score != nullptr && flags != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(!WINDOWED || window != nullptr, EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (M == 0) return topk_launch_fill_empty(out_pos, out_score, U, k, s);
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
  a.window = window;
  a.exclude = exclude;
  a.out_pos = out_pos;
  a.out_score = out_score;
  a.flags = flags;
  a.U = U;
  a.M = M;
  a.n_rows = n_rows;
  a.F = F;
  a.X = X;
  a.k = k;
  a.mode = mode;
  a.n_splits = splits;
  a.tiles_per_split = static_cast<int32_t>(ebn_ceil_div(ebn_ceil_div(M, TK_BN), splits));
  const int rc = topk_bind_workspace(a, splits, workspace, workspace_bytes);
  if (rc != EBN_OK) return rc;
  constexpr int extra = WINDOWED ? TK_WINDOW_LDS_BYTES : 0;
  const int64_t lds = topk_lds_bytes(k) + extra;
  // above the 64 KB a kernel may use without asking (k > 44); set per call: the attribute belongs to the current device
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(topk_score_kernel<WINDOWED>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(topk_lds_bytes(TK_MAX_K)) + extra) != hipSuccess) {
    (void)hipGetLastError();
    return EBN_ERR_UNSUPPORTED;
  }
  EBN_LAUNCH(topk_score_kernel<WINDOWED>, dim3(static_cast<unsigned>(user_tiles), static_cast<unsigned>(splits)), dim3(TK_THREADS),
             static_cast<size_t>(lds), s, a);
  EBN_CHECK_LAUNCH();
  if (splits > 1) return topk_launch_merge(a, s);
  return EBN_OK;
}

}  // namespace

extern "C" int ebn_topk_score_f32(const float* users, const float* news_all, int64_t n_rows, const int32_t* cand_rows, int64_t M,
                                  const int32_t* exclude, int32_t X, int32_t k, int32_t mode, int32_t n_splits, int32_t* out_pos,
                                  float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U, int32_t F,
                                  ebn_stream_t stream) {
  return topk_score<false>(users, news_all, n_rows, cand_rows, M, nullptr, exclude, X, k, mode, n_splits, out_pos, out_score, flags,
                           workspace, workspace_bytes, U, F, stream);
}

extern "C" int ebn_topk_score_window_f32(const float* users, const float* news_all, int64_t n_rows, const int32_t* cand_rows, int64_t M,
                                         const int32_t* window, const int32_t* exclude, int32_t X, int32_t k, int32_t mode,
                                         int32_t n_splits, int32_t* out_pos, float* out_score, int32_t* flags, void* workspace,
                                         int64_t workspace_bytes, int64_t U, int32_t F, ebn_stream_t stream) {
  return topk_score<true>(users, news_all, n_rows, cand_rows, M, window, exclude, X, k, mode, n_splits, out_pos, out_score, flags,
                          workspace, workspace_bytes, U, F, stream);
}
