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
// Everything ahead of the selection -- operand staging, the MFMA step, the window reductions and tile spans, the tile's catalogue
// rows -- is ebn_catalogue_walk.h, shared with ebn_target_rank.hip and the two NPA kernels: this file is the epilogue.
//
// Windowed form (ebn_topk_score_window_f32, the WINDOWED instantiation): user u may only receive the candidate positions of
// window[u] = [lo, hi), clamped to [0, M).  The workgroup keeps its 128 users' clamped ranges in LDS behind the list plan (1 KB),
// reduces them to their union [wlo, whi) and walks only the candidate tiles that meet it, dealt evenly over the n_splits ranges of
// ITS OWN tile span -- with the candidates sorted by what the windows are about (publish time) and the users of a launch sorted
// alike, the cost follows the window, not the catalogue.  A wave whose 32 users' union misses a visited tile only takes the
// barriers; an accumulator element is a survivor only when its column also lies in its row's window (a tile inside every window of
// the wave takes the plain compare), so nothing outside a window reaches the queue, the NaN flag or the lists.  A pair's dot
// product is the same fma chain as in the plain form: the same bits, whatever the windows, the split and the other users are.
#include "ebn_catalogue_walk.h"
#include "ebn_topk_list.h"

namespace {

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

  const WalkSlab sl = walk_slab(tid);
  const float* pa[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) pa[i] = a.users + walk_slab_user(u0, a.U, tid, i) * F + sl.kq4;
  bool saw_nan = false;

  int64_t t_beg, t_end;
  walk_span(a.M, TK_BN, split, a.tiles_per_split, t_beg, t_end);

  // WINDOWED: the users' clamped ranges in LDS (a row past the last user is [0, 0)); the workgroup's union picks the tiles
  volatile int* win_lo = lds.lps + TK_BM * k;  // the end of the plan: topk_lds_bytes(k)
  volatile int* win_hi = win_lo + TK_BM;
  WalkSpans sp;
  if constexpr (WINDOWED) {
    if (tid < TK_BM) {
      const int64_t u = u0 + tid;
      int lo = 0, hi = 0;
      if (u < a.U) walk_clamp(a.window, u, a.M, lo, hi);
      win_lo[tid] = lo;
      win_hi[tid] = hi;
    }
    __syncthreads();
    sp = walk_spans_table(win_lo, win_hi, u0, a.U, wave, lane);
    walk_span(sp, TK_BN, split, a.n_splits, t_beg, t_end);
  }

  for (int64_t t = t_beg; t < t_end; ++t) {
    const int64_t n0 = t * TK_BN;
    __syncthreads();  // every wave is done with the previous tile's candrow (and the lists are initialised)
    walk_rows<WINDOWED>(a, sp, n0, TK_BN, tid, candrow);
    __syncthreads();
    const float* pb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = candrow[walk_slab_row(tid, i)];
      pb[i] = a.news + static_cast<int64_t>(r > 0 ? r : 0) * F + sl.kq4;
    }

    // WINDOWED: a wave none of whose users' windows meets the tile fills the operand images and takes the barriers, nothing else
    const bool wave_on = !WINDOWED || walk_meets(sp, n0, TK_BN);
    f32x16 acc[TK_TILES];
    walk_zero(acc);
    walk_run(As, Bs, sl, pa, pb, nullptr, F, wave_on, [&](int buf) { walk_mma<true>(As, Bs, buf, wave, kl, il, acc); });
    if (!wave_on) continue;

    // ---- selection.  C/D map of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int rbase = wave * 32 + 4 * kl;
    // WINDOWED: the column must lie in the row's window as well -- unless the tile is inside every window of this wave's users
    const bool gated = WINDOWED && walk_gated(sp, n0, TK_BN);
    const int c0 = static_cast<int>(n0) + il;  // this lane's column of MFMA tile 0
    auto row_gate = [&](int rl) {
      WalkGate g;
      if constexpr (WINDOWED) {
        if (gated) g = walk_gate(win_lo[rl], win_hi[rl]);
      }
      return g;
    };
    bool any = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = rbase + (r & 3) + 8 * (r >> 2);
      const float th = thr[rl];
      const WalkGate g = row_gate(rl);
#pragma unroll
      for (int j = 0; j < TK_TILES; ++j) any |= !(acc[j][r] < th) && (!WINDOWED || g.pass(c0 + 32 * j));
    }
    if (__ballot(any) == 0ull) continue;

#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = rbase + (r & 3) + 8 * (r >> 2);
      const float th = thr[rl];
      const WalkGate g = row_gate(rl);
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < TK_TILES; ++j) {
        const bool pass = !(acc[j][r] < th) && (!WINDOWED || g.pass(c0 + 32 * j));
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

}  // namespace

extern "C" int ebn_topk_auto_splits(int64_t n_users, int64_t n_cand) {
  if (!ebn_dim_ok(n_users, n_cand) || n_users == 0 || n_cand == 0) return 1;
  return walk_resolve_splits(n_users, n_cand, TK_BN, 0);
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
  const int splits = walk_resolve_splits(U, M, TK_BN, n_splits);
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
  a.tiles_per_split = walk_units_per_split(M, TK_BN, splits);
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
