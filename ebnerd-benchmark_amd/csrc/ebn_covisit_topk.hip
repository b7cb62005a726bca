// Co-visitation top-N lists and clicked-article ranks over the WHOLE catalogue (contract in include/ebnerd_hip.h): the second
// outlet of the co-visitation baseline, beside the in-view scores of ebn_covisit.hip.
//
//   score(u, c) = sum_j w_j S[c, h_j]  (or the max) over the history entries of u with a stored S[c, h_j]
//
// ebn_cv_scores_f32 finds S[c, h_j] per (candidate, entry) pair by binary search: right for 10 in-view items, hopeless for a
// 125 000-row catalogue per user.  Here the matrix comes transposed (row h of T: every c with a stored S[c, h]) and a 256-thread
// workgroup per (user, split) walks ranges of CVT_R catalogue rows: the history's rows of T are accumulated into an LDS tile
// (ebn_covisit_tile.h: the chain of a score, its order and its rounding are there, once), and the tile is scanned:
//   * ebn_cv_topk_f32: wave w scans the rows w * 64 + lane, + 256, ... and keeps ITS OWN sorted list of k <= 64 entries in
//     registers, lane t slot t; a survivor past the list's k-th entry is inserted by the whole wave (rank by ballot popcount, the
//     tail moves down one lane -- topk_list_drain's insertion without the LDS round trip).  The total order (score descending,
//     position ascending; positions are distinct) makes a list independent of the order of arrival, so the four lists are merged
//     by wave 0 through 1.5 KiB of LDS at the end, and the lists of the splits by topk_merge_kernel (ebn_topk_list.h).
//   * ebn_cv_target_rank_f32: first the target's own chain -- the catalogue row of target_pos (through the inverse of cand_pos,
//     which one small launch writes into the workspace once per call), then
//     one thread per history entry looks the row up in its row of T and thread 0 folds the products in history order: the steps
//     and the order of cvt_accumulate, so t has the tile's bits and every split can compare against it.  Then the same walk with
//     two integer counters per thread in place of the list.
// No floating-point atomics anywhere; the integer ones (LDS bit masks) do not depend on order.  Bit-identical for every n_splits,
// from run to run and whoever shares the launch.
#include "ebn_covisit_tile.h"
#include "ebn_topk_list.h"

namespace {

constexpr int CVK_MERGE_FLOATS = 2 * 3 * 64;                  // the lists of waves 1 .. 3: score[3][64] | position[3][64]
constexpr int CVR_OWN_FLOATS = 2 * CVT_THREADS + 16;          // product[256] | found[256] | misc
static_assert(TK_MAX_SPLITS == CVT_MAX_SPLITS, "the merge launch holds one split per lane");

struct CvTopkArgs : CvTileArgs {
  int32_t* out_pos;
  float* out_score;
  int32_t* part_pos;  // [n_splits, U, k] (n_splits > 1)
  float* part_score;
  int32_t k;
};

struct CvRankArgs : CvTileArgs {
  const int32_t* target_pos;
  int32_t* out_rank;
  int32_t* out_count;
  float* out_score;
  int32_t* part;  // [2, n_splits, U]: admissible, ahead (n_splits > 1)
  float* part_t;  // [U]: the target score, NaN = no rank
  const int32_t* row_of_pos;  // [M]: the inverse of cand_pos (cand_pos != NULL), written by cv_row_of_pos_kernel
};

inline int64_t cv_topk_lds_bytes() { return static_cast<int64_t>(CVT_TILE_FLOATS + CVK_MERGE_FLOATS) * 4; }
inline int64_t cv_rank_lds_bytes() { return static_cast<int64_t>(CVT_TILE_FLOATS + CVR_OWN_FLOATS) * 4; }

template <bool MAX>
__global__ __launch_bounds__(CVT_THREADS, 2) void cv_topk_kernel(CvTopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const CvTile t = cvt_tile(smem);
  float* ms = t.own;
  int* mp = reinterpret_cast<int*>(t.own + 3 * 64);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t u = blockIdx.x;
  const int split = blockIdx.y, k = a.k;

  int32_t hb, he;
  cvt_history(a, u, hb, he);
  int wlo, whi;
  cvt_window(a, u, wlo, whi);
  int64_t g_beg, g_end;
  cvt_span(a, split, g_beg, g_end);

  float es = -INFINITY;  // slot `lane` of this wave's list
  int ep = TK_EMPTY;
  bool oob = false, nan = false;
  if (he > hb) {  // a user without history touches nothing
    for (int64_t g = g_beg; g < g_end; ++g) {
      const int32_t r0 = static_cast<int32_t>(g * CVT_R);
      const int32_t r1 = static_cast<int32_t>(a.n_rows - r0 < CVT_R ? a.n_rows : r0 + CVT_R);
      cvt_accumulate<MAX>(a, t, u, hb, he, r0, r1, tid);
      const int n = r1 - r0;
      for (int base = 0; base < n; base += CVT_THREADS) {
        const int c = base + tid;
        int pos = 0;
        float s = 0.f;
        const bool ok = c < n && cvt_admissible(a, t, r0, c, wlo, whi, pos, s, oob, nan);
        if (__ballot(ok) != 0ull) topk_wave_offer(es, ep, k, lane, ok, s, pos);
      }
    }
  }
  if (oob) a.flags[0] = 1;
  if (nan) a.flags[1] = 1;

  // the lists of waves 1 .. 3 into wave 0's
  if (wave > 0 && lane < k) {
    ms[(wave - 1) * 64 + lane] = es;
    mp[(wave - 1) * 64 + lane] = ep;
  }
  __syncthreads();
  if (wave != 0) return;
  for (int w = 0; w < 3; ++w) {
    const float s = lane < k ? ms[w * 64 + lane] : 0.f;
    const int pos = lane < k ? mp[w * 64 + lane] : TK_EMPTY;
    topk_wave_offer(es, ep, k, lane, pos != TK_EMPTY, s, pos);
  }
  if (lane < k) {
    if (a.n_splits == 1) {
      const bool empty = ep == TK_EMPTY;
      a.out_pos[u * k + lane] = empty ? -1 : ep;
      a.out_score[u * k + lane] = empty ? -INFINITY : es;
    } else {
      const int64_t o = (static_cast<int64_t>(split) * a.U + u) * k + lane;
      a.part_pos[o] = ep;
      a.part_score[o] = es;
    }
  }
}

__device__ __forceinline__ void cvr_write(const CvRankArgs& a, int64_t u, int count, int ahead, float t) {
  const bool ranked = t == t;
  a.out_rank[u] = ranked ? 1 + ahead : 0;
  a.out_count[u] = count;
  a.out_score[u] = ranked ? t : -INFINITY;
}

template <bool MAX>
__global__ __launch_bounds__(CVT_THREADS, 2) void cv_rank_kernel(CvRankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const CvTile t = cvt_tile(smem);
  float* s_p = t.own;
  int* s_f = reinterpret_cast<int*>(t.own + CVT_THREADS);
  int* s_misc = s_f + CVT_THREADS;  // [1] the target's row is excluded, [2] its position or -1, [4 .. 11] the waves' counts
  float* s_t = reinterpret_cast<float*>(s_misc + 3);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t u = blockIdx.x;
  const int split = blockIdx.y;

  int32_t hb, he;
  cvt_history(a, u, hb, he);
  int wlo, whi;
  cvt_window(a, u, wlo, whi);
  int64_t g_beg, g_end;
  cvt_span(a, split, g_beg, g_end);
  bool oob = false, nan = false;

  // ---- the target: its row, then its chain in history order
  int tp = a.target_pos[u];
  if (static_cast<int64_t>(tp) >= a.M) {
    oob = true;
    tp = -1;
  }
  if (tp < wlo || tp >= whi) tp = -1;  // also tp < 0
  if (he <= hb) tp = -1;               // nothing is touched
  int trow = tp;  // without cand_pos the position is the row
  if (tp >= 0 && a.cand_pos != nullptr) {  // through the inverse map; a slot no row wrote holds anything: checked against cand_pos
    const int r = a.row_of_pos[tp];
    trow = (r >= 0 && r < a.n_rows && a.cand_pos[r] == tp) ? r : -1;
  }
  if (tid == 0) s_misc[1] = 0;
  __syncthreads();
  if (trow >= 0) {
    for (int x = tid; x < a.X; x += CVT_THREADS)
      if (a.exclude[u * a.X + x] == trow) s_misc[1] = 1;
  }
  __syncthreads();
  const bool chase = trow >= 0 && s_misc[1] == 0;
  float acc = 0.f;  // thread 0's
  bool any = false;
  if (chase) {
    const int32_t rows = static_cast<int32_t>(a.n_rows);
    for (int32_t jb = hb; jb < he; jb += CVT_THREADS) {
      const int32_t left = he - jb;
      float p = 0.f;
      int f = 0;
      if (tid < left) {
        const int32_t j = jb + tid;
        const int32_t h = a.hist_rows[j];
        if (h >= 0 && h < rows) {
          int32_t lo, hi;
          cvt_row(a, h, lo, hi);
          const int32_t at = cvt_lower_bound(a.t_cols, lo, hi, trow);
          if (at < hi && a.t_cols[at] == trow) {
            f = 1;
            p = __fmul_rn(a.hist_weights != nullptr ? a.hist_weights[j] : 1.0f, a.t_vals[at]);
          }
        }
      }
      s_p[tid] = p;
      s_f[tid] = f;
      __syncthreads();
      if (tid == 0) {
        const int n = left < CVT_THREADS ? left : CVT_THREADS;
        for (int i = 0; i < n; ++i) {
          if (s_f[i] == 0) continue;
          acc = any ? cvt_step<MAX>(acc, s_p[i]) : s_p[i];
          any = true;
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    float tt = __builtin_nanf("");
    if (any) {
      if (acc != acc) nan = true;  // admissible but for the NaN
      else tt = acc;
    }
    s_t[0] = tt;
    s_misc[2] = tt == tt ? tp : -1;
  }
  __syncthreads();
  const float tt = s_t[0];
  const int ttp = s_misc[2];

  // ---- the walk
  int n_adm = 0, n_ahd = 0;
  if (he > hb) {
    for (int64_t g = g_beg; g < g_end; ++g) {
      const int32_t r0 = static_cast<int32_t>(g * CVT_R);
      const int32_t r1 = static_cast<int32_t>(a.n_rows - r0 < CVT_R ? a.n_rows : r0 + CVT_R);
      cvt_accumulate<MAX>(a, t, u, hb, he, r0, r1, tid);
      const int n = r1 - r0;
      for (int c = tid; c < n; c += CVT_THREADS) {
        int pos = 0;
        float s = 0.f;
        if (cvt_admissible(a, t, r0, c, wlo, whi, pos, s, oob, nan)) {
          ++n_adm;
          n_ahd += (s > tt || (s == tt && pos < ttp)) ? 1 : 0;
        }
      }
    }
  }
  if (oob) a.flags[0] = 1;
  if (nan) a.flags[1] = 1;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_adm += __shfl_xor(n_adm, off, 64);
    n_ahd += __shfl_xor(n_ahd, off, 64);
  }
  __syncthreads();  // s_misc[2] has been read
  if (lane == 0) {
    s_misc[4 + wave] = n_adm;
    s_misc[8 + wave] = n_ahd;
  }
  __syncthreads();
  if (tid == 0) {
    const int count = s_misc[4] + s_misc[5] + s_misc[6] + s_misc[7];
    const int ahead = s_misc[8] + s_misc[9] + s_misc[10] + s_misc[11];
    if (a.n_splits == 1) {
      cvr_write(a, u, count, ahead, tt);
    } else {
      a.part[static_cast<int64_t>(split) * a.U + u] = count;
      a.part[(static_cast<int64_t>(a.n_splits) + split) * a.U + u] = ahead;
      if (split == 0) a.part_t[u] = tt;
    }
  }
}

// the inverse of cand_pos, once per call: row_of_pos[cand_pos[r]] = r for the positions inside [0, M).  The other slots are left as
// they are -- a reader checks cand_pos[row_of_pos[p]] == p -- so one launch does, without a fill ahead of it
__global__ __launch_bounds__(256) void cv_row_of_pos_kernel(const int32_t* __restrict__ cand_pos, int64_t n_rows, int64_t M,
                                                            int32_t* __restrict__ row_of_pos) {
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; r < n_rows; r += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t p = cand_pos[r];
    if (p >= 0 && p < M) row_of_pos[p] = static_cast<int32_t>(r);
  }
}

// adds the n_splits partial counts of a user: integer sums, any order gives the same
__global__ __launch_bounds__(256) void cv_rank_merge_kernel(CvRankArgs a) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (u >= a.U) return;
  int count = 0, ahead = 0;
  for (int s = 0; s < a.n_splits; ++s) {
    count += a.part[static_cast<int64_t>(s) * a.U + u];
    ahead += a.part[(static_cast<int64_t>(a.n_splits) + s) * a.U + u];
  }
  cvr_write(a, u, count, ahead, a.part_t[u]);
}

// an empty matrix or no candidate position: nobody has a rank; a target position >= M is still reported
__global__ __launch_bounds__(256) void cv_rank_empty_kernel(const int32_t* __restrict__ target_pos, int64_t M, int32_t* __restrict__ out_rank,
                                                            int32_t* __restrict__ out_count, float* __restrict__ out_score,
                                                            int32_t* __restrict__ flags, int64_t U) {
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; u < U; u += static_cast<int64_t>(gridDim.x) * 256) {
    if (static_cast<int64_t>(target_pos[u]) >= M) flags[0] = 1;
    out_rank[u] = 0;
    out_count[u] = 0;
    out_score[u] = -INFINITY;
  }
}

// what both entry points check first, in this order
int cv_check(int64_t n_rows, int64_t nnz, int64_t n_hists, int64_t n_hist_items, const int32_t* cand_pos, int64_t M, int32_t X, int32_t k,
             int32_t mode, int32_t n_splits, int64_t workspace_bytes, int64_t U) {
  EBN_REQUIRE(ebn_dim_ok(n_rows, nnz, n_hists, n_hist_items) && ebn_dim_ok(M, U) && X >= 0 && n_splits >= 0 && workspace_bytes >= 0,
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE((mode == 0 || mode == 1) && (n_hist_items == 0 || n_hists >= 1) && (cand_pos != nullptr || M == n_rows), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(k >= 1 && k <= TK_MAX_K && X <= TK_MAX_X, EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

// the operands a launch reads
bool cv_operands_ok(const CvTileArgs& a) {
  return a.t_indptr != nullptr && a.t_cols != nullptr && a.t_vals != nullptr && (a.n_hists == 0 || a.hist_offsets != nullptr) &&
         (a.n_hist_items == 0 || a.hist_rows != nullptr);
}

template <class Kernel>
bool cv_allow_lds(Kernel kernel, int64_t bytes) {
  // only a build with a larger tile (-DEBN_CVT_R=16384 and up) is above the 64 KB a kernel may use without asking; set per call:
  // the attribute belongs to the current device
  if (bytes <= 64 * 1024) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)) !=
      hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

}  // namespace

extern "C" int64_t ebn_cv_topk_range(void) { return CVT_R; }

extern "C" int ebn_cv_topk_auto_splits(int64_t n_users, int64_t n_rows) {
  if (!ebn_dim_ok(n_users, n_rows) || n_users == 0 || n_rows == 0) return 1;
  return cvt_resolve_splits(n_users, n_rows, 0);
}

extern "C" int64_t ebn_cv_topk_workspace_bytes(int64_t n_users, int32_t k, int32_t n_splits) {
  return ebn_topk_workspace_bytes(n_users, k, n_splits);  // the partial lists are ebn_topk_score_f32's
}

extern "C" int64_t ebn_cv_target_rank_workspace_bytes(int64_t n_users, int32_t n_splits, int64_t n_positions) {
  if (!ebn_dim_ok(n_users, n_positions) || n_splits < 1) return 0;
  if (n_users == 0) return 16;
  // [M] int32: the inverse of cand_pos (n_positions = M with a cand_pos, else 0); then, for more than one split (one writes the
  // outputs directly), [2, s, U] int32 partial counts and [U] float target scores
  const int64_t s = n_splits > CVT_MAX_SPLITS ? CVT_MAX_SPLITS : n_splits;
  const int64_t parts = n_splits == 1 ? 0 : ebn_sat_add(ebn_sat_mul(2 * s, n_users), n_users);
  return ebn_sat_add(ebn_sat_mul(ebn_sat_add(parts, n_positions), 4), 16);
}

extern "C" int ebn_cv_topk_f32(const int64_t* t_indptr, const int32_t* t_cols, const float* t_vals, int64_t n_rows, int64_t nnz,
                               const int32_t* hist_rows, const float* hist_weights, const int64_t* hist_offsets, int64_t n_hists,
                               int64_t n_hist_items, const int32_t* user_hist, const int32_t* cand_pos, int64_t M, const int32_t* window,
                               const int32_t* exclude, int32_t X, int32_t k, int32_t mode, int32_t n_splits, int32_t* out_pos,
                               float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U,
                               ebn_stream_t stream) {
  const int rc0 = cv_check(n_rows, nnz, n_hists, n_hist_items, cand_pos, M, X, k, mode, n_splits, workspace_bytes, U);
  if (rc0 != EBN_OK) return rc0;
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(out_pos != nullptr && out_score != nullptr && flags != nullptr, EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (n_rows == 0 || nnz == 0 || M == 0) return topk_launch_fill_empty(out_pos, out_score, U, k, s);
  CvTopkArgs a;
  a.t_indptr = t_indptr;
  a.t_cols = t_cols;
  a.t_vals = t_vals;
  a.hist_rows = hist_rows;
  a.hist_weights = hist_weights;
  a.hist_offsets = hist_offsets;
  a.user_hist = user_hist;
  a.cand_pos = cand_pos;
  a.window = window;
  a.exclude = exclude;
  a.flags = flags;
  a.n_rows = n_rows;
  a.nnz = nnz;
  a.n_hists = n_hists;
  a.n_hist_items = n_hist_items;
  a.M = M;
  a.U = U;
  a.X = exclude != nullptr ? X : 0;
  a.k = k;
  a.out_pos = out_pos;
  a.out_score = out_score;
  EBN_REQUIRE(cv_operands_ok(a), EBN_ERR_BAD_ARG);
  const int splits = cvt_resolve_splits(U, n_rows, n_splits);
  a.n_splits = splits;
  a.ranges_per_split = static_cast<int32_t>(ebn_ceil_div(ebn_ceil_div(n_rows, CVT_R), splits));
  TopkList l;
  l.exclude = nullptr;
  l.out_pos = out_pos;
  l.out_score = out_score;
  l.flags = flags;
  l.U = U;
  l.X = 0;
  l.k = k;
  l.mode = 0;  // the kept values are written as they are
  l.n_splits = splits;
  const int rc = topk_bind_workspace(l, splits, workspace, workspace_bytes);
  if (rc != EBN_OK) return rc;
  a.part_pos = l.part_pos;
  a.part_score = l.part_score;
  const dim3 grid(static_cast<unsigned>(U), static_cast<unsigned>(splits)), block(CVT_THREADS);
  const size_t lds = static_cast<size_t>(cv_topk_lds_bytes());
  if (mode == 1) {
    EBN_REQUIRE(cv_allow_lds(cv_topk_kernel<true>, cv_topk_lds_bytes()), EBN_ERR_UNSUPPORTED);
    EBN_LAUNCH(cv_topk_kernel<true>, grid, block, lds, s, a);
  } else {
    EBN_REQUIRE(cv_allow_lds(cv_topk_kernel<false>, cv_topk_lds_bytes()), EBN_ERR_UNSUPPORTED);
    EBN_LAUNCH(cv_topk_kernel<false>, grid, block, lds, s, a);
  }
  EBN_CHECK_LAUNCH();
  if (splits > 1) return topk_launch_merge(l, s);
  return EBN_OK;
}

extern "C" int ebn_cv_target_rank_f32(const int64_t* t_indptr, const int32_t* t_cols, const float* t_vals, int64_t n_rows, int64_t nnz,
                                      const int32_t* hist_rows, const float* hist_weights, const int64_t* hist_offsets, int64_t n_hists,
                                      int64_t n_hist_items, const int32_t* user_hist, const int32_t* cand_pos, int64_t M,
                                      const int32_t* target_pos, const int32_t* window, const int32_t* exclude, int32_t X, int32_t mode,
                                      int32_t n_splits, int32_t* out_rank, int32_t* out_count, float* out_score, int32_t* flags,
                                      void* workspace, int64_t workspace_bytes, int64_t U, ebn_stream_t stream) {
  const int rc0 = cv_check(n_rows, nnz, n_hists, n_hist_items, cand_pos, M, X, 1, mode, n_splits, workspace_bytes, U);
  if (rc0 != EBN_OK) return rc0;
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(target_pos != nullptr && out_rank != nullptr && out_count != nullptr && out_score != nullptr && flags != nullptr,
              EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (n_rows == 0 || nnz == 0 || M == 0) {
    const int64_t blocks = ebn_ceil_div(U, 256);
    EBN_LAUNCH(cv_rank_empty_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, target_pos, M, out_rank,
               out_count, out_score, flags, U);
    EBN_CHECK_LAUNCH();
    return EBN_OK;
  }
  CvRankArgs a;
  a.t_indptr = t_indptr;
  a.t_cols = t_cols;
  a.t_vals = t_vals;
  a.hist_rows = hist_rows;
  a.hist_weights = hist_weights;
  a.hist_offsets = hist_offsets;
  a.user_hist = user_hist;
  a.cand_pos = cand_pos;
  a.window = window;
  a.exclude = exclude;
  a.flags = flags;
  a.n_rows = n_rows;
  a.nnz = nnz;
  a.n_hists = n_hists;
  a.n_hist_items = n_hist_items;
  a.M = M;
  a.U = U;
  a.X = exclude != nullptr ? X : 0;
  a.target_pos = target_pos;
  a.out_rank = out_rank;
  a.out_count = out_count;
  a.out_score = out_score;
  a.part = nullptr;
  a.part_t = nullptr;
  EBN_REQUIRE(cv_operands_ok(a), EBN_ERR_BAD_ARG);
  const int splits = cvt_resolve_splits(U, n_rows, n_splits);
  a.n_splits = splits;
  a.ranges_per_split = static_cast<int32_t>(ebn_ceil_div(ebn_ceil_div(n_rows, CVT_R), splits));
  a.row_of_pos = nullptr;
  if (splits > 1 || cand_pos != nullptr) {
    const int64_t need = ebn_cv_target_rank_workspace_bytes(U, splits, cand_pos != nullptr ? M : 0);
    EBN_REQUIRE(workspace != nullptr && workspace_bytes >= need, EBN_ERR_BAD_ARG);
    EBN_REQUIRE(ebn_aligned16(workspace), EBN_ERR_ALIGN);
    int32_t* w = static_cast<int32_t*>(workspace);
    if (cand_pos != nullptr) {
      a.row_of_pos = w;
      w += M;
    }
    if (splits > 1) {
      a.part = w;
      a.part_t = reinterpret_cast<float*>(w + 2 * static_cast<int64_t>(splits) * U);
    }
  }
  if (cand_pos != nullptr) {
    const int64_t blocks = ebn_ceil_div(n_rows, 256);
    EBN_LAUNCH(cv_row_of_pos_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, cand_pos, n_rows, M,
               static_cast<int32_t*>(workspace));
    EBN_CHECK_LAUNCH();
  }
  const dim3 grid(static_cast<unsigned>(U), static_cast<unsigned>(splits)), block(CVT_THREADS);
  const size_t lds = static_cast<size_t>(cv_rank_lds_bytes());
  if (mode == 1) {
    EBN_REQUIRE(cv_allow_lds(cv_rank_kernel<true>, cv_rank_lds_bytes()), EBN_ERR_UNSUPPORTED);
    EBN_LAUNCH(cv_rank_kernel<true>, grid, block, lds, s, a);
  } else {
    EBN_REQUIRE(cv_allow_lds(cv_rank_kernel<false>, cv_rank_lds_bytes()), EBN_ERR_UNSUPPORTED);
    EBN_LAUNCH(cv_rank_kernel<false>, grid, block, lds, s, a);
  }
  EBN_CHECK_LAUNCH();
  if (splits > 1) {
    EBN_LAUNCH(cv_rank_merge_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(U, 256))), dim3(256), 0, s, a);
    EBN_CHECK_LAUNCH();
  }
  return EBN_OK;
}
