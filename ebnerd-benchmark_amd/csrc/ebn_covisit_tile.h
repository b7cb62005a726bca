// The catalogue tile of the co-visitation top-N kernels (ebn_covisit_topk.hip: ebn_cv_topk_f32 keeps a sorted list,
// ebn_cv_target_rank_f32 counts): everything a score's bits depend on is in here, ONCE, so that a target's rank is the index of its
// slot in the top-k list, with that slot's score bits.
//
//   score(u, c) = the chain over the present entries j of u's history, in history order, that have a stored S[c, h_j]:
//                 acc = p_first, then acc = acc + p_j (mode 0) or max(acc, p_j) (mode 1), p_j = w_j * S[c, h_j]; every product and
//                 every add rounds once (__fmul_rn, __fadd_rn: no contraction into an fma).
//
// A 256-thread workgroup owns ONE user and walks ranges of CVT_R catalogue rows.  Per range an fp32 tile of CVT_R scores and a
// bit per row ("touched") live in LDS.  T = S^T in CSR: row h of T holds the catalogue rows c with a stored S[c, h], ascending, so
// the part of it inside the range is one segment, found by two binary searches; the threads stride over the segment -- the
// columns of one row are distinct, so no two threads meet in a tile element -- and a barrier between entries fixes the order of
// the chain without a floating-point atomic.  The first product of a row is stored, not added to a zero: -0.0 stays -0.0, and
// "never co-visited" is not "score 0".  The touched bits are set with an integer ds_or.
// A second bit per row marks the rows of the range in the user's exclusion list.
#pragma once
#include <math.h>

#include "ebn_common.h"

namespace {

#ifndef EBN_CVT_R
#define EBN_CVT_R 8192                  // -DEBN_CVT_R=...: the probe's alternatives (tools/covisit_topn_probe.py)
#endif
// catalogue rows of one tile: 32 KiB of fp32, four workgroups per CU.  Measured at cv-c1 against 2048, 4096, 16384 and 32768 (DESIGN.md
// section 31): larger tiles leave fewer workgroups in flight to hide the latency of the searches and the scattered LDS updates, smaller
// ones pay two more binary searches per history entry and range
constexpr int CVT_R = EBN_CVT_R;
static_assert(CVT_R % 256 == 0 && CVT_R >= 1024 && CVT_R <= 32768, "whole mask words per thread; tile and masks inside the 160 KiB of LDS");
constexpr int CVT_THREADS = 256;
constexpr int CVT_WORDS = CVT_R / 32;   // words of one bit-per-row mask
constexpr int CVT_MAX_SPLITS = 64;
constexpr int CVT_TILE_FLOATS = CVT_R + 2 * CVT_WORDS;  // tile | touched | excluded; a kernel's own plan follows

struct CvTileArgs {
  const int64_t* t_indptr;
  const int32_t* t_cols;
  const float* t_vals;
  const int32_t* hist_rows;
  const float* hist_weights;
  const int64_t* hist_offsets;
  const int32_t* user_hist;
  const int32_t* cand_pos;
  const int32_t* window;
  const int32_t* exclude;
  int32_t* flags;
  int64_t n_rows, nnz, n_hists, n_hist_items, M, U;
  int32_t X, n_splits, ranges_per_split;
};

struct CvTile {
  float* tile;
  unsigned* touched;
  unsigned* excluded;
  float* own;
};

__device__ __forceinline__ CvTile cvt_tile(float* smem) {
  CvTile t;
  t.tile = smem;
  t.touched = reinterpret_cast<unsigned*>(smem + CVT_R);
  t.excluded = t.touched + CVT_WORDS;
  t.own = smem + CVT_TILE_FLOATS;
  return t;
}

__device__ __forceinline__ int32_t cvt_clamp(int64_t v, int64_t hi) { return static_cast<int32_t>(v < 0 ? 0 : (v > hi ? hi : v)); }

// one step of a chain.  max: a NaN product is taken (it has to reach the flag) and a NaN accumulator stays; of equal values
// (+0.0 and -0.0) the earlier one stays
template <bool MAX>
__device__ __forceinline__ float cvt_step(float acc, float p) {
  if (MAX) return (p > acc || p != p) ? p : acc;
  return __fadd_rn(acc, p);
}

// the entries [hb, he) of user u's history, clamped to [0, n_hist_items]; empty for a user without one
__device__ __forceinline__ void cvt_history(const CvTileArgs& a, int64_t u, int32_t& hb, int32_t& he) {
  const int64_t h = a.user_hist != nullptr ? static_cast<int64_t>(a.user_hist[u]) : u;
  hb = he = 0;
  if (h >= 0 && h < a.n_hists) {
    hb = cvt_clamp(a.hist_offsets[h], a.n_hist_items);
    he = cvt_clamp(a.hist_offsets[h + 1], a.n_hist_items);
    if (he < hb) he = hb;
  }
}

// the clamped window of user u: [0, M) without windows, [0, 0) for an empty one
__device__ __forceinline__ void cvt_window(const CvTileArgs& a, int64_t u, int& lo, int& hi) {
  lo = 0;
  hi = static_cast<int>(a.M);  // M <= INT32_MAX
  if (a.window != nullptr) {
    lo = a.window[2 * u];
    hi = a.window[2 * u + 1];
    lo = lo > 0 ? lo : 0;
    hi = static_cast<int64_t>(hi) < a.M ? hi : static_cast<int>(a.M);
    if (lo >= hi) lo = hi = 0;
  }
}

// the extent of row h of T inside [0, nnz]
__device__ __forceinline__ void cvt_row(const CvTileArgs& a, int32_t h, int32_t& lo, int32_t& hi) {
  lo = cvt_clamp(a.t_indptr[h], a.nnz);
  hi = cvt_clamp(a.t_indptr[h + 1], a.nnz);
}

// first position in [lo, hi) whose column is at least key (hi if none; lo when lo >= hi)
__device__ __forceinline__ int32_t cvt_lower_bound(const int32_t* __restrict__ cols, int32_t lo, int32_t hi, int32_t key) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (cols[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The ranges [g_beg, g_end) of split `split`
__device__ __forceinline__ void cvt_span(const CvTileArgs& a, int split, int64_t& g_beg, int64_t& g_end) {
  const int64_t n_ranges = (a.n_rows + CVT_R - 1) / CVT_R;
  g_beg = static_cast<int64_t>(split) * a.ranges_per_split;
  g_end = g_beg + a.ranges_per_split;
  g_end = g_end < n_ranges ? g_end : n_ranges;
}

// Fills the tile for the rows [r0, r1) (r1 - r0 <= CVT_R) from the history entries [hb, he) of user u, and the excluded bits.
// Every thread of the workgroup calls it with the same arguments; it starts and ends with a barrier.
template <bool MAX>
__device__ __forceinline__ void cvt_accumulate(const CvTileArgs& a, const CvTile& t, int64_t u, int32_t hb, int32_t he, int32_t r0,
                                               int32_t r1, int tid) {
  __syncthreads();  // everybody is done with the previous range
  for (int i = tid; i < 2 * CVT_WORDS; i += CVT_THREADS) t.touched[i] = 0u;  // touched | excluded
  __syncthreads();
  const int32_t rows = static_cast<int32_t>(a.n_rows);  // <= EBN_DIM_MAX
  const unsigned n = static_cast<unsigned>(r1 - r0);
  for (int32_t j = hb; j < he; ++j) {
    const int32_t h = a.hist_rows[j];
    if (h < 0 || h >= rows) continue;  // absent
    int32_t lo, hi;
    cvt_row(a, h, lo, hi);
    const int32_t sb = cvt_lower_bound(a.t_cols, lo, hi, r0);
    const int32_t se = cvt_lower_bound(a.t_cols, sb, hi, r1);
    if (sb >= se) continue;  // nothing of this entry in the range (the same for every thread: no barrier is skipped by a part)
    const float w = a.hist_weights != nullptr ? a.hist_weights[j] : 1.0f;
    for (int32_t i = sb + tid; i < se; i += CVT_THREADS) {
      const unsigned c = static_cast<unsigned>(a.t_cols[i] - r0);
      if (c >= n) continue;  // columns that do not ascend: never an LDS address outside the tile
      const float p = __fmul_rn(w, a.t_vals[i]);
      const unsigned bit = 1u << (c & 31u);
      if (t.touched[c >> 5] & bit) {
        t.tile[c] = cvt_step<MAX>(t.tile[c], p);
      } else {
        t.tile[c] = p;
        atomicOr(&t.touched[c >> 5], bit);
      }
    }
    __syncthreads();  // the next entry finds this one's sums: the order of a chain is the order of the history
  }
  for (int x = tid; x < a.X; x += CVT_THREADS) {
    const int64_t row = a.exclude[u * a.X + x];
    if (row >= r0 && row < r1) atomicOr(&t.excluded[(row - r0) >> 5], 1u << ((row - r0) & 31));
  }
  __syncthreads();
}

// Row r0 + c of the tile for a user with the clamped window [wlo, whi): admissible -> its position and score.  A touched row whose
// position is >= M raises oob, a NaN score of a row that is admissible otherwise raises nan
__device__ __forceinline__ bool cvt_admissible(const CvTileArgs& a, const CvTile& t, int32_t r0, int c, int wlo, int whi, int& pos, float& s,
                                               bool& oob, bool& nan) {
  if (((t.touched[c >> 5] >> (c & 31)) & 1u) == 0u) return false;
  const int64_t p = a.cand_pos != nullptr ? static_cast<int64_t>(a.cand_pos[static_cast<int64_t>(r0) + c]) : static_cast<int64_t>(r0) + c;
  if (p < 0) return false;
  if (p >= a.M) {
    oob = true;
    return false;
  }
  if (p < wlo || p >= whi) return false;
  if ((t.excluded[c >> 5] >> (c & 31)) & 1u) return false;
  const float v = t.tile[c];
  if (v != v) {
    nan = true;
    return false;
  }
  pos = static_cast<int>(p);
  s = v;
  return true;
}

// ---- host.  n_splits ranges divide the ceil(n_rows / CVT_R) tiles of a user.  Automatic: about 16 384 workgroups when the users alone do
// not give them -- a user's cost follows the lengths of its history's rows of T, which a Zipf law spreads over three orders of
// magnitude, so many short workgroups balance better than one long one per user (measured: DESIGN.md section 31).  U, n_rows >= 1
inline int cvt_resolve_splits(int64_t U, int64_t n_rows, int32_t n_splits) {
  const int64_t ranges = ebn_ceil_div(n_rows, CVT_R);
  int64_t s = n_splits > 0 ? n_splits : ebn_ceil_div(16384, U);
  if (s > ranges) s = ranges;
  if (s > CVT_MAX_SPLITS) s = CVT_MAX_SPLITS;
  return static_cast<int>(s < 1 ? 1 : s);
}

}  // namespace
