// The catalogue tiles of the history-kNN top-N kernels (ebn_knn_topk.hip: ebn_knn_topk_f32 keeps a sorted list,
// ebn_knn_target_rank_f32 counts): everything a score's bits depend on is in here, ONCE, so that a target's rank is the index of its
// slot in the top-k list, with that slot's score bits.
//
//   score(u, c) = the chain over the present neighbours j of u's neighbour row, in list order, whose set holds row c:
//                 acc = sim_first, then acc = acc + sim_j (__fadd_rn); closed by one __fmul_rn with item_scale[c] where there is one.
//
// A 256-thread workgroup owns ONE user and walks ranges of KNT_R catalogue rows; the user's neighbour row is staged once in LDS as
// (set begin, set end, sim), an absent neighbour as an empty set.  The sets are SHORT and many, so a range is cut into four
// WAVE-PRIVATE tiles of KNT_WR = KNT_R / 4 rows (fp32 scores, a touched and an excluded bit per row): a wave cuts every set to its
// tile with one LANE per neighbour (two binary searches each, 64 neighbours at a time), then takes the neighbours that have a
// segment one after the other in list order, its lanes striding over the segment.  The rows of one set are distinct, so no two
// lanes meet in a tile element, and one wave's LDS operations are executed in program order: the order of a chain is the order of
// the list without a single workgroup barrier and without a floating-point atomic.  The first sim of a row is stored, not added
// to a zero ("no neighbour read it" is not "score 0"); the bits are set with an integer ds_or.
#pragma once
#include <math.h>

#include "ebn_common.h"

namespace {

#ifndef EBN_KNT_R
#define EBN_KNT_R 8192                  // -DEBN_KNT_R=...: the probe's alternatives (tools/knn_topn_probe.py)
#endif
constexpr int KNT_R = EBN_KNT_R;        // catalogue rows of one range = four wave tiles
constexpr int KNT_THREADS = 256, KNT_WAVES = 4;
constexpr int KNT_WR = KNT_R / KNT_WAVES;      // rows of one wave's tile
constexpr int KNT_WWORDS = KNT_WR / 32;        // words of one bit-per-row mask of a wave
static_assert(KNT_R % 1024 == 0 && KNT_R >= 1024 && KNT_R <= 8192, "whole mask words per wave; tiles, masks and staging inside 64 KiB of LDS");
constexpr int KNT_MAX_SPLITS = 64;
constexpr int KNT_NBR = EBN_KNN_MAX_K;         // staged neighbour slots
// tiles [4][KNT_WR] | masks [4][touched KNT_WWORDS | excluded KNT_WWORDS] | set begin [512] | set end [512] | sim [512]; a kernel's own follows
#ifdef EBN_KNT_SHARED                   // the probe's other form: one workgroup-shared tile, a barrier between neighbours
constexpr int KNT_CUT_FLOATS = 2 * KNT_NBR;    // segment begin [512] | segment end [512] of the range in hand
#else
constexpr int KNT_CUT_FLOATS = 0;
#endif
constexpr int KNT_TILE_FLOATS = KNT_R + 2 * KNT_WAVES * KNT_WWORDS + 3 * KNT_NBR + KNT_CUT_FLOATS;

struct KnnTileArgs {
  const int64_t* s_indptr;
  const int32_t* s_items;
  const float* item_scale;
  const int32_t* nbr_seq;
  const float* nbr_sim;
  const int32_t* user_hist;
  const int32_t* cand_pos;
  const int32_t* window;
  const int32_t* exclude;
  int32_t* flags;
  int64_t n_seqs, nnz_s, n_rows, n_hists, M, U;
  int32_t k_nbr, X, n_splits, ranges_per_split;
};

struct KnnTile {
  float* tile;         // this wave's [KNT_WR]
  unsigned* touched;   // this wave's [KNT_WWORDS]
  unsigned* excluded;  // this wave's [KNT_WWORDS], right behind touched
  int32_t* nb_lo;      // [KNT_NBR] the staged neighbour row, shared by the waves
  int32_t* nb_hi;
  float* nb_sim;
  float* own;
};

__device__ __forceinline__ KnnTile knt_tile(float* smem, int wave) {
  KnnTile t;
  t.tile = smem + wave * KNT_WR;
  t.touched = reinterpret_cast<unsigned*>(smem + KNT_R) + wave * 2 * KNT_WWORDS;
  t.excluded = t.touched + KNT_WWORDS;
  t.nb_lo = reinterpret_cast<int32_t*>(smem + KNT_R + 2 * KNT_WAVES * KNT_WWORDS);
  t.nb_hi = t.nb_lo + KNT_NBR;
  t.nb_sim = reinterpret_cast<float*>(t.nb_hi + KNT_NBR);
  t.own = smem + KNT_TILE_FLOATS;
  return t;
}

__device__ __forceinline__ int32_t knt_clamp(int64_t v, int64_t hi) { return static_cast<int32_t>(v < 0 ? 0 : (v > hi ? hi : v)); }

// one step of a chain: a single rounding
__device__ __forceinline__ float knt_step(float acc, float sim) { return __fadd_rn(acc, sim); }

// what closes a chain
__device__ __forceinline__ float knt_close(const KnnTileArgs& a, float acc, int64_t row) {
  return a.item_scale != nullptr ? __fmul_rn(acc, a.item_scale[row]) : acc;
}

// a wave's LDS operations are executed in order; this keeps the compiler from moving them across the point
__device__ __forceinline__ void knt_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the neighbour row of user u, or -1 for a user without one
__device__ __forceinline__ int64_t knt_history(const KnnTileArgs& a, int64_t u) {
  const int64_t h = a.user_hist != nullptr ? static_cast<int64_t>(a.user_hist[u]) : u;
  return (h >= 0 && h < a.n_hists) ? h : -1;
}

// Stages the neighbour row h (h < 0: nobody) as set extents inside [0, nnz_s] and sims; an absent neighbour is an empty set.  Every
// thread of the workgroup calls it; it ends with a barrier.  Returns whether any neighbour is present.
__device__ __forceinline__ bool knt_stage(const KnnTileArgs& a, const KnnTile& t, int64_t h, int tid) {
  bool any = false;
  for (int j = tid; j < a.k_nbr; j += KNT_THREADS) {
    int32_t lo = 0, hi = 0;
    float sim = 0.f;
    if (h >= 0) {
      const int64_t s = a.nbr_seq[h * a.k_nbr + j];
      if (s >= 0 && s < a.n_seqs) {
        any = true;
        lo = knt_clamp(a.s_indptr[s], a.nnz_s);
        hi = knt_clamp(a.s_indptr[s + 1], a.nnz_s);
        if (hi < lo) hi = lo;
        sim = a.nbr_sim[h * a.k_nbr + j];
      }
    }
    t.nb_lo[j] = lo;
    t.nb_hi[j] = hi;
    t.nb_sim[j] = sim;
  }
  return __syncthreads_or(any ? 1 : 0) != 0;
}

// the clamped window of user u: [0, M) without windows, [0, 0) for an empty one
__device__ __forceinline__ void knt_window(const KnnTileArgs& a, int64_t u, int& lo, int& hi) {
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

// first position in [lo, hi) whose row is at least key (hi if none; lo when lo >= hi)
__device__ __forceinline__ int32_t knt_lower_bound(const int32_t* __restrict__ items, int32_t lo, int32_t hi, int32_t key) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (items[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The ranges [g_beg, g_end) of split `split`
__device__ __forceinline__ void knt_span(const KnnTileArgs& a, int split, int64_t& g_beg, int64_t& g_end) {
  const int64_t n_ranges = (a.n_rows + KNT_R - 1) / KNT_R;
  g_beg = static_cast<int64_t>(split) * a.ranges_per_split;
  g_end = g_beg + a.ranges_per_split;
  g_end = g_end < n_ranges ? g_end : n_ranges;
}

// Fills THIS WAVE's tile for the rows [r0, r1) (0 < r1 - r0 <= KNT_WR) from the staged neighbour row, and the excluded bits.  The 64
// lanes of the wave call it with the same arguments; no workgroup barrier inside.
__device__ __forceinline__ void knt_accumulate(const KnnTileArgs& a, const KnnTile& t, int64_t u, int32_t r0, int32_t r1, int lane) {
  knt_wave_sync();  // the wave is done with its previous tile
  for (int i = lane; i < 2 * KNT_WWORDS; i += 64) t.touched[i] = 0u;  // touched | excluded
  knt_wave_sync();
  const unsigned n = static_cast<unsigned>(r1 - r0);
  for (int jb = 0; jb < a.k_nbr; jb += 64) {
    const int j = jb + lane;
    int32_t sb = 0, se = 0, first = 0;
    float sim = 0.f;
    if (j < a.k_nbr) {
      const int32_t lo = t.nb_lo[j], hi = t.nb_hi[j];
      if (hi > lo) {  // the cut of this lane's set to the tile
        sb = knt_lower_bound(a.s_items, lo, hi, r0);
        se = knt_lower_bound(a.s_items, sb, hi, r1);
        if (se > sb) {
          first = a.s_items[sb];  // most segments are one row long: it is here before the neighbour's turn
          sim = t.nb_sim[j];
        }
      }
    }
    unsigned long long m = __ballot(se > sb);
    while (m != 0ull) {  // the neighbours with a segment, in list order
      const int src = __builtin_ctzll(m);
      m &= m - 1ull;
      const int32_t b = __shfl(sb, src, 64), e = __shfl(se, src, 64), f = __shfl(first, src, 64);
      const float w = __shfl(sim, src, 64);
      for (int32_t i = b + lane; i < e; i += 64) {
        const unsigned c = static_cast<unsigned>((i == b ? f : a.s_items[i]) - r0);
        if (c >= n) continue;  // rows that do not ascend: never an LDS address outside the tile
        const unsigned bit = 1u << (c & 31u);
        if (t.touched[c >> 5] & bit) {
          t.tile[c] = knt_step(t.tile[c], w);
        } else {
          t.tile[c] = w;
          atomicOr(&t.touched[c >> 5], bit);
        }
      }
      knt_wave_sync();  // the next neighbour finds this one's sums: the order of a chain is the order of the list
    }
  }
  for (int x = lane; x < a.X; x += 64) {
    const int64_t row = a.exclude[u * a.X + x];
    if (row >= r0 && row < r1) atomicOr(&t.excluded[(row - r0) >> 5], 1u << ((row - r0) & 31));
  }
  knt_wave_sync();
}

// this wave's rows of range g: [r0, r1), empty past the catalogue's end
__device__ __forceinline__ bool knt_wave_rows(const KnnTileArgs& a, int64_t g, int wave, int32_t& r0, int32_t& r1) {
  const int64_t b = g * KNT_R + static_cast<int64_t>(wave) * KNT_WR;
  if (b >= a.n_rows) return false;
  r0 = static_cast<int32_t>(b);
  r1 = static_cast<int32_t>(a.n_rows - b < KNT_WR ? a.n_rows : b + KNT_WR);
  return true;
}

#ifdef EBN_KNT_SHARED
// The other form, kept for the probe: the four wave tiles are ONE tile of KNT_R rows that the 256 threads fill together -- one thread
// per neighbour cuts its set to the range, then the neighbours with a segment follow one another with a barrier in between (the
// device of ebn_covisit_tile.h).  Row c of the range lives in wave c / KNT_WR's tile and masks, so the scan is the same.  The same bits.
__device__ __forceinline__ void knt_accumulate_shared(const KnnTileArgs& a, const KnnTile& t, float* smem, int64_t u, int32_t r0, int32_t r1,
                                                      int tid) {
  float* tile = smem;
  unsigned* masks = reinterpret_cast<unsigned*>(smem + KNT_R);
  int32_t* cut_b = reinterpret_cast<int32_t*>(t.nb_sim + KNT_NBR);
  int32_t* cut_e = cut_b + KNT_NBR;
  __syncthreads();  // everybody is done with the previous range
  for (int i = tid; i < 2 * KNT_WAVES * KNT_WWORDS; i += KNT_THREADS) masks[i] = 0u;
  for (int j = tid; j < a.k_nbr; j += KNT_THREADS) {
    const int32_t lo = t.nb_lo[j], hi = t.nb_hi[j];
    int32_t sb = 0, se = 0;
    if (hi > lo) {
      sb = knt_lower_bound(a.s_items, lo, hi, r0);
      se = knt_lower_bound(a.s_items, sb, hi, r1);
    }
    cut_b[j] = sb;
    cut_e[j] = se;
  }
  __syncthreads();
  const unsigned n = static_cast<unsigned>(r1 - r0);
  for (int j = 0; j < a.k_nbr; ++j) {
    const int32_t b = cut_b[j], e = cut_e[j];
    if (e <= b) continue;  // the same for every thread: no barrier is skipped by a part
    const float w = t.nb_sim[j];
    for (int32_t i = b + tid; i < e; i += KNT_THREADS) {
      const unsigned c = static_cast<unsigned>(a.s_items[i] - r0);
      if (c >= n) continue;
      unsigned* word = masks + (c / KNT_WR) * 2 * KNT_WWORDS + ((c % KNT_WR) >> 5);
      const unsigned bit = 1u << (c & 31u);
      if (*word & bit) {
        tile[c] = knt_step(tile[c], w);
      } else {
        tile[c] = w;
        atomicOr(word, bit);
      }
    }
    __syncthreads();
  }
  for (int x = tid; x < a.X; x += KNT_THREADS) {
    const int64_t row = a.exclude[u * a.X + x];
    if (row >= r0 && row < r1) {
      const unsigned c = static_cast<unsigned>(row - r0);
      atomicOr(masks + (c / KNT_WR) * 2 * KNT_WWORDS + KNT_WWORDS + ((c % KNT_WR) >> 5), 1u << (c & 31u));
    }
  }
  __syncthreads();
}
#endif

// Range g for this wave: fills its tile, false when the wave has no row of the range.  Every thread of the workgroup calls it for
// every range of the split (the shared form has barriers inside).
__device__ __forceinline__ bool knt_fill_range(const KnnTileArgs& a, const KnnTile& t, float* smem, int64_t u, int64_t g, int tid, int32_t& r0,
                                               int32_t& r1) {
#ifdef EBN_KNT_SHARED
  const int32_t g0 = static_cast<int32_t>(g * KNT_R);
  knt_accumulate_shared(a, t, smem, u, g0, static_cast<int32_t>(a.n_rows - g0 < KNT_R ? a.n_rows : g0 + KNT_R), tid);
  return knt_wave_rows(a, g, tid >> 6, r0, r1);
#else
  if (!knt_wave_rows(a, g, tid >> 6, r0, r1)) return false;
  knt_accumulate(a, t, u, r0, r1, tid & 63);
  return true;
#endif
}

// Row r0 + c of this wave's tile (its touched bit is set) for a user with the clamped window [wlo, whi): admissible -> its
// position and score.  A position >= M raises oob, a NaN score of a row that is admissible otherwise raises nan
__device__ __forceinline__ bool knt_admissible(const KnnTileArgs& a, const KnnTile& t, int32_t r0, int c, int wlo, int whi, int& pos, float& s,
                                               bool& oob, bool& nan) {
  const int64_t row = static_cast<int64_t>(r0) + c;
  const int64_t p = a.cand_pos != nullptr ? static_cast<int64_t>(a.cand_pos[row]) : row;
  if (p < 0) return false;
  if (p >= a.M) {
    oob = true;
    return false;
  }
  if (p < wlo || p >= whi) return false;
  if ((t.excluded[c >> 5] >> (c & 31)) & 1u) return false;
  const float v = knt_close(a, t.tile[c], row);
  if (v != v) {
    nan = true;
    return false;
  }
  pos = static_cast<int>(p);
  s = v;
  return true;
}

// ---- host.  n_splits ranges divide the ceil(n_rows / KNT_R) ranges of a user.  Automatic: about 2 048 workgroups when the users
// alone do not give them -- not co-visitation's 16 384: a workgroup here first stages up to 512 neighbours (two loads of s_indptr
// each) and ends with a merge, and its ranges are cheap, so many short workgroups cost more than they balance (measured at knn-c1
// with 1 024 users: 1 / 2 / 4 / 16 splits).  U, n_rows >= 1
constexpr int KNT_AUTO_WORKGROUPS = 2048;
inline int knt_resolve_splits(int64_t U, int64_t n_rows, int32_t n_splits) {
  const int64_t ranges = ebn_ceil_div(n_rows, KNT_R);
  int64_t s = n_splits > 0 ? n_splits : ebn_ceil_div(KNT_AUTO_WORKGROUPS, U);
  if (s > ranges) s = ranges;
  if (s > KNT_MAX_SPLITS) s = KNT_MAX_SPLITS;
  return static_cast<int>(s < 1 ? 1 : s);
}

}  // namespace
