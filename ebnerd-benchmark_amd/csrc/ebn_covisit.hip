// Co-visitation baseline (item-to-item collaborative filtering; contract in include/ebnerd_hip.h): the pair keys a sparse item-item
// count matrix is built from, and the scores of ragged candidate lists against ragged click histories through that matrix (CSR).
//   * PAIR KEYS: one lane per sequence entry, 256-entry workgroups.  The workgroup finds the sequence of its first entry with ONE
//     upper_bound over seq_offsets (uniform: the scalar unit) and stages the next CV_T boundaries in LDS, a lane finds its own
//     sequence with an 8-step search of that tile and goes on to a search of the rest of seq_offsets only when the tile holds more
//     than CV_T boundaries (a run of empty sequences) -- wc_counts_kernel's search.  Every lane leaves its sequence's end (relative
//     to the tile, 0 for an entry without a sequence) and the workgroup the rows of its 256 + G entries in LDS; the 256 K slots of
//     the tile are then written in slot order, thread t the slots t, t + 256, ...: consecutive 8-byte stores, however long K is.
//   * SCORES: 256-item workgroups.  Phase 1, one lane per item: the item's list (the same search), its history's extent and its
//     matrix row's extent -- clamped to [0, n_hist_items] and [0, nnz], so 32-bit from here on -- go to LDS; an unknown candidate or
//     history leaves an empty extent.  Phase 2, one WAVE per item (CV_GW = 64), 4 items per round, 64 rounds: round r takes the
//     items 4 r .. 4 r + 3, one per wave, so the workgroup's waves work on neighbours (mostly one list, one history: the history
//     loads hit in cache).  Lane s takes the history entries s, s + 64, ... in order; for each present one it binary-searches the
//     entry's row among the columns of the candidate's matrix row and leaves at a hit (the columns are strictly ascending: no
//     second read of cols).  All lanes of a wave search ONE row: they walk the same search tree, whose upper levels are one
//     cached line per load instruction.  A 6-step butterfly (xor 32 .. 1) adds or maximises the lanes' partials: the order is
//     fixed, two runs give the same bits.  The scores of the tile leave through LDS in one coalesced store.
//     Why a wave and not a fraction of one, although histories of 5 to 50 entries leave more than half of its lanes idle: measured
//     at cv-c1 16 lanes per item take 13.3 ms, 32 take 11.8 ms, the wave 11.1 ms.  The kernel is bound by the
//     dependent loads of the searches (about log2(row length) per present entry), not by lanes or bandwidth, and a load whose
//     lanes search four different rows touches four times the cache lines of one whose lanes share the tree.  It wants many
//     waves in flight: 26 registers, 7 KiB of LDS.
//   * no atomics, no workspace.
#include "ebn_common.h"

#define CV_T 256   // entries / items of a workgroup = staged boundaries
#define CV_GW 64   // lanes of one item in the scores kernel (a wave): CV_T / CV_GW = 4 items per round

static_assert(EBN_CV_MAX_GAP >= 1 && EBN_CV_MAX_GAP <= 64, "the pair-key kernel stages CV_T + 64 rows");
static_assert(CV_T % CV_GW == 0 && EBN_WAVE % CV_GW == 0, "whole groups per wave and per workgroup");

// first position in [lo, hi) whose value is above key (hi if none)
static __device__ __forceinline__ int64_t cv_upper_bound(const int64_t* __restrict__ v, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The list (sequence) of element i = i0 + threadIdx.x among offsets [n + 1]: #{ k in [0, n] : offsets[k] <= i } - 1, in [-1, n].
// Every thread of the workgroup calls it (a barrier inside); s_bound [CV_T] is scratch.
static __device__ __forceinline__ int64_t cv_list_of(const int64_t* __restrict__ offsets, int64_t n, int64_t i0, int64_t* s_bound) {
  const int t = threadIdx.x;
  const int64_t i = i0 + t;
  const int64_t base = cv_upper_bound(offsets, 0, n + 1, i0);
  const int64_t k = base + t;
  s_bound[t] = k <= n ? offsets[k] : INT64_MAX;
  __syncthreads();
  int c = 0;
#pragma unroll
  for (int step = CV_T / 2; step > 0; step >>= 1) c += s_bound[c + step - 1] <= i ? step : 0;  // #{ staged <= i } in [0, CV_T - 1]
  c += s_bound[c] <= i ? 1 : 0;
  int64_t l = base + c;
  if (c == CV_T && l <= n) l = cv_upper_bound(offsets, l, n + 1, i);  // more than CV_T boundaries inside the tile
  return l - 1;
}

static __device__ __forceinline__ int64_t cv_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- pair keys -----------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(CV_T) void cv_pair_keys_kernel(const int32_t* __restrict__ seq_rows,
                                                                   const int64_t* __restrict__ seq_offsets, int64_t n_seqs,
                                                                   int64_t n_entries, int64_t n_rows, int G, int K,
                                                                   int64_t* __restrict__ keys) {
  __shared__ int64_t s_bound[CV_T];
  __shared__ int32_t s_end[CV_T];                   // the end of the entry's sequence, relative to i0, at most CV_T + G; 0: none
  __shared__ int32_t s_row[CV_T + EBN_CV_MAX_GAP];  // rows of the entries i0 .. i0 + CV_T + G - 1 (-1 past n_entries)
  const int t = threadIdx.x;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * CV_T, i = i0 + t;
  const int64_t s = cv_list_of(seq_offsets, n_seqs, i0, s_bound);
  int32_t end = 0;
  if (i < n_entries && s >= 0 && s < n_seqs) {  // s == n_seqs: at or past seq_offsets[n_seqs]
    const int64_t e = cv_clamp(seq_offsets[s + 1], n_entries) - i0;
    end = e > CV_T + G ? CV_T + G : static_cast<int32_t>(e);
  }
  s_end[t] = end;
  for (int k = t; k < CV_T + G; k += CV_T) s_row[k] = i0 + k < n_entries ? seq_rows[i0 + k] : -1;
  __syncthreads();
  const int64_t left = n_entries - i0;
  const unsigned n_slots = static_cast<unsigned>(left < CV_T ? left : CV_T) * static_cast<unsigned>(K);
  int64_t* __restrict__ out = keys + i0 * K;
  for (unsigned q = t; q < n_slots; q += CV_T) {
    const unsigned e = q / static_cast<unsigned>(K), k = q - e * static_cast<unsigned>(K);
    const bool mirrored = k >= static_cast<unsigned>(G);
    const unsigned j = e + (mirrored ? k - G : k) + 1;
    int64_t key = EBN_CV_NO_PAIR;
    if (static_cast<int32_t>(j) < s_end[e]) {
      const int64_t ri = s_row[e], rj = s_row[j];
      if (ri >= 0 && ri < n_rows && rj >= 0 && rj < n_rows && ri != rj) key = mirrored ? ri * n_rows + rj : rj * n_rows + ri;
    }
    out[q] = key;
  }
}

extern "C" int ebn_cv_pair_keys_i64(const int32_t* seq_rows, const int64_t* seq_offsets, int64_t n_seqs, int64_t n_entries, int64_t n_rows,
                                    int32_t max_gap, int32_t symmetric, int64_t* keys, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_seqs, n_entries, n_rows) && max_gap >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_entries == 0 || (seq_rows != nullptr && seq_offsets != nullptr && keys != nullptr), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_entries == 0 || n_seqs >= 1, EBN_ERR_BAD_ARG);  // an entry belongs to a sequence
  EBN_REQUIRE(max_gap <= EBN_CV_MAX_GAP, EBN_ERR_UNSUPPORTED);
  if (n_entries == 0) return EBN_OK;
  const int G = static_cast<int>(max_gap), K = symmetric ? 2 * G : G;
  EBN_LAUNCH(cv_pair_keys_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(n_entries, CV_T))), dim3(CV_T), 0, ebn_stream(stream), seq_rows,
             seq_offsets, n_seqs, n_entries, n_rows, G, K, keys);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

// ---- scores --------------------------------------------------------------------------------------------------------------------
template <bool MAX>
static __global__ __launch_bounds__(CV_T) void cv_scores_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ cols,
                                                                const float* __restrict__ vals, int64_t n_rows, int64_t nnz,
                                                                const int32_t* __restrict__ hist_rows,
                                                                const float* __restrict__ hist_weights,
                                                                const int64_t* __restrict__ hist_offsets, int64_t n_hists,
                                                                int64_t n_hist_items, const int32_t* __restrict__ list_hist,
                                                                const int32_t* __restrict__ cand_rows,
                                                                const int64_t* __restrict__ cand_offsets, int64_t n_lists,
                                                                int64_t n_cand_items, float* __restrict__ scores) {
  __shared__ int64_t s_bound[CV_T];
  __shared__ int32_t s_hb[CV_T], s_he[CV_T], s_lo[CV_T], s_hi[CV_T];  // the item's history entries and matrix-row positions
  __shared__ float s_score[CV_T];
  const int t = threadIdx.x;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * CV_T, i = i0 + t;
  // ---- phase 1: one lane per item
  int64_t l = cv_list_of(cand_offsets, n_lists, i0, s_bound);
  l = l < 0 ? 0 : (l >= n_lists ? n_lists - 1 : l);  // cand_offsets[n_lists] >= n_cand_items > i by contract; never an address past list_hist
  int32_t hb = 0, he = 0, lo = 0, hi = 0;
  if (i < n_cand_items) {
    const int64_t u = list_hist != nullptr ? static_cast<int64_t>(list_hist[l]) : l;
    const int64_t c = cand_rows[i];
    if (u >= 0 && u < n_hists && c >= 0 && c < n_rows) {
      hb = static_cast<int32_t>(cv_clamp(hist_offsets[u], n_hist_items));
      he = static_cast<int32_t>(cv_clamp(hist_offsets[u + 1], n_hist_items));
      lo = static_cast<int32_t>(cv_clamp(indptr[c], nnz));
      hi = static_cast<int32_t>(cv_clamp(indptr[c + 1], nnz));
    }
  }
  s_hb[t] = hb;
  s_he[t] = he;
  s_lo[t] = lo;
  s_hi[t] = hi;
  __syncthreads();
  // ---- phase 2: CV_GW lanes per item
  const int sub = t & (CV_GW - 1), grp = t / CV_GW;
  const int32_t rows = static_cast<int32_t>(n_rows);  // <= EBN_DIM_MAX
  const int64_t left = n_cand_items - i0;
  const int n_live = left < CV_T ? static_cast<int>(left) : CV_T;
#pragma unroll 1
  for (int r0 = 0; r0 < n_live; r0 += CV_T / CV_GW) {
    const int it = r0 + grp;
    const uint32_t end = static_cast<uint32_t>(s_he[it]);
    const int32_t lo0 = s_lo[it], hi0 = s_hi[it];
    float acc = MAX ? -INFINITY : 0.0f;
    for (uint32_t j = static_cast<uint32_t>(s_hb[it] + sub); j < end; j += CV_GW) {  // end <= 2^31 - 1: unsigned j + 64 does not wrap
      const int32_t h = hist_rows[j];
      if (h >= 0 && h < rows) {
        const float w = hist_weights != nullptr ? hist_weights[j] : 1.0f;
        int32_t a = lo0, b = hi0, pos = -1;
        while (a < b) {
          const int32_t mid = a + ((b - a) >> 1);
          const int32_t v = cols[mid];
          if (v == h) {
            pos = mid;
            break;
          }
          if (v < h) a = mid + 1; else b = mid;
        }
        const float p = w * (pos >= 0 ? vals[pos] : 0.0f);
        acc = MAX ? fmaxf(acc, p) : acc + p;
      }
    }
#pragma unroll
    for (int off = CV_GW / 2; off > 0; off >>= 1) {
      const float o = __shfl_xor(acc, off, EBN_WAVE);
      acc = MAX ? fmaxf(acc, o) : acc + o;
    }
    if (sub == 0) s_score[it] = (MAX && !(acc > -INFINITY)) ? 0.0f : acc;  // -inf: no present entry
  }
  __syncthreads();
  if (i < n_cand_items) scores[i] = s_score[t];
}

extern "C" int ebn_cv_scores_f32(const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int64_t nnz,
                                 const int32_t* hist_rows, const float* hist_weights, const int64_t* hist_offsets, int64_t n_hists,
                                 int64_t n_hist_items, const int32_t* list_hist, const int32_t* cand_rows, const int64_t* cand_offsets,
                                 int64_t n_lists, int64_t n_cand_items, int32_t mode, float* scores, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_rows, nnz, n_hists, n_hist_items) && ebn_dim_ok(n_lists, n_cand_items) && (mode == 0 || mode == 1),
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE((n_cand_items == 0 || n_lists >= 1) && (n_hist_items == 0 || n_hists >= 1), EBN_ERR_BAD_ARG);
  if (n_cand_items == 0) return EBN_OK;
  EBN_REQUIRE(cand_rows != nullptr && cand_offsets != nullptr && scores != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE((n_rows == 0 || indptr != nullptr) && (nnz == 0 || (cols != nullptr && vals != nullptr)) &&
                  (n_hists == 0 || hist_offsets != nullptr) && (n_hist_items == 0 || hist_rows != nullptr),
              EBN_ERR_BAD_ARG);
  const dim3 grid(static_cast<unsigned>(ebn_ceil_div(n_cand_items, CV_T))), block(CV_T);
  if (mode == 1)
    EBN_LAUNCH(cv_scores_kernel<true>, grid, block, 0, ebn_stream(stream), indptr, cols, vals, n_rows, nnz, hist_rows, hist_weights,
               hist_offsets, n_hists, n_hist_items, list_hist, cand_rows, cand_offsets, n_lists, n_cand_items, scores);
  else
    EBN_LAUNCH(cv_scores_kernel<false>, grid, block, 0, ebn_stream(stream), indptr, cols, vals, n_rows, nnz, hist_rows, hist_weights,
               hist_offsets, n_hists, n_hist_items, list_hist, cand_rows, cand_offsets, n_lists, n_cand_items, scores);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
