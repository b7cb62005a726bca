// History-kNN baseline (S-KNN / V-SKNN, Jannach & Ludewig 2017; contract in include/ebnerd_hip.h): "find the readers whose click
// sequences look most like this one, and recommend what they read" -- the neighbour search over an inverted index of the training
// sequences and the scores of ragged candidate lists through the neighbours' item sets.
//   * NEIGHBOURS: one 256-thread workgroup per history.  A candidate always lies among the last sample_size + 1 entries of every
//     posting row that holds it (the header has the argument), so only those TAILS are read and the similarities are exact.  The
//     sequence ids are walked in ranges of KNN_R from the most recent downwards: an LDS tile holds one fp32 sum and one touched
//     bit per id of the range.  Per range
//       - stage (once when the history fits one chunk of 256 entries): thread e takes history entry e, decides whether it is the
//         LAST occurrence of a present row (a scan over the later entries: the chunk's through LDS) and leaves row, weight and
//         the tail's extent in LDS;
//       - search: thread e cuts the tail of its entry to the range -- two binary searches at most, none where the tail's end
//         lies below the range's top (always after the first range of a one-chunk history: what a range took is cut off) or its
//         begin inside the range; all entries in parallel, not one after the other -- and offers the largest id BELOW the
//         range to an LDS maximum: the next range starts right there, so ranges without a single posting are never visited;
//       - accumulate: the live entries in history order; the threads stride over the segment, set the id's bit (an integer LDS
//         atomic: no order in it) and assign (first touch) or add (later ones) the weight.  Ids within one posting row are
//         distinct, so plain read-add-write is enough; one barrier between two entries with a segment;
//       - count: thread t owns word t of the bits; a suffix sum from the top (wave shuffles + 4 wave totals) gives every set bit
//         its place among the candidates, and the ones inside the quota leave as (sum * seq_scale, id) pairs.  hist_self's bit is
//         cleared first.  The walk stops when sample_size candidates are taken or no tail holds a smaller id.
//     The at most 4096 pairs are padded to a power of two and sorted by a bitonic network in LDS under the total order (sim
//     descending, id descending); the first k leave.  Every sum has one fixed order (history order), there is no floating-point
//     atomic: two runs give the same bits, and the numpy twin knn_neighbours_host gives them too.
//     LDS: 4 KNN_R + KNN_R / 8 for the tile, 8 P for the pairs (P = sample_size rounded up to a power of two), 6 KiB of staging:
//     47 KiB at sample_size 1000 (three workgroups per CU), 71 KiB at 4096 (two).
//   * SCORES: ebn_cv_scores_f32's staging.  256-item workgroups; one lane per item finds its list and history; then one wave per
//     item: lane s takes the neighbours s, s + 64, ..., binary-searches the candidate's row in the neighbour's set and adds the
//     neighbour's sim at a hit; a butterfly (xor 32 .. 1) folds the lanes, one multiply by item_scale closes.  Fixed order, no
//     atomics, no workspace.
#include "ebn_common.h"

#define KNN_T 256                   // threads of a workgroup = history entries of a chunk = items of a score workgroup
#define KNN_R 8192                  // sequence ids of one range: one touched word per thread
#define KNN_GW 64                   // lanes of one item in the scores kernel (a wave)

static_assert(KNN_R == 32 * KNN_T, "the count phase gives every thread one word of touched bits");
static_assert(EBN_KNN_MAX_K <= EBN_KNN_MAX_SAMPLE && (EBN_KNN_MAX_SAMPLE & (EBN_KNN_MAX_SAMPLE - 1)) == 0, "pairs are padded to a power of two");
static_assert(KNN_T % KNN_GW == 0 && EBN_WAVE == KNN_GW, "one wave per item");

static __device__ __forceinline__ int64_t knn_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// first position in [lo, hi) whose value is not below key (hi if none)
static __device__ __forceinline__ int32_t knn_lower_bound(const int32_t* __restrict__ v, int32_t lo, int32_t hi, int32_t key) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// (sa, ia) ranks before (sb, ib): sim descending, then id descending (the more recent sequence first)
static __device__ __forceinline__ bool knn_before(float sa, int32_t ia, float sb, int32_t ib) { return sa > sb || (sa == sb && ia > ib); }

static inline int knn_pairs(int32_t sample_size) {
  int p = 1;
  while (p < sample_size) p <<= 1;
  return p;
}
// tile | touched bits | pair sims | pair ids | staging (row, weight, tail begin, tail end, segment begin, segment end) | 8 words
static inline size_t knn_lds_bytes(int32_t sample_size) {
  return static_cast<size_t>(KNN_R) * 4 + KNN_R / 8 + static_cast<size_t>(knn_pairs(sample_size)) * 8 + 6 * KNN_T * 4 + 32;
}

// ---- neighbours ----------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(KNN_T) void knn_neighbours_kernel(
    const int64_t* __restrict__ p_indptr, const int32_t* __restrict__ p_seqs, int64_t n_rows, int64_t nnz_p, int64_t n_seqs,
    const float* __restrict__ seq_scale, const int32_t* __restrict__ hist_rows, const float* __restrict__ hist_weights,
    const int64_t* __restrict__ hist_offsets, int64_t n_hist_items, const int32_t* __restrict__ hist_self, int S, int P, int k,
    int32_t* __restrict__ out_seq, float* __restrict__ out_sim) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_sum = smem;                                                  // [KNN_R]
  unsigned* s_bits = reinterpret_cast<unsigned*>(s_sum + KNN_R);        // [KNN_T]
  float* c_sim = reinterpret_cast<float*>(s_bits + KNN_T);              // [P]
  int32_t* c_id = reinterpret_cast<int32_t*>(c_sim + P);                // [P]
  int32_t* e_row = c_id + P;                                            // [KNN_T] -1: the entry is not live
  float* e_w = reinterpret_cast<float*>(e_row + KNN_T);                 // [KNN_T]
  int32_t* e_ta = reinterpret_cast<int32_t*>(e_w + KNN_T);              // [KNN_T] the tail of the entry's posting row
  int32_t* e_tb = e_ta + KNN_T;
  int32_t* e_lo = e_tb + KNN_T;                                         // [KNN_T] its part inside the range
  int32_t* e_hi = e_lo + KNN_T;
  int32_t* s_misc = e_hi + KNN_T;                                       // [0 .. 3]: wave totals, [4]: the largest id below the range

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t u = blockIdx.x;
  const int32_t hb = static_cast<int32_t>(knn_clamp(hist_offsets[u], n_hist_items));
  const int32_t he = static_cast<int32_t>(knn_clamp(hist_offsets[u + 1], n_hist_items));
  const int32_t self = hist_self != nullptr ? hist_self[u] : -1;
  const int32_t rows = static_cast<int32_t>(n_rows), nnz = static_cast<int32_t>(nnz_p);  // <= EBN_DIM_MAX
  const bool one_chunk = he - hb <= KNN_T;

  int taken = 0;
  int32_t top = static_cast<int32_t>(n_seqs);  // the range is [r0, top)
  bool staged = false;
  while (he > hb && top > 0) {
    const int32_t r0 = top > KNN_R ? top - KNN_R : 0;
    s_bits[tid] = 0u;
    if (tid == 0) s_misc[4] = -1;
    for (int32_t c0 = hb; c0 < he; c0 += KNN_T) {
      __syncthreads();  // the bits are zero; the last chunk's staging has been read
      const int32_t j = c0 + tid;
      const int n_e = he - c0 < KNN_T ? he - c0 : KNN_T;
      if (!(one_chunk && staged)) {
        const int32_t r = j < he ? hist_rows[j] : -1;
        e_lo[tid] = r;  // the chunk's rows, for the scan below (e_lo is written for good after it)
        __syncthreads();
        int32_t row = -1, ta = 0, tb = 0;
        float w = 1.0f;
        if (r >= 0 && r < rows) {
          bool last = true;
          for (int q = tid + 1; q < n_e; ++q) last = last && e_lo[q] != r;
          for (int32_t q = c0 + KNN_T; q < he; ++q) last = last && hist_rows[q] != r;  // the chunks behind this one
          if (last) {
            row = r;
            if (hist_weights != nullptr) w = hist_weights[j];
            const int32_t a = static_cast<int32_t>(knn_clamp(p_indptr[r], nnz));
            tb = static_cast<int32_t>(knn_clamp(p_indptr[r + 1], nnz));
            ta = tb - a > S + 1 ? tb - (S + 1) : a;  // tb < a: an empty tail
          }
        }
        e_row[tid] = row;
        e_w[tid] = w;
        e_ta[tid] = ta;
        e_tb[tid] = tb;
        __syncthreads();  // everyone is done with the rows in e_lo
      }
      {
        int32_t lo = 0, hi = 0;
        const int32_t ta = e_ta[tid], tb = e_tb[tid];  // this thread's own staging: no barrier in between
        if (e_row[tid] >= 0 && tb > ta) {
          // ranges descend: what is left of a tail usually ends below `top` (always once e_tb is kept) and often begins inside the range
          hi = p_seqs[tb - 1] < top ? tb : knn_lower_bound(p_seqs, ta, tb, top);
          lo = hi > ta && p_seqs[ta] >= r0 ? ta : knn_lower_bound(p_seqs, ta, hi, r0);
          if (lo > ta) atomicMax(&s_misc[4], p_seqs[lo - 1]);
          e_tb[tid] = lo;  // the ranges below need no more of it (kept as long as the staging is: one chunk)
        }
        e_lo[tid] = lo;
        e_hi[tid] = hi;
      }
      __syncthreads();
      for (int e = 0; e < n_e; ++e) {
        const int32_t lo = e_lo[e], hi = e_hi[e];
        if (hi <= lo) continue;  // uniform: nothing of this entry in the range, nothing to order
        const float w = e_w[e];
        for (int32_t p = lo + tid; p < hi; p += KNN_T) {
          const int32_t s = p_seqs[p];
          if (s >= r0 && s < top) {  // whatever p_seqs holds, the tile is addressed inside [0, KNN_R)
            const int idx = s - r0;
            const unsigned m = 1u << (idx & 31);
            const bool touched = (atomicOr(&s_bits[idx >> 5], m) & m) != 0u;
            s_sum[idx] = touched ? s_sum[idx] + w : w;
          }
        }
        __syncthreads();
      }
    }
    staged = true;
    __syncthreads();
    if (tid == 0 && self >= r0 && self < top) s_bits[(self - r0) >> 5] &= ~(1u << ((self - r0) & 31));
    __syncthreads();
    // ---- count from the top: thread t owns the ids r0 + 32 t .. r0 + 32 t + 31
    const unsigned word = s_bits[tid];
    const int cnt = __popc(word);
    int suf = cnt;  // the set bits of this wave's words tid' >= tid
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_down(suf, off, 64);
      if (lane + off < 64) suf += o;
    }
    if (lane == 0) s_misc[wave] = suf;
    __syncthreads();
    int above = suf - cnt, total = 0;
#pragma unroll
    for (int w = 0; w < KNN_T / 64; ++w) {
      const int c = s_misc[w];
      total += c;
      if (w > wave) above += c;
    }
    const int quota = S - taken;
    unsigned rest = word;
    for (int place = above; rest != 0u && place < quota; ++place) {
      const int b = 31 - __clz(rest);
      rest &= ~(1u << b);
      const int idx = 32 * tid + b;
      const int32_t s = r0 + idx;
      const float dot = s_sum[idx];
      c_sim[taken + place] = seq_scale != nullptr ? dot * seq_scale[s] : dot;
      c_id[taken + place] = s;
    }
    taken += total < quota ? total : quota;
    const int32_t next = s_misc[4];
    __syncthreads();  // everyone has read the totals and the maximum before the next range resets them
    if (taken >= S || next < 0) break;
    top = next + 1;
  }

  // ---- sort the pairs (padded to a power of two) and write the first k
  int n_sort = 1;
  while (n_sort < taken) n_sort <<= 1;
  for (int i = taken + tid; i < n_sort; i += KNN_T) {
    c_sim[i] = -INFINITY;
    c_id[i] = -1;
  }
  __syncthreads();
  for (int size = 2; size <= n_sort; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < n_sort; i += KNN_T) {
        const int o = i ^ stride;
        if (o > i) {
          const float sa = c_sim[i], sb = c_sim[o];
          const int32_t ia = c_id[i], ib = c_id[o];
          const bool best_first = (i & size) == 0;
          if (best_first ? knn_before(sb, ib, sa, ia) : knn_before(sa, ia, sb, ib)) {
            c_sim[i] = sb;
            c_id[i] = ib;
            c_sim[o] = sa;
            c_id[o] = ia;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < k; i += KNN_T) {
    out_seq[u * k + i] = i < taken ? c_id[i] : -1;
    out_sim[u * k + i] = i < taken ? c_sim[i] : -INFINITY;
  }
}

extern "C" int64_t ebn_knn_range(void) { return KNN_R; }

extern "C" int ebn_knn_neighbours_f32(const int64_t* p_indptr, const int32_t* p_seqs, int64_t n_rows, int64_t nnz_p, int64_t n_seqs,
                                      const float* seq_scale, const int32_t* hist_rows, const float* hist_weights,
                                      const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items, const int32_t* hist_self,
                                      int32_t sample_size, int32_t k, int32_t* out_seq, float* out_sim, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_rows, nnz_p, n_seqs, n_hists) && ebn_dim_ok(n_hist_items), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(sample_size >= 1 && k >= 1 && k <= sample_size, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_hist_items == 0 || n_hists >= 1, EBN_ERR_BAD_ARG);  // an entry belongs to a history
  EBN_REQUIRE(n_hists == 0 || (hist_offsets != nullptr && out_seq != nullptr && out_sim != nullptr), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_hists == 0 || ((n_rows == 0 || p_indptr != nullptr) && (nnz_p == 0 || p_seqs != nullptr) &&
                               (n_hist_items == 0 || hist_rows != nullptr)),
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE(k <= EBN_KNN_MAX_K && sample_size <= EBN_KNN_MAX_SAMPLE, EBN_ERR_UNSUPPORTED);
  if (n_hists == 0) return EBN_OK;
  const size_t lds = knn_lds_bytes(sample_size);
  // above the 64 KiB a kernel may use without asking (sample_size > 2048); set per call: the attribute belongs to the current device
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_neighbours_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(knn_lds_bytes(EBN_KNN_MAX_SAMPLE))) != hipSuccess) {
    (void)hipGetLastError();
    return EBN_ERR_UNSUPPORTED;
  }
  EBN_LAUNCH(knn_neighbours_kernel, dim3(static_cast<unsigned>(n_hists)), dim3(KNN_T), lds, ebn_stream(stream), p_indptr, p_seqs, n_rows,
             nnz_p, n_seqs, seq_scale, hist_rows, hist_weights, hist_offsets, n_hist_items, hist_self, static_cast<int>(sample_size),
             knn_pairs(sample_size), static_cast<int>(k), out_seq, out_sim);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

// ---- scores --------------------------------------------------------------------------------------------------------------------
// first position in [lo, hi) whose value is above key (hi if none)
static __device__ __forceinline__ int64_t knn_upper_bound(const int64_t* __restrict__ v, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The list of element i = i0 + threadIdx.x among offsets [n + 1]: #{ k in [0, n] : offsets[k] <= i } - 1, in [-1, n] (cv_list_of of
// ebn_covisit.hip: one uniform search per workgroup, KNN_T staged boundaries, a fallback search behind a run of empty lists).
static __device__ __forceinline__ int64_t knn_list_of(const int64_t* __restrict__ offsets, int64_t n, int64_t i0, int64_t* s_bound) {
  const int t = threadIdx.x;
  const int64_t i = i0 + t;
  const int64_t base = knn_upper_bound(offsets, 0, n + 1, i0);
  const int64_t q = base + t;
  s_bound[t] = q <= n ? offsets[q] : INT64_MAX;
  __syncthreads();
  int c = 0;
#pragma unroll
  for (int step = KNN_T / 2; step > 0; step >>= 1) c += s_bound[c + step - 1] <= i ? step : 0;
  c += s_bound[c] <= i ? 1 : 0;
  int64_t l = base + c;
  if (c == KNN_T && l <= n) l = knn_upper_bound(offsets, l, n + 1, i);
  return l - 1;
}

static __global__ __launch_bounds__(KNN_T) void knn_scores_kernel(const int64_t* __restrict__ s_indptr, const int32_t* __restrict__ s_items,
                                                                  int64_t n_seqs, int64_t nnz_s, int64_t n_rows,
                                                                  const float* __restrict__ item_scale, const int32_t* __restrict__ nbr_seq,
                                                                  const float* __restrict__ nbr_sim, int64_t n_hists, int k,
                                                                  const int32_t* __restrict__ list_hist, const int32_t* __restrict__ cand_rows,
                                                                  const int64_t* __restrict__ cand_offsets, int64_t n_lists,
                                                                  int64_t n_cand_items, float* __restrict__ scores) {
  __shared__ int64_t s_bound[KNN_T];
  __shared__ int32_t s_u[KNN_T], s_c[KNN_T];  // the item's history (-1: nothing to score) and row
  __shared__ float s_score[KNN_T];
  const int t = threadIdx.x;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * KNN_T, i = i0 + t;
  // ---- phase 1: one lane per item
  int64_t l = knn_list_of(cand_offsets, n_lists, i0, s_bound);
  l = l < 0 ? 0 : (l >= n_lists ? n_lists - 1 : l);  // never an address past list_hist
  int32_t hu = -1, hc = 0;
  if (i < n_cand_items) {
    const int64_t u = list_hist != nullptr ? static_cast<int64_t>(list_hist[l]) : l;
    const int64_t c = cand_rows[i];
    if (u >= 0 && u < n_hists && c >= 0 && c < n_rows) {
      hu = static_cast<int32_t>(u);
      hc = static_cast<int32_t>(c);
    }
  }
  s_u[t] = hu;
  s_c[t] = hc;
  __syncthreads();
  // ---- phase 2: one wave per item
  const int sub = t & (KNN_GW - 1), grp = t / KNN_GW;
  const int32_t seqs = static_cast<int32_t>(n_seqs), nnz = static_cast<int32_t>(nnz_s);
  const int64_t left = n_cand_items - i0;
  const int n_live = left < KNN_T ? static_cast<int>(left) : KNN_T;
#pragma unroll 1
  for (int r0 = 0; r0 < n_live; r0 += KNN_T / KNN_GW) {
    const int it = r0 + grp;  // items past n_live hold u = -1
    const int32_t u = s_u[it], c = s_c[it];
    float acc = 0.0f;
    bool any = false;
    if (u >= 0) {
      const int64_t base = static_cast<int64_t>(u) * k;
      for (int n = sub; n < k; n += KNN_GW) {
        const int32_t s = nbr_seq[base + n];
        if (s >= 0 && s < seqs) {
          any = true;
          int32_t a = static_cast<int32_t>(knn_clamp(s_indptr[s], nnz)), b = static_cast<int32_t>(knn_clamp(s_indptr[s + 1], nnz));
          bool hit = false;
          while (a < b) {
            const int32_t mid = a + ((b - a) >> 1);
            const int32_t v = s_items[mid];
            if (v == c) {
              hit = true;
              break;
            }
            if (v < c) a = mid + 1; else b = mid;
          }
          if (hit) acc += nbr_sim[base + n];
        }
      }
    }
#pragma unroll
    for (int off = KNN_GW / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, EBN_WAVE);
    const bool scored = __ballot(any) != 0ull;  // a history without neighbours: exact +0
    if (sub == 0) s_score[it] = scored ? (item_scale != nullptr ? item_scale[c] * acc : acc) : 0.0f;
  }
  __syncthreads();
  if (i < n_cand_items) scores[i] = s_score[t];
}

extern "C" int ebn_knn_scores_f32(const int64_t* s_indptr, const int32_t* s_items, int64_t n_seqs, int64_t nnz_s, int64_t n_rows,
                                  const float* item_scale, const int32_t* nbr_seq, const float* nbr_sim, int64_t n_hists, int32_t k,
                                  const int32_t* list_hist, const int32_t* cand_rows, const int64_t* cand_offsets, int64_t n_lists,
                                  int64_t n_cand_items, float* scores, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_seqs, nnz_s, n_rows, n_hists) && ebn_dim_ok(n_lists, n_cand_items) && k >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_cand_items == 0 || n_lists >= 1, EBN_ERR_BAD_ARG);  // an item belongs to a list
  EBN_REQUIRE(n_cand_items == 0 || (cand_rows != nullptr && cand_offsets != nullptr && scores != nullptr), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_cand_items == 0 || ((n_seqs == 0 || s_indptr != nullptr) && (nnz_s == 0 || s_items != nullptr) &&
                                    (n_hists == 0 || (nbr_seq != nullptr && nbr_sim != nullptr))),
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE(k <= EBN_KNN_MAX_K, EBN_ERR_UNSUPPORTED);
  if (n_cand_items == 0) return EBN_OK;
  EBN_LAUNCH(knn_scores_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(n_cand_items, KNN_T))), dim3(KNN_T), 0, ebn_stream(stream), s_indptr,
             s_items, n_seqs, nnz_s, n_rows, item_scale, nbr_seq, nbr_sim, n_hists, static_cast<int>(k), list_hist, cand_rows, cand_offsets,
             n_lists, n_cand_items, scores);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
