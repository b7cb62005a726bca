// EASE top-N lists and clicked-article ranks over the WHOLE catalogue (contract in include/ebnerd_hip.h): the second outlet of the
// EASE baseline, beside the in-view scores of ebn_ease.hip.
//
//   score(u, c) = sum_j w_j B[h_j, c] over the present entries of u's history, in history order
//
// ebn_ease_scores_f32 is one wave per (item, history) pair: right for 12 in-view items, hopeless for 16 384 columns per user.  B
// is dense and row-major, so a user's score row is the sum of a few CONTIGUOUS rows of B: a 256-thread workgroup per (user, split)
// walks ranges of EZK_R columns, every thread owns EZK_V groups of four adjacent columns of the range in registers (group v of
// thread t: columns v * 1024 + 4 t .. + 3; one group as built), and per history entry reads its 16 bytes of each group -- a wave
// reads 1 KiB of one row at a time -- with EZK_UNROLL rows' loads in flight.  No LDS tile, no barrier between history entries, no
// touched bits.
//   * the history is staged ONCE per workgroup: chunks of 256 entries are compacted in order (ballot prefix) to the present ones,
//     row and weight, in LDS.  A history of more than 256 entries is staged chunk by chunk inside every range; the accumulators
//     stay in registers across the chunk boundary, so the chain order holds.
//   * the chain (ezk_accumulate): the first present entry's product is STORED (-0.0 stays -0.0), every later one is added with
//     __fadd_rn to a product of __fmul_rn: no contraction.  The vector path (B 16-byte aligned, ldb % 4 == 0) and the scalar path
//     give a thread the same columns and the same operations, hence the same bits.
//   * ebn_ease_topk_f32: per group element a wave offers its 64 columns to ITS OWN sorted list of k <= 64 entries in registers
//     (topk_wave_offer, ebn_topk_list.h); the four lists are merged by wave 0 through 1.5 KiB of LDS, the lists of the splits by
//     topk_merge_kernel.
//   * ebn_ease_target_rank_f32: first the target column's own chain -- one thread per staged entry loads B[h_j, target] and forms
//     the product, thread 0 folds them in history order: the steps of ezk_accumulate, so t has the walk's bits -- then the same
//     walk with two integer counters per thread.
//   * exclusion: one bit per column of the range in LDS, set with an integer ds_or (-DEBN_EZK_EX_DIRECT: the probe's alternative,
//     a compare against the staged list per column).
// No floating-point atomics anywhere.  Bit-identical for every n_splits, from run to run and whoever shares the launch.
#include <math.h>

#include "ebn_topk_list.h"

namespace {

#ifndef EBN_EZK_V
#define EBN_EZK_V 1  // -DEBN_EZK_V=2 / 4: the probe's alternatives (tools/ease_topn_probe.py)
#endif
// one group per thread, a range of 1024 columns: measured at ease-c1 against 2 and 4 groups (2 groups take about
// 1.25 x the time, 4 groups about 2.1 x) -- fewer registers per thread leave more waves in flight to hide the latency of the row loads
constexpr int EZK_THREADS = 256;
constexpr int EZK_V = EBN_EZK_V;            // groups of four columns a thread owns
constexpr int EZK_STRIP = EZK_THREADS * 4;  // columns one group of every thread covers
constexpr int EZK_R = EZK_V * EZK_STRIP;    // columns of one range
constexpr int EZK_WORDS = EZK_R / 32;       // words of the excluded mask
constexpr int EZK_STAGE = 256;              // history entries of one staging chunk: one per thread
constexpr int EZK_UNROLL = 4;               // rows of B whose loads are in flight
constexpr int EZK_MAX_SPLITS = 64;
static_assert(EZK_V >= 1 && EZK_V <= 8, "the accumulators and EZK_UNROLL rows of operands stay in registers");
static_assert(EZK_STAGE == EZK_THREADS, "one staged entry per thread");
static_assert(TK_MAX_SPLITS == EZK_MAX_SPLITS, "the merge launch holds one split per lane");

struct EzkArgs {
  const float* B;
  const int32_t* hist_rows;
  const float* hist_weights;
  const int64_t* hist_offsets;
  const int32_t* user_hist;
  const int32_t* cand_pos;
  const int32_t* window;
  const int32_t* exclude;
  int32_t* flags;
  int64_t ldb, n_rows, n_hists, n_hist_items, M, U;
  int32_t X, n_splits, ranges_per_split;
};

struct EzkTopkArgs : EzkArgs {
  int32_t* out_pos;
  float* out_score;
  int32_t* part_pos;  // [n_splits, U, k] (n_splits > 1)
  float* part_score;
  int32_t k;
};

struct EzkRankArgs : EzkArgs {
  const int32_t* target_pos;
  int32_t* out_rank;
  int32_t* out_count;
  float* out_score;
  int32_t* part;              // [2, n_splits, U]: admissible, ahead (n_splits > 1)
  float* part_t;              // [U]: the target score, NaN = no rank
  const int32_t* row_of_pos;  // [M]: the inverse of cand_pos (cand_pos != NULL), written by ezk_row_of_pos_kernel
};

// the LDS of both kernels
struct EzkLds {
  int* rows;      // [EZK_STAGE] the present entries of the staged chunk, in history order
  float* w;       // [EZK_STAGE] their weights (1 without weights)
  int* cnt;       // [4] present entries per wave of the chunk
  unsigned* ex;   // [EZK_WORDS] excluded bit per column of the range; EBN_EZK_EX_DIRECT: [TK_MAX_X] the user's list
};

__device__ __forceinline__ void ezk_user_split(int64_t& u, int& split) {
#ifdef EBN_EZK_SPLIT_X  // the probe's alternative: the splits of a user are neighbours in launch order
  u = blockIdx.y;
  split = blockIdx.x;
#else
  u = blockIdx.x;
  split = blockIdx.y;
#endif
}

__device__ __forceinline__ int32_t ezk_clamp(int64_t v, int64_t hi) { return static_cast<int32_t>(v < 0 ? 0 : (v > hi ? hi : v)); }

// the entries [hb, he) of user u's history, clamped to [0, n_hist_items]; empty for a user without one
__device__ __forceinline__ void ezk_history(const EzkArgs& a, int64_t u, int32_t& hb, int32_t& he) {
  const int64_t h = a.user_hist != nullptr ? static_cast<int64_t>(a.user_hist[u]) : u;
  hb = he = 0;
  if (h >= 0 && h < a.n_hists) {
    hb = ezk_clamp(a.hist_offsets[h], a.n_hist_items);
    he = ezk_clamp(a.hist_offsets[h + 1], a.n_hist_items);
    if (he < hb) he = hb;
  }
}

// the clamped window of user u: [0, M) without windows, [0, 0) for an empty one
__device__ __forceinline__ void ezk_window(const EzkArgs& a, int64_t u, int& lo, int& hi) {
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

// the ranges [g_beg, g_end) of split `split`
__device__ __forceinline__ void ezk_span(const EzkArgs& a, int split, int64_t& g_beg, int64_t& g_end) {
  const int64_t n_ranges = (a.n_rows + EZK_R - 1) / EZK_R;
  g_beg = static_cast<int64_t>(split) * a.ranges_per_split;
  g_end = g_beg + a.ranges_per_split;
  g_end = g_end < n_ranges ? g_end : n_ranges;
}

// Stages the entries [jb, min(jb + 256, he)) of a history: the present ones (row inside [0, n_rows)) are compacted IN ORDER into
// l.rows / l.w; returns their number.  Every thread of the workgroup calls it with the same arguments; it starts and ends with a
// barrier.
__device__ __forceinline__ int ezk_stage(const EzkArgs& a, const EzkLds& l, int32_t jb, int32_t he, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  __syncthreads();  // everybody is done with the previous chunk
  const int32_t j = jb + tid;
  int32_t h = -1;
  if (j < he) h = a.hist_rows[j];
  const bool present = h >= 0 && h < static_cast<int32_t>(a.n_rows);  // n_rows <= EBN_EASE_MAX_ITEMS
  const unsigned long long m = __ballot(present);
  if (lane == 0) l.cnt[wave] = __popcll(m);
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int c = l.cnt[w];
    base += w < wave ? c : 0;
    total += c;
  }
  if (present) {
    const int at = base + __popcll(m & ((1ull << lane) - 1ull));
    l.rows[at] = h;
    l.w[at] = a.hist_weights != nullptr ? a.hist_weights[j] : 1.0f;
  }
  __syncthreads();
  return total;
}

// the EZK_V groups of row h a thread owns: columns c0 + v * EZK_STRIP .. + 3 (c0 = r0 + 4 tid); a column at or past n_rows reads 0
// and is never an address
template <bool VEC>
__device__ __forceinline__ void ezk_load(const EzkArgs& a, int h, int32_t c0, float (&x)[EZK_V][4]) {
  const float* __restrict__ row = a.B + static_cast<int64_t>(h) * a.ldb;
  const int32_t n = static_cast<int32_t>(a.n_rows);
#pragma unroll
  for (int v = 0; v < EZK_V; ++v) {
    const int32_t c = c0 + v * EZK_STRIP;
    if (VEC && c + 3 < n) {
      const float4 q = *reinterpret_cast<const float4*>(row + c);
      x[v][0] = q.x;
      x[v][1] = q.y;
      x[v][2] = q.z;
      x[v][3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[v][e] = c + e < n ? row[c + e] : 0.f;
    }
  }
}

// one product of a chain: the stored value itself without weights
__device__ __forceinline__ float ezk_product(bool weighted, float w, float b) { return weighted ? __fmul_rn(w, b) : b; }

// The chain over the n staged entries for the columns of this thread: the first entry of a chain (started == false) is stored, the
// others are added.  started is the same for every thread of the workgroup.
template <bool VEC>
__device__ __forceinline__ void ezk_accumulate(const EzkArgs& a, const EzkLds& l, int n, int32_t c0, float (&acc)[EZK_V][4], bool& started) {
  const bool weighted = a.hist_weights != nullptr;
  int i = 0;
  if (!started && n > 0) {
    float x[EZK_V][4];
    ezk_load<VEC>(a, l.rows[0], c0, x);
    const float w = l.w[0];
#pragma unroll
    for (int v = 0; v < EZK_V; ++v)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[v][e] = ezk_product(weighted, w, x[v][e]);
    started = true;
    i = 1;
  }
  for (; i + EZK_UNROLL <= n; i += EZK_UNROLL) {
    float x[EZK_UNROLL][EZK_V][4];
#pragma unroll
    for (int q = 0; q < EZK_UNROLL; ++q) ezk_load<VEC>(a, l.rows[i + q], c0, x[q]);
#pragma unroll
    for (int q = 0; q < EZK_UNROLL; ++q) {
      const float w = l.w[i + q];
#pragma unroll
      for (int v = 0; v < EZK_V; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[v][e] = __fadd_rn(acc[v][e], ezk_product(weighted, w, x[q][v][e]));
    }
  }
  for (; i < n; ++i) {
    float x[EZK_V][4];
    ezk_load<VEC>(a, l.rows[i], c0, x);
    const float w = l.w[i];
#pragma unroll
    for (int v = 0; v < EZK_V; ++v)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[v][e] = __fadd_rn(acc[v][e], ezk_product(weighted, w, x[v][e]));
  }
}

// The scores of the range at r0 for the history [hb, he) into acc; false: the history has no present entry (nothing is scored).
// n_present: the staged entries of a history of one chunk (staged by the caller, once); longer histories are staged here.
template <bool VEC>
__device__ __forceinline__ bool ezk_range_scores(const EzkArgs& a, const EzkLds& l, int32_t hb, int32_t he, int n_present, int32_t r0, int tid,
                                                 float (&acc)[EZK_V][4]) {
  bool started = false;
#pragma unroll
  for (int v = 0; v < EZK_V; ++v)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[v][e] = 0.f;
  const int32_t c0 = r0 + 4 * tid;
  if (he - hb <= EZK_STAGE) {
    ezk_accumulate<VEC>(a, l, n_present, c0, acc, started);
  } else {
    for (int32_t jb = hb; jb < he; jb += EZK_STAGE) {
      const int n = ezk_stage(a, l, jb, he, tid);
      ezk_accumulate<VEC>(a, l, n, c0, acc, started);
    }
  }
  return started;
}

// the user's exclusion list for the range [r0, r1); every thread calls it; ends with a barrier (X > 0)
__device__ __forceinline__ void ezk_exclusion(const EzkArgs& a, const EzkLds& l, int64_t u, int32_t r0, int32_t r1, int tid) {
#ifndef EBN_EZK_EX_DIRECT
  if (a.X <= 0) return;
  __syncthreads();  // everybody is done with the previous range's bits
  for (int i = tid; i < EZK_WORDS; i += EZK_THREADS) l.ex[i] = 0u;
  __syncthreads();
  for (int x = tid; x < a.X; x += EZK_THREADS) {
    const int32_t row = a.exclude[u * a.X + x];
    if (row >= r0 && row < r1) atomicOr(&l.ex[(row - r0) >> 5], 1u << ((row - r0) & 31));
  }
  __syncthreads();
#endif
}

__device__ __forceinline__ bool ezk_excluded(const EzkArgs& a, const EzkLds& l, int32_t r0, int c) {
#ifndef EBN_EZK_EX_DIRECT
  return a.X > 0 && ((l.ex[c >> 5] >> (c & 31)) & 1u) != 0u;
#else
  bool hit = false;
  for (int x = 0; x < a.X; ++x) hit |= static_cast<int32_t>(l.ex[x]) == r0 + c;
  return hit;
#endif
}

// Column r0 + c with score v for a user with the clamped window [wlo, whi): admissible -> its position.  A position >= M raises
// oob, a NaN score of a column that is admissible otherwise raises nan
__device__ __forceinline__ bool ezk_admissible(const EzkArgs& a, const EzkLds& l, int32_t r0, int c, float v, int wlo, int whi, int& pos,
                                               bool& oob, bool& nan) {
  const int64_t col = static_cast<int64_t>(r0) + c;
  if (col >= a.n_rows) return false;
  const int64_t p = a.cand_pos != nullptr ? static_cast<int64_t>(a.cand_pos[col]) : col;
  if (p < 0) return false;
  if (p >= a.M) {
    oob = true;
    return false;
  }
  if (p < wlo || p >= whi) return false;
  if (ezk_excluded(a, l, r0, c)) return false;
  if (v != v) {
    nan = true;
    return false;
  }
  pos = static_cast<int>(p);
  return true;
}

#define EZK_LDS(l)                                    \
  __shared__ int s_rows__[EZK_STAGE];                 \
  __shared__ float s_w__[EZK_STAGE];                  \
  __shared__ int s_cnt__[4];                          \
  __shared__ unsigned s_ex__[EZK_WORDS > TK_MAX_X ? EZK_WORDS : TK_MAX_X]; \
  EzkLds l;                                           \
  l.rows = s_rows__;                                  \
  l.w = s_w__;                                        \
  l.cnt = s_cnt__;                                    \
  l.ex = s_ex__

// EBN_EZK_EX_DIRECT: the user's list into LDS, once
__device__ __forceinline__ void ezk_exclusion_list(const EzkArgs& a, const EzkLds& l, int64_t u, int tid) {
#ifdef EBN_EZK_EX_DIRECT
  for (int x = tid; x < a.X; x += EZK_THREADS) l.ex[x] = static_cast<unsigned>(a.exclude[u * a.X + x]);
  __syncthreads();
#endif
}

template <bool VEC>
__global__ __launch_bounds__(EZK_THREADS) void ezk_topk_kernel(EzkTopkArgs a) {
  EZK_LDS(l);
  __shared__ float ms[3 * 64];  // the lists of waves 1 .. 3
  __shared__ int mp[3 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t u;
  int split;
  ezk_user_split(u, split);
  const int k = a.k;

  int32_t hb, he;
  ezk_history(a, u, hb, he);
  int wlo, whi;
  ezk_window(a, u, wlo, whi);
  int64_t g_beg, g_end;
  ezk_span(a, split, g_beg, g_end);

  float es = -INFINITY;  // slot `lane` of this wave's list
  int ep = TK_EMPTY;
  bool oob = false, nan = false;
  if (he > hb && g_beg < g_end) {
    ezk_exclusion_list(a, l, u, tid);
    const int n_present = he - hb <= EZK_STAGE ? ezk_stage(a, l, hb, he, tid) : 0;
    for (int64_t g = g_beg; g < g_end; ++g) {
      const int32_t r0 = static_cast<int32_t>(g * EZK_R);
      const int32_t r1 = static_cast<int32_t>(a.n_rows - r0 < EZK_R ? a.n_rows : r0 + EZK_R);
      float acc[EZK_V][4];
      if (!ezk_range_scores<VEC>(a, l, hb, he, n_present, r0, tid, acc)) break;  // no present entry: the same for every range
      ezk_exclusion(a, l, u, r0, r1, tid);
#pragma unroll
      for (int v = 0; v < EZK_V; ++v) {
        if (r0 + v * EZK_STRIP >= r1) break;  // the same for every thread
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int pos = 0;
          const bool ok = ezk_admissible(a, l, r0, v * EZK_STRIP + 4 * tid + e, acc[v][e], wlo, whi, pos, oob, nan);
          if (__ballot(ok) != 0ull) topk_wave_offer(es, ep, k, lane, ok, acc[v][e], pos);
        }
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

__device__ __forceinline__ void ezk_rank_write(const EzkRankArgs& a, int64_t u, int count, int ahead, float t) {
  const bool ranked = t == t;
  a.out_rank[u] = ranked ? 1 + ahead : 0;
  a.out_count[u] = count;
  a.out_score[u] = ranked ? t : -INFINITY;
}

template <bool VEC>
__global__ __launch_bounds__(EZK_THREADS) void ezk_rank_kernel(EzkRankArgs a) {
  EZK_LDS(l);
  __shared__ float s_p[EZK_STAGE];  // the target column's products of the staged chunk
  __shared__ int s_misc[12];        // [1] the target's row is excluded, [2] its position or -1, [4 .. 11] the waves' counts
  __shared__ float s_t[1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t u;
  int split;
  ezk_user_split(u, split);

  int32_t hb, he;
  ezk_history(a, u, hb, he);
  int wlo, whi;
  ezk_window(a, u, wlo, whi);
  int64_t g_beg, g_end;
  ezk_span(a, split, g_beg, g_end);
  bool oob = false, nan = false;

  // ---- the target: its row, then its chain in history order
  int tp = a.target_pos[u];
  if (static_cast<int64_t>(tp) >= a.M) {
    oob = true;
    tp = -1;
  }
  if (tp < wlo || tp >= whi) tp = -1;  // also tp < 0
  if (he <= hb) tp = -1;               // nothing is scored
  int trow = tp;  // without cand_pos the position is the row
  if (tp >= 0 && a.cand_pos != nullptr) {  // through the inverse map; a slot no row wrote holds anything: checked against cand_pos
    const int r = a.row_of_pos[tp];
    trow = (r >= 0 && r < a.n_rows && a.cand_pos[r] == tp) ? r : -1;
  }
  if (tid == 0) s_misc[1] = 0;
  __syncthreads();
  if (trow >= 0) {
    for (int x = tid; x < a.X; x += EZK_THREADS)
      if (a.exclude[u * a.X + x] == trow) s_misc[1] = 1;
  }
  __syncthreads();
  const bool chase = trow >= 0 && s_misc[1] == 0;
  const bool one_chunk = he - hb <= EZK_STAGE;
  int n_present = 0;
  if (he > hb) {
    ezk_exclusion_list(a, l, u, tid);
    if (one_chunk) n_present = ezk_stage(a, l, hb, he, tid);
  }
  float acc = 0.f;  // thread 0's
  bool any = false;
  if (chase) {
    const bool weighted = a.hist_weights != nullptr;
    for (int32_t jb = hb; jb < he; jb += EZK_STAGE) {
      const int n = one_chunk ? n_present : ezk_stage(a, l, jb, he, tid);
      if (tid < n) s_p[tid] = ezk_product(weighted, l.w[tid], a.B[static_cast<int64_t>(l.rows[tid]) * a.ldb + trow]);
      __syncthreads();
      if (tid == 0) {
        for (int i = 0; i < n; ++i) {
          acc = any ? __fadd_rn(acc, s_p[i]) : s_p[i];
          any = true;
        }
      }
      __syncthreads();  // s_p is free again
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
      const int32_t r0 = static_cast<int32_t>(g * EZK_R);
      const int32_t r1 = static_cast<int32_t>(a.n_rows - r0 < EZK_R ? a.n_rows : r0 + EZK_R);
      float sc[EZK_V][4];
      if (!ezk_range_scores<VEC>(a, l, hb, he, n_present, r0, tid, sc)) break;
      ezk_exclusion(a, l, u, r0, r1, tid);
#pragma unroll
      for (int v = 0; v < EZK_V; ++v) {
        if (r0 + v * EZK_STRIP >= r1) break;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int pos = 0;
          const float s = sc[v][e];
          if (ezk_admissible(a, l, r0, v * EZK_STRIP + 4 * tid + e, s, wlo, whi, pos, oob, nan)) {
            ++n_adm;
            n_ahd += (s > tt || (s == tt && pos < ttp)) ? 1 : 0;
          }
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
  if (lane == 0) {
    s_misc[4 + wave] = n_adm;
    s_misc[8 + wave] = n_ahd;
  }
  __syncthreads();
  if (tid == 0) {
    const int count = s_misc[4] + s_misc[5] + s_misc[6] + s_misc[7];
    const int ahead = s_misc[8] + s_misc[9] + s_misc[10] + s_misc[11];
    if (a.n_splits == 1) {
      ezk_rank_write(a, u, count, ahead, tt);
    } else {
      a.part[static_cast<int64_t>(split) * a.U + u] = count;
      a.part[(static_cast<int64_t>(a.n_splits) + split) * a.U + u] = ahead;
      if (split == 0) a.part_t[u] = tt;
    }
  }
}

// the inverse of cand_pos, once per call: row_of_pos[cand_pos[r]] = r for the positions inside [0, M).  The other slots are left as
// they are -- a reader checks cand_pos[row_of_pos[p]] == p -- so one launch does, without a fill ahead of it
__global__ __launch_bounds__(256) void ezk_row_of_pos_kernel(const int32_t* __restrict__ cand_pos, int64_t n_rows, int64_t M,
                                                             int32_t* __restrict__ row_of_pos) {
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; r < n_rows; r += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t p = cand_pos[r];
    if (p >= 0 && p < M) row_of_pos[p] = static_cast<int32_t>(r);
  }
}

// adds the n_splits partial counts of a user: integer sums, any order gives the same
__global__ __launch_bounds__(256) void ezk_rank_merge_kernel(EzkRankArgs a) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (u >= a.U) return;
  int count = 0, ahead = 0;
  for (int s = 0; s < a.n_splits; ++s) {
    count += a.part[static_cast<int64_t>(s) * a.U + u];
    ahead += a.part[(static_cast<int64_t>(a.n_splits) + s) * a.U + u];
  }
  ezk_rank_write(a, u, count, ahead, a.part_t[u]);
}

// an empty matrix or no candidate position: nobody has a rank; a target position >= M is still reported
__global__ __launch_bounds__(256) void ezk_rank_empty_kernel(const int32_t* __restrict__ target_pos, int64_t M, int32_t* __restrict__ out_rank,
                                                             int32_t* __restrict__ out_count, float* __restrict__ out_score,
                                                             int32_t* __restrict__ flags, int64_t U) {
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; u < U; u += static_cast<int64_t>(gridDim.x) * 256) {
    if (static_cast<int64_t>(target_pos[u]) >= M) flags[0] = 1;
    out_rank[u] = 0;
    out_count[u] = 0;
    out_score[u] = -INFINITY;
  }
}

// ---- host.  n_splits ranges divide the ceil(n_rows / EZK_R) ranges of a user.  Automatic: about 16 384 workgroups when the users
// alone do not give them (ebn_cv_topk_auto_splits' rule).  U, n_rows >= 1
inline int ezk_resolve_splits(int64_t U, int64_t n_rows, int32_t n_splits) {
  const int64_t ranges = ebn_ceil_div(n_rows, EZK_R);
  int64_t s = n_splits > 0 ? n_splits : ebn_ceil_div(16384, U);
  if (s > ranges) s = ranges;
  if (s > EZK_MAX_SPLITS) s = EZK_MAX_SPLITS;
  return static_cast<int>(s < 1 ? 1 : s);
}

// what both entry points check first, in this order
int ezk_check(int64_t n_rows, int64_t ldb, int64_t n_hists, int64_t n_hist_items, const int32_t* cand_pos, int64_t M, int32_t X, int32_t k,
              int32_t n_splits, int64_t workspace_bytes, int64_t U) {
  EBN_REQUIRE(ebn_dim_ok(n_rows, ldb, n_hists, n_hist_items) && ebn_dim_ok(M, U) && X >= 0 && n_splits >= 0 && workspace_bytes >= 0,
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ldb >= n_rows && (n_hist_items == 0 || n_hists >= 1) && (cand_pos != nullptr || M == n_rows), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(k >= 1 && k <= TK_MAX_K && X <= TK_MAX_X && n_rows <= EBN_EASE_MAX_ITEMS, EBN_ERR_UNSUPPORTED);
#ifdef EBN_EZK_SPLIT_X
  EBN_REQUIRE(U <= 65535, EBN_ERR_UNSUPPORTED);
#endif
  return EBN_OK;
}

void ezk_fill(EzkArgs& a, const float* B, int64_t n_rows, int64_t ldb, const int32_t* hist_rows, const float* hist_weights,
              const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items, const int32_t* user_hist, const int32_t* cand_pos, int64_t M,
              const int32_t* window, const int32_t* exclude, int32_t X, int32_t* flags, int64_t U) {
  a.B = B;
  a.hist_rows = hist_rows;
  a.hist_weights = hist_weights;
  a.hist_offsets = hist_offsets;
  a.user_hist = user_hist;
  a.cand_pos = cand_pos;
  a.window = window;
  a.exclude = exclude;
  a.flags = flags;
  a.ldb = ldb;
  a.n_rows = n_rows;
  a.n_hists = n_hists;
  a.n_hist_items = n_hist_items;
  a.M = M;
  a.U = U;
  a.X = exclude != nullptr ? X : 0;
}

// the operands a launch reads
bool ezk_operands_ok(const EzkArgs& a) {
  return a.B != nullptr && (a.n_hists == 0 || a.hist_offsets != nullptr) && (a.n_hist_items == 0 || a.hist_rows != nullptr);
}

// 16-byte loads of B[h, r0 + 4 t ..]: every row start and every group start is 16-byte aligned
bool ezk_vector_path(const EzkArgs& a) { return ebn_aligned16(a.B) && a.ldb % 4 == 0; }

dim3 ezk_grid(int64_t U, int splits) {
#ifdef EBN_EZK_SPLIT_X
  return dim3(static_cast<unsigned>(splits), static_cast<unsigned>(U));
#else
  return dim3(static_cast<unsigned>(U), static_cast<unsigned>(splits));
#endif
}

}  // namespace

extern "C" int64_t ebn_ease_topk_range(void) { return EZK_R; }

extern "C" int ebn_ease_topk_auto_splits(int64_t n_users, int64_t n_rows) {
  if (!ebn_dim_ok(n_users, n_rows) || n_users == 0 || n_rows == 0) return 1;
  return ezk_resolve_splits(n_users, n_rows, 0);
}

extern "C" int64_t ebn_ease_topk_workspace_bytes(int64_t n_users, int32_t k, int32_t n_splits) {
  return ebn_topk_workspace_bytes(n_users, k, n_splits);  // the partial lists are ebn_topk_score_f32's
}

extern "C" int64_t ebn_ease_target_rank_workspace_bytes(int64_t n_users, int32_t n_splits, int64_t n_positions) {
  if (!ebn_dim_ok(n_users, n_positions) || n_splits < 1) return 0;
  if (n_users == 0) return 16;
  // [M] int32: the inverse of cand_pos (n_positions = M with a cand_pos, else 0); then, for more than one split (one writes the
  // outputs directly), [2, s, U] int32 partial counts and [U] float target scores
  const int64_t s = n_splits > EZK_MAX_SPLITS ? EZK_MAX_SPLITS : n_splits;
  const int64_t parts = n_splits == 1 ? 0 : ebn_sat_add(ebn_sat_mul(2 * s, n_users), n_users);
  return ebn_sat_add(ebn_sat_mul(ebn_sat_add(parts, n_positions), 4), 16);
}

extern "C" int ebn_ease_topk_f32(const float* B, int64_t n_rows, int64_t ldb, const int32_t* hist_rows, const float* hist_weights,
                                 const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items, const int32_t* user_hist,
                                 const int32_t* cand_pos, int64_t M, const int32_t* window, const int32_t* exclude, int32_t X, int32_t k,
                                 int32_t n_splits, int32_t* out_pos, float* out_score, int32_t* flags, void* workspace,
                                 int64_t workspace_bytes, int64_t U, ebn_stream_t stream) {
  const int rc0 = ezk_check(n_rows, ldb, n_hists, n_hist_items, cand_pos, M, X, k, n_splits, workspace_bytes, U);
  if (rc0 != EBN_OK) return rc0;
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(out_pos != nullptr && out_score != nullptr && flags != nullptr, EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (n_rows == 0 || M == 0) return topk_launch_fill_empty(out_pos, out_score, U, k, s);
  EzkTopkArgs a;
  ezk_fill(a, B, n_rows, ldb, hist_rows, hist_weights, hist_offsets, n_hists, n_hist_items, user_hist, cand_pos, M, window, exclude, X, flags, U);
  a.k = k;
  a.out_pos = out_pos;
  a.out_score = out_score;
  EBN_REQUIRE(ezk_operands_ok(a), EBN_ERR_BAD_ARG);
  const int splits = ezk_resolve_splits(U, n_rows, n_splits);
  a.n_splits = splits;
  a.ranges_per_split = static_cast<int32_t>(ebn_ceil_div(ebn_ceil_div(n_rows, EZK_R), splits));
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
  const dim3 grid = ezk_grid(U, splits), block(EZK_THREADS);
  if (ezk_vector_path(a)) {
    EBN_LAUNCH(ezk_topk_kernel<true>, grid, block, 0, s, a);
  } else {
    EBN_LAUNCH(ezk_topk_kernel<false>, grid, block, 0, s, a);
  }
  EBN_CHECK_LAUNCH();
  if (splits > 1) return topk_launch_merge(l, s);
  return EBN_OK;
}

extern "C" int ebn_ease_target_rank_f32(const float* B, int64_t n_rows, int64_t ldb, const int32_t* hist_rows, const float* hist_weights,
                                        const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items, const int32_t* user_hist,
                                        const int32_t* cand_pos, int64_t M, const int32_t* target_pos, const int32_t* window,
                                        const int32_t* exclude, int32_t X, int32_t n_splits, int32_t* out_rank, int32_t* out_count,
                                        float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U,
                                        ebn_stream_t stream) {
  const int rc0 = ezk_check(n_rows, ldb, n_hists, n_hist_items, cand_pos, M, X, 1, n_splits, workspace_bytes, U);
  if (rc0 != EBN_OK) return rc0;
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(target_pos != nullptr && out_rank != nullptr && out_count != nullptr && out_score != nullptr && flags != nullptr,
              EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (n_rows == 0 || M == 0) {
    const int64_t blocks = ebn_ceil_div(U, 256);
    EBN_LAUNCH(ezk_rank_empty_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, target_pos, M, out_rank,
               out_count, out_score, flags, U);
    EBN_CHECK_LAUNCH();
    return EBN_OK;
  }
  EzkRankArgs a;
  ezk_fill(a, B, n_rows, ldb, hist_rows, hist_weights, hist_offsets, n_hists, n_hist_items, user_hist, cand_pos, M, window, exclude, X, flags, U);
  a.target_pos = target_pos;
  a.out_rank = out_rank;
  a.out_count = out_count;
  a.out_score = out_score;
  a.part = nullptr;
  a.part_t = nullptr;
  a.row_of_pos = nullptr;
  EBN_REQUIRE(ezk_operands_ok(a), EBN_ERR_BAD_ARG);
  const int splits = ezk_resolve_splits(U, n_rows, n_splits);
  a.n_splits = splits;
  a.ranges_per_split = static_cast<int32_t>(ebn_ceil_div(ebn_ceil_div(n_rows, EZK_R), splits));
  if (splits > 1 || cand_pos != nullptr) {
    const int64_t need = ebn_ease_target_rank_workspace_bytes(U, splits, cand_pos != nullptr ? M : 0);
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
    EBN_LAUNCH(ezk_row_of_pos_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, cand_pos, n_rows, M,
               static_cast<int32_t*>(workspace));
    EBN_CHECK_LAUNCH();
  }
  const dim3 grid = ezk_grid(U, splits), block(EZK_THREADS);
  if (ezk_vector_path(a)) {
    EBN_LAUNCH(ezk_rank_kernel<true>, grid, block, 0, s, a);
  } else {
    EBN_LAUNCH(ezk_rank_kernel<false>, grid, block, 0, s, a);
  }
  EBN_CHECK_LAUNCH();
  if (splits > 1) {
    EBN_LAUNCH(ezk_rank_merge_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(U, 256))), dim3(256), 0, s, a);
    EBN_CHECK_LAUNCH();
  }
  return EBN_OK;
}
