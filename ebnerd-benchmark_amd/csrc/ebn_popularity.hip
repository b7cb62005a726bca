// Trailing-window event counts, the popularity baseline's hot path: for item i of list l (an in-view article of an impression at
// t = list_times[l]) and window w, counts[w, i] = #{ e in row item_rows[i] : t - max_age_w <= e < t - min_age } over per-row ascending
// event times (contract in include/ebnerd_hip.h).
//   * one lane per item, 256-item workgroups.  The workgroup finds the list of its first item with ONE upper_bound over list_offsets
//     (the same search in every lane: uniform, so it runs on the scalar unit) and stages the next WC_T list boundaries in LDS; a lane
//     finds its own list with an 8-step search of that tile.  Only a tile with more than WC_T boundaries inside 256 items (a run of
//     empty lists) sends a lane on to a search of the rest of list_offsets.  No per-item list array comes from the host;
//   * per item one lower_bound for t - min_age over the row, then one lower_bound per window inside [previous result, that position):
//     the host sorts the windows by descending max_age, so the lower ends ascend and every search starts where the last one ended.
//     With 1 h / 6 h / 24 h windows over weeks of events only the first two searches are as long as log2(row length), and those two
//     -- the upper end and the longest window's lower end -- run side by side in one loop (wc_lower_bound2);
//   * all compares and indices are int64; t - age saturates at the int64 limits; EBN_WC_UNBOUNDED is "from the row's first event";
//   * unknown rows (-1 from the host layer) and lanes past n_items get an empty event range under a lane predicate: they read
//     nothing, run no search step and still reach the barrier;
//   * no atomics, no workspace: a count depends on its own item only.
// The kernel is bound by the latency of dependent loads (about log2(row length) + a few per item and 4 bytes in, 4 W bytes out);
// the upper levels of a popular row's search tree are shared by every item that asks for it and stay in L2 / Infinity Cache.
#include "ebn_common.h"

#define WC_T 256  // items of a workgroup = staged list boundaries

struct WcWindows {
  int64_t max_age[EBN_WC_MAX_WINDOWS];  // descending
  int32_t dst[EBN_WC_MAX_WINDOWS];      // the caller's window number of each
};

static __device__ __forceinline__ int64_t wc_sat_sub(int64_t t, int64_t age) {  // age >= 0
  int64_t r;
  return __builtin_sub_overflow(t, age, &r) ? INT64_MIN : r;
}

// first position in [lo, hi) whose value is not below key (hi if none)
static __device__ __forceinline__ int64_t wc_lower_bound(const int64_t* __restrict__ v, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// two lower_bounds over the same [lo, hi) at once: the two chains of dependent loads overlap, and until the keys part they read
// the same elements
static __device__ __forceinline__ void wc_lower_bound2(const int64_t* __restrict__ v, int64_t lo, int64_t hi, int64_t key_a, int64_t key_b,
                                                       int64_t& pos_a, int64_t& pos_b) {
  int64_t la = lo, ha = hi, lb = lo, hb = hi;
  while (la < ha || lb < hb) {
    const bool a = la < ha, b = lb < hb;
    const int64_t ma = la + ((ha - la) >> 1), mb = lb + ((hb - lb) >> 1);
    const int64_t va = a ? v[ma] : 0, vb = b ? v[mb] : 0;  // both loads issue before either compare
    if (a) {
      if (va < key_a) la = ma + 1; else ha = ma;
    }
    if (b) {
      if (vb < key_b) lb = mb + 1; else hb = mb;
    }
  }
  pos_a = la;
  pos_b = lb;
}

// first position in [lo, hi) whose value is above key (hi if none)
static __device__ __forceinline__ int64_t wc_upper_bound(const int64_t* __restrict__ v, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

static __global__ __launch_bounds__(WC_T) void wc_counts_kernel(const int64_t* __restrict__ event_times, const int64_t* __restrict__ row_offsets,
                                                                int64_t n_rows, const int32_t* __restrict__ item_rows, int64_t n_items,
                                                                const int64_t* __restrict__ list_offsets,
                                                                const int64_t* __restrict__ list_times, int64_t n_lists, WcWindows win,
                                                                int n_windows, int first_bounded, int64_t first_age, int64_t min_age,
                                                                int32_t* __restrict__ counts, int64_t ld) {
  __shared__ int64_t s_bound[WC_T];
  const int t = threadIdx.x;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * WC_T, i = i0 + t;
  // list_offsets has n_lists + 1 entries; item i is in list #{ k in [0, n_lists] : list_offsets[k] <= i } - 1
  const int64_t base = wc_upper_bound(list_offsets, 0, n_lists + 1, i0);  // >= 1: list_offsets[0] = 0 <= i0
  const int64_t k = base + t;
  s_bound[t] = k <= n_lists ? list_offsets[k] : INT64_MAX;
  __syncthreads();
  const bool live = i < n_items;
  int64_t l = 0, ev_begin = 0, ev_end = 0, tl = 0;
  if (live) {
    int c = 0;
#pragma unroll
    for (int step = WC_T / 2; step > 0; step >>= 1) c += s_bound[c + step - 1] <= i ? step : 0;  // #{ staged <= i } in [0, WC_T - 1]
    c += s_bound[c] <= i ? 1 : 0;
    l = base + c;
    if (c == WC_T && l <= n_lists) l = wc_upper_bound(list_offsets, l, n_lists + 1, i);  // more than WC_T boundaries inside the tile
    l = (l > n_lists ? n_lists : l) - 1;  // list_offsets[n_lists] >= n_items > i by contract; never an address past list_times
    if (l < 0) l = 0;
    tl = list_times[l];
    const int64_t r = item_rows[i];
    if (r >= 0 && r < n_rows) {
      ev_begin = row_offsets[r];
      ev_end = row_offsets[r + 1];
    }
  }
  // dead lanes and unknown rows: [0, 0), every search below is zero steps and reads nothing
  // the two searches over the whole row -- the upper end and the lower end of the longest bounded window -- run side by side
  int64_t p_hi, p = ev_begin;
  if (first_bounded < n_windows) {
    wc_lower_bound2(event_times, ev_begin, ev_end, wc_sat_sub(tl, first_age), wc_sat_sub(tl, min_age), p, p_hi);
    p = p < p_hi ? p : p_hi;  // max_age < min_age: an empty window
  } else {
    p_hi = wc_lower_bound(event_times, ev_begin, ev_end, wc_sat_sub(tl, min_age));
  }
#pragma unroll
  for (int w = 0; w < EBN_WC_MAX_WINDOWS; ++w) {
    if (w < n_windows) {
      // unbounded windows come first and count from ev_begin; the first bounded one has its end already
      if (w > first_bounded) p = wc_lower_bound(event_times, p, p_hi, wc_sat_sub(tl, win.max_age[w]));
      if (live) counts[static_cast<int64_t>(win.dst[w]) * ld + i] = static_cast<int32_t>(p_hi - (w < first_bounded ? ev_begin : p));
    }
  }
}

extern "C" int ebn_window_counts_i32(const int64_t* event_times, const int64_t* row_offsets, int64_t n_rows, const int32_t* item_rows,
                                     int64_t n_items, const int64_t* list_offsets, const int64_t* list_times, int64_t n_lists,
                                     int32_t n_windows, int64_t max_age0, int64_t max_age1, int64_t max_age2, int64_t max_age3,
                                     int64_t max_age4, int64_t max_age5, int64_t max_age6, int64_t max_age7, int64_t min_age,
                                     int32_t* counts, int64_t ld, ebn_stream_t stream) {
  EBN_REQUIRE(n_windows >= 1 && n_windows <= EBN_WC_MAX_WINDOWS, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_dim_ok(n_items, n_lists, n_rows) && ld >= n_items && ld <= INT64_MAX / (4 * EBN_WC_MAX_WINDOWS) && min_age >= 0,
              EBN_ERR_BAD_ARG);
  const int64_t ages[EBN_WC_MAX_WINDOWS] = {max_age0, max_age1, max_age2, max_age3, max_age4, max_age5, max_age6, max_age7};
  for (int w = 0; w < n_windows; ++w) EBN_REQUIRE(ages[w] >= 0, EBN_ERR_BAD_ARG);
  if (n_items == 0) return EBN_OK;
  EBN_REQUIRE(n_lists >= 1, EBN_ERR_BAD_ARG);  // an item belongs to a list
  EBN_REQUIRE(item_rows != nullptr && list_offsets != nullptr && list_times != nullptr && counts != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_rows == 0 || (row_offsets != nullptr && event_times != nullptr), EBN_ERR_BAD_ARG);
  // descending max_age, equal ages in the caller's order (insertion sort of at most 8)
  WcWindows win;
  for (int w = 0; w < EBN_WC_MAX_WINDOWS; ++w) {
    win.max_age[w] = 0;
    win.dst[w] = 0;
  }
  for (int w = 0; w < n_windows; ++w) {
    int at = w;
    for (; at > 0 && win.max_age[at - 1] < ages[w]; --at) {
      win.max_age[at] = win.max_age[at - 1];
      win.dst[at] = win.dst[at - 1];
    }
    win.max_age[at] = ages[w];
    win.dst[at] = w;
  }
  int first_bounded = 0;  // the windows before it are EBN_WC_UNBOUNDED
  while (first_bounded < n_windows && win.max_age[first_bounded] == EBN_WC_UNBOUNDED) ++first_bounded;
  EBN_LAUNCH(wc_counts_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(n_items, WC_T))), dim3(WC_T), 0, ebn_stream(stream), event_times,
             row_offsets, n_rows, item_rows, n_items, list_offsets, list_times, n_lists, win, static_cast<int>(n_windows), first_bounded,
             first_bounded < n_windows ? win.max_age[first_bounded] : 0, min_age, counts, ld);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
