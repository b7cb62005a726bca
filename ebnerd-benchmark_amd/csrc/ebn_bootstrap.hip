// Poisson bootstrap of per-item metric columns: sums[b, c] = sum_i w(i, b) x[c, i] and weight_sums[b] = sum_i w(i, b) for B resamples,
// w(i, b) ~ Poisson(1) from the counter-based stream of include/ebnerd_hip.h (mirrored in ebrec/evaluation/bootstrap.py).
//   * lanes own resamples: a lane keeps r_b of BS_RPL resamples (b, b + 256) and their n_cols + 1 accumulators in registers; a
//     workgroup of 256 lanes covers EBN_BS_RESAMPLES = 512 resamples and walks ONE contiguous range of items;
//   * a tile of EBN_BS_TILE items -- a_i = lowbias32(key_i ^ k) and the column values -- is staged through LDS with coalesced loads
//     and read back with every lane at the same address (a broadcast), so the inner loop has no cross-lane traffic: one hash and one
//     inverse-CDF count per (item, resample) on the integer ALU, then n_cols fp64 fma;
//   * the item ranges are whole tiles and depend on n_items alone; a lane adds its items in ascending order with one explicit fma per
//     column, the ranges' partials go to the workspace and a closing launch adds them in ascending order.  So a column's bits do not
//     depend on the other columns of the call, a resample's not on the other resamples, and two runs agree.  No atomics.
#include "ebn_common.h"

#define BS_T EBN_BS_TILE
#define BS_THREADS 256
#define BS_RPL (EBN_BS_RESAMPLES / BS_THREADS)  // resamples per lane
#define BS_MAX_RANGES 512  // 2048 workgroups at 2000 resamples: enough waves per SIMD to hide the compare-to-carry wait states

static_assert(BS_T == BS_THREADS, "a tile is staged one item per thread");
static_assert(EBN_BS_RESAMPLES % BS_THREADS == 0, "whole resamples per lane");

static constexpr uint32_t kBsC[EBN_BS_MAX_WEIGHT] = EBN_BS_THRESHOLDS;

// inverse CDF of Poisson(1): the number of thresholds at or below u.  Above the fourth threshold lie 0.37 % of all draws, so the
// other eight comparisons sit behind a branch most waves skip.
static __device__ __forceinline__ uint32_t bs_weight(uint32_t u) {
  uint32_t w = (u >= kBsC[0]) + (u >= kBsC[1]) + (u >= kBsC[2]) + (u >= kBsC[3]);
  if (u >= kBsC[4]) {
#pragma unroll
    for (int j = 4; j < EBN_BS_MAX_WEIGHT; ++j) w += u >= kBsC[j];
  }
  return w;
}

template <int NC>
struct BsAcc {
  double s[BS_RPL][NC];
  uint32_t w[BS_RPL];  // at most 12 * items of a range < 2^32: see bs_sizes_ok
};

template <int NC>
static __device__ __forceinline__ void bs_item(BsAcc<NC>& acc, const uint32_t (&r)[BS_RPL], uint32_t a, const double (*sx)[BS_T], int j) {
#pragma unroll
  for (int q = 0; q < BS_RPL; ++q) {
    const uint32_t w = bs_weight(ebn_lowbias32(a + r[q]));
    acc.w[q] += w;
    const double wd = static_cast<double>(w);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc.s[q][c] = fma(wd, sx[c][j], acc.s[q][c]);
  }
}

template <int NC>
static __global__ __launch_bounds__(BS_THREADS) void bs_ranges_kernel(const double* __restrict__ values, int64_t ld, int64_t n_items,
                                                                      const uint32_t* __restrict__ keys, uint32_t first_key, uint32_t k,
                                                                      uint32_t first_resample, int64_t n_resamples, int64_t tiles_per_range,
                                                                      double* __restrict__ part_sums, int64_t* __restrict__ part_w) {
  __shared__ __attribute__((aligned(16))) uint32_t sa[BS_T];
  __shared__ double sx[NC][BS_T];
  const int t = threadIdx.x;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * EBN_BS_RESAMPLES, g = blockIdx.y;
  uint32_t r[BS_RPL];
#pragma unroll
  for (int q = 0; q < BS_RPL; ++q) {
    const uint32_t b = first_resample + static_cast<uint32_t>(b0 + q * BS_THREADS + t);  // rows past n_resamples are computed, not stored
    r[q] = ebn_lowbias32((b * 0x9E3779B9u) ^ ~k);
  }
  BsAcc<NC> acc;
#pragma unroll
  for (int q = 0; q < BS_RPL; ++q) {
    acc.w[q] = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc.s[q][c] = 0.0;
  }
  const int64_t i_begin = g * tiles_per_range * BS_T;
  const int64_t i_stop = i_begin + tiles_per_range * BS_T;
  const int64_t i_end = i_stop < n_items ? i_stop : n_items;
  for (int64_t i0 = i_begin; i0 < i_end; i0 += BS_T) {
    const int tn = i_end - i0 < BS_T ? static_cast<int>(i_end - i0) : BS_T;
    __syncthreads();  // the previous tile has been read
    if (t < tn) {     // nothing at or past n_items is read: padding there may hold anything
      const int64_t i = i0 + t;
      const uint32_t key = keys != nullptr ? keys[i] : first_key + static_cast<uint32_t>(i);
      sa[t] = ebn_lowbias32(key ^ k);
#pragma unroll
      for (int c = 0; c < NC; ++c) sx[c][t] = values[static_cast<int64_t>(c) * ld + i];
    }
    __syncthreads();
    int j = 0;
    for (; j + 4 <= tn; j += 4) {  // four items a step: the 16-byte LDS reads of a_i and of two values per column
      const uint4 a4 = *reinterpret_cast<const uint4*>(&sa[j]);
      bs_item<NC>(acc, r, a4.x, sx, j);
      bs_item<NC>(acc, r, a4.y, sx, j + 1);
      bs_item<NC>(acc, r, a4.z, sx, j + 2);
      bs_item<NC>(acc, r, a4.w, sx, j + 3);
    }
    for (; j < tn; ++j) bs_item<NC>(acc, r, sa[j], sx, j);
  }
#pragma unroll
  for (int q = 0; q < BS_RPL; ++q) {
    const int64_t row = b0 + q * BS_THREADS + t;
    if (row < n_resamples) {
      const int64_t at = g * n_resamples + row;
      part_w[at] = static_cast<int64_t>(acc.w[q]);
#pragma unroll
      for (int c = 0; c < NC; ++c) part_sums[at * NC + c] = acc.s[q][c];
    }
  }
}

// closing pass: one thread per (resample, column or weight), over the ranges in ascending order
static __global__ __launch_bounds__(256) void bs_close_kernel(const double* __restrict__ part_sums, const int64_t* __restrict__ part_w,
                                                              int64_t n_ranges, int64_t n_resamples, int n_cols, double* __restrict__ sums,
                                                              int64_t* __restrict__ weight_sums) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= n_resamples * (n_cols + 1)) return;
  const int64_t b = idx / (n_cols + 1);
  const int c = static_cast<int>(idx % (n_cols + 1));
  if (c < n_cols) {
    double s = 0.0;
    for (int64_t g = 0; g < n_ranges; ++g) s += part_sums[(g * n_resamples + b) * n_cols + c];
    sums[b * n_cols + c] = s;
  } else {
    int64_t w = 0;
    for (int64_t g = 0; g < n_ranges; ++g) w += part_w[g * n_resamples + b];
    weight_sums[b] = w;
  }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------
// item ranges: whole tiles, at most BS_MAX_RANGES, a function of n_items alone
static inline int64_t bs_tiles(int64_t n_items) { return ebn_ceil_div(n_items, BS_T); }
static inline int64_t bs_tiles_per_range(int64_t n_items) {
  const int64_t per = ebn_ceil_div(bs_tiles(n_items), BS_MAX_RANGES);
  return per > 0 ? per : 1;
}
static inline int64_t bs_ranges(int64_t n_items) {
  const int64_t n = ebn_ceil_div(bs_tiles(n_items), bs_tiles_per_range(n_items));
  return n > 0 ? n : 1;  // n_items == 0: one empty range, whose zeros the closing pass writes
}

// a range holds at most (2^31 / 256 / 512 + 1) * 256 items, times 12 < 2^32: the 32-bit weight accumulator of a lane cannot wrap
static inline bool bs_sizes_ok(int64_t n_items, int64_t n_resamples, int32_t n_cols) {
  return ebn_dim_ok(n_items, n_resamples) && n_items <= EBN_DIM_MAX - 256 && n_cols >= 1 && n_cols <= EBN_BS_MAX_COLS;
}

extern "C" int64_t ebn_poisson_bootstrap_workspace_bytes(int64_t n_items, int64_t n_resamples, int32_t n_cols) {
  if (!bs_sizes_ok(n_items, n_resamples, n_cols)) return 0;
  return ebn_sat_mul(ebn_sat_mul(bs_ranges(n_items), n_resamples), (static_cast<int64_t>(n_cols) + 1) * 8);
}

template <int NC>
static void bs_launch(dim3 grid, hipStream_t s, const double* values, int64_t ld, int64_t n_items, const uint32_t* keys, uint32_t first_key,
                      uint32_t k, uint32_t first_resample, int64_t n_resamples, int64_t tiles_per_range, double* part_sums, int64_t* part_w) {
  EBN_LAUNCH((bs_ranges_kernel<NC>), grid, dim3(BS_THREADS), 0, s, values, ld, n_items, keys, first_key, k, first_resample, n_resamples,
             tiles_per_range, part_sums, part_w);
}

extern "C" int ebn_poisson_bootstrap_f64(const double* values, int64_t ld, int64_t n_items, int32_t n_cols, const uint32_t* keys,
                                         uint32_t first_key, uint32_t seed, int64_t first_resample, int64_t n_resamples, double* sums,
                                         int64_t* weight_sums, void* workspace, int64_t workspace_bytes, ebn_stream_t stream) {
  EBN_REQUIRE(n_cols >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_cols <= EBN_BS_MAX_COLS, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(bs_sizes_ok(n_items, n_resamples, n_cols) && ld >= n_items && ld <= INT64_MAX / (8 * EBN_BS_MAX_COLS) && first_resample >= 0 &&
                  first_resample <= (int64_t{1} << 32) - n_resamples,
              EBN_ERR_BAD_ARG);
  if (n_resamples == 0) return EBN_OK;
  EBN_REQUIRE((values != nullptr || n_items == 0) && sums != nullptr && weight_sums != nullptr && workspace != nullptr, EBN_ERR_BAD_ARG);
  const int64_t need = ebn_poisson_bootstrap_workspace_bytes(n_items, n_resamples, n_cols);
  EBN_REQUIRE(workspace_bytes >= need && ebn_aligned16(workspace), EBN_ERR_BAD_ARG);
  const int64_t ranges = bs_ranges(n_items), per = bs_tiles_per_range(n_items);
  double* part_sums = static_cast<double*>(workspace);
  int64_t* part_w = reinterpret_cast<int64_t*>(part_sums + ranges * n_resamples * n_cols);
  const uint32_t k = ebn_lowbias32(seed ^ 0x9E3779B9u);
  const dim3 grid(static_cast<unsigned>(ebn_ceil_div(n_resamples, EBN_BS_RESAMPLES)), static_cast<unsigned>(ranges));
  hipStream_t s = ebn_stream(stream);
  const uint32_t fr = static_cast<uint32_t>(first_resample);
  switch (n_cols) {
#define BS_CASE(NC) \
  case NC: bs_launch<NC>(grid, s, values, ld, n_items, keys, first_key, k, fr, n_resamples, per, part_sums, part_w); break;
    BS_CASE(1) BS_CASE(2) BS_CASE(3) BS_CASE(4) BS_CASE(5) BS_CASE(6) BS_CASE(7) BS_CASE(8)
    BS_CASE(9) BS_CASE(10) BS_CASE(11) BS_CASE(12) BS_CASE(13) BS_CASE(14) BS_CASE(15) BS_CASE(16)
#undef BS_CASE
    default: return EBN_ERR_UNSUPPORTED;
  }
  EBN_CHECK_LAUNCH();
  const int64_t entries = n_resamples * (static_cast<int64_t>(n_cols) + 1);
  EBN_LAUNCH(bs_close_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(entries, 256))), dim3(256), 0, s, part_sums, part_w, ranges, n_resamples,
             n_cols, sums, weight_sums);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
