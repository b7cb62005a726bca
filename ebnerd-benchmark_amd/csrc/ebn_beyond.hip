// Beyond-accuracy list metrics (reference: evaluation/beyond_accuracy.py, evaluation/metrics/_beyond_accuracy.py): intralist
// diversity, serendipity, novelty / sentiment list means and the candidate-diversity subset sums over a device-resident table
// of UNIT rows.  Every kernel is "gather a few rows, small dense math, segmented reduce":
//   * lists arrive as int32 row numbers + int64 CSR offsets; a row number outside [0, n_rows) is a MISSING id (get_keys_in_dict,
//     utils.py:155-169) -- it is skipped, never used as an address; an offsets pair outside [0, n_ids] makes its list empty;
//   * distances are taken pair by pair, clip(1 - u_i . u_j, 0, 2) (sklearn cosine_distances), summed per lane and then as a tree.
//     The closed form n^2 - |sum u|^2 is NOT used: it cancels for the near-duplicate lists the metric is defined on;
//   * two forms of the pair loop: lists of at most EBN_BA_FAST_MAX positions run one wave per list with a slice of every row in
//     registers (top-5 / top-10 lists: the gather, not the math, is the cost; for the cross mean the short side of a pair stays in
//     registers, D <= 1024); every other length runs one workgroup per list over 16 x 16 tiles of pairs with 64-column slabs of
//     the rows in LDS (any length, any D).
#include "ebn_common.h"

#define EBN_BA_FAST_MAX 10
#define EBN_BA_FAST_PAIRS (EBN_BA_FAST_MAX * (EBN_BA_FAST_MAX - 1) / 2)
#define EBN_BA_T 16   // tile edge of the general form: 256 threads = 16 x 16 pairs
#define EBN_BA_KC 64  // columns per LDS slab
#define EBN_BA_LD 68  // slab row pitch in floats: 16-byte aligned rows, 16 rows on 16 different 4-bank slots

static __device__ __forceinline__ float ba_nan() { return __builtin_nanf(""); }
static __device__ __forceinline__ float ba_dist(float dot) { return fminf(fmaxf(1.0f - dot, 0.0f), 2.0f); }

// [beg, beg + len) of list l; offsets that leave [0, n_ids] or run backwards give an empty list
static __device__ __forceinline__ void ba_span(const int64_t* __restrict__ offsets, int64_t l, int64_t n_ids, int64_t& beg, int64_t& len) {
  const int64_t o0 = offsets[l], o1 = offsets[l + 1];
  const bool ok = o0 >= 0 && o1 >= o0 && o1 <= n_ids;
  beg = ok ? o0 : 0;
  len = ok ? o1 - o0 : 0;
}

// table row of position p of a list, -1 for a missing id or a position past the end
static __device__ __forceinline__ int ba_row(const int32_t* __restrict__ ids, int64_t beg, int64_t p, int64_t len, int64_t n_rows) {
  if (p >= len) return -1;
  const int32_t r = ids[beg + p];
  return (r >= 0 && static_cast<int64_t>(r) < n_rows) ? r : -1;
}

// ---- unit rows (sklearn.preprocessing.normalize inside cosine_distances) -------------------------------------------------
static __global__ __launch_bounds__(256) void ba_unit_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n_rows,
                                                                  int64_t D) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const float* s = src + r * D;
  float ss = 0.f;
  for (int64_t c = lane; c < D; c += 64) ss += s[c] * s[c];
  float nrm = sqrtf(ebn_wave_sum(ss));
  if (nrm == 0.f) nrm = 1.f;  // a zero row is divided by 1: it stays zero
  float* d = dst + r * D;
  for (int64_t c = lane; c < D; c += 64) d[c] = s[c] / nrm;
}

// ---- fast form: one wave per list of at most EBN_BA_FAST_MAX positions ------------------------------------------------------
template <bool VEC4>
static __global__ __launch_bounds__(256) void ba_intralist_fast_kernel(const float* __restrict__ unit, int64_t n_rows, int64_t D,
                                                                       const int32_t* __restrict__ ids, int64_t n_ids,
                                                                       const int64_t* __restrict__ offsets, int64_t n_lists,
                                                                       float* __restrict__ out) {
  constexpr int W = VEC4 ? 4 : 1;
  const int lane = threadIdx.x & 63;
  const int64_t l = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (l >= n_lists) return;
  int64_t beg, len64;
  ba_span(offsets, l, n_ids, beg, len64);
  if (len64 > EBN_BA_FAST_MAX) return;  // the tiled kernel owns this list
  const int len = static_cast<int>(len64);
  int row[EBN_BA_FAST_MAX];
  int nv = 0;
#pragma unroll
  for (int k = 0; k < EBN_BA_FAST_MAX; ++k) {
    row[k] = __builtin_amdgcn_readfirstlane(ba_row(ids, beg, k, len, n_rows));  // wave-uniform
    nv += row[k] >= 0;
  }
  float acc[EBN_BA_FAST_PAIRS];
#pragma unroll
  for (int p = 0; p < EBN_BA_FAST_PAIRS; ++p) acc[p] = 0.f;
  for (int64_t c0 = 0; c0 < D; c0 += 64 * W) {
    const int64_t c = c0 + lane * W;
    float v[EBN_BA_FAST_MAX][W];
#pragma unroll
    for (int k = 0; k < EBN_BA_FAST_MAX; ++k) {  // every row's slice is requested before the first is used
#pragma unroll
      for (int e = 0; e < W; ++e) v[k][e] = 0.f;
      if (row[k] >= 0 && c < D) {  // VEC4: D % 4 == 0, so c < D covers c + 3
        const float* p = unit + static_cast<int64_t>(row[k]) * D + c;
        if constexpr (VEC4) {
          const float4 q = *reinterpret_cast<const float4*>(p);
          v[k][0] = q.x, v[k][1] = q.y, v[k][2] = q.z, v[k][3] = q.w;
        } else {
          v[k][0] = p[0];
        }
      }
    }
    int p = 0;
#pragma unroll
    for (int i = 0; i < EBN_BA_FAST_MAX; ++i)
#pragma unroll
      for (int j = i + 1; j < EBN_BA_FAST_MAX; ++j, ++p)
        if (j < len) {
#pragma unroll
          for (int e = 0; e < W; ++e) acc[p] = fmaf(v[i][e], v[j][e], acc[p]);
        }
  }
  float mine = 0.f;  // lane p % 64 keeps pair p's distance: per-lane partial sums, then a tree
  int p = 0;
#pragma unroll
  for (int i = 0; i < EBN_BA_FAST_MAX; ++i)
#pragma unroll
    for (int j = i + 1; j < EBN_BA_FAST_MAX; ++j, ++p)
      if (j < len && row[i] >= 0 && row[j] >= 0) {
        const float d = ba_dist(ebn_wave_sum(acc[p]));
        if (lane == (p & 63)) mine += d;
      }
  const float tot = ebn_wave_sum(mine);
  if (lane == 0) out[l] = nv >= 2 ? 2.0f * tot / static_cast<float>(nv * (nv - 1)) : ba_nan();
}

// Fast form of the cross mean: one wave per list pair whose SHORTER side has at most EBN_BA_FAST_MAX positions (a top-10 list
// against a click history of any length).  That side's rows stay whole in registers -- NCH slabs of 256 columns, one float4 per lane
// and slab, D <= 256 NCH -- and the other side streams past them G rows at a time; lane k keeps the distances of register row k.
template <int NCH, int G>
static __global__ __launch_bounds__(256) void ba_cross_fast_kernel(const float* __restrict__ unit, int64_t n_rows, int64_t D,
                                                                   const int32_t* __restrict__ ids_r, int64_t n_ids_r,
                                                                   const int64_t* __restrict__ off_r, const int32_t* __restrict__ ids_h,
                                                                   int64_t n_ids_h, const int64_t* __restrict__ off_h, int64_t n_lists,
                                                                   float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t l = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (l >= n_lists) return;
  int64_t begA, lenA64, begB, lenB;
  ba_span(off_r, l, n_ids_r, begA, lenA64);
  ba_span(off_h, l, n_ids_h, begB, lenB);
  const int32_t* __restrict__ ids_a = ids_r;
  const int32_t* __restrict__ ids_b = ids_h;
  if (lenA64 > EBN_BA_FAST_MAX) {  // the mean is symmetric in the two sides: keep the short one in registers
    if (lenB > EBN_BA_FAST_MAX) return;  // the tiled kernel owns this pair
    const int64_t tb = begA, tl = lenA64;
    begA = begB, lenA64 = lenB, begB = tb, lenB = tl;
    ids_a = ids_h, ids_b = ids_r;
  }
  const int lenA = static_cast<int>(lenA64);
  int rowA[EBN_BA_FAST_MAX];
  float4 a[EBN_BA_FAST_MAX][NCH];
  int nA = 0;
#pragma unroll
  for (int k = 0; k < EBN_BA_FAST_MAX; ++k) {
    rowA[k] = __builtin_amdgcn_readfirstlane(ba_row(ids_a, begA, k, lenA, n_rows));
    nA += rowA[k] >= 0;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int64_t c = ch * 256 + lane * 4;
      a[k][ch] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rowA[k] >= 0 && c < D) a[k][ch] = *reinterpret_cast<const float4*>(unit + static_cast<int64_t>(rowA[k]) * D + c);
    }
  }
  float mine = 0.f;
  int64_t nB = 0;
  if (nA > 0)
    for (int64_t j0 = 0; j0 < lenB; j0 += G) {
      int rb[G];
      float4 b[G][NCH];
#pragma unroll
      for (int g = 0; g < G; ++g) {  // G rows requested before the first is used
        rb[g] = __builtin_amdgcn_readfirstlane(ba_row(ids_b, begB, j0 + g, lenB, n_rows));
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int64_t c = ch * 256 + lane * 4;
          b[g][ch] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (rb[g] >= 0 && c < D) b[g][ch] = *reinterpret_cast<const float4*>(unit + static_cast<int64_t>(rb[g]) * D + c);
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (rb[g] >= 0) {
          ++nB;
#pragma unroll
          for (int k = 0; k < EBN_BA_FAST_MAX; ++k)
            if (k < lenA && rowA[k] >= 0) {
              float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
              for (int ch = 0; ch < NCH; ++ch) {
                d0 = fmaf(a[k][ch].x, b[g][ch].x, d0), d1 = fmaf(a[k][ch].y, b[g][ch].y, d1);
                d2 = fmaf(a[k][ch].z, b[g][ch].z, d2), d3 = fmaf(a[k][ch].w, b[g][ch].w, d3);
              }
              const float d = ba_dist(ebn_wave_sum((d0 + d1) + (d2 + d3)));
              if (lane == k) mine += d;
            }
        }
    }
  const float tot = ebn_wave_sum(mine);
  if (lane == 0) out[l] = (nA > 0 && nB > 0) ? tot / static_cast<float>(nA * nB) : ba_nan();
}

// ---- general form: 16 x 16 tiles of pairs, 64-column slabs of both row sets in LDS ------------------------------------------
struct BaTileSmem {
  float sI[EBN_BA_T][EBN_BA_LD];
  float sJ[EBN_BA_T][EBN_BA_LD];
  int rI[EBN_BA_T];
  int rJ[EBN_BA_T];
};

// element e (0..3) of thread t's share of a 16 x 64 slab: VEC4 -> row t/16, columns 4(t%16)..+3 (one 16-byte load);
// otherwise elements t, t + 256, ... (row-contiguous 4-byte loads, any D and alignment)
template <bool VEC4>
static __device__ __forceinline__ void ba_slab_pos(int t, int e, int& r, int& c) {
  if (VEC4) {
    r = t >> 4, c = (t & 15) * 4 + e;
  } else {
    const int idx = t + 256 * e;
    r = idx >> 6, c = idx & 63;
  }
}

template <bool VEC4>
static __device__ __forceinline__ void ba_slab_load(const float* __restrict__ unit, int64_t D, const int* rows, int64_t c0, float (&v)[4]) {
  const int t = threadIdx.x;
  if (VEC4) {
    int r, c;
    ba_slab_pos<true>(t, 0, r, c);
    const int row = rows[r];
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row >= 0 && c0 + c < D) q = *reinterpret_cast<const float4*>(unit + static_cast<int64_t>(row) * D + c0 + c);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int r, c;
      ba_slab_pos<false>(t, e, r, c);
      const int row = rows[r];
      v[e] = (row >= 0 && c0 + c < D) ? unit[static_cast<int64_t>(row) * D + c0 + c] : 0.f;
    }
  }
}

template <bool VEC4>
static __device__ __forceinline__ void ba_slab_store(float (*s)[EBN_BA_LD], const float (&v)[4]) {
  const int t = threadIdx.x;
  if (VEC4) {
    int r, c;
    ba_slab_pos<true>(t, 0, r, c);
    *reinterpret_cast<float4*>(&s[r][c]) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int r, c;
      ba_slab_pos<false>(t, e, r, c);
      s[r][c] = v[e];
    }
  }
}

// u_i . u_j of this thread's pair (i = t / 16 of sm.rI, j = t % 16 of sm.rJ); sm.rI / sm.rJ are set and visible (a barrier has passed).
// Missing rows read as zeros.  Ends with a barrier, so the slabs may be refilled at once.
template <bool VEC4>
static __device__ __forceinline__ float ba_tile_dot(const float* __restrict__ unit, int64_t D, BaTileSmem& sm) {
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  float a4[4], b4[4];
  ba_slab_load<VEC4>(unit, D, sm.rI, 0, a4);
  ba_slab_load<VEC4>(unit, D, sm.rJ, 0, b4);
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
  for (int64_t c0 = 0; c0 < D; c0 += EBN_BA_KC) {
    ba_slab_store<VEC4>(sm.sI, a4);
    ba_slab_store<VEC4>(sm.sJ, b4);
    __syncthreads();
    if (c0 + EBN_BA_KC < D) {  // the next slab travels while this one is multiplied
      ba_slab_load<VEC4>(unit, D, sm.rI, c0 + EBN_BA_KC, a4);
      ba_slab_load<VEC4>(unit, D, sm.rJ, c0 + EBN_BA_KC, b4);
    }
#pragma unroll
    for (int k = 0; k < EBN_BA_KC; k += 4) {
      const float4 a = *reinterpret_cast<const float4*>(&sm.sI[ti][k]);
      const float4 b = *reinterpret_cast<const float4*>(&sm.sJ[tj][k]);
      d0 = fmaf(a.x, b.x, d0), d1 = fmaf(a.y, b.y, d1), d2 = fmaf(a.z, b.z, d2), d3 = fmaf(a.w, b.w, d3);
    }
    __syncthreads();
  }
  return (d0 + d1) + (d2 + d3);
}

static __device__ __forceinline__ int ba_wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// INTRA: sum over positions i != j of one list / (n (n - 1));  else: mean over R x H of a list pair.  n = VALID positions.
template <bool INTRA, bool VEC4>
static __global__ __launch_bounds__(256) void ba_tiled_kernel(const float* __restrict__ unit, int64_t n_rows, int64_t D,
                                                              const int32_t* __restrict__ ids_r, int64_t n_ids_r,
                                                              const int64_t* __restrict__ off_r, const int32_t* __restrict__ ids_h,
                                                              int64_t n_ids_h, const int64_t* __restrict__ off_h, int skip_short,
                                                              float* __restrict__ out) {
  __shared__ BaTileSmem sm;
  __shared__ float red_f[4];
  __shared__ int red_i[2][4];
  const int64_t l = blockIdx.x;
  const int t = threadIdx.x, ti = t >> 4, tj = t & 15, wave = t >> 6, lane = t & 63;
  int64_t begR, lenR, begH, lenH;
  ba_span(off_r, l, n_ids_r, begR, lenR);
  if (INTRA) {
    begH = begR, lenH = lenR;
    if (skip_short && lenR <= EBN_BA_FAST_MAX) return;  // the wave-per-list kernel owns this list (uniform over the workgroup)
  } else {
    ba_span(off_h, l, n_ids_h, begH, lenH);
    if (skip_short && (lenR <= EBN_BA_FAST_MAX || lenH <= EBN_BA_FAST_MAX)) return;  // ba_cross_fast_kernel owns this pair
  }
  int cR = 0, cH = 0;
  for (int64_t p = t; p < lenR; p += 256) cR += ba_row(ids_r, begR, p, lenR, n_rows) >= 0;
  if (!INTRA)
    for (int64_t p = t; p < lenH; p += 256) cH += ba_row(ids_h, begH, p, lenH, n_rows) >= 0;
  cR = ba_wave_sum_i(cR), cH = ba_wave_sum_i(cH);
  if (lane == 0) red_i[0][wave] = cR, red_i[1][wave] = cH;
  __syncthreads();
  const int64_t nR = (red_i[0][0] + red_i[0][1]) + (red_i[0][2] + red_i[0][3]);
  const int64_t nH = INTRA ? nR : (red_i[1][0] + red_i[1][1]) + (red_i[1][2] + red_i[1][3]);
  const bool defined = INTRA ? nR >= 2 : (nR >= 1 && nH >= 1);
  float sum = 0.f;
  if (defined) {
    for (int64_t I0 = 0; I0 < lenR; I0 += EBN_BA_T)
      for (int64_t J0 = INTRA ? I0 : 0; J0 < lenH; J0 += EBN_BA_T) {  // INTRA: the upper triangle of tiles, off-diagonal ones count twice
        __syncthreads();
        if (t < EBN_BA_T) sm.rI[t] = ba_row(ids_r, begR, I0 + t, lenR, n_rows);
        else if (t < 2 * EBN_BA_T) sm.rJ[t - EBN_BA_T] = ba_row(ids_h, begH, J0 + (t - EBN_BA_T), lenH, n_rows);
        __syncthreads();
        const float dot = ba_tile_dot<VEC4>(unit, D, sm);
        const bool on = sm.rI[ti] >= 0 && sm.rJ[tj] >= 0 && !(INTRA && I0 + ti == J0 + tj);
        if (on) sum += ((INTRA && J0 > I0) ? 2.0f : 1.0f) * ba_dist(dot);
      }
  }
  sum = ebn_wave_sum(sum);
  if (lane == 0) red_f[wave] = sum;
  __syncthreads();
  if (t == 0) {
    const float tot = (red_f[0] + red_f[1]) + (red_f[2] + red_f[3]);
    const float den = INTRA ? static_cast<float>(nR * (nR - 1)) : static_cast<float>(nR * nH);
    out[l] = defined ? tot / den : ba_nan();
  }
}

// The m x m matrix of one candidate list (IntralistDiversity._candidate_diversity): out[i, j] = clipped distance, exactly 0 on
// the diagonal of POSITIONS (cosine_distances(X, X)), NaN where either id is missing.  grid = (ceil(m/16), ceil(m/16)).
template <bool VEC4>
static __global__ __launch_bounds__(256) void ba_pairdist_kernel(const float* __restrict__ unit, int64_t n_rows, int64_t D,
                                                                 const int32_t* __restrict__ ids, int64_t m, float* __restrict__ out) {
  __shared__ BaTileSmem sm;
  const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
  const int64_t I0 = static_cast<int64_t>(blockIdx.x) * EBN_BA_T, J0 = static_cast<int64_t>(blockIdx.y) * EBN_BA_T;
  if (t < EBN_BA_T) sm.rI[t] = ba_row(ids, 0, I0 + t, m, n_rows);
  else if (t < 2 * EBN_BA_T) sm.rJ[t - EBN_BA_T] = ba_row(ids, 0, J0 + (t - EBN_BA_T), m, n_rows);
  __syncthreads();
  const float dot = ba_tile_dot<VEC4>(unit, D, sm);
  const int64_t i = I0 + ti, j = J0 + tj;
  if (i < m && j < m) out[i * m + j] = (sm.rI[ti] < 0 || sm.rJ[tj] < 0) ? ba_nan() : (i == j ? 0.0f : ba_dist(dot));
}

// ---- list means of a scalar column (Sentiment: the value; Novelty: -log2 of it) ---------------------------------------------
static __global__ __launch_bounds__(256) void ba_list_mean_kernel(const float* __restrict__ values, int64_t n_rows,
                                                                  const int32_t* __restrict__ ids, int64_t n_ids,
                                                                  const int64_t* __restrict__ offsets, int64_t n_lists, int transform,
                                                                  float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t l = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (l >= n_lists) return;
  int64_t beg, len;
  ba_span(offsets, l, n_ids, beg, len);
  float s = 0.f;
  int n = 0;
  for (int64_t p = lane; p < len; p += 64) {
    const int r = ba_row(ids, beg, p, len, n_rows);
    if (r >= 0) {
      const float v = values[r];
      s += transform ? -log2f(v) : v;
      ++n;
    }
  }
  s = ebn_wave_sum(s);
  n = ba_wave_sum_i(n);
  if (lane == 0) out[l] = n > 0 ? s / static_cast<float>(n) : ba_nan();
}

// ---- diversity of index k-tuples into an m x m distance matrix: one wave per tuple --------------------------------------------
static __global__ __launch_bounds__(256) void ba_subset_sums_kernel(const float* __restrict__ dist, int64_t m, const int32_t* __restrict__ subsets,
                                                                    int64_t k, int64_t n_subsets, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t s = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (s >= n_subsets) return;
  const int32_t* sub = subsets + s * k;
  float acc = 0.f;
  int n = 0;
  for (int64_t a = lane; a < k; a += 64) n += ba_row(sub, 0, a, k, m) >= 0;
  n = ba_wave_sum_i(n);
  for (int64_t p = lane; p < k * k; p += 64) {
    const int64_t a = p / k, b = p - a * k;
    const int ra = ba_row(sub, 0, a, k, m), rb = ba_row(sub, 0, b, k, m);
    if (a != b && ra >= 0 && rb >= 0) acc += dist[static_cast<int64_t>(ra) * m + rb];
  }
  acc = ebn_wave_sum(acc);
  if (lane == 0) out[s] = n >= 2 ? acc / static_cast<float>(static_cast<int64_t>(n) * (n - 1)) : ba_nan();
}

// ---- entry points ------------------------------------------------------------------------------------------------------------
static inline unsigned ba_blocks4(int64_t n) { return static_cast<unsigned>(ebn_ceil_div(n, 4)); }

extern "C" int ebn_ba_unit_rows_f32(const float* src, float* dst, int64_t n_rows, int64_t D, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_rows, D), EBN_ERR_BAD_ARG);
  if (n_rows == 0 || D == 0) return EBN_OK;
  EBN_REQUIRE(src != nullptr && dst != nullptr, EBN_ERR_BAD_ARG);
  EBN_LAUNCH(ba_unit_rows_kernel, dim3(ba_blocks4(n_rows)), dim3(256), 0, ebn_stream(stream), src, dst, n_rows, D);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ba_intralist_f32(const float* unit, int64_t n_rows, int64_t D, const int32_t* ids, int64_t n_ids, const int64_t* offsets,
                                    int64_t n_lists, int32_t form, float* out, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_rows, D, n_lists) && n_ids >= 0 && (form == 0 || form == 1), EBN_ERR_BAD_ARG);
  if (n_lists == 0) return EBN_OK;
  EBN_REQUIRE(D >= 1 && offsets != nullptr && out != nullptr && (ids != nullptr || n_ids == 0) && (unit != nullptr || n_rows == 0),
              EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  const bool vec4 = (D % 4 == 0) && ebn_aligned16(unit);
  if (form == 0) {
    if (vec4)
      EBN_LAUNCH(ba_intralist_fast_kernel<true>, dim3(ba_blocks4(n_lists)), dim3(256), 0, s, unit, n_rows, D, ids, n_ids, offsets, n_lists, out);
    else
      EBN_LAUNCH(ba_intralist_fast_kernel<false>, dim3(ba_blocks4(n_lists)), dim3(256), 0, s, unit, n_rows, D, ids, n_ids, offsets, n_lists, out);
    EBN_CHECK_LAUNCH();
  }
  const int skip_short = form == 0;
  if (vec4)
    EBN_LAUNCH((ba_tiled_kernel<true, true>), dim3(static_cast<unsigned>(n_lists)), dim3(256), 0, s, unit, n_rows, D, ids, n_ids, offsets, ids,
               n_ids, offsets, skip_short, out);
  else
    EBN_LAUNCH((ba_tiled_kernel<true, false>), dim3(static_cast<unsigned>(n_lists)), dim3(256), 0, s, unit, n_rows, D, ids, n_ids, offsets, ids,
               n_ids, offsets, skip_short, out);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

#ifndef EBN_BA_CROSS_G
#define EBN_BA_CROSS_G 2  // rows of the streamed side in flight per wave
#endif
template <int NCH>
static inline void ba_launch_cross_fast(hipStream_t s, const float* unit, int64_t n_rows, int64_t D, const int32_t* ids_r, int64_t n_ids_r,
                                        const int64_t* off_r, const int32_t* ids_h, int64_t n_ids_h, const int64_t* off_h, int64_t n_lists,
                                        float* out) {
  EBN_LAUNCH((ba_cross_fast_kernel<NCH, EBN_BA_CROSS_G>), dim3(ba_blocks4(n_lists)), dim3(256), 0, s, unit, n_rows, D, ids_r, n_ids_r, off_r,
             ids_h, n_ids_h, off_h, n_lists, out);
}

extern "C" int ebn_ba_cross_f32(const float* unit, int64_t n_rows, int64_t D, const int32_t* ids_r, int64_t n_ids_r, const int64_t* off_r,
                                const int32_t* ids_h, int64_t n_ids_h, const int64_t* off_h, int64_t n_lists, int32_t form, float* out,
                                ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_rows, D, n_lists) && n_ids_r >= 0 && n_ids_h >= 0 && (form == 0 || form == 1), EBN_ERR_BAD_ARG);
  if (n_lists == 0) return EBN_OK;
  EBN_REQUIRE(D >= 1 && off_r != nullptr && off_h != nullptr && out != nullptr && (ids_r != nullptr || n_ids_r == 0) &&
                  (ids_h != nullptr || n_ids_h == 0) && (unit != nullptr || n_rows == 0),
              EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  const bool vec4 = (D % 4 == 0) && ebn_aligned16(unit);
  const bool fast = form == 0 && vec4 && D <= 1024;  // the register form holds a whole row per wave: 4 slabs of 256 columns at most
  if (fast) {
    switch ((D + 255) / 256) {
      case 1: ba_launch_cross_fast<1>(s, unit, n_rows, D, ids_r, n_ids_r, off_r, ids_h, n_ids_h, off_h, n_lists, out); break;
      case 2: ba_launch_cross_fast<2>(s, unit, n_rows, D, ids_r, n_ids_r, off_r, ids_h, n_ids_h, off_h, n_lists, out); break;
      case 3: ba_launch_cross_fast<3>(s, unit, n_rows, D, ids_r, n_ids_r, off_r, ids_h, n_ids_h, off_h, n_lists, out); break;
      default: ba_launch_cross_fast<4>(s, unit, n_rows, D, ids_r, n_ids_r, off_r, ids_h, n_ids_h, off_h, n_lists, out); break;
    }
    EBN_CHECK_LAUNCH();
  }
  if (vec4)
    EBN_LAUNCH((ba_tiled_kernel<false, true>), dim3(static_cast<unsigned>(n_lists)), dim3(256), 0, s, unit, n_rows, D, ids_r, n_ids_r, off_r,
               ids_h, n_ids_h, off_h, fast ? 1 : 0, out);
  else
    EBN_LAUNCH((ba_tiled_kernel<false, false>), dim3(static_cast<unsigned>(n_lists)), dim3(256), 0, s, unit, n_rows, D, ids_r, n_ids_r, off_r,
               ids_h, n_ids_h, off_h, 0, out);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ba_pairdist_f32(const float* unit, int64_t n_rows, int64_t D, const int32_t* ids, int64_t m, float* out,
                                   ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_rows, D, m), EBN_ERR_BAD_ARG);
  if (m == 0) return EBN_OK;
  EBN_REQUIRE(D >= 1 && ids != nullptr && out != nullptr && (unit != nullptr || n_rows == 0), EBN_ERR_BAD_ARG);
  const int64_t tiles = ebn_ceil_div(m, EBN_BA_T);
  EBN_REQUIRE(tiles <= 65535, EBN_ERR_UNSUPPORTED);  // grid.y; a million candidates would be a 4 TB matrix
  const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(tiles));
  if ((D % 4 == 0) && ebn_aligned16(unit))
    EBN_LAUNCH(ba_pairdist_kernel<true>, grid, dim3(256), 0, ebn_stream(stream), unit, n_rows, D, ids, m, out);
  else
    EBN_LAUNCH(ba_pairdist_kernel<false>, grid, dim3(256), 0, ebn_stream(stream), unit, n_rows, D, ids, m, out);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ba_list_mean_f32(const float* values, int64_t n_rows, const int32_t* ids, int64_t n_ids, const int64_t* offsets,
                                    int64_t n_lists, int32_t transform, float* out, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_rows, n_lists) && n_ids >= 0 && (transform == 0 || transform == 1), EBN_ERR_BAD_ARG);
  if (n_lists == 0) return EBN_OK;
  EBN_REQUIRE(offsets != nullptr && out != nullptr && (ids != nullptr || n_ids == 0) && (values != nullptr || n_rows == 0), EBN_ERR_BAD_ARG);
  EBN_LAUNCH(ba_list_mean_kernel, dim3(ba_blocks4(n_lists)), dim3(256), 0, ebn_stream(stream), values, n_rows, ids, n_ids, offsets, n_lists,
             static_cast<int>(transform), out);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ba_subset_sums_f32(const float* dist, int64_t m, const int32_t* subsets, int64_t k, int64_t n_subsets, float* out,
                                      ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(m, k, n_subsets), EBN_ERR_BAD_ARG);
  if (n_subsets == 0) return EBN_OK;
  EBN_REQUIRE(out != nullptr && (subsets != nullptr || k == 0) && (dist != nullptr || m == 0), EBN_ERR_BAD_ARG);
  EBN_LAUNCH(ba_subset_sums_kernel, dim3(ba_blocks4(n_subsets)), dim3(256), 0, ebn_stream(stream), dist, m, subsets, k, n_subsets, out);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
