// Score blending over ragged lists (host layer: ebrec/models/ensemble.py; contract: include/ebnerd_hip.h):
//   * ebn_blend_features_f32 / ebn_blend_combine_f64: per-list transforms (raw, z-score, min-max, mid-rank, reciprocal rank) of M
//     stacked score rows, written as fp32 features or folded straight into the weighted sum;
//   * ebn_blend_sums_f64: loss, gradient and centred Hessian of the listwise softmax cross-entropy at given weights, summed over
//     all lists -- what one Newton trial of the fit needs.
// The layout is that of ebn_rankmetrics.hip: one workgroup owns BL_LPB consecutive lists and takes each in the cheapest form its
// length allows -- up to 16 items in a 16-lane group (four lists per wave), up to 32 in half a wave, up to 64 in one wave, longer
// ones (form 1: every list) with the whole workgroup over LDS tiles.  EVERY floating-point sum is taken in ONE order that does not depend on the form: a
// list's sums run over its items in ascending order (each lane walks the whole list; the lanes differ in WHAT they sum, not in
// how much of it), list l of a workgroup is added into the running sum of slot l % 16 in ascending l, a workgroup's 16 slots are
// added in ascending order into its partial, and a closing launch adds the partials.  No floating-point atomics; no contraction
// (the pragma below), so that the same expression rounds the same way in every form.
#include "ebn_common.h"

#pragma clang fp contract(off)

#define BL_LPB 256                                       // lists per workgroup
#define BL_TILE 1024                                     // features: items of one source of one list kept in LDS
#define BL_NE_MAX (1 + EBN_BL_MAX_SOURCES + EBN_BL_MAX_SOURCES * (EBN_BL_MAX_SOURCES + 1) / 2)  // loss, g, upper triangle of H
#define BL_FLAG_NONFINITE 2

struct BlLists {
  int beg[BL_LPB], len[BL_LPB];
  unsigned long long mask[4][4];  // per wave of list numbers: 16-lane, 32-lane, wave and workgroup form
};

// begin, length and form of the workgroup's lists; a list whose offsets leave [0, n_items] or run backwards is empty
static __device__ __forceinline__ void bl_prologue(BlLists& ls, const int64_t* __restrict__ offsets, int64_t n_items, int64_t n_lists, int form) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t l = static_cast<int64_t>(blockIdx.x) * BL_LPB + t;
  int beg = 0, len = 0, cls = 4;
  if (l < n_lists) {
    const int64_t o0 = offsets[l], o1 = offsets[l + 1];
    if (o0 >= 0 && o1 >= o0 && o1 <= n_items) beg = static_cast<int>(o0), len = static_cast<int>(o1 - o0);  // n_items <= INT32_MAX
    cls = form == 1 ? 3 : (len <= 16 ? 0 : (len <= 32 ? 1 : (len <= 64 ? 2 : 3)));
  }
  ls.beg[t] = beg, ls.len[t] = len;
  const unsigned long long m0 = __ballot(cls == 0), m1 = __ballot(cls == 1), m2 = __ballot(cls == 2), m3 = __ballot(cls == 3);
  if (lane == 0) ls.mask[0][wave] = m0, ls.mask[1][wave] = m1, ls.mask[2][wave] = m2, ls.mask[3][wave] = m3;
}

// ---- transforms ----------------------------------------------------------------------------------------------------------------
template <typename T>
struct BlStat {
  double sum;
  T mn, mx;
  int gt, eq;  // s_j > s_i; s_j == s_i, i itself included
  bool nonf;
};
template <typename T>
static __device__ __forceinline__ void bl_stat_init(BlStat<T>& a) {
  a.sum = 0.0, a.mn = static_cast<T>(INFINITY), a.mx = static_cast<T>(-INFINITY), a.gt = 0, a.eq = 0, a.nonf = false;
}
template <typename T>
static __device__ __forceinline__ void bl_visit(BlStat<T>& a, T si, T sj) {
  a.sum += static_cast<double>(sj);
  a.mn = sj < a.mn ? sj : a.mn, a.mx = sj > a.mx ? sj : a.mx;
  a.gt += sj > si, a.eq += sj == si;
  a.nonf |= !isfinite(sj);
}
static __device__ __forceinline__ void bl_visit_sq(double& ssq, double mean, double sj) {
  const double d = sj - mean;
  ssq += d * d;
}

// the feature of one item from its list's statistics; all arithmetic fp64, one rounding to fp32
template <typename T>
static __device__ __forceinline__ float bl_feature(int kind, double param, T s, int n, const BlStat<T>& a, double ssq) {
  const float nan = __builtin_nanf("");
  if (kind == EBN_BL_RAW) return static_cast<float>(s);
  if (a.nonf) return nan;
  const double dn = static_cast<double>(n), ds = static_cast<double>(s);
  const double r = 1.0 + static_cast<double>(a.gt) + 0.5 * static_cast<double>(a.eq - 1);  // mid-rank
  switch (kind) {
    case EBN_BL_ZSCORE: {
      const double sd = sqrt(ssq / dn);
      return (a.mx == a.mn || sd == 0.0) ? 0.f : static_cast<float>((ds - a.sum / dn) / sd);
    }
    case EBN_BL_MINMAX:
      return a.mx == a.mn ? 0.f : static_cast<float>((ds - static_cast<double>(a.mn)) / (static_cast<double>(a.mx) - static_cast<double>(a.mn)));
    case EBN_BL_RANK: return n == 1 ? 0.f : static_cast<float>((dn - r) / (dn - 1.0));
    case EBN_BL_RRF: return static_cast<float>(1.0 / (param + r));
    default: return nan;
  }
}

template <typename T>
struct BlFeatSmem {
  BlLists ls;
  int kind[EBN_BL_MAX_SOURCES];
  double param[EBN_BL_MAX_SOURCES], w[EBN_BL_MAX_SOURCES];
  T ts[BL_TILE];
};

// lists of up to GW items in aligned groups of GW lanes, one item per lane; every lane of the wave calls it
template <typename T, bool COMBINE, int GW>
static __device__ __forceinline__ void bl_feat_lanes(const BlFeatSmem<T>& sm, const T* __restrict__ scores, int64_t n_items, int M, bool mine,
                                                     int beg, int len, int64_t l, float* __restrict__ features, double* __restrict__ out,
                                                     uint8_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63, gl = lane & (GW - 1), gbase = lane & ~(GW - 1);
  const bool valid = gl < len;
  const int jn = GW == 64 ? len : GW;  // the wave form's bound is the same in every lane
  double acc = 0.0;
  bool nonf_any = false;
  for (int m = 0; m < M; ++m) {
    const T* sc = scores + static_cast<int64_t>(m) * n_items;
    const T s = valid ? sc[beg + gl] : static_cast<T>(0);
    BlStat<T> a;
    bl_stat_init(a);
    for (int j = 0; j < jn; ++j) {
      const T sj = __shfl(s, gbase + j, 64);
      if (j < len) bl_visit(a, s, sj);
    }
    const int kind = sm.kind[m];
    double ssq = 0.0;
    if (kind == EBN_BL_ZSCORE) {
      const double mean = a.sum / static_cast<double>(len);
      for (int j = 0; j < jn; ++j) {
        const T sj = __shfl(s, gbase + j, 64);
        if (j < len) bl_visit_sq(ssq, mean, static_cast<double>(sj));
      }
    }
    const float f = bl_feature(kind, sm.param[m], s, len, a, ssq);
    nonf_any |= a.nonf;
    if (COMBINE)
      acc += sm.w[m] * static_cast<double>(f);
    else if (valid)
      features[static_cast<int64_t>(m) * n_items + beg + gl] = f;
  }
  if (COMBINE && valid) out[beg + gl] = nonf_any ? __builtin_nan("") : acc;
  if (mine && gl == 0) flags[l] = nonf_any ? BL_FLAG_NONFINITE : 0;
}

// one list with the whole workgroup: item i0 + t per thread, every j from LDS tiles of BL_TILE items
template <typename T, bool COMBINE>
static __device__ void bl_feat_block(BlFeatSmem<T>& sm, const T* __restrict__ scores, int64_t n_items, int M, int beg, int n, int64_t l,
                                     float* __restrict__ features, double* __restrict__ out, uint8_t* __restrict__ flags) {
  const int t = threadIdx.x;
  bool nonf_any = false;  // every thread walks every item of every source: the same value in all of them
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + t;  // n <= INT32_MAX - 256 is checked by the entry point
    const bool valid = i < n;
    double acc = 0.0;
    for (int m = 0; m < M; ++m) {
      const T* sc = scores + static_cast<int64_t>(m) * n_items + beg;
      const T s = valid ? sc[i] : static_cast<T>(0);
      BlStat<T> a;
      bl_stat_init(a);
      for (int j0 = 0; j0 < n; j0 += BL_TILE) {
        const int tn = n - j0 < BL_TILE ? n - j0 : BL_TILE;
        __syncthreads();
        for (int j = t; j < tn; j += 256) sm.ts[j] = sc[j0 + j];
        __syncthreads();
        for (int j = 0; j < tn; ++j) bl_visit(a, s, sm.ts[j]);
      }
      const int kind = sm.kind[m];
      double ssq = 0.0;
      if (kind == EBN_BL_ZSCORE) {
        const double mean = a.sum / static_cast<double>(n);
        for (int j0 = 0; j0 < n; j0 += BL_TILE) {
          const int tn = n - j0 < BL_TILE ? n - j0 : BL_TILE;
          __syncthreads();
          for (int j = t; j < tn; j += 256) sm.ts[j] = sc[j0 + j];
          __syncthreads();
          for (int j = 0; j < tn; ++j) bl_visit_sq(ssq, mean, static_cast<double>(sm.ts[j]));
        }
      }
      const float f = bl_feature(kind, sm.param[m], s, n, a, ssq);
      nonf_any |= a.nonf;
      if (COMBINE)
        acc += sm.w[m] * static_cast<double>(f);
      else if (valid)
        features[static_cast<int64_t>(m) * n_items + beg + i] = f;
    }
    if (COMBINE && valid) out[beg + i] = nonf_any ? __builtin_nan("") : acc;
  }
  if (t == 0) flags[l] = nonf_any ? BL_FLAG_NONFINITE : 0;
}

template <typename T, bool COMBINE>
static __global__ __launch_bounds__(256) void bl_features_kernel(const T* __restrict__ scores, int M, int64_t n_items,
                                                                 const int64_t* __restrict__ offsets, int64_t n_lists,
                                                                 const int32_t* __restrict__ kinds, const double* __restrict__ params,
                                                                 const double* __restrict__ weights, int form, float* __restrict__ features,
                                                                 double* __restrict__ out, uint8_t* __restrict__ flags) {
  __shared__ BlFeatSmem<T> sm;
  const int t = threadIdx.x, wave = t >> 6;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * BL_LPB;
  bl_prologue(sm.ls, offsets, n_items, n_lists, form);
  if (t < EBN_BL_MAX_SOURCES) {
    sm.kind[t] = t < M ? kinds[t] : -1, sm.param[t] = t < M ? params[t] : 0.0;
    sm.w[t] = (COMBINE && t < M) ? weights[t] : 0.0;
  }
  __syncthreads();
  // up to 16 items: four lists per wave, one per 16-lane group
  {
    const int g = t >> 4;
    for (int it = 0; it < BL_LPB / 16; ++it) {
      if ((sm.ls.mask[0][it >> 2] >> ((it & 3) * 16) & 0xFFFFull) == 0) continue;  // none of these 16 lists takes this form (uniform)
      const int li = it * 16 + g;
      const bool mine = (sm.ls.mask[0][li >> 6] >> (li & 63)) & 1;
      bl_feat_lanes<T, COMBINE, 16>(sm, scores, n_items, M, mine, sm.ls.beg[li], mine ? sm.ls.len[li] : 0, base + li, features, out, flags);
    }
  }
  // 17 to 32 items: two of the wave's lists at a time, one per half
  for (unsigned long long m1 = sm.ls.mask[1][wave]; m1 != 0;) {
    const int first = __builtin_ctzll(m1);
    m1 &= m1 - 1;
    const int second = m1 != 0 ? __builtin_ctzll(m1) : -1;
    m1 &= m1 - 1;  // 0 stays 0
    const int pick = (t & 32) ? second : first;
    const bool mine = pick >= 0;
    const int li = wave * 64 + (mine ? pick : first);
    bl_feat_lanes<T, COMBINE, 32>(sm, scores, n_items, M, mine, sm.ls.beg[li], mine ? sm.ls.len[li] : 0, base + li, features, out, flags);
  }
  // 33 to 64 items: one wave per list
  for (unsigned long long m2 = sm.ls.mask[2][wave]; m2 != 0; m2 &= m2 - 1) {
    const int li = wave * 64 + __builtin_ctzll(m2);
    bl_feat_lanes<T, COMBINE, 64>(sm, scores, n_items, M, true, sm.ls.beg[li], sm.ls.len[li], base + li, features, out, flags);
  }
  // longer lists (form 1: every list): the whole workgroup
  for (int w = 0; w < 4; ++w)
    for (unsigned long long m2 = sm.ls.mask[3][w]; m2 != 0; m2 &= m2 - 1) {
      const int li = w * 64 + __builtin_ctzll(m2);
      bl_feat_block<T, COMBINE>(sm, scores, n_items, M, sm.ls.beg[li], sm.ls.len[li], base + li, features, out, flags);
    }
}

// ---- sums of the listwise softmax cross-entropy ------------------------------------------------------------------------------------
#define BL_FLD 65    // row stride of a wave's [16][64] feature tile in LDS: lanes a = 0..15 read rows a at one column
#define BL_FLDB 257  // the same for the workgroup form's [16][256] tile

struct BlSumSmem {
  BlLists ls;
  double w[EBN_BL_MAX_SOURCES];
  float F[4 * EBN_BL_MAX_SOURCES * BL_FLD];  // wave w: F + w * 16 * BL_FLD, [m][lane]; workgroup form: [m][t] at stride BL_FLDB
  double P[256], D[256], LP[256];           // p_i (first e_i), p_i - t_i, y_i log p_i: wave w at [w * 64 + lane], workgroup form at [t]
  double acc[16][BL_NE_MAX];                // slot s: the running sums of the lists l % 16 == s
  long long cnt[16][3];
  double ub[EBN_BL_MAX_SOURCES];
  double red[4];
  int redi[4][2];
};
static_assert(4 * EBN_BL_MAX_SOURCES * BL_FLD >= EBN_BL_MAX_SOURCES * BL_FLDB, "the workgroup form's tile fits the four waves' tiles");

// lanes of one wave that exchange data through LDS: order the accesses, no workgroup barrier
static __device__ __forceinline__ void bl_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

static __device__ __forceinline__ int bl_tri(int M, int a, int b) { return 1 + M + a * M - a * (a - 1) / 2 + (b - a); }  // a <= b

// an item's features, label, z = w . f (m ascending) and whether a feature is not finite
static __device__ __forceinline__ void bl_item_load(const BlSumSmem& sm, const float* __restrict__ feat, const uint8_t* __restrict__ labels,
                                                    int64_t n_items, int M, bool valid, int pos, float (&f)[EBN_BL_MAX_SOURCES], int& y,
                                                    double& z, bool& nf) {
  y = valid ? (labels[pos] != 0) : 0;
  z = 0.0, nf = false;
#pragma unroll
  for (int m = 0; m < EBN_BL_MAX_SOURCES; ++m) {
    f[m] = (valid && m < M) ? feat[static_cast<int64_t>(m) * n_items + pos] : 0.f;
    if (m < M) z += sm.w[m] * static_cast<double>(f[m]), nf |= !isfinite(f[m]);
  }
}

// a list of up to GW items in an aligned group of GW lanes (16, 32 or 64).  Phase 1, lane = item: z, the softmax, p - t and the features into the
// wave's LDS tile.  Phase 2, lane = (a = gl % 16, q = gl / 16): row a of g, u and H, columns [q NB, (q + 1) NB), item by item.
template <int GW>
static __device__ __forceinline__ void bl_sums_lanes(BlSumSmem& sm, const float* __restrict__ feat, const uint8_t* __restrict__ labels,
                                                     int64_t n_items, int M, bool mine, int beg, int len, int slot) {
  constexpr int NB = 16 / (GW / 16);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gl = lane & (GW - 1), gbase = lane & ~(GW - 1);
  const bool valid = gl < len;
  float f[EBN_BL_MAX_SOURCES];
  int y;
  double z;
  bool nf;
  bl_item_load(sm, feat, labels, n_items, M, valid, beg + gl, f, y, z, nf);
  int packed = (y ? 1 : 0) | (nf ? 1 << 8 : 0);  // each count <= 64
  double zmax = valid ? z : -INFINITY;
#pragma unroll
  for (int off = GW / 2; off > 0; off >>= 1) {
    packed += __shfl_xor(packed, off, 64);
    zmax = fmax(zmax, __shfl_xor(zmax, off, 64));
  }
  const int np = packed & 255;
  const bool bad = (packed >> 8) != 0, one = !(np > 0 && np < len);
  if (mine && gl == 0) sm.cnt[slot][one ? 1 : (bad ? 2 : 0)] += 1;
  if (!mine || one || bad) return;  // the same in every lane of the group

  float* F = sm.F + wave * (EBN_BL_MAX_SOURCES * BL_FLD);
  double *P = sm.P + wave * 64 + gbase, *D = sm.D + wave * 64 + gbase, *LP = sm.LP + wave * 64 + gbase;
  const double e = valid ? exp(z - zmax) : 0.0;
  P[gl] = e;
  bl_wave_sync();
  double S = 0.0;
  for (int j = 0; j < len; ++j) S += P[j];
  bl_wave_sync();
  const double logS = log(S), p = e / S;
  P[gl] = p, D[gl] = p - (y ? 1.0 / static_cast<double>(np) : 0.0), LP[gl] = y ? (z - zmax) - logS : 0.0;
#pragma unroll
  for (int m = 0; m < EBN_BL_MAX_SOURCES; ++m)
    if (m < M) F[m * BL_FLD + lane] = f[m];
  bl_wave_sync();

  const int a = gl & 15, q = gl >> 4;
  const float* Fa = F + (a < M ? a : 0) * BL_FLD + gbase;
  double u = 0.0, g = 0.0;
  for (int i = 0; i < len; ++i) {
    const double fa = static_cast<double>(Fa[i]);
    u += P[i] * fa, g += D[i] * fa;
  }
  double ub[NB], H[NB];
#pragma unroll
  for (int bb = 0; bb < NB; ++bb) ub[bb] = __shfl(u, gbase + q * NB + bb, 64), H[bb] = 0.0;  // lane (a = q NB + bb, q = 0) holds u_b
  for (int i = 0; i < len; ++i) {
    const double ca = P[i] * (static_cast<double>(Fa[i]) - u);
#pragma unroll
    for (int bb = 0; bb < NB; ++bb)
      if (q * NB + bb < M) H[bb] += ca * (static_cast<double>(F[(q * NB + bb) * BL_FLD + gbase + i]) - ub[bb]);
  }
  double* acc = sm.acc[slot];
  if (a < M) {
    if (q == 0) acc[1 + a] += g;
#pragma unroll
    for (int bb = 0; bb < NB; ++bb) {
      const int b = q * NB + bb;
      if (b < M && b >= a) acc[bl_tri(M, a, b)] += H[bb];
    }
  }
  if (gl == 0) {
    double ls = 0.0;
    for (int i = 0; i < len; ++i) ls += LP[i];
    acc[0] += -(ls / static_cast<double>(np));
  }
  bl_wave_sync();  // the tile is free for the wave's next list
}

// one list with the whole workgroup, 256 items per tile: thread (a = t / 16, b = t % 16) owns H_ab, the threads b == 0 own g_a, every
// thread of row a sums u_a; the same expressions in the same item order as bl_sums_lanes
static __device__ void bl_sums_block(BlSumSmem& sm, const float* __restrict__ feat, const uint8_t* __restrict__ labels, int64_t n_items, int M,
                                     int beg, int n, int slot) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, a = t >> 4, b = t & 15;
  float f[EBN_BL_MAX_SOURCES];
  int y;
  double z;
  bool nf;
  // pass 1: the largest z, the positives, a feature that is not finite (none of them depends on an order)
  double zmax = -INFINITY;
  int npT = 0, nfT = 0;
  for (int i = t; i < n; i += 256) {
    bl_item_load(sm, feat, labels, n_items, M, true, beg + i, f, y, z, nf);
    zmax = fmax(zmax, z), npT += y, nfT += nf;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    zmax = fmax(zmax, __shfl_xor(zmax, off, 64));
    npT += __shfl_xor(npT, off, 64), nfT += __shfl_xor(nfT, off, 64);
  }
  if (lane == 0) sm.red[wave] = zmax, sm.redi[wave][0] = npT, sm.redi[wave][1] = nfT;
  __syncthreads();
  zmax = fmax(fmax(sm.red[0], sm.red[1]), fmax(sm.red[2], sm.red[3]));
  const int np = sm.redi[0][0] + sm.redi[1][0] + sm.redi[2][0] + sm.redi[3][0];
  const bool bad = (sm.redi[0][1] + sm.redi[1][1] + sm.redi[2][1] + sm.redi[3][1]) != 0, one = !(np > 0 && np < n);
  if (t == 0) sm.cnt[slot][one ? 1 : (bad ? 2 : 0)] += 1;
  __syncthreads();  // sm.red is free
  if (one || bad) return;
  // pass 2: S = sum_i exp(z_i - zmax), i ascending
  double S = 0.0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int tn = n - i0 < 256 ? n - i0 : 256;
    bl_item_load(sm, feat, labels, n_items, M, t < tn, beg + i0 + t, f, y, z, nf);
    sm.P[t] = t < tn ? exp(z - zmax) : 0.0;
    __syncthreads();
    for (int j = 0; j < tn; ++j) S += sm.P[j];
    __syncthreads();
  }
  const double logS = log(S);
  // pass 3: u_a, g_a, the loss
  const float* Fa = sm.F + (a < M ? a : 0) * BL_FLDB;
  double u = 0.0, g = 0.0, ls = 0.0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int tn = n - i0 < 256 ? n - i0 : 256;
    bl_item_load(sm, feat, labels, n_items, M, t < tn, beg + i0 + t, f, y, z, nf);
    const double e = t < tn ? exp(z - zmax) : 0.0, p = e / S;
    sm.P[t] = p, sm.D[t] = p - (y ? 1.0 / static_cast<double>(np) : 0.0), sm.LP[t] = y ? (z - zmax) - logS : 0.0;
#pragma unroll
    for (int m = 0; m < EBN_BL_MAX_SOURCES; ++m)
      if (m < M) sm.F[m * BL_FLDB + t] = f[m];
    __syncthreads();
    for (int j = 0; j < tn; ++j) {
      const double fa = static_cast<double>(Fa[j]);
      u += sm.P[j] * fa, g += sm.D[j] * fa;
    }
    if (t == 0)
      for (int j = 0; j < tn; ++j) ls += sm.LP[j];
    __syncthreads();
  }
  if (b == 0) sm.ub[a] = u;
  __syncthreads();
  const double ubb = sm.ub[b];
  // pass 4: H_ab = sum_i p_i (f_ia - u_a) (f_ib - u_b)
  const bool own = a < M && b < M && b >= a;
  const float* Fb = sm.F + (b < M ? b : 0) * BL_FLDB;
  double H = 0.0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int tn = n - i0 < 256 ? n - i0 : 256;
    bl_item_load(sm, feat, labels, n_items, M, t < tn, beg + i0 + t, f, y, z, nf);
    const double e = t < tn ? exp(z - zmax) : 0.0;
    sm.P[t] = e / S;
#pragma unroll
    for (int m = 0; m < EBN_BL_MAX_SOURCES; ++m)
      if (m < M) sm.F[m * BL_FLDB + t] = f[m];
    __syncthreads();
    if (own)
      for (int j = 0; j < tn; ++j) {
        const double ca = sm.P[j] * (static_cast<double>(Fa[j]) - u);
        H += ca * (static_cast<double>(Fb[j]) - ubb);
      }
    __syncthreads();
  }
  double* acc = sm.acc[slot];
  if (a < M && b == 0) acc[1 + a] += g;
  if (own) acc[bl_tri(M, a, b)] += H;
  if (t == 0) acc[0] += -(ls / static_cast<double>(np));
}

// three workgroups per CU is what the LDS allows: ask for the registers to allow it too (168 instead of 192, nothing spilled)
static __global__ __launch_bounds__(256, 3) void bl_sums_kernel(const float* __restrict__ feat, const uint8_t* __restrict__ labels, int M,
                                                             int64_t n_items, const int64_t* __restrict__ offsets, int64_t n_lists,
                                                             const double* __restrict__ weights, int form, int n_e,
                                                             double* __restrict__ part_sums, long long* __restrict__ part_cnt) {
  __shared__ BlSumSmem sm;
  const int t = threadIdx.x, wave = t >> 6, g = t >> 4;
  bl_prologue(sm.ls, offsets, n_items, n_lists, form);
  if (t < EBN_BL_MAX_SOURCES) sm.w[t] = t < M ? weights[t] : 0.0;
  for (int k = t; k < 16 * BL_NE_MAX; k += 256) sm.acc[k / BL_NE_MAX][k % BL_NE_MAX] = 0.0;
  if (t < 48) sm.cnt[t / 3][t % 3] = 0;
  __syncthreads();
  // round `it` holds the lists it * 16 + s, s = 0..15: one per slot, so that slot s sums its lists in ascending order whatever form
  // each takes.  Wave w owns the slots 4 w .. 4 w + 3 in the group and wave forms.
  for (int it = 0; it < BL_LPB / 16; ++it) {
    const int sh = (it & 3) * 16;
    const unsigned r0 = static_cast<unsigned>(sm.ls.mask[0][it >> 2] >> sh) & 0xFFFFu, r1 = static_cast<unsigned>(sm.ls.mask[1][it >> 2] >> sh) & 0xFFFFu,
                   r2 = static_cast<unsigned>(sm.ls.mask[2][it >> 2] >> sh) & 0xFFFFu, r3 = static_cast<unsigned>(sm.ls.mask[3][it >> 2] >> sh) & 0xFFFFu;
    if ((r0 >> (wave * 4)) & 0xFu) {
      const int li = it * 16 + g;
      const bool mine = (r0 >> g) & 1;
      bl_sums_lanes<16>(sm, feat, labels, n_items, M, mine, sm.ls.beg[li], mine ? sm.ls.len[li] : 0, g);
    }
    for (unsigned m1 = (r1 >> (wave * 4)) & 0xFu; m1 != 0;) {  // two of the wave's lists at a time, one per half
      const int first = __builtin_ctz(m1);
      m1 &= m1 - 1;
      const int second = m1 != 0 ? __builtin_ctz(m1) : -1;
      m1 &= m1 - 1;  // 0 stays 0
      const int pick = (t & 32) ? second : first;
      const bool mine = pick >= 0;
      const int s = wave * 4 + (mine ? pick : first), li = it * 16 + s;
      bl_sums_lanes<32>(sm, feat, labels, n_items, M, mine, sm.ls.beg[li], mine ? sm.ls.len[li] : 0, s);
    }
    for (unsigned m2 = (r2 >> (wave * 4)) & 0xFu; m2 != 0; m2 &= m2 - 1) {
      const int s = wave * 4 + __builtin_ctz(m2), li = it * 16 + s;
      bl_sums_lanes<64>(sm, feat, labels, n_items, M, true, sm.ls.beg[li], sm.ls.len[li], s);
    }
    if (r3 != 0) {  // the same in every thread of the workgroup
      __syncthreads();
      for (unsigned m2 = r3; m2 != 0; m2 &= m2 - 1) {
        const int s = __builtin_ctz(m2), li = it * 16 + s;
        bl_sums_block(sm, feat, labels, n_items, M, sm.ls.beg[li], sm.ls.len[li], s);
        __syncthreads();
      }
    }
  }
  __syncthreads();
  if (t < n_e) {
    double v = 0.0;
    for (int s = 0; s < 16; ++s) v += sm.acc[s][t];
    part_sums[static_cast<int64_t>(blockIdx.x) * n_e + t] = v;
  } else if (t >= 192 && t < 195) {
    long long c = 0;
    for (int s = 0; s < 16; ++s) c += sm.cnt[s][t - 192];
    part_cnt[static_cast<int64_t>(blockIdx.x) * 3 + (t - 192)] = c;
  }
}

// closing pass: workgroup e sums entry e (e >= n_e: counter e - n_e) of the workgroups' partials, thread t over the partials
// t, t + 256, ... in ascending order, then the 256 threads' sums in ascending order
static __global__ __launch_bounds__(256) void bl_close_kernel(const double* __restrict__ part_sums, const long long* __restrict__ part_cnt,
                                                              int64_t n_blocks, int n_e, double* __restrict__ sums, int64_t* __restrict__ counters) {
  __shared__ double red[256];
  __shared__ long long redc[256];
  const int e = blockIdx.x, t = threadIdx.x;
  double v = 0.0;
  long long c = 0;
  if (e < n_e)
    for (int64_t b = t; b < n_blocks; b += 256) v += part_sums[b * n_e + e];
  else
    for (int64_t b = t; b < n_blocks; b += 256) c += part_cnt[b * 3 + (e - n_e)];
  red[t] = v, redc[t] = c;
  __syncthreads();
  if (t != 0) return;
  v = 0.0, c = 0;
  for (int k = 0; k < 256; ++k) v += red[k], c += redc[k];
  if (e < n_e)
    sums[e] = v;
  else
    counters[e - n_e] = c;
}

// ---- entry points ------------------------------------------------------------------------------------------------------------
static inline int64_t bl_blocks(int64_t n_lists) { return ebn_ceil_div(n_lists, BL_LPB); }
static inline int bl_entries(int M) { return 1 + M + M * (M + 1) / 2; }
// items are addressed with 32-bit positions inside a list; the workgroup form steps past the end by up to 255
static inline bool bl_sizes_ok(int64_t n_items, int64_t n_lists, int32_t M) {
  return ebn_dim_ok(n_items, n_lists) && n_items <= EBN_DIM_MAX - 256 && M >= 1 && M <= EBN_BL_MAX_SOURCES;
}

template <bool COMBINE>
static int bl_features_launch(const void* scores, int32_t score_kind, int32_t M, int64_t n_items, const int64_t* offsets, int64_t n_lists,
                              const int32_t* kinds, const double* params, const double* weights, int32_t form, float* features, double* out,
                              uint8_t* flags, ebn_stream_t stream) {
  EBN_REQUIRE(bl_sizes_ok(n_items, n_lists, M) && (form == 0 || form == 1) && (score_kind == EBN_RM_F32 || score_kind == EBN_RM_F64),
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE(offsets != nullptr && flags != nullptr && kinds != nullptr && params != nullptr && (!COMBINE || weights != nullptr) &&
                  ((scores != nullptr && (COMBINE ? static_cast<const void*>(out) : static_cast<const void*>(features)) != nullptr) || n_items == 0),
              EBN_ERR_BAD_ARG);
  if (n_lists == 0) return EBN_OK;
  const dim3 grid(static_cast<unsigned>(bl_blocks(n_lists)));
  hipStream_t s = ebn_stream(stream);
  if (score_kind == EBN_RM_F32)
    EBN_LAUNCH((bl_features_kernel<float, COMBINE>), grid, dim3(256), 0, s, static_cast<const float*>(scores), M, n_items, offsets, n_lists, kinds,
               params, weights, form, features, out, flags);
  else
    EBN_LAUNCH((bl_features_kernel<double, COMBINE>), grid, dim3(256), 0, s, static_cast<const double*>(scores), M, n_items, offsets, n_lists, kinds,
               params, weights, form, features, out, flags);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_blend_features_f32(const void* scores, int32_t score_kind, int32_t M, int64_t n_items, const int64_t* offsets, int64_t n_lists,
                                      const int32_t* kinds, const double* params, int32_t form, float* features, uint8_t* flags,
                                      ebn_stream_t stream) {
  return bl_features_launch<false>(scores, score_kind, M, n_items, offsets, n_lists, kinds, params, nullptr, form, features, nullptr, flags, stream);
}

extern "C" int ebn_blend_combine_f64(const void* scores, int32_t score_kind, int32_t M, int64_t n_items, const int64_t* offsets, int64_t n_lists,
                                     const int32_t* kinds, const double* params, const double* weights, int32_t form, double* out, uint8_t* flags,
                                     ebn_stream_t stream) {
  return bl_features_launch<true>(scores, score_kind, M, n_items, offsets, n_lists, kinds, params, weights, form, nullptr, out, flags, stream);
}

extern "C" int64_t ebn_blend_sums_workspace_bytes(int64_t n_lists, int32_t M) {
  if (!ebn_dim_ok(n_lists) || M < 1 || M > EBN_BL_MAX_SOURCES) return 0;
  return bl_blocks(n_lists) * (bl_entries(M) + 3) * static_cast<int64_t>(sizeof(double));
}

extern "C" int ebn_blend_sums_f64(const float* features, const uint8_t* labels, int32_t M, int64_t n_items, const int64_t* offsets, int64_t n_lists,
                                  const double* weights, int32_t form, double* sums, int64_t* counters, void* workspace, int64_t workspace_bytes,
                                  ebn_stream_t stream) {
  EBN_REQUIRE(bl_sizes_ok(n_items, n_lists, M) && (form == 0 || form == 1), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(sums != nullptr && counters != nullptr && weights != nullptr, EBN_ERR_BAD_ARG);
  const int64_t blocks = bl_blocks(n_lists);
  const int n_e = bl_entries(M);
  if (n_lists > 0) {
    EBN_REQUIRE(offsets != nullptr && workspace != nullptr && ((features != nullptr && labels != nullptr) || n_items == 0), EBN_ERR_BAD_ARG);
    EBN_REQUIRE(workspace_bytes >= ebn_blend_sums_workspace_bytes(n_lists, M) && ebn_aligned16(workspace), EBN_ERR_BAD_ARG);
  }
  double* part_sums = static_cast<double*>(workspace);
  long long* part_cnt = reinterpret_cast<long long*>(part_sums + blocks * n_e);
  hipStream_t s = ebn_stream(stream);
  if (n_lists > 0) {
    EBN_LAUNCH(bl_sums_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, features, labels, M, n_items, offsets, n_lists, weights, form, n_e,
               part_sums, part_cnt);
    EBN_CHECK_LAUNCH();
  }
  EBN_LAUNCH(bl_close_kernel, dim3(static_cast<unsigned>(n_e + 3)), dim3(256), 0, s, part_sums, part_cnt, blocks, n_e, sums, counters);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
