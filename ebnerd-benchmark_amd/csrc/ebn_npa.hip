// NPA (reference npa.py:120-136, layers.py:312-339): the CNN title encoder as an implicit GEMM on the exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32), and PersonalizedAttentivePooling.
//
// Conv1D(F, window, relu, padding="same") over the gathered tokens X[R = n_titles * T, E] (row-major, titles contiguous):
//   Y[r, f] = b[f] + sum_{j < window} sum_e X[r + j - pad, e] * W[j * E + e, f]       pad = (window - 1) / 2
// where a tap that leaves the title of row r reads zero.  The A operand row of token r is the window of rows r - pad ..
// r + window - 1 - pad of X itself -- no im2col image, no padded copy: the tile loader maps the contraction index k = (j, e)
// to (row r + j - pad, column e) and zero-fills the taps outside the title.  Three products, one kernel template:
//   MODE 0  forward        C[R, F]          = A(X) . W                   epilogue: bias, ReLU, Dropout(p) and PAP's Dropout(0.2)
//   MODE 1  backward-data  C[R, E]          = A(dY') . W^T (taps reversed: row r + pad - j)
//   MODE 2  backward-weight C[window*E + 1, F] = A(X)^T . dY'           the extra row = column sums of dY' (the bias gradient),
//                                                                       as deterministic split-K slices over the R rows
// dY' = d(pre-activation) is not stored: it is derived while the operand is fetched from the forward's one output Vd and its
// gradient dVd.  Vd = relu(pre) * m1 / (1 - p) * m2 / (1 - 0.2) is > 0 exactly where the ReLU passes AND both dropout masks
// keep, so dY' = dVd * 1/(1-p) * 1/(1-0.2) where Vd > 0, else 0 -- no mask is recomputed in the backward.
//
// Block tile 128 x 128 x 16, 4 waves as 2 x 2, each wave 64 x 64 in four 32 x 32 MFMA tiles.  Both operands are staged
// through registers into [k][mn] LDS images (the window mapping and the zero taps are per-element selects on the loaded
// float4: no direct-to-LDS fetch), double-buffered with one barrier per 16-deep slab.
#include "ebn_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CV_BM = 128, CV_BN = 128, CV_BK = 16, CV_PAD = 4, CV_THREADS = 256;
constexpr int CV_LD = CV_BM + CV_PAD;            // LDS row stride (floats) of both images
constexpr int CV_PER_THREAD = CV_BM * CV_BK / 4 / CV_THREADS;  // float4 per operand and thread: 2

struct ConvArgs {
  const float* X;    // MODE 0 / 2: gathered tokens [R, E]
  const float* W;    // MODE 0 / 1: kernel [window * E, F]
  const float* G;    // MODE 1 / 2: dVd [R, F]
  const float* Vd;   // MODE 1 / 2: forward output [R, F] (the gate)
  const float* bias; // MODE 0
  float* out;        // MODE 0: Vd; MODE 1: dX [R, E]; MODE 2: slices [splits][window*E + 1][F]
  int64_t R;
  int32_t T, E, F, window, pad;
  float gscale;      // MODE 1 / 2: 1/(1-p) * 1/(1-0.2) of the dropouts that were active
  EbnDrop d1, d2;    // MODE 0: conv-output dropout, PAP-input dropout
  int64_t k_per_split;
};

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// 4 consecutive floats at P + off when `ok`, zeros otherwise; the load itself is unconditional (offset 0 is always valid)
__device__ __forceinline__ float4 load4_or_zero(const float* __restrict__ P, int64_t off, bool ok) {
  const float4 v = *reinterpret_cast<const float4*>(P + (ok ? off : 0));
  return ok ? v : f4_zero();
}

// dY' from (dVd, Vd): the ReLU + both dropouts gate
__device__ __forceinline__ float4 gated4(const ConvArgs& a, int64_t off, bool ok) {
  const float4 g = load4_or_zero(a.G, off, ok);
  const float4 v = load4_or_zero(a.Vd, off, ok);
  float4 r;
  r.x = v.x > 0.f ? g.x * a.gscale : 0.f;
  r.y = v.y > 0.f ? g.y * a.gscale : 0.f;
  r.z = v.z > 0.f ? g.z * a.gscale : 0.f;
  r.w = v.w > 0.f ? g.w * a.gscale : 0.f;
  return r;
}

// (tap, channel) of contraction index k with channel extent C
__device__ __forceinline__ void tap_of(int64_t k, int32_t C, int32_t& j, int32_t& c) {
  j = static_cast<int32_t>(k / C);
  c = static_cast<int32_t>(k - static_cast<int64_t>(j) * C);
}

template <int MODE>
__device__ __forceinline__ int64_t dim_m(const ConvArgs& a) {
  return MODE == 2 ? static_cast<int64_t>(a.window) * a.E + 1 : a.R;
}
template <int MODE>
__device__ __forceinline__ int64_t dim_n(const ConvArgs& a) {
  return MODE == 1 ? a.E : a.F;
}
template <int MODE>
__device__ __forceinline__ int64_t dim_k(const ConvArgs& a) {
  return MODE == 0 ? static_cast<int64_t>(a.window) * a.E : (MODE == 1 ? static_cast<int64_t>(a.window) * a.F : a.R);
}

// A operand, float4 slot v of the slab at k0.  MODE 0 / 1: k-contiguous (row m = v / 4, k = k0 + 4 (v % 4)); MODE 2:
// m-contiguous (k = k0 + v / 32, m = m0 + 4 (v % 32)).
template <int MODE>
__device__ __forceinline__ float4 load_a(const ConvArgs& a, int64_t m0, int64_t k0, int64_t kend, int v) {
  const int64_t M = dim_m<MODE>(a);
  if (MODE == 0 || MODE == 1) {
    const int64_t r = m0 + (v >> 2), k = k0 + 4 * (v & 3);
    const int32_t C = MODE == 0 ? a.E : a.F;
    int32_t j, c;
    tap_of(k, C, j, c);
    const int32_t t = static_cast<int32_t>(r % a.T);
    const int32_t shift = MODE == 0 ? j - a.pad : a.pad - j;  // source row offset of this tap
    const bool ok = r < M && k < kend && t + shift >= 0 && t + shift < a.T;
    const int64_t off = (r + shift) * C + c;
    return MODE == 0 ? load4_or_zero(a.X, off, ok) : gated4(a, off, ok);
  } else {
    const int64_t r = k0 + (v >> 5), m = m0 + 4 * (v & 31);
    const int64_t WE = static_cast<int64_t>(a.window) * a.E;
    if (m >= WE) {  // the bias row (m == WE): a column of ones; beyond it nothing
      float4 o = f4_zero();
      o.x = (m == WE && r < kend) ? 1.f : 0.f;
      return o;
    }
    int32_t j, c;
    tap_of(m, a.E, j, c);
    const int32_t t = static_cast<int32_t>(r % a.T);
    const int32_t shift = j - a.pad;
    const bool ok = r < kend && t + shift >= 0 && t + shift < a.T;
    return load4_or_zero(a.X, (r + shift) * a.E + c, ok);
  }
}

// B operand.  MODE 0 / 2: n-contiguous (k = k0 + v / 32, n = n0 + 4 (v % 32)); MODE 1: k-contiguous (n = n0 + v / 4,
// k = k0 + 4 (v % 4)), B[k = (j, f)][n = e] = W[(j * E + e) * F + f].
template <int MODE>
__device__ __forceinline__ float4 load_b(const ConvArgs& a, int64_t n0, int64_t k0, int64_t kend, int v) {
  const int64_t N = dim_n<MODE>(a);
  if (MODE == 1) {
    const int64_t n = n0 + (v >> 2), k = k0 + 4 * (v & 3);
    int32_t j, f;
    tap_of(k, a.F, j, f);
    const bool ok = n < N && k < kend;
    return load4_or_zero(a.W, (static_cast<int64_t>(j) * a.E + n) * a.F + f, ok);
  } else {
    const int64_t k = k0 + (v >> 5), n = n0 + 4 * (v & 31);
    const bool ok = n < N && k < kend;
    const int64_t off = k * a.F + n;
    return MODE == 0 ? load4_or_zero(a.W, off, ok) : gated4(a, off, ok);
  }
}

// LDS image S[k][mn]: k-contiguous float4 -> four scalar stores down a column, mn-contiguous -> one float4 store
template <bool KCONTIG>
__device__ __forceinline__ void store_tile(float* __restrict__ S, int v, float4 r) {
  if (KCONTIG) {
    const int mn = v >> 2, k = 4 * (v & 3);
    S[(k + 0) * CV_LD + mn] = r.x;
    S[(k + 1) * CV_LD + mn] = r.y;
    S[(k + 2) * CV_LD + mn] = r.z;
    S[(k + 3) * CV_LD + mn] = r.w;
  } else {
    const int k = v >> 5, mn = 4 * (v & 31);
    *reinterpret_cast<float4*>(&S[k * CV_LD + mn]) = r;
  }
}

template <int MODE>
__global__ __launch_bounds__(CV_THREADS) void conv_gemm_kernel(ConvArgs a) {
  constexpr bool A_KC = MODE != 2, B_KC = MODE == 1;
  constexpr int TILE = CV_BK * CV_LD;
  __shared__ __attribute__((aligned(16))) float smem[4 * TILE];  // [buf][A | B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int kl = lane >> 5, il = lane & 31;
  const int64_t M = dim_m<MODE>(a), N = dim_n<MODE>(a), K = dim_k<MODE>(a);
  const int64_t m0 = static_cast<int64_t>(blockIdx.y) * CV_BM, n0 = static_cast<int64_t>(blockIdx.x) * CV_BN;
  const int64_t kbeg = MODE == 2 ? static_cast<int64_t>(blockIdx.z) * a.k_per_split : 0;
  const int64_t kend = MODE == 2 ? (kbeg + a.k_per_split < K ? kbeg + a.k_per_split : K) : K;
  const int nk = kend > kbeg ? static_cast<int>((kend - kbeg + CV_BK - 1) / CV_BK) : 0;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[CV_PER_THREAD], rb[CV_PER_THREAD];
  auto fetch = [&](int kt) {
    const int64_t k0 = kbeg + static_cast<int64_t>(kt) * CV_BK;
#pragma unroll
    for (int i = 0; i < CV_PER_THREAD; ++i) {
      ra[i] = load_a<MODE>(a, m0, k0, kend, tid + i * CV_THREADS);
      rb[i] = load_b<MODE>(a, n0, k0, kend, tid + i * CV_THREADS);
    }
  };
  auto stash = [&](int buf) {
    float* As = smem + buf * 2 * TILE;
    float* Bs = As + TILE;
#pragma unroll
    for (int i = 0; i < CV_PER_THREAD; ++i) {
      store_tile<A_KC>(As, tid + i * CV_THREADS, ra[i]);
      store_tile<B_KC>(Bs, tid + i * CV_THREADS, rb[i]);
    }
  };
  if (nk > 0) {
    fetch(0);
    stash(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) fetch(kt + 1);
    const float* As = smem + cur * 2 * TILE + wm * 64 + il;
    const float* Bs = smem + cur * 2 * TILE + TILE + wn * 64 + il;
#pragma unroll
    for (int s = 0; s < CV_BK / 2; ++s) {
      const int k = 2 * s + kl;  // MFMA 32x32x2: lane half kl supplies contraction index kl of the step
      const float a0 = As[k * CV_LD], a1 = As[k * CV_LD + 32];
      const float b0 = Bs[k * CV_LD], b1 = Bs[k * CV_LD + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (kt + 1 < nk) stash(cur ^ 1);
    __syncthreads();
  }

  // epilogue; C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const bool drop1 = MODE == 0 && a.d1.key_ptr != nullptr, drop2 = MODE == 0 && a.d2.key_ptr != nullptr;
  const uint32_t key1 = drop1 ? *a.d1.key_ptr : 0u, key2 = drop2 ? *a.d2.key_ptr : 0u;
  float* out = MODE == 2 ? a.out + static_cast<int64_t>(blockIdx.z) * M * N : a.out;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t col = n0 + wn * 64 + j * 32 + il;
      if (col >= N) continue;
      const float bv = MODE == 0 ? a.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
        if (row >= M) continue;
        float v = acc[i][j][r];
        if (MODE == 0) {
          v = fmaxf(v + bv, 0.f);
          const uint64_t idx = static_cast<uint64_t>(row) * static_cast<uint64_t>(N) + static_cast<uint64_t>(col);
          if (drop1) v *= ebn_drop_mult(key1, idx, a.d1.thresh, a.d1.scale);
          if (drop2) v *= ebn_drop_mult(key2, idx, a.d2.thresh, a.d2.scale);
        }
        out[row * N + col] = v;
      }
    }
  }
}

// ---- PersonalizedAttentivePooling (layers.py:312-339) --------------------------------------------------------------------
constexpr int PAP_THREADS = 256;
constexpr int PAP_WAVES = PAP_THREADS / 64;
constexpr int PAP_MAX_L = 256;
constexpr int PAP_MAX_F = 4096;

__device__ __forceinline__ int64_t pap_q_row(const int32_t* q_idx, int64_t n, int64_t n_q) {
  const int64_t i = q_idx[n];
  return (i >= 0 && i < n_q) ? i : 0;
}

// one workgroup per sequence n: U <- tanh(U + ba); s_l = q . U_l; w = softmax_l(s) (max-subtracted, no epsilon);
// out[n] = sum_l w_l V_l; out_d[n] = Dropout(out[n]) for n < n_drop
__global__ __launch_bounds__(PAP_THREADS) void pap_fwd_kernel(float* __restrict__ U, const float* __restrict__ ba,
                                                              const float* __restrict__ Q, const int32_t* __restrict__ q_idx,
                                                              int64_t n_q, const float* __restrict__ V, float* __restrict__ out,
                                                              float* __restrict__ w, float* __restrict__ out_d, int64_t n_drop,
                                                              EbnDrop dr, int L, int F, int A) {
  __shared__ float sm[PAP_MAX_L];
  __shared__ float red[2];
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* q = Q + pap_q_row(q_idx, n, n_q) * A;
  for (int l = wave; l < L; l += PAP_WAVES) {
    float* urow = U + (n * L + l) * A;
    float part = 0.f;
    for (int k = lane; k < A; k += 64) {
      const float u = tanhf(urow[k] + ba[k]);
      urow[k] = u;
      part = fmaf(q[k], u, part);
    }
    part = ebn_wave_sum(part);
    if (lane == 0) sm[l] = part;
  }
  __syncthreads();
  if (wave == 0) {
    float mx = -INFINITY;
    for (int l = lane; l < L; l += 64) mx = fmaxf(mx, sm[l]);
    mx = ebn_wave_max(mx);
    float s = 0.f;
    for (int l = lane; l < L; l += 64) s += expf(sm[l] - mx);
    s = ebn_wave_sum(s);
    if (lane == 0) {
      red[0] = mx;
      red[1] = s;
    }
  }
  __syncthreads();
  const float mx = red[0], s = red[1];
  __syncthreads();
  for (int l = tid; l < L; l += PAP_THREADS) {
    const float wl = expf(sm[l] - mx) / s;
    sm[l] = wl;
    w[n * L + l] = wl;
  }
  __syncthreads();
  const bool drop = out_d != nullptr && n < n_drop && dr.key_ptr != nullptr;
  const uint32_t key = drop ? *dr.key_ptr : 0u;
  for (int c = tid; c < F; c += PAP_THREADS) {
    float acc = 0.f;
    for (int l = 0; l < L; ++l) acc = fmaf(sm[l], V[(n * L + l) * F + c], acc);
    out[n * F + c] = acc;
    if (out_d != nullptr && n < n_drop)
      out_d[n * F + c] = drop ? acc * ebn_drop_mult(key, static_cast<uint64_t>(n) * F + c, dr.thresh, dr.scale) : acc;
  }
}

// one workgroup per sequence n (U holds tanh from the forward):
//   dout[n] *= dropout multiplier (n < n_drop; in place: the backward of pap_fwd's out_d)
//   dw_l = dout . V_l;  ds_l = w_l (dw_l - sum w dw);  dq[n] = sum_l ds_l U_l;  U_l <- ds_l q (1 - U_l^2);  dV_l = w_l dout
__global__ __launch_bounds__(PAP_THREADS) void pap_bwd_kernel(float* __restrict__ U, const float* __restrict__ Q,
                                                              const int32_t* __restrict__ q_idx, int64_t n_q,
                                                              const float* __restrict__ V, const float* __restrict__ w,
                                                              float* __restrict__ dout, float* __restrict__ dV,
                                                              float* __restrict__ dq, int64_t n_drop, EbnDrop dr, int L, int F,
                                                              int A) {
  __shared__ float sd[PAP_MAX_F];
  __shared__ float sm[PAP_MAX_L];
  __shared__ float red[PAP_WAVES];
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* q = Q + pap_q_row(q_idx, n, n_q) * A;
  const bool drop = n < n_drop && dr.key_ptr != nullptr;
  const uint32_t key = drop ? *dr.key_ptr : 0u;
  for (int c = tid; c < F; c += PAP_THREADS) {
    float d = dout[n * F + c];
    if (drop) {
      d *= ebn_drop_mult(key, static_cast<uint64_t>(n) * F + c, dr.thresh, dr.scale);
      dout[n * F + c] = d;
    }
    sd[c] = d;
  }
  __syncthreads();
  for (int l = wave; l < L; l += PAP_WAVES) {
    const float* vrow = V + (n * L + l) * F;
    float part = 0.f;
    for (int c = lane; c < F; c += 64) part = fmaf(sd[c], vrow[c], part);
    part = ebn_wave_sum(part);
    if (lane == 0) sm[l] = part;  // dw_l
  }
  __syncthreads();
  float p = 0.f;
  for (int l = tid; l < L; l += PAP_THREADS) p = fmaf(w[n * L + l], sm[l], p);
  p = ebn_wave_sum(p);
  if (lane == 0) red[wave] = p;
  __syncthreads();
  float wdw = 0.f;
#pragma unroll
  for (int i = 0; i < PAP_WAVES; ++i) wdw += red[i];
  __syncthreads();
  for (int l = tid; l < L; l += PAP_THREADS) sm[l] = w[n * L + l] * (sm[l] - wdw);  // ds_l
  __syncthreads();
  for (int k = tid; k < A; k += PAP_THREADS) {
    float acc = 0.f;
    const float qk = q[k];
    for (int l = 0; l < L; ++l) {
      float* u = U + (n * L + l) * A + k;
      const float t = *u;
      acc = fmaf(sm[l], t, acc);
      *u = sm[l] * qk * (1.f - t * t);
    }
    dq[n * A + k] = acc;
  }
  if (dV != nullptr) {
    for (int l = 0; l < L; ++l) {
      const float wl = w[n * L + l];
      for (int c = tid; c < F; c += PAP_THREADS) dV[(n * L + l) * F + c] = wl * sd[c];
    }
  }
}

// dQ[i] = sum over n (ascending) with q_idx[n] == i of dq[n]: one workgroup per query row, fixed order, no atomics
__global__ __launch_bounds__(PAP_THREADS) void pap_dq_reduce_kernel(const float* __restrict__ dq, const int32_t* __restrict__ q_idx,
                                                                    int64_t n_seq, float* __restrict__ dQ, int64_t n_q, int A) {
  const int64_t i = blockIdx.x;
  for (int k = threadIdx.x; k < A; k += PAP_THREADS) {
    float acc = 0.f;
    for (int64_t n = 0; n < n_seq; ++n) {
      const int64_t qi = q_idx[n];
      const int64_t row = (qi >= 0 && qi < n_q) ? qi : 0;
      if (row == i) acc += dq[n * A + k];
    }
    dQ[i * A + k] = acc;
  }
}

constexpr int CONV_MAX_WINDOW = 15;
constexpr int CONV_MAX_SPLITS = 64;

// shared argument checks of the three conv entry points
int conv_check(int64_t n_titles, int32_t T, int32_t E, int32_t F, int32_t window) {
  EBN_REQUIRE(n_titles >= 0 && T >= 1 && E >= 1 && F >= 1 && window >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(window <= CONV_MAX_WINDOW && E <= 65536 && F <= 65536, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(E % 4 == 0 && F % 4 == 0, EBN_ERR_UNSUPPORTED);
  int64_t R;
  EBN_REQUIRE(!__builtin_mul_overflow(n_titles, static_cast<int64_t>(T), &R), EBN_ERR_UNSUPPORTED);
  // every element index of X, Vd and the weight-gradient slices stays below 2^62
  EBN_REQUIRE(R <= EBN_DIM_MAX && ebn_sat_mul(R, E > F ? E : F) < (int64_t(1) << 40), EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

bool drop_p_ok(float p) { return p >= 0.f && p < 1.f; }

float gate_scale(const ebn_step_state* st, float p_conv, float p_pap) {
  if (st == nullptr) return 1.f;
  const float a = p_conv > 0.f ? 1.f / (1.f - p_conv) : 1.f;
  const float b = p_pap > 0.f ? 1.f / (1.f - p_pap) : 1.f;
  return a * b;
}

ConvArgs conv_args(int64_t n_titles, int32_t T, int32_t E, int32_t F, int32_t window) {
  ConvArgs a{};
  a.R = n_titles * T;
  a.T = T;
  a.E = E;
  a.F = F;
  a.window = window;
  a.pad = (window - 1) / 2;
  a.gscale = 1.f;
  a.d1 = ebn_make_drop(nullptr, -1, 0.f);
  a.d2 = a.d1;
  a.k_per_split = 0;
  return a;
}

}  // namespace

extern "C" int ebn_conv1d_fwd_f32(const float* X, const float* W, const float* bias, float* Vd, int64_t n_titles, int32_t T,
                                  int32_t E, int32_t F, int32_t window, const ebn_step_state* st, int32_t conv_site, float conv_p,
                                  int32_t pap_site, float pap_p, ebn_stream_t stream) {
  EBN_REQUIRE(X && W && bias && Vd, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(drop_p_ok(conv_p) && drop_p_ok(pap_p), EBN_ERR_BAD_ARG);
  const int rc = conv_check(n_titles, T, E, F, window);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(ebn_aligned16(X) && ebn_aligned16(W), EBN_ERR_ALIGN);
  ConvArgs a = conv_args(n_titles, T, E, F, window);
  if (a.R == 0) return EBN_OK;
  a.X = X;
  a.W = W;
  a.bias = bias;
  a.out = Vd;
  a.d1 = ebn_make_drop(st, conv_site, conv_p);
  a.d2 = ebn_make_drop(st, pap_site, pap_p);
  const dim3 grid(static_cast<uint32_t>(ebn_ceil_div(F, CV_BN)), static_cast<uint32_t>(ebn_ceil_div(a.R, CV_BM)));
  EBN_REQUIRE(grid.y <= 0x7FFFFFFFu, EBN_ERR_UNSUPPORTED);
  EBN_LAUNCH(conv_gemm_kernel<0>, grid, dim3(CV_THREADS), 0, ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_conv1d_bwd_data_f32(const float* dVd, const float* Vd, const float* W, float* dX, int64_t n_titles, int32_t T,
                                       int32_t E, int32_t F, int32_t window, const ebn_step_state* st, float conv_p, float pap_p,
                                       ebn_stream_t stream) {
  EBN_REQUIRE(dVd && Vd && W && dX, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(drop_p_ok(conv_p) && drop_p_ok(pap_p), EBN_ERR_BAD_ARG);
  const int rc = conv_check(n_titles, T, E, F, window);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(ebn_aligned16(dVd) && ebn_aligned16(Vd) && ebn_aligned16(W), EBN_ERR_ALIGN);
  ConvArgs a = conv_args(n_titles, T, E, F, window);
  if (a.R == 0) return EBN_OK;
  a.G = dVd;
  a.Vd = Vd;
  a.W = W;
  a.out = dX;
  a.gscale = gate_scale(st, conv_p, pap_p);
  const dim3 grid(static_cast<uint32_t>(ebn_ceil_div(E, CV_BN)), static_cast<uint32_t>(ebn_ceil_div(a.R, CV_BM)));
  EBN_LAUNCH(conv_gemm_kernel<1>, grid, dim3(CV_THREADS), 0, ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_conv1d_wgrad_splits(int64_t n_titles, int32_t T, int32_t E, int32_t F, int32_t window) {
  if (conv_check(n_titles, T, E, F, window) != EBN_OK) return 1;
  const int64_t R = n_titles * T;
  const int64_t tiles = ebn_ceil_div(static_cast<int64_t>(window) * E + 1, CV_BM) * ebn_ceil_div(F, CV_BN);
  int64_t s = ebn_ceil_div(512, tiles);           // about two workgroups per CU
  const int64_t by_rows = ebn_ceil_div(R, 256);  // at least 256 rows per slice
  s = s < by_rows ? s : by_rows;
  s = s < CONV_MAX_SPLITS ? s : CONV_MAX_SPLITS;
  return static_cast<int>(s < 1 ? 1 : s);
}

extern "C" int64_t ebn_conv1d_wgrad_workspace_floats(int64_t n_titles, int32_t T, int32_t E, int32_t F, int32_t window,
                                                     int32_t splits) {
  if (conv_check(n_titles, T, E, F, window) != EBN_OK || splits < 1 || splits > CONV_MAX_SPLITS) return 0;
  return ebn_sat_mul(ebn_sat_mul(splits, static_cast<int64_t>(window) * E + 1), F);
}

extern "C" int ebn_conv1d_bwd_weight_f32(const float* X, const float* dVd, const float* Vd, float* partials, int32_t splits,
                                         int64_t n_titles, int32_t T, int32_t E, int32_t F, int32_t window,
                                         const ebn_step_state* st, float conv_p, float pap_p, ebn_stream_t stream) {
  EBN_REQUIRE(X && dVd && Vd && partials, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(drop_p_ok(conv_p) && drop_p_ok(pap_p), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(splits >= 1 && splits <= CONV_MAX_SPLITS, EBN_ERR_BAD_ARG);
  const int rc = conv_check(n_titles, T, E, F, window);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(ebn_aligned16(X) && ebn_aligned16(dVd) && ebn_aligned16(Vd), EBN_ERR_ALIGN);
  ConvArgs a = conv_args(n_titles, T, E, F, window);
  a.X = X;
  a.G = dVd;
  a.Vd = Vd;
  a.out = partials;
  a.gscale = gate_scale(st, conv_p, pap_p);
  // rows per slice: a multiple of the slab depth; every slice is launched (an empty one writes zeros)
  a.k_per_split = ebn_ceil_div(ebn_ceil_div(a.R, splits), CV_BK) * CV_BK;
  if (a.k_per_split == 0) a.k_per_split = CV_BK;
  const int64_t M = static_cast<int64_t>(window) * E + 1;
  const dim3 grid(static_cast<uint32_t>(ebn_ceil_div(F, CV_BN)), static_cast<uint32_t>(ebn_ceil_div(M, CV_BM)),
                  static_cast<uint32_t>(splits));
  EBN_LAUNCH(conv_gemm_kernel<2>, grid, dim3(CV_THREADS), 0, ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

static int pap_check(int64_t n_seq, int32_t L, int32_t F, int32_t A, int64_t n_q) {
  EBN_REQUIRE(n_seq >= 0 && L >= 1 && F >= 1 && A >= 1 && n_q >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(L <= PAP_MAX_L && F <= PAP_MAX_F && A <= 65536, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(n_seq <= 0x7FFFFFFF && n_q <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

extern "C" int ebn_pap_fwd_f32(float* U, const float* ba, const float* Q, const int32_t* q_idx, int64_t n_q, const float* V,
                               float* out, float* w, float* out_d, int64_t n_drop, int64_t n_seq, int32_t L, int32_t F, int32_t A,
                               const ebn_step_state* st, int32_t site, float drop_p, ebn_stream_t stream) {
  EBN_REQUIRE(U && ba && Q && q_idx && V && out && w, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(drop_p_ok(drop_p) && n_drop >= 0, EBN_ERR_BAD_ARG);
  const int rc = pap_check(n_seq, L, F, A, n_q);
  if (rc != EBN_OK) return rc;
  if (n_seq == 0) return EBN_OK;
  EBN_LAUNCH(pap_fwd_kernel, dim3(static_cast<uint32_t>(n_seq)), dim3(PAP_THREADS), 0, ebn_stream(stream), U, ba, Q, q_idx, n_q, V,
             out, w, out_d, n_drop, ebn_make_drop(st, site, drop_p), L, F, A);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_pap_bwd_f32(float* U, const float* Q, const int32_t* q_idx, int64_t n_q, const float* V, const float* w,
                               float* dout, float* dV, float* dq, int64_t n_drop, int64_t n_seq, int32_t L, int32_t F, int32_t A,
                               const ebn_step_state* st, int32_t site, float drop_p, ebn_stream_t stream) {
  EBN_REQUIRE(U && Q && q_idx && V && w && dout && dq, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(drop_p_ok(drop_p) && n_drop >= 0, EBN_ERR_BAD_ARG);
  const int rc = pap_check(n_seq, L, F, A, n_q);
  if (rc != EBN_OK) return rc;
  if (n_seq == 0) return EBN_OK;
  EBN_LAUNCH(pap_bwd_kernel, dim3(static_cast<uint32_t>(n_seq)), dim3(PAP_THREADS), 0, ebn_stream(stream), U, Q, q_idx, n_q, V, w,
             dout, dV, dq, n_drop, ebn_make_drop(st, site, drop_p), L, F, A);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_pap_dq_reduce_f32(const float* dq, const int32_t* q_idx, int64_t n_seq, float* dQ, int64_t n_q, int32_t A,
                                     ebn_stream_t stream) {
  EBN_REQUIRE(dq && q_idx && dQ, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_seq >= 0 && n_q >= 0 && A >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_q <= 0x7FFFFFFF && n_seq <= EBN_DIM_MAX && A <= 65536, EBN_ERR_UNSUPPORTED);
  if (n_q == 0) return EBN_OK;
  EBN_LAUNCH(pap_dq_reduce_kernel, dim3(static_cast<uint32_t>(n_q)), dim3(PAP_THREADS), 0, ebn_stream(stream), dq, q_idx, n_seq, dQ,
             n_q, A);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
