// LSTUR (reference lstur.py:56-144, layers.py:55-81, 273-309): AttLayer2 under the mask of the title encoder's Masking(), and
// the masked recurrence of the user encoder's Keras GRU (TF2 defaults: reset_after=True, sigmoid / tanh, gate blocks [z, r, h]).
//
// Masked AttLayer2, one workgroup per title (same arithmetic as ebn_attpool_fwd_f32, plus the mask):
//   U <- tanh(U + b);  m_l = (id_l != 0) && any_f(X_l != 0);  a_l = m_l ? exp(U_l . q) : 0 (no max-subtraction);
//   w_l = a_l / (sum a + 1e-7);  out = sum_l w_l X_l.
// A masked row gets w_l == 0 exactly, so the existing ebn_attpool_bwd_pool_f32 / ebn_attpool_bwd_dpre_f32 (both linear in w)
// hand it zero gradients.
//
// GRU, per step t of the B sequences (x_t = X[b*H + t] the history news vector, gx = X.W_k computed beforehand by one GEMM):
//   gh = h.U_rec + b'       z = sig(gx_z + b_z + gh_z)   r = sig(gx_r + b_r + gh_r)   n = tanh(gx_h + b_h + r * gh_h)
//   h' = z h + (1 - z) n    step masked (x_t all zero: Masking(0.0)) -> h' = h
// One launch per step: the grid is (blocks of 16 sequences) x (slices of 16 units) and a workgroup contracts its 16 rows of h
// with the three gate columns of its units (VALU fp32, k ascending: a fixed order), so the gate math is its epilogue.  Steps
// depend on each other through kernel boundaries only -- no inter-workgroup synchronisation.
// Backward, reverse time: launch t (H .. 0) computes dh_t = masked_t ? dh_{t+1} : dh_{t+1} z_t + dgh_t.U_rec^T for its units
// (launch H takes dh_H as given) and, in its epilogue, the gate gradients of step t - 1 from dh_t.  dh is updated in place in
// the dh0 buffer (each element by the thread that owns it), so after launch 0 it holds dh0.
#include "ebn_common.h"

namespace {

// ---- masked AttLayer2 ------------------------------------------------------------------------------------------------------
constexpr int MP_THREADS = 256;
constexpr int MP_WAVES = MP_THREADS / 64;
constexpr int MP_MAX_L = 8192;
constexpr float KERAS_EPS = 1e-7f;  // K.epsilon(), layers.py:75-77

__global__ __launch_bounds__(MP_THREADS) void attpool_masked_fwd_kernel(float* __restrict__ U, const float* __restrict__ b,
                                                                         const float* __restrict__ q, const float* __restrict__ X,
                                                                         const int32_t* __restrict__ ids, float* __restrict__ out,
                                                                         float* __restrict__ w, int L, int E, int A) {
  extern __shared__ float sm[];  // a / w of this title: L floats
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int l = wave; l < L; l += MP_WAVES) {
    const int64_t row = n * L + l;
    float* urow = U + row * A;
    float part = 0.f;
    for (int k = lane; k < A; k += 64) {
      const float u = tanhf(urow[k] + b[k]);
      urow[k] = u;
      part = fmaf(u, q[k], part);
    }
    part = ebn_wave_sum(part);
    const float* xr = X + row * E;
    int nz = 0;
    for (int c = lane; c < E; c += 64) nz |= xr[c] != 0.f ? 1 : 0;
    const bool live = __any(nz) && ids[row] != 0;
    if (lane == 0) sm[l] = live ? expf(part) : 0.f;
  }
  __syncthreads();
  if (wave == 0) {
    float s = 0.f;
    for (int l = lane; l < L; l += 64) s += sm[l];
    s = ebn_wave_sum(s) + KERAS_EPS;
    for (int l = lane; l < L; l += 64) {
      const float wl = sm[l] / s;  // a masked row: 0 / s == 0 exactly
      sm[l] = wl;
      w[n * L + l] = wl;
    }
  }
  __syncthreads();
  for (int c = tid; c < E; c += MP_THREADS) {
    float acc = 0.f;
    for (int l = 0; l < L; ++l) acc = fmaf(sm[l], X[(n * L + l) * E + c], acc);
    out[n * E + c] = acc;
  }
}

// ---- GRU recurrence --------------------------------------------------------------------------------------------------------
constexpr int GRU_BM = 16;   // sequences per workgroup
constexpr int GRU_BU = 16;   // units per workgroup
constexpr int GRU_BK = 128;  // contraction slab
constexpr int GRU_THREADS = GRU_BM * GRU_BU;
constexpr int GRU_MAX_H = 4096;
constexpr int GRU_MAX_DIM = 65536;

struct GruArgs {
  const float* gx;    // (B*H, 3U) = X.W_k, row b*H + t
  const float* X;     // (B*H, F) history news vectors: the step mask
  const float* Wrec;  // (U, 3U) recurrent kernel, column blocks [z | r | h]
  const float* bias;  // (2, 3U): row 0 input bias, row 1 recurrent bias
  const float* h0;    // (B, U) or NULL (zeros)
  float* Hs;          // (H+1, B, U), time-major; Hs[0] = h0
  float* act;         // (H, B, 4U): z | r | n | gh_h (= h.U_h + b'_h)
  const float* dhH;   // (B, U)
  float* dgx;         // (B*H, 3U)
  float* dgh;         // (H, B, 3U)
  float* dh;          // (B, U): dh_{t+1} -> dh_t in place; dh0 at the end
  int64_t B;
  int32_t H, F, U, t;
};

__device__ __forceinline__ float4 ld4(const float* __restrict__ p, int64_t off, bool ok) {
  if (!ok) return make_float4(0.f, 0.f, 0.f, 0.f);
  return *reinterpret_cast<const float4*>(p + off);
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// live[r] = any(X[(b0 + r) * H + s] != 0) for the workgroup's 16 sequences (16 threads per row, float4 along F)
__device__ __forceinline__ void step_mask(const GruArgs& a, int64_t b0, int s, int* live) {
  const int tid = threadIdx.x, r = tid / 16, j = tid % 16;
  const int64_t b = b0 + r;
  int nz = 0;
  if (b < a.B) {
    const float* x = a.X + (b * a.H + s) * a.F;
    for (int c = 4 * j; c < a.F; c += 64) {
      const float4 v = *reinterpret_cast<const float4*>(x + c);
      nz |= (v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f) ? 1 : 0;
    }
  }
  if (nz) live[r] = 1;  // benign: every writer stores 1
}

// MODE 0 (forward step t): acc[g] = sum_k h_t[b, k] U_rec[k, g U + u], g = z, r, h
// MODE 1 (backward step t < H): acc[0] = sum_k dgh_t[b, k] U_rec[u, k], k < 3U
template <int MODE>
__device__ __forceinline__ void gru_tile_gemm(const GruArgs& a, const float* __restrict__ A, int64_t b0, int u0, float* acc) {
  constexpr int NC = MODE == 0 ? 3 * GRU_BU : GRU_BU;            // B-tile columns
  constexpr int A4 = GRU_BM * GRU_BK / 4 / GRU_THREADS;          // float4 of the A tile per thread: 2
  constexpr int B4 = GRU_BK * NC / 4 / GRU_THREADS;              // 6 (forward) / 2 (backward)
  __shared__ float sa[GRU_BK][GRU_BM + 1];
  __shared__ float sb[GRU_BK][NC + 1];
  const int tid = threadIdx.x, tx = tid % GRU_BU, ty = tid / GRU_BU;
  const int64_t U = a.U, U3 = 3 * U;
  const int64_t K = MODE == 0 ? U : U3;  // multiple of 4
  const int64_t lda = K;
  float4 ra[A4], rb[B4];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < A4; ++i) {
      const int v = tid + i * GRU_THREADS, r = v / (GRU_BK / 4), k = 4 * (v % (GRU_BK / 4));
      const int64_t b = b0 + r;
      ra[i] = ld4(A, b * lda + k0 + k, A != nullptr && b < a.B && k0 + k < K);
    }
#pragma unroll
    for (int i = 0; i < B4; ++i) {
      const int v = tid + i * GRU_THREADS;
      if (MODE == 0) {  // row k of U_rec, 4 units of gate g
        const int kk = v / (NC / 4), c4 = v % (NC / 4), g = c4 / (GRU_BU / 4), uu = u0 + 4 * (c4 % (GRU_BU / 4));
        rb[i] = ld4(a.Wrec, (k0 + kk) * U3 + g * U + uu, k0 + kk < K && uu < U);
      } else {  // row u0 + c of U_rec, 4 consecutive k
        const int c = v / (GRU_BK / 4), k = 4 * (v % (GRU_BK / 4));
        rb[i] = ld4(a.Wrec, (u0 + c) * U3 + k0 + k, u0 + c < U && k0 + k < K);
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < A4; ++i) {
      const int v = tid + i * GRU_THREADS, r = v / (GRU_BK / 4), k = 4 * (v % (GRU_BK / 4));
      sa[k][r] = ra[i].x;
      sa[k + 1][r] = ra[i].y;
      sa[k + 2][r] = ra[i].z;
      sa[k + 3][r] = ra[i].w;
    }
#pragma unroll
    for (int i = 0; i < B4; ++i) {
      const int v = tid + i * GRU_THREADS;
      if (MODE == 0) {
        const int kk = v / (NC / 4), c = 4 * (v % (NC / 4));
        sb[kk][c] = rb[i].x;
        sb[kk][c + 1] = rb[i].y;
        sb[kk][c + 2] = rb[i].z;
        sb[kk][c + 3] = rb[i].w;
      } else {
        const int c = v / (GRU_BK / 4), k = 4 * (v % (GRU_BK / 4));
        sb[k][c] = rb[i].x;
        sb[k + 1][c] = rb[i].y;
        sb[k + 2][c] = rb[i].z;
        sb[k + 3][c] = rb[i].w;
      }
    }
  };
  fetch(0);
  for (int64_t k0 = 0; k0 < K; k0 += GRU_BK) {
    __syncthreads();  // the previous slab's readers are done
    stash();
    __syncthreads();
    if (k0 + GRU_BK < K) fetch(k0 + GRU_BK);  // in flight while this slab is consumed
    const int kn = K - k0 < GRU_BK ? static_cast<int>(K - k0) : GRU_BK;
    for (int k = 0; k < kn; ++k) {
      const float hv = sa[k][ty];
      acc[0] = fmaf(hv, sb[k][tx], acc[0]);
      if (MODE == 0) {
        acc[1] = fmaf(hv, sb[k][GRU_BU + tx], acc[1]);
        acc[2] = fmaf(hv, sb[k][2 * GRU_BU + tx], acc[2]);
      }
    }
  }
}

// gate epilogue of unit u of one live step: gx = the sequence's row of X.W_k, acc = h.U_rec of the three gate columns; returns h'.
// Contraction is off: the training and the inference step kernel must round alike (the inference result is tested bit for bit
// against the training kernel's), and left to itself the compiler fuses r * gh_h into the add in one of them only.
__device__ __forceinline__ float gru_gates(const float* __restrict__ gx, const float* __restrict__ bias, int64_t U, int u, float h,
                                           const float* acc, float& z, float& r, float& n, float& ghh) {
#pragma clang fp contract(off)
  const float* bi = bias;
  const float* br = bias + 3 * U;
  z = sigmoidf(gx[u] + bi[u] + (acc[0] + br[u]));
  r = sigmoidf(gx[U + u] + bi[U + u] + (acc[1] + br[U + u]));
  ghh = acc[2] + br[2 * U + u];
  n = tanhf(gx[2 * U + u] + bi[2 * U + u] + r * ghh);
  return z * h + (1.f - z) * n;
}

__global__ __launch_bounds__(GRU_THREADS) void gru_fwd_step_kernel(GruArgs a) {
  __shared__ int live[GRU_BM];
  const int tid = threadIdx.x, tx = tid % GRU_BU, ty = tid / GRU_BU;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * GRU_BM;
  const int u0 = static_cast<int>(blockIdx.y) * GRU_BU;
  const int t = a.t;
  const int64_t B = a.B, U = a.U;
  if (tid < GRU_BM) live[tid] = 0;
  __syncthreads();
  step_mask(a, b0, t, live);
  const float* hprev = t == 0 ? a.h0 : a.Hs + static_cast<int64_t>(t) * B * U;
  float acc[3] = {0.f, 0.f, 0.f};
  gru_tile_gemm<0>(a, hprev, b0, u0, acc);  // its barriers also publish live[]
  const int64_t b = b0 + ty;
  const int u = u0 + tx;
  if (b >= B || u >= U) return;
  const float h = hprev != nullptr ? hprev[b * U + u] : 0.f;
  if (t == 0) a.Hs[b * U + u] = h;
  float z = 0.f, r = 0.f, n = 0.f, ghh = 0.f, hn = h;
  if (live[ty]) hn = gru_gates(a.gx + (b * a.H + t) * 3 * U, a.bias, U, u, h, acc, z, r, n, ghh);
  a.Hs[(static_cast<int64_t>(t) + 1) * B * U + b * U + u] = hn;
  float* ac = a.act + (static_cast<int64_t>(t) * B + b) * 4 * U;
  ac[u] = z;
  ac[U + u] = r;
  ac[2 * U + u] = n;
  ac[3 * U + u] = ghh;
}

// Inference step t over a once-encoded catalogue (scorer.predict from cached news vectors): the same tile GEMM and gate epilogue,
// but the sequence's gx row is GX_all[his_idx[b, t]] (GX_all = news_all.W_k, one GEMM per predict), the step mask is the per-article
// flag live_all[row] (= any(news_all[row] != 0), the predicate of step_mask, built with the cache) and h moves between two
// (B, U) buffers: nothing is kept for a backward pass.  A row number outside [0, n_rows) sets *oob and masks the step.
__global__ __launch_bounds__(GRU_THREADS) void gru_infer_step_kernel(GruArgs a, const float* __restrict__ gx_all,
                                                                     const int32_t* __restrict__ live_all, int64_t n_rows,
                                                                     const int32_t* __restrict__ his_idx, const float* hin,
                                                                     float* __restrict__ hout, int32_t* __restrict__ oob) {
  __shared__ int row[GRU_BM];  // catalogue row of the sequence's step, -1: masked
  const int tid = threadIdx.x, tx = tid % GRU_BU, ty = tid / GRU_BU;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * GRU_BM;
  const int u0 = static_cast<int>(blockIdx.y) * GRU_BU;
  const int64_t B = a.B, U = a.U;
  if (tid < GRU_BM) {
    int r = -1;
    if (b0 + tid < B) {
      const int32_t i = his_idx[(b0 + tid) * a.H + a.t];
      if (i >= 0 && static_cast<int64_t>(i) < n_rows) {
        if (live_all[i] != 0) r = i;
      } else if (oob != nullptr) {
        *oob = 1;
      }
    }
    row[tid] = r;
  }
  float acc[3] = {0.f, 0.f, 0.f};
  gru_tile_gemm<0>(a, hin, b0, u0, acc);  // its barriers also publish row[]
  const int64_t b = b0 + ty;
  const int u = u0 + tx;
  if (b >= B || u >= U) return;
  const float h = hin != nullptr ? hin[b * U + u] : 0.f;
  float z, r, n, ghh, hn = h;
  if (row[ty] >= 0) hn = gru_gates(gx_all + static_cast<int64_t>(row[ty]) * 3 * U, a.bias, U, u, h, acc, z, r, n, ghh);
  hout[b * U + u] = hn;
}

__global__ __launch_bounds__(GRU_THREADS) void gru_bwd_step_kernel(GruArgs a) {
  __shared__ int live[2][GRU_BM];  // [0]: step t, [1]: step t - 1
  const int tid = threadIdx.x, tx = tid % GRU_BU, ty = tid / GRU_BU;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * GRU_BM;
  const int u0 = static_cast<int>(blockIdx.y) * GRU_BU;
  const int t = a.t, H = a.H;
  const int64_t B = a.B, U = a.U;
  if (tid < 2 * GRU_BM) live[tid / GRU_BM][tid % GRU_BM] = 0;
  __syncthreads();
  if (t < H) step_mask(a, b0, t, live[0]);
  if (t >= 1) step_mask(a, b0, t - 1, live[1]);
  float acc[1] = {0.f};
  if (t < H) gru_tile_gemm<1>(a, a.dgh + static_cast<int64_t>(t) * B * 3 * U, b0, u0, acc);
  __syncthreads();  // live[] (the GEMM's barriers are skipped at t == H)
  const int64_t b = b0 + ty;
  const int u = u0 + tx;
  if (b >= B || u >= U) return;
  float dh;
  if (t == H) {
    dh = a.dhH[b * U + u];
  } else {
    dh = a.dh[b * U + u];
    if (live[0][ty]) dh = dh * a.act[(static_cast<int64_t>(t) * B + b) * 4 * U + u] + acc[0];
  }
  a.dh[b * U + u] = dh;
  if (t == 0) return;
  // gate gradients of step s = t - 1 from dh_t = dL/dHs[t]
  const int s = t - 1;
  float* dgx = a.dgx + (b * H + s) * 3 * U;
  float* dgh = a.dgh + (static_cast<int64_t>(s) * B + b) * 3 * U;
  float dz = 0.f, dr = 0.f, dn = 0.f, dnh = 0.f;
  if (live[1][ty]) {
    const float* ac = a.act + (static_cast<int64_t>(s) * B + b) * 4 * U;
    const float z = ac[u], r = ac[U + u], n = ac[2 * U + u], ghh = ac[3 * U + u];
    const float h = a.Hs[static_cast<int64_t>(s) * B * U + b * U + u];
    dz = dh * (h - n) * z * (1.f - z);
    dn = dh * (1.f - z) * (1.f - n * n);
    dr = dn * ghh * r * (1.f - r);
    dnh = dn * r;
  }
  dgx[u] = dz;
  dgx[U + u] = dr;
  dgx[2 * U + u] = dn;
  dgh[u] = dz;
  dgh[U + u] = dr;
  dgh[2 * U + u] = dnh;
}

int gru_check(int64_t B, int32_t H, int32_t F, int32_t U) {
  EBN_REQUIRE(B >= 0 && H >= 1 && F >= 1 && U >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(H <= GRU_MAX_H && F <= GRU_MAX_DIM && U <= GRU_MAX_DIM && F % 4 == 0 && U % 4 == 0, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(B <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  // every element index of X, gx, dgx, Hs, act and dgh stays far below 2^62
  const int64_t steps = ebn_sat_mul(B, static_cast<int64_t>(H) + 1);
  EBN_REQUIRE(steps <= EBN_DIM_MAX && ebn_sat_mul(steps, 4 * static_cast<int64_t>(U > F ? U : F)) < (int64_t(1) << 40),
              EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

GruArgs gru_args(int64_t B, int32_t H, int32_t F, int32_t U) {
  GruArgs a{};
  a.B = B;
  a.H = H;
  a.F = F;
  a.U = U;
  return a;
}

dim3 gru_grid(int64_t B, int32_t U) {
  return dim3(static_cast<uint32_t>(ebn_ceil_div(B, GRU_BM)), static_cast<uint32_t>(ebn_ceil_div(U, GRU_BU)));
}

}  // namespace

extern "C" int ebn_attpool_masked_fwd_f32(float* U, const float* b, const float* q, const float* X, const int32_t* ids, float* out,
                                          float* w, int64_t n_seq, int32_t L, int32_t E, int32_t A, ebn_stream_t stream) {
  EBN_REQUIRE(U && b && q && X && ids && out && w, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_seq >= 0 && L > 0 && E > 0 && A > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(L <= MP_MAX_L && E <= GRU_MAX_DIM && A <= GRU_MAX_DIM && n_seq <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(ebn_sat_mul(n_seq, L) <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  if (n_seq == 0) return EBN_OK;
  EBN_LAUNCH(attpool_masked_fwd_kernel, dim3(static_cast<uint32_t>(n_seq)), dim3(MP_THREADS), L * sizeof(float),
             ebn_stream(stream), U, b, q, X, ids, out, w, L, E, A);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_gru_fwd_f32(const float* gx, const float* X, const float* Wrec, const float* bias, const float* h0, float* Hs,
                               float* act, int64_t B, int32_t H, int32_t F, int32_t U, ebn_stream_t stream) {
  EBN_REQUIRE(gx && X && Wrec && bias && Hs && act, EBN_ERR_BAD_ARG);
  const int rc = gru_check(B, H, F, U);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(ebn_aligned16(X) && ebn_aligned16(Wrec) && ebn_aligned16(h0) && ebn_aligned16(Hs), EBN_ERR_ALIGN);
  if (B == 0) return EBN_OK;
  GruArgs a = gru_args(B, H, F, U);
  a.gx = gx;
  a.X = X;
  a.Wrec = Wrec;
  a.bias = bias;
  a.h0 = h0;
  a.Hs = Hs;
  a.act = act;
  const dim3 grid = gru_grid(B, U);
  for (int32_t t = 0; t < H; ++t) {
    a.t = t;
    EBN_LAUNCH(gru_fwd_step_kernel, grid, dim3(GRU_THREADS), 0, ebn_stream(stream), a);
    EBN_CHECK_LAUNCH();
  }
  return EBN_OK;
}

extern "C" int ebn_gru_bwd_f32(const float* dhH, const float* X, const float* Wrec, const float* Hs, const float* act, float* dgx,
                               float* dgh, float* dh0, int64_t B, int32_t H, int32_t F, int32_t U, ebn_stream_t stream) {
  EBN_REQUIRE(dhH && X && Wrec && Hs && act && dgx && dgh && dh0, EBN_ERR_BAD_ARG);
  const int rc = gru_check(B, H, F, U);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(ebn_aligned16(X) && ebn_aligned16(Wrec) && ebn_aligned16(dgh), EBN_ERR_ALIGN);
  EBN_REQUIRE(static_cast<const void*>(dhH) != static_cast<const void*>(dh0), EBN_ERR_BAD_ARG);
  if (B == 0) return EBN_OK;
  GruArgs a = gru_args(B, H, F, U);
  a.X = X;
  a.Wrec = Wrec;
  a.Hs = const_cast<float*>(Hs);
  a.act = const_cast<float*>(act);
  a.dhH = dhH;
  a.dgx = dgx;
  a.dgh = dgh;
  a.dh = dh0;
  const dim3 grid = gru_grid(B, U);
  for (int32_t t = H; t >= 0; --t) {
    a.t = t;
    EBN_LAUNCH(gru_bwd_step_kernel, grid, dim3(GRU_THREADS), 0, ebn_stream(stream), a);
    EBN_CHECK_LAUNCH();
  }
  return EBN_OK;
}

extern "C" int ebn_gru_infer_indexed_f32(const float* gx_all, const int32_t* live_all, int64_t n_rows, const int32_t* his_idx,
                                         const float* Wrec, const float* bias, const float* h0, float* h_work, float* h_out, int64_t B,
                                         int32_t H, int32_t U, int32_t* oob_flag, ebn_stream_t stream) {
  EBN_REQUIRE(his_idx && Wrec && bias && h_work && h_out && n_rows >= 0 && (n_rows == 0 || (gx_all && live_all)), EBN_ERR_BAD_ARG);
  const int rc = gru_check(B, H, U, U);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(n_rows <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(ebn_aligned16(Wrec) && ebn_aligned16(h0) && ebn_aligned16(h_work) && ebn_aligned16(h_out), EBN_ERR_ALIGN);
  EBN_REQUIRE(h_work != h_out && h0 != h_work && h0 != h_out, EBN_ERR_BAD_ARG);  // a step reads one buffer and writes the other
  if (B == 0) return EBN_OK;
  GruArgs a = gru_args(B, H, U, U);
  a.Wrec = Wrec;
  a.bias = bias;
  const dim3 grid = gru_grid(B, U);
  for (int32_t t = 0; t < H; ++t) {
    a.t = t;
    float* hout = (H - 1 - t) % 2 == 0 ? h_out : h_work;  // the last step writes h_out
    const float* hin = t == 0 ? h0 : ((H - t) % 2 == 0 ? h_out : h_work);
    EBN_LAUNCH(gru_infer_step_kernel, grid, dim3(GRU_THREADS), 0, ebn_stream(stream), a, gx_all, live_all, n_rows, his_idx, hin, hout,
               oob_flag);
    EBN_CHECK_LAUNCH();
  }
  return EBN_OK;
}
