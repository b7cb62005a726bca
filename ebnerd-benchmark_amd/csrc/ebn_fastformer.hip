// Fastformer (reference models/fastformer/fastformer.py): everything between the projections' GEMMs (ebn_gemm_f32).
//
//   bias + dropout + residual + LayerNorm in the two orders the model uses, forward and backward;
//   the fast additive attention core (FastSelfAttention without its three big Linear layers), forward and backward;
//   bias + erf-gelu, forward and backward;  AttentionPooling after its first Linear (scalar bias, mask, 1e-8), forward and backward;
//   the scoring head (concat-dot + sigmoid), forward and backward;
//   for Fastformer_wu (reference models/fastformer/fastformer_wu.py): the embedding LayerNorm with one position row per token
//   (forward; its backward is the mode-0 backward plus a column-sum finish over dX) and the class head with a stable softmax
//   cross-entropy, forward and backward.
//
// Exact fp32, fixed summation orders, no float atomics: the same bits on every run.  Column sums (bias / gamma / beta / logit-weight
// gradients) leave one partial per workgroup, each summed in a fixed order, and ebn_ff_colsum_finish_f32 adds the partials in ascending
// order.  Dropout uses the counter stream of ebn_common.h; the key of a call site travels BY VALUE in the call (the module derives it
// from its seed, its own step counter and the site number), so ebn_step_state is not involved.
#include "ebn_common.h"
#include "ebn_ff_attn.h"
#include "ebn_reduce.h"

namespace {

constexpr int FF_LN_MAX_D = 1024;      // LayerNorm backward keeps 4 waves x 3 column accumulators of D floats in LDS (48 KiB)
constexpr int FF_MAX_PARTS = 512;      // workgroups (= partials) of a LayerNorm backward
constexpr int FF_ATT_ACC = 16;         // logit-weight gradient elements a thread keeps: heads * D <= 256 * 16
constexpr int FF_POOL_MAX_L = 4096;
constexpr float FF_POOL_EPS = 1e-8f;   // fastformer.py AttentionPooling.forward

struct FfDrop {
  uint32_t key, thresh;
  float scale;
};

FfDrop ff_make_drop(uint32_t key, float p) {
  FfDrop d;
  d.key = key;
  d.thresh = p > 0.f ? ebn_dropout_threshold(p) : 0u;
  d.scale = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
  return d;
}

__device__ __forceinline__ float ff_mult(const FfDrop& d, int64_t idx) {
  return d.thresh ? ebn_drop_mult(d.key, static_cast<uint64_t>(idx), d.thresh, d.scale) : 1.0f;
}

// ---- bias + dropout + residual + LayerNorm ------------------------------------------------------------------------------------
// mode 0 (embedding): z = x + bias + row,            y = drop(gamma * xhat + beta)
// mode 1 (BERT block): z = drop(x + bias) + res[r],  y = gamma * xhat + beta
// one wave per row; the pre-normalisation row z is parked in Y between the passes (each lane re-reads only what it wrote)
__global__ __launch_bounds__(FF_THREADS) void ff_ln_fwd_kernel(const float* __restrict__ X, const float* __restrict__ bias,
                                                               const float* __restrict__ res, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, int mode, FfDrop dr,
                                                               float* __restrict__ Y, float* __restrict__ xhat,
                                                               float* __restrict__ rstd, int64_t R, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * FF_WAVES + (threadIdx.x >> 6);
  if (r >= R) return;
  const int64_t off = r * D;
  float s = 0.f;
  for (int c = lane; c < D; c += 64) {
    float z = X[off + c] + bias[c];
    if (mode == 0) {
      z += res[c];
    } else {
      z = z * ff_mult(dr, off + c) + res[off + c];
    }
    Y[off + c] = z;
    s += z;
  }
  const float mean = ebn_wave_sum(s) / static_cast<float>(D);
  float v = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float d = Y[off + c] - mean;
    v = fmaf(d, d, v);
  }
  const float rs = 1.0f / sqrtf(ebn_wave_sum(v) / static_cast<float>(D) + eps);
  if (lane == 0 && rstd != nullptr) rstd[r] = rs;
  for (int c = lane; c < D; c += 64) {
    const float xh = (Y[off + c] - mean) * rs;
    if (xhat != nullptr) xhat[off + c] = xh;
    float y = fmaf(xh, gamma[c], beta[c]);
    if (mode == 0) y *= ff_mult(dr, off + c);
    Y[off + c] = y;
  }
}

// backward: workgroup b owns rows [b * rpb, (b + 1) * rpb), wave w every fourth of them; per-wave column accumulators in LDS (a lane
// owns its columns), combined (w0 + w1) + (w2 + w3) into partials[b][3][D] = dgamma | dbeta | dbias
__global__ __launch_bounds__(FF_THREADS) void ff_ln_bwd_kernel(const float* __restrict__ dY, const float* __restrict__ xhat,
                                                               const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                               int mode, FfDrop dr, float* __restrict__ dX,
                                                               float* __restrict__ dres, float* __restrict__ partials, int64_t R,
                                                               int D, int64_t rpb) {
  extern __shared__ float4 ff_lds4[];
  float* acc = reinterpret_cast<float*>(ff_lds4);  // [FF_WAVES][3][D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* mine = acc + static_cast<int64_t>(wave) * 3 * D;
  for (int c = lane; c < 3 * D; c += 64) mine[c] = 0.f;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rpb;
  const int64_t r1 = r0 + rpb < R ? r0 + rpb : R;
  const float invD = 1.0f / static_cast<float>(D);
  for (int64_t r = r0 + wave; r < r1; r += FF_WAVES) {
    const int64_t off = r * D;
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < D; c += 64) {
      float g = dY[off + c];
      if (mode == 0) g *= ff_mult(dr, off + c);
      const float dxh = g * gamma[c];
      s1 += dxh;
      s2 = fmaf(dxh, xhat[off + c], s2);
    }
    s1 = ebn_wave_sum(s1) * invD;
    s2 = ebn_wave_sum(s2) * invD;
    const float rs = rstd[r];
    for (int c = lane; c < D; c += 64) {
      float g = dY[off + c];
      if (mode == 0) g *= ff_mult(dr, off + c);
      const float xh = xhat[off + c];
      const float dx = rs * (g * gamma[c] - s1 - xh * s2);
      float dxin = dx;
      if (mode != 0) {
        dres[off + c] = dx;
        dxin = dx * ff_mult(dr, off + c);
      }
      dX[off + c] = dxin;
      mine[c] = fmaf(g, xh, mine[c]);
      mine[D + c] += g;
      mine[2 * D + c] += dxin;
    }
  }
  __syncthreads();
  float* out = partials + static_cast<int64_t>(blockIdx.x) * 3 * D;
  for (int i = threadIdx.x; i < 3 * D; i += FF_THREADS)
    out[i] = (acc[i] + acc[3 * D + i]) + (acc[6 * D + i] + acc[9 * D + i]);
}

// out[i] = sum_p partials[p * stride + i], p ascending within each of 4 interleaved lanes, lanes combined (0 + 1) + (2 + 3)
__global__ __launch_bounds__(FF_THREADS) void ff_colsum_finish_kernel(const float* __restrict__ partials, int64_t n_parts,
                                                                      int64_t stride, int64_t W, float* __restrict__ out) {
  __shared__ float sm[4][64];
  const int cl = threadIdx.x & 63, pl = threadIdx.x >> 6;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 64 + cl;
  float a = 0.f;
  if (i < W)
    for (int64_t p = pl; p < n_parts; p += 4) a += partials[p * stride + i];
  sm[pl][cl] = a;
  __syncthreads();
  if (pl == 0 && i < W) out[i] = (sm[0][cl] + sm[1][cl]) + (sm[2][cl] + sm[3][cl]);
}

// ---- bias + gelu (erf form) ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ff_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float ff_gelu_grad(float v) {
  return 0.5f * (1.0f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}

__global__ __launch_bounds__(FF_THREADS) void ff_gelu_fwd_kernel(const float* __restrict__ X, const float* __restrict__ bias,
                                                                 float* __restrict__ Y, int64_t n, int C) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * FF_THREADS + threadIdx.x;
  if (i < n) Y[i] = ff_gelu(X[i] + bias[i % C]);
}

struct FfGeluBwd {
  const float* X;
  const float* bias;
  const float* dY;
  float* dX;
  int C;
  __device__ __forceinline__ void row(int64_t r, int c, float& a0, float& a1) const {
    const int64_t i = r * C + c;
    const float dx = dY[i] * ff_gelu_grad(X[i] + bias[c]);
    dX[i] = dx;
    a0 += dx;
  }
};

// ---- AttentionPooling after att_fc1's GEMM --------------------------------------------------------------------------------------
// one workgroup per sequence: U <- tanh(U + b1) in place; a_l = exp(U_l . w2 + b2) * m_l (no max-subtraction);
// w_l = a_l / (sum a + 1e-8); out = sum_l w_l X_l (l ascending)
__global__ __launch_bounds__(FF_THREADS) void ff_pool_fwd_kernel(float* __restrict__ U, const float* __restrict__ b1,
                                                                 const float* __restrict__ w2, const float* __restrict__ b2,
                                                                 const float* __restrict__ X, const float* __restrict__ mask,
                                                                 float* __restrict__ out, float* __restrict__ w,
                                                                 float* __restrict__ sinv, int L, int D) {
  extern __shared__ float4 ff_lds4[];
  float* sa = reinterpret_cast<float*>(ff_lds4);  // [L] weights, then [1] the sum
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = blockIdx.x;
  const float bias2 = b2[0];
  for (int l = wave; l < L; l += FF_WAVES) {
    float* u = U + (n * L + l) * D;
    float p = 0.f;
    for (int k = lane; k < D; k += 64) {
      const float e = tanhf(u[k] + b1[k]);
      u[k] = e;
      p = fmaf(e, w2[k], p);
    }
    p = ebn_wave_sum(p);
    if (lane == 0) sa[l] = expf(p + bias2) * mask[n * L + l];
  }
  __syncthreads();
  if (wave == 0) {
    float s = 0.f;
    for (int l = lane; l < L; l += 64) s += sa[l];
    s = ebn_wave_sum(s) + FF_POOL_EPS;
    if (lane == 0) {
      sa[L] = s;
      sinv[n] = 1.0f / s;
    }
  }
  __syncthreads();
  const float s = sa[L];
  for (int l = threadIdx.x; l < L; l += FF_THREADS) {
    const float wl = sa[l] / s;
    sa[l] = wl;
    w[n * L + l] = wl;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += FF_THREADS) {
    float acc = 0.f;
    for (int l = 0; l < L; ++l) acc = fmaf(sa[l], X[(n * L + l) * D + c], acc);
    out[n * D + c] = acc;
  }
}

// backward's direct part: dw_l = dout . X_l, s = sum_l w_l dw_l, de_l = w_l (dw_l - s), dX_l = w_l dout, and the sequence's term of
// d(b2) = sum_l de_l, in its closed form s * (1 - sum w) = s * 1e-8 / (sum a + 1e-8) (the literal sum cancels to rounding noise)
__global__ __launch_bounds__(FF_THREADS) void ff_pool_bwd_kernel(const float* __restrict__ X, const float* __restrict__ w,
                                                                 const float* __restrict__ sinv, const float* __restrict__ dout,
                                                                 float* __restrict__ dX, float* __restrict__ de,
                                                                 float* __restrict__ db2n, int L, int D) {
  extern __shared__ float4 ff_lds4[];
  float* sdw = reinterpret_cast<float*>(ff_lds4);  // [L] dw, then [1] s
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = blockIdx.x;
  const float* dn = dout + n * D;
  for (int l = wave; l < L; l += FF_WAVES) {
    const float* x = X + (n * L + l) * D;
    float p = 0.f;
    for (int k = lane; k < D; k += 64) p = fmaf(dn[k], x[k], p);
    p = ebn_wave_sum(p);
    if (lane == 0) sdw[l] = p;
  }
  __syncthreads();
  if (wave == 0) {
    float s = 0.f;
    for (int l = lane; l < L; l += 64) s = fmaf(w[n * L + l], sdw[l], s);
    s = ebn_wave_sum(s);
    if (lane == 0) {
      sdw[L] = s;
      db2n[n] = s * FF_POOL_EPS * sinv[n];
    }
  }
  __syncthreads();
  const float s = sdw[L];
  for (int l = threadIdx.x; l < L; l += FF_THREADS) de[n * L + l] = w[n * L + l] * (sdw[l] - s);
  for (int64_t i = threadIdx.x; i < static_cast<int64_t>(L) * D; i += FF_THREADS) {
    const int l = static_cast<int>(i / D), c = static_cast<int>(i - static_cast<int64_t>(l) * D);
    dX[n * L * D + i] = w[n * L + l] * dn[c];
  }
}

// ---- head: sigmoid([user | cand] . W + b) ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(FF_THREADS) void ff_head_fwd_kernel(const float* __restrict__ user, const float* __restrict__ cand,
                                                                 const float* __restrict__ W, const float* __restrict__ b,
                                                                 float* __restrict__ score, int64_t N, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t n = static_cast<int64_t>(blockIdx.x) * FF_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;
  float p = 0.f;
  for (int k = lane; k < D; k += 64) p = fmaf(user[n * D + k], W[k], p);
  for (int k = lane; k < D; k += 64) p = fmaf(cand[n * D + k], W[D + k], p);
  p = ebn_wave_sum(p) + b[0];
  if (lane == 0) score[n] = 1.0f / (1.0f + expf(-p));
}

__device__ __forceinline__ float ff_head_dz(const float* score, const float* dscore, int64_t n) {
  const float s = score[n];
  return dscore[n] * s * (1.0f - s);
}

// blocks [0, col_blocks): dW[c] = sum_n dz_n [user | cand][n, c] (n ascending), block 0 / wave 0 also db = sum_n dz_n;
// blocks behind them: duser / dcand rows
__global__ __launch_bounds__(FF_THREADS) void ff_head_bwd_kernel(const float* __restrict__ user, const float* __restrict__ cand,
                                                                 const float* __restrict__ W, const float* __restrict__ score,
                                                                 const float* __restrict__ dscore, float* __restrict__ duser,
                                                                 float* __restrict__ dcand, float* __restrict__ dW,
                                                                 float* __restrict__ db, int64_t N, int D, int col_blocks) {
  const int lane = threadIdx.x & 63;
  if (static_cast<int>(blockIdx.x) < col_blocks) {
    const int c = blockIdx.x * FF_THREADS + threadIdx.x;
    if (c < 2 * D) {
      const float* src = c < D ? user + c : cand + (c - D);
      float acc = 0.f;
      for (int64_t n = 0; n < N; ++n) acc = fmaf(ff_head_dz(score, dscore, n), src[n * D], acc);
      dW[c] = acc;
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {
      float s = 0.f;
      for (int64_t n = lane; n < N; n += 64) s += ff_head_dz(score, dscore, n);
      s = ebn_wave_sum(s);
      if (lane == 0) db[0] = s;
    }
    return;
  }
  const int64_t n = static_cast<int64_t>(blockIdx.x - col_blocks) * FF_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;
  const float dz = ff_head_dz(score, dscore, n);
  for (int k = lane; k < D; k += 64) {
    duser[n * D + k] = dz * W[k];
    dcand[n * D + k] = dz * W[D + k];
  }
}

// ---- Fastformer_wu (reference models/fastformer/fastformer_wu.py) -----------------------------------------------------------------
// StandardFastformerEncoder's embedding LayerNorm: mode 0 of ff_ln_fwd_kernel with one position row PER TOKEN, row r reads
// pos[r % T]; bias may be NULL.  z = x (+ bias) + pos[r % T],  y = drop(gamma * xhat + beta).  One wave per row, z parked in Y.
__global__ __launch_bounds__(FF_THREADS) void ff_ln_pos_fwd_kernel(const float* __restrict__ X, const float* __restrict__ bias,
                                                                   const float* __restrict__ pos, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float eps, FfDrop dr,
                                                                   float* __restrict__ Y, float* __restrict__ xhat,
                                                                   float* __restrict__ rstd, int64_t R, int T, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * FF_WAVES + (threadIdx.x >> 6);
  if (r >= R) return;
  const int64_t off = r * D;
  const float* prow = pos + (r % T) * D;
  float s = 0.f;
  for (int c = lane; c < D; c += 64) {
    float z = X[off + c];
    if (bias != nullptr) z += bias[c];
    z += prow[c];
    Y[off + c] = z;
    s += z;
  }
  const float mean = ebn_wave_sum(s) / static_cast<float>(D);
  float v = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float d = Y[off + c] - mean;
    v = fmaf(d, d, v);
  }
  const float rs = 1.0f / sqrtf(ebn_wave_sum(v) / static_cast<float>(D) + eps);
  if (lane == 0 && rstd != nullptr) rstd[r] = rs;
  for (int c = lane; c < D; c += 64) {
    const float xh = (Y[off + c] - mean) * rs;
    if (xhat != nullptr) xhat[off + c] = xh;
    Y[off + c] = fmaf(xh, gamma[c], beta[c]) * ff_mult(dr, off + c);
  }
}

// the class head: logits = X . W^T + b, a stable log-softmax per row and the row's cross-entropy term.  One wave per row; lane c
// keeps class c's logit (C <= 64).  rowloss[n] = log(sum_c exp(l_c - m)) + m - l_y, or 0 and flag[0] = 1 for a target outside [0, C)
__global__ __launch_bounds__(FF_THREADS) void ff_cls_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                                const float* __restrict__ b, const int64_t* __restrict__ targets,
                                                                float* __restrict__ logits, float* __restrict__ prob,
                                                                float* __restrict__ rowloss, int32_t* __restrict__ flag, int64_t N,
                                                                int D, int C) {
  const int lane = threadIdx.x & 63;
  const int64_t n = static_cast<int64_t>(blockIdx.x) * FF_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* x = X + n * D;
  float mine = -INFINITY;
  for (int c = 0; c < C; ++c) {
    const float* w = W + static_cast<int64_t>(c) * D;
    float p = 0.f;
    for (int k = lane; k < D; k += 64) p = fmaf(x[k], w[k], p);
    p = ebn_wave_sum(p) + b[c];
    if (lane == c) mine = p;
  }
  const float m = ebn_wave_max(mine);
  const float e = lane < C ? expf(mine - m) : 0.f;
  const float s = ebn_wave_sum(e);
  if (lane < C) {
    logits[n * C + lane] = mine;
    prob[n * C + lane] = e / s;
  }
  const int64_t y = targets[n];
  const bool ok = y >= 0 && y < C;
  const float ly = __shfl(mine, ok ? static_cast<int>(y) : 0, 64);
  if (lane == 0) {
    rowloss[n] = ok ? (logf(s) + m) - ly : 0.f;
    if (!ok) flag[0] = 1;
  }
}

// loss[0] = (sum_n rowloss[n]) / N: 256 chains of ascending n, combined by a fixed halving tree in LDS
__global__ __launch_bounds__(FF_THREADS) void ff_cls_loss_kernel(const float* __restrict__ rowloss, float* __restrict__ loss,
                                                                 int64_t N) {
  __shared__ float sm[FF_THREADS];
  float a = 0.f;
  for (int64_t n = threadIdx.x; n < N; n += FF_THREADS) a += rowloss[n];
  sm[threadIdx.x] = a;
  __syncthreads();
  for (int h = FF_THREADS / 2; h > 0; h >>= 1) {
    if (static_cast<int>(threadIdx.x) < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = N > 0 ? sm[0] / static_cast<float>(N) : 0.f;
}

constexpr int FF_CLS_MAX_C = 64;
constexpr int FF_CLS_MAX_D = 1024;
constexpr int FF_CLS_TILE = 32;        // rows whose dlogits a workgroup of the backward keeps in LDS at a time
constexpr int FF_CLS_MAX_PARTS = 128;  // workgroups (= partials) of the backward

// backward: workgroup g owns rows [g * rpb, (g + 1) * rpb) and walks them in tiles of 32: dlogits of the tile into LDS
// (dloss / N * (p - onehot), nothing from a row whose target is out of range, + dscore), dX rows by the waves (c ascending), then
// every thread adds the tile's rows in ascending order to the elements it owns of partials[g] = dW [C, D] | db [C]
__global__ __launch_bounds__(FF_THREADS) void ff_cls_bwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                                const float* __restrict__ prob, const int64_t* __restrict__ targets,
                                                                const float* __restrict__ dloss, const float* __restrict__ dscore,
                                                                float* __restrict__ dX, float* __restrict__ partials, int64_t N,
                                                                int D, int C, int64_t rpb) {
  __shared__ float sdl[FF_CLS_TILE * FF_CLS_MAX_C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rpb;
  const int64_t r1 = r0 + rpb < N ? r0 + rpb : N;
  const float scale = (dloss != nullptr && N > 0) ? dloss[0] / static_cast<float>(N) : 0.f;
  const int width = C * D + C;
  float* out = partials + static_cast<int64_t>(blockIdx.x) * width;
  for (int i = threadIdx.x; i < width; i += FF_THREADS) out[i] = 0.f;  // a thread only ever touches the elements it owns
  for (int64_t t0 = r0; t0 < r1; t0 += FF_CLS_TILE) {
    const int rows = static_cast<int>(r1 - t0 < FF_CLS_TILE ? r1 - t0 : FF_CLS_TILE);
    __syncthreads();  // the previous tile's readers are done
    for (int i = threadIdx.x; i < rows * C; i += FF_THREADS) {
      const int r = i / C, c = i - r * C;
      const int64_t n = t0 + r;
      const int64_t y = targets[n];
      float g = (y >= 0 && y < C) ? scale * (prob[n * C + c] - (c == y ? 1.0f : 0.0f)) : 0.f;
      if (dscore != nullptr) g += dscore[n * C + c];
      sdl[i] = g;
    }
    __syncthreads();
    for (int r = wave; r < rows; r += FF_WAVES) {
      float* dx = dX + (t0 + r) * D;
      for (int k = lane; k < D; k += 64) {
        float a = 0.f;
        for (int c = 0; c < C; ++c) a = fmaf(sdl[r * C + c], W[static_cast<int64_t>(c) * D + k], a);
        dx[k] = a;
      }
    }
    for (int i = threadIdx.x; i < width; i += FF_THREADS) {
      float a = out[i];
      if (i < C * D) {
        const int c = i / D, k = i - c * D;
        for (int r = 0; r < rows; ++r) a = fmaf(sdl[r * C + c], X[(t0 + r) * D + k], a);
      } else {
        const int c = i - C * D;
        for (int r = 0; r < rows; ++r) a += sdl[r * C + c];
      }
      out[i] = a;
    }
  }
}

int64_t ff_cls_blocks(int64_t N) {
  int64_t nb = ebn_ceil_div(N, FF_CLS_TILE);
  if (nb > FF_CLS_MAX_PARTS) nb = FF_CLS_MAX_PARTS;
  return nb < 1 ? 1 : nb;
}

int ff_cls_check(int64_t N, int32_t D, int32_t C) {
  EBN_REQUIRE(N >= 0 && D > 0 && C > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(C <= FF_CLS_MAX_C && D <= FF_CLS_MAX_D && N <= EBN_DIM_MAX && ebn_sat_mul(N, D) < (int64_t(1) << 40), EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

// ---- fast additive attention core (FfAttn and the softmax routines: ebn_ff_attn.h) ------------------------------------------------
// logits of one LDS row against the [heads, D] weight: every head reads the WHOLE row
__device__ __forceinline__ void ff_row_logits(const float* row, const float* __restrict__ Wa, const float* __restrict__ ba, float* sw,
                                              int t, int T, int D, int H, float inv, float maskterm) {
  const int lane = threadIdx.x & 63;
  for (int h = 0; h < H; ++h) {
    const float* wrow = Wa + static_cast<int64_t>(h) * D;
    float p = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
      const float4 x = *reinterpret_cast<const float4*>(row + c);
      const float4 y = *reinterpret_cast<const float4*>(wrow + c);
      p = fmaf(x.x, y.x, p);
      p = fmaf(x.y, y.y, p);
      p = fmaf(x.z, y.z, p);
      p = fmaf(x.w, y.w, p);
    }
    p = ebn_wave_sum(p);
    if (lane == 0) sw[h * T + t] = (p + ba[h]) * inv + maskterm;
  }
}

__host__ __device__ inline int64_t ff_attn_fwd_lds_floats(int T, int D, int H) {
  return static_cast<int64_t>(T) * (D + 4) + 2 * static_cast<int64_t>(D) + static_cast<int64_t>(H) * T + T + static_cast<int64_t>(FF_WAVES) * D;
}
__host__ __device__ inline int64_t ff_attn_bwd_lds_floats(int T, int D, int H) {
  return static_cast<int64_t>(T) * (D + 4) + 4 * static_cast<int64_t>(D) + 4 * static_cast<int64_t>(H) * T;
}

__global__ __launch_bounds__(FF_THREADS) void ff_attn_fwd_kernel(FfAttn a) {
  extern __shared__ float4 ff_lds4[];
  float* lds = reinterpret_cast<float*>(ff_lds4);
  const int T = a.T, D = a.D, H = a.heads, hd = D / H, ldq = D + 4, D4 = D / 4;
  float* sq = lds;                   // [T][D + 4] the biased Q rows (row pitch off a multiple of 32 banks)
  float* spq = sq + T * ldq;         // [D]
  float* spk = spq + D;              // [D]
  float* swr = spk + D;              // [FF_WAVES][D] one K * pooled_query row per wave
  float* sw = swr + FF_WAVES * D;    // [H][T]
  float* sm = sw + H * T;            // [T] additive mask term
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t n = blockIdx.x;
  const int64_t base = n * T * D;

  for (int i = threadIdx.x; i < T * D4; i += FF_THREADS) {
    const int t = i / D4, c = (i - t * D4) * 4;
    float4 q = *reinterpret_cast<const float4*>(a.Q + base + t * D + c);
    const float4 b = *reinterpret_cast<const float4*>(a.bq + c);
    q.x += b.x; q.y += b.y; q.z += b.z; q.w += b.w;
    *reinterpret_cast<float4*>(sq + t * ldq + c) = q;
    *reinterpret_cast<float4*>(a.Q + base + t * D + c) = q;
    if (a.SV0 != nullptr) {
      const float4 bt = *reinterpret_cast<const float4*>(a.btr + c);
      *reinterpret_cast<float4*>(a.SV0 + base + t * D + c) = make_float4(q.x + bt.x, q.y + bt.y, q.z + bt.z, q.w + bt.w);
    }
  }
  for (int t = threadIdx.x; t < T; t += FF_THREADS) sm[t] = (1.0f - a.mask[n * T + t]) * FF_MASK_NEG;
  __syncthreads();
  for (int t = wave; t < T; t += FF_WAVES) ff_row_logits(sq + t * ldq, a.Wqa, a.bqa, sw, t, T, D, H, a.inv, sm[t]);
  __syncthreads();
  ff_softmax_rows(sw, a.qw + n * H * T, T, H);
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += FF_THREADS) {
    const float* wr = sw + (c / hd) * T;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc = fmaf(wr[t], sq[t * ldq + c], acc);
    spq[c] = acc;
    a.pq[n * D + c] = acc;
  }
  __syncthreads();
  // second stage on K * pooled_query; the biased K goes back to global for the pooling below and for the backward
  for (int t0 = 0; t0 < T; t0 += FF_WAVES) {
    const int t = t0 + wave;
    float* row = swr + wave * D;
    if (t < T) {
      for (int c = lane * 4; c < D; c += 256) {
        float4 k = *reinterpret_cast<const float4*>(a.K + base + t * D + c);
        const float4 b = *reinterpret_cast<const float4*>(a.bk + c);
        k.x += b.x; k.y += b.y; k.z += b.z; k.w += b.w;
        *reinterpret_cast<float4*>(a.K + base + t * D + c) = k;
        const float4 p = *reinterpret_cast<const float4*>(spq + c);
        *reinterpret_cast<float4*>(row + c) = make_float4(k.x * p.x, k.y * p.y, k.z * p.z, k.w * p.w);
      }
    }
    __syncthreads();
    if (t < T) ff_row_logits(row, a.Wka, a.bka, sw, t, T, D, H, a.inv, sm[t]);
    __syncthreads();
  }
  ff_softmax_rows(sw, a.kw + n * H * T, T, H);
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += FF_THREADS) {
    const float* wr = sw + (c / hd) * T;
    const float p = spq[c];
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc = fmaf(wr[t], a.K[base + t * D + c] * p, acc);
    spk[c] = acc;
    a.pk[n * D + c] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T * D4; i += FF_THREADS) {
    const int t = i / D4, c = (i - t * D4) * 4;
    const float4 q = *reinterpret_cast<const float4*>(sq + t * ldq + c);
    const float4 p = *reinterpret_cast<const float4*>(spk + c);
    *reinterpret_cast<float4*>(a.AO + base + t * D + c) = make_float4(q.x * p.x, q.y * p.y, q.z * p.z, q.w * p.w);
  }
}

// workgroup g walks the sequences g, g + grid, ...; the logit-weight gradients and the three column sums stay in registers across them
__global__ __launch_bounds__(FF_THREADS) void ff_attn_bwd_kernel(FfAttn a) {
  extern __shared__ float4 ff_lds4[];
  float* lds = reinterpret_cast<float*>(ff_lds4);
  const int T = a.T, D = a.D, H = a.heads, hd = D / H, ldq = D + 4, D4 = D / 4, HD = H * D;
  float* sq = lds;             // [T][D + 4]
  float* spq = sq + T * ldq;   // [D]
  float* spk = spq + D;
  float* sdpq = spk + D;
  float* sdpk = sdpq + D;
  float* sa = sdpk + D;        // [H][T] query weights
  float* sb = sa + H * T;      // key weights
  float* sd1 = sb + H * T;     // d(query logits)
  float* sd2 = sd1 + H * T;    // d(key logits)
  float accq[FF_ATT_ACC], acck[FF_ATT_ACC], accb[3][FF_ATT_MAX_D / FF_THREADS];
#pragma unroll
  for (int j = 0; j < FF_ATT_ACC; ++j) accq[j] = acck[j] = 0.f;
#pragma unroll
  for (int j = 0; j < FF_ATT_MAX_D / FF_THREADS; ++j) accb[0][j] = accb[1][j] = accb[2][j] = 0.f;

  for (int64_t n = blockIdx.x; n < a.n_seq; n += gridDim.x) {
    const int64_t base = n * T * D;
    for (int i = threadIdx.x; i < T * D4; i += FF_THREADS) {
      const int t = i / D4, c = (i - t * D4) * 4;
      *reinterpret_cast<float4*>(sq + t * ldq + c) = *reinterpret_cast<const float4*>(a.Q + base + t * D + c);
    }
    for (int i = threadIdx.x; i < H * T; i += FF_THREADS) {
      sa[i] = a.qw[n * H * T + i];
      sb[i] = a.kw[n * H * T + i];
    }
    for (int c = threadIdx.x; c < D; c += FF_THREADS) {
      spq[c] = a.pq[n * D + c];
      spk[c] = a.pk[n * D + c];
    }
    __syncthreads();
    // d(pooled key)
    for (int c = threadIdx.x; c < D; c += FF_THREADS) {
      float acc = 0.f;
      for (int t = 0; t < T; ++t) acc = fmaf(a.dAO[base + t * D + c], sq[t * ldq + c], acc);
      sdpk[c] = acc;
    }
    __syncthreads();
    // d(key weights)[h][t] = sum over the head's columns of d(pooled key) * K * pooled_query
    for (int i = threadIdx.x; i < H * T; i += FF_THREADS) {
      const int t = i / H, h = i - t * H;
      float acc = 0.f;
      for (int j = 0; j < hd; ++j) {
        const int c = h * hd + j;
        acc = fmaf(sdpk[c], a.K[base + t * D + c] * spq[c], acc);
      }
      sd2[h * T + t] = acc;
    }
    __syncthreads();
    ff_softmax_bwd_rows(sb, sd2, T, H);
    __syncthreads();
    // d(K * pooled_query) per element -> dK, d(pooled query), column sum of dK
#pragma unroll
    for (int j = 0; j < FF_ATT_MAX_D / FF_THREADS; ++j) {
      const int c = threadIdx.x + j * FF_THREADS;
      if (c < D) {
        const int h = c / hd;
        const float dpk = sdpk[c], pqc = spq[c];
        float dpq = 0.f, colk = 0.f;
        for (int t = 0; t < T; ++t) {
          float lin = 0.f;
          for (int g = 0; g < H; ++g) lin = fmaf(sd2[g * T + t], a.Wka[g * D + c], lin);
          const float dkp = fmaf(sb[h * T + t], dpk, a.inv * lin);
          const float dk = dkp * pqc;
          a.dK[base + t * D + c] = dk;
          colk += dk;
          dpq = fmaf(dkp, a.K[base + t * D + c], dpq);
        }
        sdpq[c] = dpq;
        accb[1][j] += colk;
      }
    }
    // d(key logit weight)[h][c] += sum_t d(logit)[h][t] K[t][c] pooled_query[c]
#pragma unroll
    for (int j = 0; j < FF_ATT_ACC; ++j) {
      const int e = threadIdx.x + j * FF_THREADS;
      if (e < HD) {
        const int h = e / D, c = e - h * D;
        float acc = 0.f;
        for (int t = 0; t < T; ++t) acc = fmaf(sd2[h * T + t], a.K[base + t * D + c], acc);
        acck[j] = fmaf(acc, spq[c], acck[j]);
      }
    }
    __syncthreads();
    // d(query weights)[h][t]
    for (int i = threadIdx.x; i < H * T; i += FF_THREADS) {
      const int t = i / H, h = i - t * H;
      float acc = 0.f;
      for (int j = 0; j < hd; ++j) {
        const int c = h * hd + j;
        acc = fmaf(sdpq[c], sq[t * ldq + c], acc);
      }
      sd1[h * T + t] = acc;
    }
    __syncthreads();
    ff_softmax_bwd_rows(sa, sd1, T, H);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FF_ATT_MAX_D / FF_THREADS; ++j) {
      const int c = threadIdx.x + j * FF_THREADS;
      if (c < D) {
        const int h = c / hd;
        const float pkc = spk[c], dpq = sdpq[c];
        float colq = 0.f, colt = 0.f;
        for (int t = 0; t < T; ++t) {
          float lin = 0.f;
          for (int g = 0; g < H; ++g) lin = fmaf(sd1[g * T + t], a.Wqa[g * D + c], lin);
          float dq = fmaf(a.dAO[base + t * D + c], pkc, sa[h * T + t] * dpq);
          dq = fmaf(a.inv, lin, dq);
          if (a.dSV != nullptr) {
            const float ds = a.dSV[base + t * D + c];
            dq += ds;
            colt += ds;
          }
          a.dQ[base + t * D + c] = dq;
          colq += dq;
        }
        accb[0][j] += colq;
        accb[2][j] += colt;
      }
    }
#pragma unroll
    for (int j = 0; j < FF_ATT_ACC; ++j) {
      const int e = threadIdx.x + j * FF_THREADS;
      if (e < HD) {
        const int h = e / D, c = e - h * D;
        float acc = 0.f;
        for (int t = 0; t < T; ++t) acc = fmaf(sd1[h * T + t], sq[t * ldq + c], acc);
        accq[j] += acc;
      }
    }
    __syncthreads();
  }
  float* out = a.partials + static_cast<int64_t>(blockIdx.x) * (2 * static_cast<int64_t>(HD) + 3 * static_cast<int64_t>(D));
#pragma unroll
  for (int j = 0; j < FF_ATT_ACC; ++j) {
    const int e = threadIdx.x + j * FF_THREADS;
    if (e < HD) {
      out[e] = accq[j] * a.inv;
      out[HD + e] = acck[j] * a.inv;
    }
  }
#pragma unroll
  for (int j = 0; j < FF_ATT_MAX_D / FF_THREADS; ++j) {
    const int c = threadIdx.x + j * FF_THREADS;
    if (c < D) {
      out[2 * HD + c] = accb[0][j];
      out[2 * HD + D + c] = accb[1][j];
      out[2 * HD + 2 * D + c] = accb[2][j];
    }
  }
}

int64_t ff_ln_blocks(int64_t R) {
  int64_t nb = ebn_ceil_div(R, 32);
  if (nb > FF_MAX_PARTS) nb = FF_MAX_PARTS;
  return nb < 1 ? 1 : nb;
}

int ff_ln_check(int64_t R, int32_t D, int32_t mode) {
  EBN_REQUIRE(R >= 0 && D > 0 && (mode == 0 || mode == 1), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(D <= FF_LN_MAX_D && R <= EBN_DIM_MAX && ebn_sat_mul(R, D) < (int64_t(1) << 40), EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(ebn_ceil_div(R, FF_WAVES) <= INT32_MAX, EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

int ff_attn_check(int64_t n_seq, int32_t T, int32_t D, int32_t heads, bool bwd) {
  EBN_REQUIRE(n_seq >= 0 && T > 0 && D > 0 && heads > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(D % heads == 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(D % 4 == 0 && D <= FF_ATT_MAX_D && T <= 4096 && n_seq <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(static_cast<int64_t>(heads) * D <= FF_ATT_ACC * FF_THREADS, EBN_ERR_UNSUPPORTED);
  const int64_t fl = bwd ? ff_attn_bwd_lds_floats(T, D, heads) : ff_attn_fwd_lds_floats(T, D, heads);
  EBN_REQUIRE(fl * 4 <= FF_LDS_BYTES, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(ebn_sat_mul(ebn_sat_mul(n_seq, T), D) < (int64_t(1) << 40), EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

int ff_pool_check(int64_t n_seq, int32_t L, int32_t D) {
  EBN_REQUIRE(n_seq >= 0 && L > 0 && D > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(L <= FF_POOL_MAX_L && D <= 65536 && n_seq <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(ebn_sat_mul(ebn_sat_mul(n_seq, L), D) < (int64_t(1) << 40), EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

}  // namespace

extern "C" int ebn_ff_ln_fwd_f32(const float* X, const float* bias, const float* res, const float* gamma, const float* beta,
                                 float eps, int32_t mode, uint32_t drop_key, float drop_p, float* Y, float* xhat, float* rstd,
                                 int64_t R, int32_t D, ebn_stream_t stream) {
  EBN_REQUIRE(X && bias && res && gamma && beta && Y, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(drop_p >= 0.f && drop_p < 1.f, EBN_ERR_BAD_ARG);
  const int rc = ff_ln_check(R, D, mode);
  if (rc != EBN_OK) return rc;
  if (R == 0) return EBN_OK;
  EBN_LAUNCH(ff_ln_fwd_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(R, FF_WAVES))), dim3(FF_THREADS), 0, ebn_stream(stream), X,
             bias, res, gamma, beta, eps, mode, ff_make_drop(drop_key, drop_p), Y, xhat, rstd, R, D);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int64_t ebn_ff_ln_partials_len(int64_t R, int32_t D) {
  if (!ebn_dim_ok(R, D) || D > FF_LN_MAX_D) return 0;
  return ff_ln_blocks(R) * 3 * D;
}

extern "C" int ebn_ff_ln_bwd_f32(const float* dY, const float* xhat, const float* rstd, const float* gamma, int32_t mode,
                                 uint32_t drop_key, float drop_p, float* dX, float* dres, float* partials, int32_t* n_parts,
                                 int64_t R, int32_t D, ebn_stream_t stream) {
  EBN_REQUIRE(dY && xhat && rstd && gamma && dX && partials && n_parts, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(drop_p >= 0.f && drop_p < 1.f, EBN_ERR_BAD_ARG);
  const int rc = ff_ln_check(R, D, mode);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(mode == 0 || dres != nullptr, EBN_ERR_BAD_ARG);
  const int64_t nb = ff_ln_blocks(R);
  *n_parts = static_cast<int32_t>(nb);
  // R == 0 still writes one (zero) partial: the finishing pass then yields zero gradients
  EBN_LAUNCH(ff_ln_bwd_kernel, dim3(static_cast<uint32_t>(nb)), dim3(FF_THREADS), static_cast<size_t>(FF_WAVES) * 3 * D * sizeof(float),
             ebn_stream(stream), dY, xhat, rstd, gamma, mode, ff_make_drop(drop_key, drop_p), dX, dres, partials, R, D,
             ebn_ceil_div(R > 0 ? R : 1, nb));
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_colsum_finish_f32(const float* partials, int64_t n_parts, int64_t stride, int64_t width, float* out,
                                        ebn_stream_t stream) {
  EBN_REQUIRE(partials && out && n_parts >= 0 && width >= 0 && stride >= width, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_ceil_div(width, 64) <= INT32_MAX && ebn_sat_mul(n_parts, stride) < (int64_t(1) << 40), EBN_ERR_UNSUPPORTED);
  if (width == 0) return EBN_OK;
  EBN_LAUNCH(ff_colsum_finish_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(width, 64))), dim3(FF_THREADS), 0, ebn_stream(stream),
             partials, n_parts, stride, width, out);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_gelu_fwd_f32(const float* X, const float* bias, float* Y, int64_t R, int32_t C, ebn_stream_t stream) {
  EBN_REQUIRE(X && bias && Y && R >= 0 && C > 0, EBN_ERR_BAD_ARG);
  const int64_t n = ebn_sat_mul(R, C);
  EBN_REQUIRE(R <= EBN_DIM_MAX && n < (int64_t(1) << 38), EBN_ERR_UNSUPPORTED);
  if (n == 0) return EBN_OK;
  EBN_LAUNCH(ff_gelu_fwd_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(n, FF_THREADS))), dim3(FF_THREADS), 0, ebn_stream(stream), X,
             bias, Y, n, C);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_gelu_bwd_f32(const float* X, const float* bias, const float* dY, float* dX, float* dbias, float* partials,
                                   int64_t R, int32_t C, ebn_stream_t stream) {
  EBN_REQUIRE(X && bias && dY && dX && dbias && partials && R >= 0 && C > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(R <= EBN_DIM_MAX && C <= (1 << 22) && ebn_sat_mul(R, C) < (int64_t(1) << 38), EBN_ERR_UNSUPPORTED);
  FfGeluBwd f{X, bias, dY, dX, C};
  int64_t nb = 0;
  ebn_colred_stage1(f, partials, R, C, ebn_stream(stream), &nb);
  EBN_CHECK_LAUNCH();
  EBN_LAUNCH(ff_colsum_finish_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(C, 64))), dim3(FF_THREADS), 0, ebn_stream(stream),
             partials, nb, static_cast<int64_t>(2) * C, static_cast<int64_t>(C), dbias);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_pool_fwd_f32(float* U, const float* b1, const float* w2, const float* b2, const float* X, const float* mask,
                                   float* out, float* w, float* sinv, int64_t n_seq, int32_t L, int32_t D, ebn_stream_t stream) {
  EBN_REQUIRE(U && b1 && w2 && b2 && X && mask && out && w && sinv, EBN_ERR_BAD_ARG);
  const int rc = ff_pool_check(n_seq, L, D);
  if (rc != EBN_OK) return rc;
  if (n_seq == 0) return EBN_OK;
  EBN_LAUNCH(ff_pool_fwd_kernel, dim3(static_cast<uint32_t>(n_seq)), dim3(FF_THREADS), static_cast<size_t>(L + 4) * sizeof(float),
             ebn_stream(stream), U, b1, w2, b2, X, mask, out, w, sinv, L, D);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_pool_bwd_f32(const float* X, const float* w, const float* sinv, const float* dout, float* dX, float* de,
                                   float* db2n, int64_t n_seq, int32_t L, int32_t D, ebn_stream_t stream) {
  EBN_REQUIRE(X && w && sinv && dout && dX && de && db2n, EBN_ERR_BAD_ARG);
  const int rc = ff_pool_check(n_seq, L, D);
  if (rc != EBN_OK) return rc;
  if (n_seq == 0) return EBN_OK;
  EBN_LAUNCH(ff_pool_bwd_kernel, dim3(static_cast<uint32_t>(n_seq)), dim3(FF_THREADS), static_cast<size_t>(L + 4) * sizeof(float),
             ebn_stream(stream), X, w, sinv, dout, dX, de, db2n, L, D);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_head_fwd_f32(const float* user, const float* cand, const float* W, const float* b, float* score, int64_t N,
                                   int32_t D, ebn_stream_t stream) {
  EBN_REQUIRE(user && cand && W && b && score && N >= 0 && D > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(N <= EBN_DIM_MAX && D <= 65536, EBN_ERR_UNSUPPORTED);
  if (N == 0) return EBN_OK;
  EBN_LAUNCH(ff_head_fwd_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(N, FF_WAVES))), dim3(FF_THREADS), 0, ebn_stream(stream),
             user, cand, W, b, score, N, D);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_head_bwd_f32(const float* user, const float* cand, const float* W, const float* score, const float* dscore,
                                   float* duser, float* dcand, float* dW, float* db, int64_t N, int32_t D, ebn_stream_t stream) {
  EBN_REQUIRE(user && cand && W && score && dscore && duser && dcand && dW && db && N >= 0 && D > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(N <= EBN_DIM_MAX && D <= 65536, EBN_ERR_UNSUPPORTED);
  const int col_blocks = static_cast<int>(ebn_ceil_div(2 * static_cast<int64_t>(D), FF_THREADS));
  EBN_LAUNCH(ff_head_bwd_kernel, dim3(static_cast<uint32_t>(col_blocks + ebn_ceil_div(N, FF_WAVES))), dim3(FF_THREADS), 0,
             ebn_stream(stream), user, cand, W, score, dscore, duser, dcand, dW, db, N, D, col_blocks);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_attn_fwd_f32(float* Q, float* K, const float* bq, const float* bk, const float* btr, const float* Wqa,
                                   const float* bqa, const float* Wka, const float* bka, const float* mask, float* AO, float* SV0,
                                   float* qw, float* kw, float* pq, float* pk, int64_t n_seq, int32_t T, int32_t D, int32_t heads,
                                   ebn_stream_t stream) {
  EBN_REQUIRE(Q && K && bq && bk && Wqa && bqa && Wka && bka && mask && AO && qw && kw && pq && pk, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(SV0 == nullptr || btr != nullptr, EBN_ERR_BAD_ARG);
  const int rc = ff_attn_check(n_seq, T, D, heads, false);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(ebn_aligned16(Q) && ebn_aligned16(K) && ebn_aligned16(bq) && ebn_aligned16(bk) && ebn_aligned16(Wqa) &&
                  ebn_aligned16(Wka) && ebn_aligned16(AO) && ebn_aligned16(SV0) && ebn_aligned16(btr),
              EBN_ERR_ALIGN);
  if (n_seq == 0) return EBN_OK;
  FfAttn a{};
  a.Q = Q; a.K = K; a.bq = bq; a.bk = bk; a.btr = btr; a.Wqa = Wqa; a.bqa = bqa; a.Wka = Wka; a.bka = bka; a.mask = mask;
  a.AO = AO; a.SV0 = SV0; a.qw = qw; a.kw = kw; a.pq = pq; a.pk = pk;
  a.n_seq = n_seq; a.T = T; a.D = D; a.heads = heads;
  a.inv = 1.0f / sqrtf(static_cast<float>(D / heads));
  EBN_LAUNCH(ff_attn_fwd_kernel, dim3(static_cast<uint32_t>(n_seq)), dim3(FF_THREADS),
             static_cast<size_t>(ff_attn_fwd_lds_floats(T, D, heads)) * sizeof(float), ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_attn_supported(int32_t T, int32_t D, int32_t heads, int32_t with_backward) {
  const int rc = ff_attn_check(0, T, D, heads, false);
  if (rc != EBN_OK || !with_backward) return rc;
  return ff_attn_check(0, T, D, heads, true);
}

extern "C" int64_t ebn_ff_attn_partials_len(int64_t n_seq, int32_t D, int32_t heads) {
  if (!ebn_dim_ok(n_seq, D, heads)) return 0;
  return ebn_sat_mul(ff_attn_grid(n_seq), 2 * static_cast<int64_t>(heads) * D + 3 * static_cast<int64_t>(D));
}

extern "C" int ebn_ff_attn_bwd_f32(const float* Q, const float* K, const float* Wqa, const float* Wka, const float* qw,
                                   const float* kw, const float* pq, const float* pk, const float* dAO, const float* dSV, float* dQ,
                                   float* dK, float* partials, int32_t* n_parts, int64_t n_seq, int32_t T, int32_t D, int32_t heads,
                                   ebn_stream_t stream) {
  EBN_REQUIRE(Q && K && Wqa && Wka && qw && kw && pq && pk && dAO && dQ && dK && partials && n_parts, EBN_ERR_BAD_ARG);
  const int rc = ff_attn_check(n_seq, T, D, heads, true);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(ebn_aligned16(Q), EBN_ERR_ALIGN);
  const int64_t grid = ff_attn_grid(n_seq);
  *n_parts = static_cast<int32_t>(grid);
  FfAttn a{};
  a.Q = const_cast<float*>(Q); a.K = const_cast<float*>(K); a.Wqa = Wqa; a.Wka = Wka;
  a.qw = const_cast<float*>(qw); a.kw = const_cast<float*>(kw); a.pq = const_cast<float*>(pq); a.pk = const_cast<float*>(pk);
  a.dAO = dAO; a.dSV = dSV; a.dQ = dQ; a.dK = dK; a.partials = partials;
  a.n_seq = n_seq; a.T = T; a.D = D; a.heads = heads;
  a.inv = 1.0f / sqrtf(static_cast<float>(D / heads));
  // n_seq == 0: one workgroup writes one zero partial
  EBN_LAUNCH(ff_attn_bwd_kernel, dim3(static_cast<uint32_t>(grid)), dim3(FF_THREADS),
             static_cast<size_t>(ff_attn_bwd_lds_floats(T, D, heads)) * sizeof(float), ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_ln_pos_fwd_f32(const float* X, const float* bias, const float* pos, const float* gamma, const float* beta,
                                     float eps, uint32_t drop_key, float drop_p, float* Y, float* xhat, float* rstd, int64_t n_seq,
                                     int32_t T, int32_t D, ebn_stream_t stream) {
  EBN_REQUIRE(X && pos && gamma && beta && Y, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(drop_p >= 0.f && drop_p < 1.f, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_seq >= 0 && T > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_seq <= EBN_DIM_MAX && ebn_sat_mul(n_seq, T) <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  const int64_t R = n_seq * T;
  const int rc = ff_ln_check(R, D, 0);
  if (rc != EBN_OK) return rc;
  if (R == 0) return EBN_OK;
  EBN_LAUNCH(ff_ln_pos_fwd_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(R, FF_WAVES))), dim3(FF_THREADS), 0, ebn_stream(stream), X,
             bias, pos, gamma, beta, eps, ff_make_drop(drop_key, drop_p), Y, xhat, rstd, R, T, D);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ff_cls_fwd_f32(const float* X, const float* W, const float* b, const int64_t* targets, float* logits, float* prob,
                                  float* rowloss, float* loss, int32_t* flag, int64_t N, int32_t D, int32_t C, ebn_stream_t stream) {
  EBN_REQUIRE(X && W && b && targets && logits && prob && rowloss && loss && flag, EBN_ERR_BAD_ARG);
  const int rc = ff_cls_check(N, D, C);
  if (rc != EBN_OK) return rc;
  if (N > 0) {
    EBN_LAUNCH(ff_cls_fwd_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(N, FF_WAVES))), dim3(FF_THREADS), 0, ebn_stream(stream), X,
               W, b, targets, logits, prob, rowloss, flag, N, D, C);
    EBN_CHECK_LAUNCH();
  }
  EBN_LAUNCH(ff_cls_loss_kernel, dim3(1), dim3(FF_THREADS), 0, ebn_stream(stream), rowloss, loss, N);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int64_t ebn_ff_cls_partials_len(int64_t N, int32_t D, int32_t C) {
  if (!ebn_dim_ok(N, D, C) || D > FF_CLS_MAX_D || C > FF_CLS_MAX_C) return 0;
  return ff_cls_blocks(N) * (static_cast<int64_t>(C) * D + C);
}

extern "C" int ebn_ff_cls_bwd_f32(const float* X, const float* W, const float* prob, const int64_t* targets, const float* dloss,
                                  const float* dscore, float* dX, float* partials, int32_t* n_parts, int64_t N, int32_t D, int32_t C,
                                  ebn_stream_t stream) {
  EBN_REQUIRE(X && W && prob && targets && dX && partials && n_parts, EBN_ERR_BAD_ARG);
  const int rc = ff_cls_check(N, D, C);
  if (rc != EBN_OK) return rc;
  const int64_t nb = ff_cls_blocks(N);
  *n_parts = static_cast<int32_t>(nb);
  // N == 0 still writes one (zero) partial: the finishing pass then yields zero gradients
  EBN_LAUNCH(ff_cls_bwd_kernel, dim3(static_cast<uint32_t>(nb)), dim3(FF_THREADS), 0, ebn_stream(stream), X, W, prob, targets, dloss,
             dscore, dX, partials, N, D, C, ebn_ceil_div(N > 0 ? N : 1, nb));
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
