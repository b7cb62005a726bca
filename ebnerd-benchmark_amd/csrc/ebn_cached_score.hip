// Scoring from a once-encoded article catalogue (scorer.predict of LSTUR / NAML over an eval loader): everything that depends on
// the article alone is computed once per predict() -- the news vector, and for NAML the user encoder's AttLayer2 logit
// a = exp(tanh(x.W + b).q) (naml.py user encoder: an UNMASKED AttLayer2, layers.py:55-81, so a history item's logit does not depend
// on its neighbours) -- and an impression then costs index-driven row reads:
//   * att_logit_rows_kernel: a[r] of every catalogue row from the pre-activations X.W (one wave per row, the arithmetic of
//     ebn_attpool_fwd_f32: lane-strided fmaf over A, wave tree, expf, no max-subtraction);
//   * indexed_attpool_score_kernel: one workgroup per impression -- w_l = a[idx_l] / (sum a + 1e-7), user = sum_l w_l news[idx_l]
//     (kept in LDS), then act(user . news[cand]) for every candidate of the impression's CSR span.
// The second kernel is bound by row reads: rows are read as float4, four rows in flight per wave (the register-gather form of
// random whole rows), and every sum has a fixed order (no atomics): two runs give the same bits.  A row number outside
// [0, n_rows) sets *oob_flag and is never turned into an address; an offsets pair that runs backwards or leaves [0, n_cand] makes
// that impression's candidate list empty.
#include "ebn_common.h"

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_WAVES = CS_THREADS / 64;
constexpr int CS_ROWS = 4;          // rows in flight per wave / per column group
constexpr int CS_MAX_H = 2048;      // history positions of one impression (LDS: 8 bytes each)
constexpr int CS_MAX_F = 8192;      // news vector width (LDS: 4 bytes each)
constexpr int CS_PART = 4 * CS_THREADS;  // floats of the pooling's per-group partial sums
constexpr float KERAS_EPS = 1e-7f;  // K.epsilon(), layers.py:75-77

__global__ __launch_bounds__(CS_THREADS) void att_logit_rows_kernel(const float* __restrict__ U, const float* __restrict__ b,
                                                                    const float* __restrict__ q, float* __restrict__ a, int64_t n, int A) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * CS_WAVES + (threadIdx.x >> 6);
  if (r >= n) return;
  const float* urow = U + r * A;
  float part = 0.f;
  for (int k = lane; k < A; k += 64) part = fmaf(tanhf(urow[k] + b[k]), q[k], part);
  part = ebn_wave_sum(part);
  if (lane == 0) a[r] = expf(part);
}

__device__ __forceinline__ float4 cs_fma4(float w, float4 x, float4 acc) {
  acc.x = fmaf(w, x.x, acc.x);
  acc.y = fmaf(w, x.y, acc.y);
  acc.z = fmaf(w, x.z, acc.z);
  acc.w = fmaf(w, x.w, acc.w);
  return acc;
}

// LDS (dynamic): hrow int[H] | hw float[H] | user float[F] | part float[CS_PART]
__global__ __launch_bounds__(CS_THREADS) void indexed_attpool_score_kernel(const float* __restrict__ news, const float* __restrict__ a_all,
                                                                           int64_t n_rows, const int32_t* __restrict__ his_idx,
                                                                           const int32_t* __restrict__ cand_idx,
                                                                           const int64_t* __restrict__ offsets, int64_t n_cand,
                                                                           float* __restrict__ scores, float* __restrict__ user_out,
                                                                           int32_t* __restrict__ oob_flag, int H, int F, int mode) {
  extern __shared__ float4 cs_smem[];
  const int Hp = (H + 1) & ~1;  // the user vector behind the two H-long arrays stays 16-byte aligned
  int* hrow = reinterpret_cast<int*>(cs_smem);
  float* hw = reinterpret_cast<float*>(hrow + Hp);
  float* user = hw + Hp;
  float* part = user + F;
  __shared__ float s_sum;
  const int64_t imp = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int F4 = F / 4;
  bool bad = false;

  // 1. the history's logits: a missing row contributes nothing
  for (int l = tid; l < H; l += CS_THREADS) {
    const int32_t r = his_idx[imp * H + l];
    const bool ok = r >= 0 && static_cast<int64_t>(r) < n_rows;
    bad |= !ok;
    hrow[l] = ok ? r : -1;
    hw[l] = ok ? a_all[r] : 0.f;
  }
  __syncthreads();
  if (wave == 0) {
    float s = 0.f;
    for (int l = lane; l < H; l += 64) s += hw[l];
    s = ebn_wave_sum(s) + KERAS_EPS;
    if (lane == 0) s_sum = s;
  }
  __syncthreads();
  const float denom = s_sum;
  for (int l = tid; l < H; l += CS_THREADS) hw[l] = hw[l] / denom;  // w_l; a missing row: 0 / s == 0 exactly
  __syncthreads();

  // 2. user = sum_l w_l news[idx_l]: ncol float4 columns x ng groups of history positions (group g takes l = g, g + ng, ...),
  //    CS_ROWS rows requested before the first is used; the groups' partial sums are added in group order
  const int ncol = F4 < CS_THREADS ? F4 : CS_THREADS;
  const int ng = CS_THREADS / ncol;
  const int g = tid / ncol, tc = tid - g * ncol;
  for (int c0 = 0; c0 < F4; c0 += ncol) {
    const int c4 = c0 + tc;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g < ng && c4 < F4) {
      for (int l0 = g; l0 < H; l0 += ng * CS_ROWS) {
        float4 x[CS_ROWS];
        float w[CS_ROWS];
#pragma unroll
        for (int j = 0; j < CS_ROWS; ++j) {
          const int l = l0 + j * ng;
          const int r = l < H ? hrow[l] : -1;
          x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
          w[j] = 0.f;
          if (r >= 0) {
            x[j] = *reinterpret_cast<const float4*>(news + static_cast<int64_t>(r) * F + 4 * c4);
            w[j] = hw[l];
          }
        }
#pragma unroll
        for (int j = 0; j < CS_ROWS; ++j) acc = cs_fma4(w[j], x[j], acc);
      }
    }
    if (ng == 1) {
      if (g < ng && c4 < F4) *reinterpret_cast<float4*>(user + 4 * c4) = acc;
    } else {  // F4 <= 128: one pass over the columns, ng * F <= CS_PART floats
      if (g < ng) *reinterpret_cast<float4*>(part + (g * ncol + tc) * 4) = acc;
      __syncthreads();
      for (int c = tid; c < F; c += CS_THREADS) {
        float s = 0.f;
        for (int k = 0; k < ng; ++k) s += part[k * F + c];
        user[c] = s;
      }
    }
  }
  __syncthreads();
  if (user_out != nullptr)
    for (int c = tid; c < F; c += CS_THREADS) user_out[imp * F + c] = user[c];

  // 3. the impression's candidates: one wave per candidate, CS_ROWS candidates in flight per wave
  const int64_t o0 = offsets[imp], o1 = offsets[imp + 1];
  const bool span_ok = o0 >= 0 && o1 >= o0 && o1 <= n_cand;
  const int64_t beg = span_ok ? o0 : 0, len = span_ok ? o1 - o0 : 0;
  for (int64_t p0 = static_cast<int64_t>(wave) * CS_ROWS; p0 < len; p0 += CS_WAVES * CS_ROWS) {
    int row[CS_ROWS];
    float dot[CS_ROWS];
#pragma unroll
    for (int j = 0; j < CS_ROWS; ++j) {
      int32_t r = -1;
      if (p0 + j < len) {
        r = cand_idx[beg + p0 + j];
        const bool ok = r >= 0 && static_cast<int64_t>(r) < n_rows;
        bad |= !ok;
        if (!ok) r = -1;
      }
      row[j] = r;
      dot[j] = 0.f;
    }
    for (int c4 = lane; c4 < F4; c4 += 64) {
      float4 x[CS_ROWS];
#pragma unroll
      for (int j = 0; j < CS_ROWS; ++j) {
        x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row[j] >= 0) x[j] = *reinterpret_cast<const float4*>(news + static_cast<int64_t>(row[j]) * F + 4 * c4);
      }
      const float4 u = *reinterpret_cast<const float4*>(user + 4 * c4);
#pragma unroll
      for (int j = 0; j < CS_ROWS; ++j)
        dot[j] = fmaf(u.w, x[j].w, fmaf(u.z, x[j].z, fmaf(u.y, x[j].y, fmaf(u.x, x[j].x, dot[j]))));
    }
#pragma unroll
    for (int j = 0; j < CS_ROWS; ++j) {
      const float s = ebn_wave_sum(dot[j]);
      if (lane == 0 && p0 + j < len) scores[beg + p0 + j] = (mode == 1) ? 1.0f / (1.0f + expf(-s)) : s;
    }
  }
  if (bad && oob_flag != nullptr) *oob_flag = 1;
}

}  // namespace

extern "C" int ebn_att_logit_rows_f32(const float* U, const float* b, const float* q, float* a, int64_t n_rows, int32_t A,
                                      ebn_stream_t stream) {
  EBN_REQUIRE(n_rows >= 0 && A >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_rows <= EBN_DIM_MAX && A <= CS_MAX_F, EBN_ERR_UNSUPPORTED);
  if (n_rows == 0) return EBN_OK;
  EBN_REQUIRE(U && b && q && a, EBN_ERR_BAD_ARG);
  EBN_LAUNCH(att_logit_rows_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(n_rows, CS_WAVES))), dim3(CS_THREADS), 0, ebn_stream(stream), U, b,
             q, a, n_rows, static_cast<int>(A));
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_indexed_attpool_score_f32(const float* news_all, const float* a_all, int64_t n_rows, const int32_t* his_idx,
                                             const int32_t* cand_idx, const int64_t* offsets, int64_t n_cand, float* scores, float* user,
                                             int32_t* oob_flag, int64_t B, int32_t H, int32_t F, int32_t mode, ebn_stream_t stream) {
  EBN_REQUIRE(n_rows >= 0 && n_cand >= 0 && B >= 0 && H >= 1 && F >= 1 && (mode == 0 || mode == 1), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_rows <= EBN_DIM_MAX && n_cand <= EBN_DIM_MAX && B <= EBN_DIM_MAX && H <= CS_MAX_H && F <= CS_MAX_F && F % 4 == 0,
              EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(ebn_sat_mul(B, H) <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  if (B == 0) return EBN_OK;
  EBN_REQUIRE(his_idx && offsets && (news_all || n_rows == 0) && (a_all || n_rows == 0) && (cand_idx || n_cand == 0) &&
                  (scores || n_cand == 0),
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_aligned16(news_all) && ebn_aligned16(user), EBN_ERR_ALIGN);
  const int Hp = (H + 1) & ~1;
  const size_t smem = static_cast<size_t>(Hp) * 8 + static_cast<size_t>(F) * 4 + static_cast<size_t>(CS_PART) * 4;
  EBN_LAUNCH(indexed_attpool_score_kernel, dim3(static_cast<unsigned>(B)), dim3(CS_THREADS), smem, ebn_stream(stream), news_all, a_all, n_rows,
             his_idx, cand_idx, offsets, n_cand, scores, user, oob_flag, static_cast<int>(H), static_cast<int>(F), static_cast<int>(mode));
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
