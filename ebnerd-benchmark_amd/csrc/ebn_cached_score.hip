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
// NPA (further down): the catalogue keeps each title's conv output Vd and tanh'd attention keys Ua; pap_indexed_kernel pools a
// title under a query (and scores it against a user vector) from those two blocks, bit-equal to ebn_pap_fwd_f32.
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

// ---- NPA from a once-encoded catalogue (npa.py:120-136, layers.py:312-339) --------------------------------------------------
// The personalised news vector depends on the user only through the logits s_l = q . Ua_l: the conv output Vd [L, F] and
// Ua = tanh(Vd.Wa + ba) [L, A] of a title are functions of the article alone and are kept per catalogue row.  A (query, article)
// pair then reads two contiguous blocks, L*A and L*F floats, and does A MACs per word and L MACs per column.
constexpr int PI_THREADS = 256;
constexpr int PI_WAVES = PI_THREADS / 64;
constexpr int PI_MAX_L = 256;     // as ebn_pap_fwd_f32
constexpr int PI_MAX_F = 4096;
constexpr int PI_STAGE = 8192;    // floats of Ua staged in LDS per pass (A above it, or A % 4 != 0: lane-strided reads from HBM)
constexpr int PI_ROWS = 8;        // Vd rows in flight per column group

// Ua <- tanh(Ua + ba): the expression of pap_fwd_kernel (ebn_npa.hip), so the catalogue holds the bits ebn_pap_fwd_f32 leaves in U
__global__ __launch_bounds__(PI_THREADS) void bias_tanh_rows_kernel(float* __restrict__ U, const float* __restrict__ ba, int64_t total,
                                                                    int A) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * PI_THREADS;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * PI_THREADS + threadIdx.x; i < total; i += stride)
    U[i] = tanhf(U[i] + ba[static_cast<int>(i % A)]);
}

// the query row of sequence n; an index outside [0, n_q) reads row 0 (pap_q_row of ebn_npa.hip)
__device__ __forceinline__ int64_t pap_q_row_cs(const int32_t* q_idx, int64_t n, int64_t n_q) {
  const int64_t i = q_idx[n];
  return (i >= 0 && i < n_q) ? i : 0;
}

// One workgroup per sequence n (the operations and their order are pap_fwd_kernel's: a word's logit is one wave's lane-strided
// fmaf over A and ebn_wave_sum, the softmax is max-subtracted, a column's pooled value is fmaf over l ascending -- with the same
// Ua and Vd bits, `out` equals ebn_pap_fwd_f32's on the gathered rows bit for bit).
// LDS (dynamic): pooled float[F] | stage float[stage_floats]
__global__ __launch_bounds__(PI_THREADS) void pap_indexed_kernel(const float* __restrict__ Ua_all, const float* __restrict__ Vd_all,
                                                                 int64_t n_rows, const int32_t* __restrict__ row_idx,
                                                                 const float* __restrict__ Q, const int32_t* __restrict__ q_idx,
                                                                 int64_t n_q, float* __restrict__ out, const float* __restrict__ users,
                                                                 float* __restrict__ scores, int32_t* __restrict__ oob_flag, int L, int F,
                                                                 int A, int G, int mode) {
  extern __shared__ float4 pi_smem[];
  float* pooled = reinterpret_cast<float*>(pi_smem);
  float* stage = pooled + F;
  __shared__ float sm[PI_MAX_L];
  __shared__ float red[PI_WAVES];
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int F4 = F / 4;
  const int64_t row = row_idx[n];
  if (row < 0 || row >= n_rows) {  // never an address: a zero vector, act(0)
    if (tid == 0) {
      if (oob_flag != nullptr) *oob_flag = 1;
      if (scores != nullptr) scores[n] = (mode == 1) ? 1.0f / (1.0f + expf(-0.f)) : 0.f;
    }
    if (out != nullptr)
      for (int c = tid; c < F; c += PI_THREADS) out[n * F + c] = 0.f;
    return;
  }
  const int64_t qrow = pap_q_row_cs(q_idx, n, n_q);
  const float* q = Q + qrow * A;
  const float* Ua = Ua_all + row * L * A;  // 64-bit: row * L * (A | F) passes 2^32 at catalogue sizes in use
  const float* Vd = Vd_all + row * L * F;

  // 1. logits.  G > 0: G words at a time go through LDS as float4 (the block of G words is contiguous and 16-byte aligned), and a
  //    wave then reads its word lane-strided from LDS -- the same k per lane, in the same order, as the direct form below
  if (G > 0) {
    for (int l0 = 0; l0 < L; l0 += G) {
      const int g = L - l0 < G ? L - l0 : G;
      const int n4 = g * (A / 4);
      const float4* src = reinterpret_cast<const float4*>(Ua + static_cast<int64_t>(l0) * A);
      for (int i = tid; i < n4; i += PI_THREADS) reinterpret_cast<float4*>(stage)[i] = src[i];
      __syncthreads();
      for (int j = wave; j < g; j += PI_WAVES) {
        const float* urow = stage + j * A;
        float part = 0.f;
        for (int k = lane; k < A; k += 64) part = fmaf(q[k], urow[k], part);
        part = ebn_wave_sum(part);
        if (lane == 0) sm[l0 + j] = part;
      }
      __syncthreads();
    }
  } else {
    for (int l = wave; l < L; l += PI_WAVES) {
      const float* urow = Ua + static_cast<int64_t>(l) * A;
      float part = 0.f;
      for (int k = lane; k < A; k += 64) part = fmaf(q[k], urow[k], part);
      part = ebn_wave_sum(part);
      if (lane == 0) sm[l] = part;
    }
    __syncthreads();
  }

  // 2. softmax over l
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
  for (int l = tid; l < L; l += PI_THREADS) sm[l] = expf(sm[l] - mx) / s;
  __syncthreads();

  // 3. pooled_c = sum_l w_l Vd[l, c]: a float4 column per thread, PI_ROWS rows requested before the first is used
  for (int c4 = tid; c4 < F4; c4 += PI_THREADS) {
    const float4* v = reinterpret_cast<const float4*>(Vd) + c4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l0 = 0; l0 < L; l0 += PI_ROWS) {
      float4 x[PI_ROWS];
#pragma unroll
      for (int j = 0; j < PI_ROWS; ++j)
        if (l0 + j < L) x[j] = v[static_cast<int64_t>(l0 + j) * F4];
#pragma unroll
      for (int j = 0; j < PI_ROWS; ++j)
        if (l0 + j < L) acc = cs_fma4(sm[l0 + j], x[j], acc);
    }
    *reinterpret_cast<float4*>(pooled + 4 * c4) = acc;
    if (out != nullptr) *reinterpret_cast<float4*>(out + n * F + 4 * c4) = acc;
  }
  if (scores == nullptr) return;
  __syncthreads();

  // 4. act(pooled . users[q]): the candidate vector never leaves the chip
  const float* u = users + qrow * F;
  float part = 0.f;
  for (int c = tid; c < F; c += PI_THREADS) part = fmaf(pooled[c], u[c], part);
  part = ebn_wave_sum(part);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  if (tid == 0) {
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < PI_WAVES; ++i) d += red[i];
    scores[n] = (mode == 1) ? 1.0f / (1.0f + expf(-d)) : d;
  }
}

}  // namespace

extern "C" int ebn_bias_tanh_rows_f32(float* U, const float* ba, int64_t n_rows, int32_t A, ebn_stream_t stream) {
  EBN_REQUIRE(n_rows >= 0 && A >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(A <= 65536 && ebn_sat_mul(n_rows, A) < (int64_t(1) << 40), EBN_ERR_UNSUPPORTED);
  if (n_rows == 0) return EBN_OK;
  EBN_REQUIRE(U && ba, EBN_ERR_BAD_ARG);
  const int64_t total = n_rows * A;
  const int64_t blocks = ebn_ceil_div(total, PI_THREADS);
  EBN_LAUNCH(bias_tanh_rows_kernel, dim3(static_cast<unsigned>(blocks < 16384 ? blocks : 16384)), dim3(PI_THREADS), 0, ebn_stream(stream), U,
             ba, total, static_cast<int>(A));
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_pap_indexed_f32(const float* Ua_all, const float* Vd_all, int64_t n_rows, const int32_t* row_idx, const float* Q,
                                   const int32_t* q_idx, int64_t n_q, float* out, const float* users, float* scores, int32_t mode,
                                   int32_t* oob_flag, int64_t n_seq, int32_t L, int32_t F, int32_t A, ebn_stream_t stream) {
  EBN_REQUIRE(n_rows >= 0 && n_seq >= 0 && L >= 1 && F >= 1 && A >= 1 && n_q >= 1 && (mode == 0 || mode == 1), EBN_ERR_BAD_ARG);
  EBN_REQUIRE((out || scores) && (users || !scores), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(L <= PI_MAX_L && F <= PI_MAX_F && F % 4 == 0 && A <= 65536, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(n_seq <= 0x7FFFFFFF && n_q <= EBN_DIM_MAX && n_rows <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  if (n_seq == 0) return EBN_OK;
  EBN_REQUIRE(row_idx && Q && q_idx && (Ua_all || n_rows == 0) && (Vd_all || n_rows == 0), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_aligned16(Ua_all) && ebn_aligned16(Vd_all) && ebn_aligned16(out), EBN_ERR_ALIGN);
  // words of Ua staged per pass: float4 staging needs every word 16-byte aligned and at least one word in the stage
  const int G = (A % 4 == 0 && A <= PI_STAGE) ? PI_STAGE / A : 0;
  const int words = G < L ? G : L;
  const size_t smem = (static_cast<size_t>(F) + static_cast<size_t>(words) * A) * 4;
  EBN_LAUNCH(pap_indexed_kernel, dim3(static_cast<unsigned>(n_seq)), dim3(PI_THREADS), smem, ebn_stream(stream), Ua_all, Vd_all, n_rows,
             row_idx, Q, q_idx, n_q, out, users, scores, oob_flag, static_cast<int>(L), static_cast<int>(F), static_cast<int>(A), G,
             static_cast<int>(mode));
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

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
