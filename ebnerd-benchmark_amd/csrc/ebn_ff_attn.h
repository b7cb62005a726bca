// What the two Fastformer attention pairs share: the resident pair of ebn_fastformer.hip (the sequence's biased Q rows in LDS) and
// the streamed pair of ebn_fastformer_streamed.hip (Q and K re-read from global memory).  Launch geometry, the argument block and
// the two softmax routines over the [heads][T] arrays in LDS.
#pragma once
#include "ebn_common.h"

namespace {

constexpr int FF_THREADS = 256;
constexpr int FF_WAVES = FF_THREADS / 64;
constexpr int FF_ATT_MAX_PARTS = 256;  // workgroups (= partials) of the attention backward
constexpr int FF_ATT_MAX_D = 1024;     // 4 column sums per thread
constexpr int FF_LDS_BYTES = 64 * 1024;
constexpr float FF_MASK_NEG = -10000.0f;

// ---- fast additive attention core -------------------------------------------------------------------------------------------------
struct FfAttn {
  float* Q;           // [n_seq*T, D] in: x.Wq^T, out: + bq (mixed_query_layer)
  float* K;           // likewise with bk
  const float* bq;
  const float* bk;
  const float* btr;   // transform.bias (only with SV0)
  const float* Wqa;   // [heads, D]
  const float* bqa;   // [heads]
  const float* Wka;
  const float* bka;
  const float* mask;  // [n_seq, T] 1 = token, 0 = padding
  float* AO;          // [n_seq*T, D] pooled_key * Q
  float* SV0;         // [n_seq*T, D] Q + btr, or NULL
  float* qw;          // [n_seq, heads, T]
  float* kw;
  float* pq;          // [n_seq, D]
  float* pk;
  // backward
  const float* dAO;
  const float* dSV;   // gradient reaching Q through "+ mixed_query_layer", or NULL
  float* dQ;
  float* dK;
  float* partials;    // [grid][2 * heads * D + 3 * D]
  int64_t n_seq;
  int32_t T, D, heads;
  float inv;          // 1 / sqrt(head size)
};

// softmax over the T logits of each head, in place in LDS and out to global; wave per head
__device__ __forceinline__ void ff_softmax_rows(float* sw, float* __restrict__ gout, int T, int H) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int h = wave; h < H; h += FF_WAVES) {
    float* row = sw + h * T;
    float m = -INFINITY;
    for (int t = lane; t < T; t += 64) m = fmaxf(m, row[t]);
    m = ebn_wave_max(m);
    float s = 0.f;
    for (int t = lane; t < T; t += 64) {
      const float e = expf(row[t] - m);
      row[t] = e;
      s += e;
    }
    s = ebn_wave_sum(s);
    for (int t = lane; t < T; t += 64) {
      const float p = row[t] / s;
      row[t] = p;
      gout[h * T + t] = p;
    }
  }
}

// softmax backward per head in LDS: sd <- p * (sd - sum_t p sd); wave per head
__device__ __forceinline__ void ff_softmax_bwd_rows(const float* sp, float* sd, int T, int H) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int h = wave; h < H; h += FF_WAVES) {
    float s = 0.f;
    for (int t = lane; t < T; t += 64) s = fmaf(sp[h * T + t], sd[h * T + t], s);
    s = ebn_wave_sum(s);
    for (int t = lane; t < T; t += 64) sd[h * T + t] = sp[h * T + t] * (sd[h * T + t] - s);
  }
}

int64_t ff_attn_grid(int64_t n_seq) { return n_seq < FF_ATT_MAX_PARTS ? (n_seq < 1 ? 1 : n_seq) : FF_ATT_MAX_PARTS; }

}  // namespace
