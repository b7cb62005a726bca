// Fastformer's fast additive attention core for sequences that do not fit the resident pair of ebn_fastformer.hip (ordinary BERT
// sizes: hidden 768 / 12 heads, hidden 1024 / 16 heads, titles of hundreds of tokens).  The same inputs, the same saved tensors and
// the same arithmetic in the same places as the resident pair -- the biased Q and K written back to global memory included -- but
// nothing T x D lives in LDS: a token row is held in the registers of the wave that works on it (D / 64 <= 16 floats per lane),
// and the passes that walk the sequence re-read Q and K from global memory (30 x 768 x 4 B = 92 KB each at the BERT shape, L2
// resident), column owners reading coalesced rows.
//
// LDS per workgroup, all of it O(heads * T + D):
//   forward   4 * (heads * T + T + 2 * D) bytes     the [heads][T] logits / weights, the mask term, pooled query and pooled key
//   backward  4 * (2 * heads * T + 4 * D) bytes     ONE [heads][T] pair (weights | logit gradients), used for the key stage and
//                                                   then again for the query stage, and pq | pk | d(pq) | d(pk)
// both <= 64 KiB: T <= 1142 forward and T <= 554 backward at D = 768, 12 heads.
//
// The backward keeps no logit-weight gradient on chip.  It writes the logit gradients behind the two softmax backwards, d1 and d2
// [n_seq*T, heads], and the rows KP = K * pooled_query [n_seq*T, D]; the caller forms dWqa = inv * d1^T.Q and dWka = inv * d2^T.KP
// with the deterministic split-K GEMM (ebn_gemm_f32_ws) that every other weight gradient of the model uses.  So heads * D is not
// bounded here.  The three bias column sums stay per-workgroup partials for ebn_ff_colsum_finish_f32.
//
// Exact fp32, fixed summation orders, no float atomics, wave64: the same bits on every run.  Every sum over the tokens of a sequence
// is blocked (FFS_TBLOCK tokens per running sum, block sums added in ascending order), so that T = 512 costs no more digits than a
// pairwise sum would; up to T = 32 that is the resident pair's order.
#include "ebn_common.h"
#include "ebn_ff_attn.h"

namespace {

constexpr int FFS_ROW_F4 = FF_ATT_MAX_D / 256;  // float4 pieces of a row in one lane: lane l holds columns 4 l + 256 j .. + 3
constexpr int FFS_W_REGS = 16;                  // heads up to which a column owner keeps its logit-weight column in registers
constexpr int FFS_TBLOCK = 32;                  // a sum over the T tokens of a sequence runs in blocks of this many tokens, whose sums
                                                // are then added in ascending order: hundreds of tokens in one running fp32 sum cost digits

struct FfAttnStreamed {
  FfAttn a;   // partials: [grid][3 * D] = colsum(dQ) | colsum(dK) | colsum(dSV)
  float* d1;  // [n_seq*T, heads] d(query logits) behind the softmax backward
  float* d2;  // likewise for the key logits
  float* kp;  // [n_seq*T, D] K * pooled_query
};

__host__ __device__ inline int64_t ffs_fwd_lds_floats(int T, int D, int H) {
  return static_cast<int64_t>(H) * T + T + 2 * static_cast<int64_t>(D);
}
__host__ __device__ inline int64_t ffs_bwd_lds_floats(int T, int D, int H) {
  return 2 * static_cast<int64_t>(H) * T + 4 * static_cast<int64_t>(D);
}

// logits of one row held in registers against the [heads, D] weight: every head reads the WHOLE row; the sum runs in the order of
// the resident pair's ff_row_logits
__device__ __forceinline__ void ffs_row_logits(const float4 (&x)[FFS_ROW_F4], const float* __restrict__ Wa, const float* __restrict__ ba,
                                               float* sw, int t, int T, int D, int H, float inv, float maskterm) {
  const int lane = threadIdx.x & 63;
  for (int h = 0; h < H; ++h) {
    const float* wrow = Wa + static_cast<int64_t>(h) * D;
    float p = 0.f;
#pragma unroll
    for (int j = 0; j < FFS_ROW_F4; ++j) {
      const int c = lane * 4 + 256 * j;
      if (c < D) {
        const float4 y = *reinterpret_cast<const float4*>(wrow + c);
        p = fmaf(x[j].x, y.x, p);
        p = fmaf(x[j].y, y.y, p);
        p = fmaf(x[j].z, y.z, p);
        p = fmaf(x[j].w, y.w, p);
      }
    }
    p = ebn_wave_sum(p);
    if (lane == 0) sw[h * T + t] = (p + ba[h]) * inv + maskterm;
  }
}

__global__ __launch_bounds__(FF_THREADS) void ff_attn_streamed_fwd_kernel(FfAttn a) {
  extern __shared__ float4 ff_lds4[];
  float* lds = reinterpret_cast<float*>(ff_lds4);
  const int T = a.T, D = a.D, H = a.heads, hd = D / H, D4 = D / 4;
  float* spq = lds;        // [D]
  float* spk = spq + D;    // [D]
  float* sm = spk + D;     // [T] additive mask term
  float* sw = sm + T;      // [H][T]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t n = blockIdx.x;
  const int64_t base = n * T * D;

  for (int t = threadIdx.x; t < T; t += FF_THREADS) sm[t] = (1.0f - a.mask[n * T + t]) * FF_MASK_NEG;
  __syncthreads();
  // query stage: bias into Q (and Q + btr into SV0), the row's logits from registers
  for (int t = wave; t < T; t += FF_WAVES) {
    const int64_t off = base + static_cast<int64_t>(t) * D;
    float4 x[FFS_ROW_F4];
#pragma unroll
    for (int j = 0; j < FFS_ROW_F4; ++j) {
      const int c = lane * 4 + 256 * j;
      x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < D) {
        float4 q = *reinterpret_cast<const float4*>(a.Q + off + c);
        const float4 b = *reinterpret_cast<const float4*>(a.bq + c);
        q.x += b.x; q.y += b.y; q.z += b.z; q.w += b.w;
        *reinterpret_cast<float4*>(a.Q + off + c) = q;
        if (a.SV0 != nullptr) {
          const float4 bt = *reinterpret_cast<const float4*>(a.btr + c);
          *reinterpret_cast<float4*>(a.SV0 + off + c) = make_float4(q.x + bt.x, q.y + bt.y, q.z + bt.z, q.w + bt.w);
        }
        x[j] = q;
      }
    }
    ffs_row_logits(x, a.Wqa, a.bqa, sw, t, T, D, H, a.inv, sm[t]);
  }
  __syncthreads();
  ff_softmax_rows(sw, a.qw + n * H * T, T, H);
  __syncthreads();
  // pooled query: a column owner walks t over the biased rows this workgroup has just written
  for (int c = threadIdx.x; c < D; c += FF_THREADS) {
    const float* wr = sw + (c / hd) * T;
    const float* col = a.Q + base + c;
    float acc = 0.f;
    for (int t0 = 0; t0 < T; t0 += FFS_TBLOCK) {
      const int t1 = t0 + FFS_TBLOCK < T ? t0 + FFS_TBLOCK : T;
      float blk = 0.f;
      for (int t = t0; t < t1; ++t) blk = fmaf(wr[t], col[static_cast<int64_t>(t) * D], blk);
      acc += blk;
    }
    spq[c] = acc;
    a.pq[n * D + c] = acc;
  }
  __syncthreads();
  // key stage on K * pooled_query; the biased K goes back to global for the pooling below and for the backward
  for (int t = wave; t < T; t += FF_WAVES) {
    const int64_t off = base + static_cast<int64_t>(t) * D;
    float4 x[FFS_ROW_F4];
#pragma unroll
    for (int j = 0; j < FFS_ROW_F4; ++j) {
      const int c = lane * 4 + 256 * j;
      x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < D) {
        float4 k = *reinterpret_cast<const float4*>(a.K + off + c);
        const float4 b = *reinterpret_cast<const float4*>(a.bk + c);
        k.x += b.x; k.y += b.y; k.z += b.z; k.w += b.w;
        *reinterpret_cast<float4*>(a.K + off + c) = k;
        const float4 p = *reinterpret_cast<const float4*>(spq + c);
        x[j] = make_float4(k.x * p.x, k.y * p.y, k.z * p.z, k.w * p.w);
      }
    }
    ffs_row_logits(x, a.Wka, a.bka, sw, t, T, D, H, a.inv, sm[t]);
  }
  __syncthreads();
  ff_softmax_rows(sw, a.kw + n * H * T, T, H);
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += FF_THREADS) {
    const float* wr = sw + (c / hd) * T;
    const float* col = a.K + base + c;
    const float p = spq[c];
    float acc = 0.f;
    for (int t0 = 0; t0 < T; t0 += FFS_TBLOCK) {
      const int t1 = t0 + FFS_TBLOCK < T ? t0 + FFS_TBLOCK : T;
      float blk = 0.f;
      for (int t = t0; t < t1; ++t) blk = fmaf(wr[t], col[static_cast<int64_t>(t) * D] * p, blk);
      acc += blk;
    }
    spk[c] = acc;
    a.pk[n * D + c] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T * D4; i += FF_THREADS) {
    const int t = i / D4, c = (i - t * D4) * 4;
    const int64_t off = base + static_cast<int64_t>(t) * D + c;
    const float4 q = *reinterpret_cast<const float4*>(a.Q + off);
    const float4 p = *reinterpret_cast<const float4*>(spk + c);
    *reinterpret_cast<float4*>(a.AO + off) = make_float4(q.x * p.x, q.y * p.y, q.z * p.z, q.w * p.w);
  }
}

// One token row, one wave: sd[h][t] = sum over head h's columns of su[c] * x[c], x = the global row, times sv[c] with KEY (and
// that product out to kprow).  16-byte accesses where a head's slice is a multiple of 4 columns.
template <bool KEY>
__device__ __forceinline__ void ffs_head_sums(const float* __restrict__ xrow, const float* su, const float* sv, float* __restrict__ kprow,
                                              float* sd, int t, int T, int hd, int H) {
  const int lane = threadIdx.x & 63;
  for (int h = 0; h < H; ++h) {
    const int c0 = h * hd;
    float acc = 0.f;
    if ((hd & 3) == 0) {
      for (int c = c0 + lane * 4; c < c0 + hd; c += 256) {
        float4 x = *reinterpret_cast<const float4*>(xrow + c);
        const float4 u = *reinterpret_cast<const float4*>(su + c);
        if (KEY) {
          const float4 v = *reinterpret_cast<const float4*>(sv + c);
          x.x *= v.x; x.y *= v.y; x.z *= v.z; x.w *= v.w;
          *reinterpret_cast<float4*>(kprow + c) = x;
        }
        acc = fmaf(u.x, x.x, acc);
        acc = fmaf(u.y, x.y, acc);
        acc = fmaf(u.z, x.z, acc);
        acc = fmaf(u.w, x.w, acc);
      }
    } else {
      for (int c = c0 + lane; c < c0 + hd; c += 64) {
        float x = xrow[c];
        if (KEY) {
          x *= sv[c];
          kprow[c] = x;
        }
        acc = fmaf(su[c], x, acc);
      }
    }
    acc = ebn_wave_sum(acc);
    if (lane == 0) sd[h * T + t] = acc;
  }
}

// lin = sum_g sd[g][t] * Wa[g][c], g ascending: the column's weights from registers (heads <= FFS_W_REGS) or from global memory
__device__ __forceinline__ float ffs_lin(const float* sd, const float (&w)[FFS_W_REGS], const float* __restrict__ Wa, int t, int T, int D,
                                         int H, int c) {
  float lin = 0.f;
  if (H <= FFS_W_REGS) {
#pragma unroll
    for (int g = 0; g < FFS_W_REGS; ++g)
      if (g < H) lin = fmaf(sd[g * T + t], w[g], lin);
  } else {
    for (int g = 0; g < H; ++g) lin = fmaf(sd[g * T + t], Wa[static_cast<int64_t>(g) * D + c], lin);
  }
  return lin;
}

__device__ __forceinline__ void ffs_load_w(float (&w)[FFS_W_REGS], const float* __restrict__ Wa, int D, int H, int c) {
#pragma unroll
  for (int g = 0; g < FFS_W_REGS; ++g) w[g] = (H <= FFS_W_REGS && g < H) ? Wa[static_cast<int64_t>(g) * D + c] : 0.f;
}

// the [heads][T] logit gradients of a sequence out as rows [T, heads] (the A operand of the caller's weight-gradient GEMM)
__device__ __forceinline__ void ffs_store_dlogits(const float* sd, float* __restrict__ out, int T, int H) {
  for (int i = threadIdx.x; i < H * T; i += FF_THREADS) {
    const int t = i / H, h = i - t * H;
    out[i] = sd[h * T + t];
  }
}

// workgroup g walks the sequences g, g + grid, ...; across them it keeps only the three bias column sums, in its own row of
// `partials` (every thread adds to the columns it owns, in the order of the sequences)
__global__ __launch_bounds__(FF_THREADS) void ff_attn_streamed_bwd_kernel(FfAttnStreamed s) {
  extern __shared__ float4 ff_lds4[];
  float* lds = reinterpret_cast<float*>(ff_lds4);
  const FfAttn& a = s.a;
  const int T = a.T, D = a.D, H = a.heads, hd = D / H;
  float* spq = lds;            // [D]
  float* spk = spq + D;
  float* sdpq = spk + D;
  float* sdpk = sdpq + D;
  float* sp = sdpk + D;        // [H][T] softmax weights: the key stage's, then the query stage's
  float* sd = sp + H * T;      // [H][T] logit gradients, likewise
  const int wave = threadIdx.x >> 6;
  float* out = a.partials + static_cast<int64_t>(blockIdx.x) * 3 * D;  // colsum(dQ) | colsum(dK) | colsum(dSV)
  for (int c = threadIdx.x; c < 3 * D; c += FF_THREADS) out[c] = 0.f;

  for (int64_t n = blockIdx.x; n < a.n_seq; n += gridDim.x) {
    const int64_t base = n * T * D;
    for (int i = threadIdx.x; i < H * T; i += FF_THREADS) sp[i] = a.kw[n * H * T + i];
    for (int c = threadIdx.x; c < D; c += FF_THREADS) {
      spq[c] = a.pq[n * D + c];
      spk[c] = a.pk[n * D + c];
      // d(pooled key)
      const float* g = a.dAO + base + c;
      const float* q = a.Q + base + c;
      float acc = 0.f;
      for (int t0 = 0; t0 < T; t0 += FFS_TBLOCK) {
        const int t1 = t0 + FFS_TBLOCK < T ? t0 + FFS_TBLOCK : T;
        float blk = 0.f;
        for (int t = t0; t < t1; ++t) blk = fmaf(g[static_cast<int64_t>(t) * D], q[static_cast<int64_t>(t) * D], blk);
        acc += blk;
      }
      sdpk[c] = acc;
    }
    __syncthreads();
    // d(key weights)[h][t] = sum over the head's columns of d(pooled key) * K * pooled_query; the rows K * pooled_query go out
    for (int t = wave; t < T; t += FF_WAVES) {
      const int64_t off = base + static_cast<int64_t>(t) * D;
      ffs_head_sums<true>(a.K + off, sdpk, spq, s.kp + off, sd, t, T, hd, H);
    }
    __syncthreads();
    ff_softmax_bwd_rows(sp, sd, T, H);
    __syncthreads();
    ffs_store_dlogits(sd, s.d2 + n * T * H, T, H);
    // d(K * pooled_query) per element -> dK, d(pooled query), column sum of dK
#pragma unroll 1
    for (int c = threadIdx.x; c < D; c += FF_THREADS) {
      {
        const int h = c / hd;
        const float dpk = sdpk[c], pqc = spq[c];
        float w[FFS_W_REGS];
        ffs_load_w(w, a.Wka, D, H, c);
        float dpq = 0.f, colk = 0.f;
        for (int t0 = 0; t0 < T; t0 += FFS_TBLOCK) {
          const int t1 = t0 + FFS_TBLOCK < T ? t0 + FFS_TBLOCK : T;
          float bpq = 0.f, bk = 0.f;
          for (int t = t0; t < t1; ++t) {
            const int64_t off = base + static_cast<int64_t>(t) * D + c;
            const float dkp = fmaf(sp[h * T + t], dpk, a.inv * ffs_lin(sd, w, a.Wka, t, T, D, H, c));
            const float dk = dkp * pqc;
            a.dK[off] = dk;
            bk += dk;
            bpq = fmaf(dkp, a.K[off], bpq);
          }
          dpq += bpq;
          colk += bk;
        }
        sdpq[c] = dpq;
        out[D + c] += colk;
      }
    }
    __syncthreads();
    // query stage in the same two arrays: d(query weights)[h][t] = sum over the head's columns of d(pooled query) * Q
    for (int i = threadIdx.x; i < H * T; i += FF_THREADS) sp[i] = a.qw[n * H * T + i];
    for (int t = wave; t < T; t += FF_WAVES)
      ffs_head_sums<false>(a.Q + base + static_cast<int64_t>(t) * D, sdpq, nullptr, nullptr, sd, t, T, hd, H);
    __syncthreads();
    ff_softmax_bwd_rows(sp, sd, T, H);
    __syncthreads();
    ffs_store_dlogits(sd, s.d1 + n * T * H, T, H);
#pragma unroll 1
    for (int c = threadIdx.x; c < D; c += FF_THREADS) {
      {
        const int h = c / hd;
        const float pkc = spk[c], dpq = sdpq[c];
        float w[FFS_W_REGS];
        ffs_load_w(w, a.Wqa, D, H, c);
        float colq = 0.f, colt = 0.f;
        for (int t0 = 0; t0 < T; t0 += FFS_TBLOCK) {
          const int t1 = t0 + FFS_TBLOCK < T ? t0 + FFS_TBLOCK : T;
          float bq = 0.f, bt = 0.f;
          for (int t = t0; t < t1; ++t) {
            const int64_t off = base + static_cast<int64_t>(t) * D + c;
            float dq = fmaf(a.dAO[off], pkc, sp[h * T + t] * dpq);
            dq = fmaf(a.inv, ffs_lin(sd, w, a.Wqa, t, T, D, H, c), dq);
            if (a.dSV != nullptr) {
              const float ds = a.dSV[off];
              dq += ds;
              bt += ds;
            }
            a.dQ[off] = dq;
            bq += dq;
          }
          colq += bq;
          colt += bt;
        }
        out[c] += colq;
        out[2 * D + c] += colt;
      }
    }
    __syncthreads();
  }
}

int ffs_attn_check(int64_t n_seq, int32_t T, int32_t D, int32_t heads, bool bwd) {
  EBN_REQUIRE(n_seq >= 0 && T > 0 && D > 0 && heads > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(D % heads == 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(D % 4 == 0 && D <= FF_ATT_MAX_D && T <= 4096 && n_seq <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  const int64_t fl = bwd ? ffs_bwd_lds_floats(T, D, heads) : ffs_fwd_lds_floats(T, D, heads);
  EBN_REQUIRE(fl * 4 <= FF_LDS_BYTES, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(ebn_sat_mul(ebn_sat_mul(n_seq, T), D) < (int64_t(1) << 40), EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

}  // namespace

extern "C" int ebn_ff_attn_streamed_supported(int32_t T, int32_t D, int32_t heads, int32_t with_backward) {
  const int rc = ffs_attn_check(0, T, D, heads, false);
  if (rc != EBN_OK || !with_backward) return rc;
  return ffs_attn_check(0, T, D, heads, true);
}

extern "C" int ebn_ff_attn_streamed_fwd_f32(float* Q, float* K, const float* bq, const float* bk, const float* btr, const float* Wqa,
                                            const float* bqa, const float* Wka, const float* bka, const float* mask, float* AO,
                                            float* SV0, float* qw, float* kw, float* pq, float* pk, int64_t n_seq, int32_t T, int32_t D,
                                            int32_t heads, ebn_stream_t stream) {
  EBN_REQUIRE(Q && K && bq && bk && Wqa && bqa && Wka && bka && mask && AO && qw && kw && pq && pk, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(SV0 == nullptr || btr != nullptr, EBN_ERR_BAD_ARG);
  const int rc = ffs_attn_check(n_seq, T, D, heads, false);
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
  EBN_LAUNCH(ff_attn_streamed_fwd_kernel, dim3(static_cast<uint32_t>(n_seq)), dim3(FF_THREADS),
             static_cast<size_t>(ffs_fwd_lds_floats(T, D, heads)) * sizeof(float), ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int64_t ebn_ff_attn_streamed_partials_len(int64_t n_seq, int32_t D) {
  if (!ebn_dim_ok(n_seq, D)) return 0;
  return ebn_sat_mul(ff_attn_grid(n_seq), 3 * static_cast<int64_t>(D));
}

extern "C" int64_t ebn_ff_attn_streamed_dlogits_len(int64_t n_seq, int32_t T, int32_t heads) {
  if (!ebn_dim_ok(n_seq, T, heads)) return 0;
  return ebn_sat_mul(ebn_sat_mul(n_seq, T), heads);
}

extern "C" int64_t ebn_ff_attn_streamed_kp_len(int64_t n_seq, int32_t T, int32_t D) {
  if (!ebn_dim_ok(n_seq, T, D)) return 0;
  return ebn_sat_mul(ebn_sat_mul(n_seq, T), D);
}

extern "C" int ebn_ff_attn_streamed_bwd_f32(const float* Q, const float* K, const float* Wqa, const float* Wka, const float* qw,
                                            const float* kw, const float* pq, const float* pk, const float* dAO, const float* dSV,
                                            float* dQ, float* dK, float* d1, float* d2, float* kp, float* partials, int32_t* n_parts,
                                            int64_t n_seq, int32_t T, int32_t D, int32_t heads, ebn_stream_t stream) {
  EBN_REQUIRE(Q && K && Wqa && Wka && qw && kw && pq && pk && dAO && dQ && dK && d1 && d2 && kp && partials && n_parts,
              EBN_ERR_BAD_ARG);
  const int rc = ffs_attn_check(n_seq, T, D, heads, true);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(ebn_aligned16(Q) && ebn_aligned16(K) && ebn_aligned16(kp), EBN_ERR_ALIGN);
  const int64_t grid = ff_attn_grid(n_seq);
  *n_parts = static_cast<int32_t>(grid);
  FfAttnStreamed s{};
  FfAttn& a = s.a;
  a.Q = const_cast<float*>(Q); a.K = const_cast<float*>(K); a.Wqa = Wqa; a.Wka = Wka;
  a.qw = const_cast<float*>(qw); a.kw = const_cast<float*>(kw); a.pq = const_cast<float*>(pq); a.pk = const_cast<float*>(pk);
  a.dAO = dAO; a.dSV = dSV; a.dQ = dQ; a.dK = dK; a.partials = partials;
  a.n_seq = n_seq; a.T = T; a.D = D; a.heads = heads;
  a.inv = 1.0f / sqrtf(static_cast<float>(D / heads));
  s.d1 = d1; s.d2 = d2; s.kp = kp;
  // n_seq == 0: one workgroup writes one zero partial
  EBN_LAUNCH(ff_attn_streamed_bwd_kernel, dim3(static_cast<uint32_t>(grid)), dim3(FF_THREADS),
             static_cast<size_t>(ffs_bwd_lds_floats(T, D, heads)) * sizeof(float), ebn_stream(stream), s);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
