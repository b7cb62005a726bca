// Implicit-feedback ALS (Hu, Koren, Volinsky 2008; contract in include/ebnerd_hip.h): one half-sweep solves, per row r of one side,
//     A_r = gram + reg I + sum_k a_k y_k y_k^T,   b_r = sum_k (1 + a_k) y_k,   x_r = A_r^{-1} b_r
// over the row's present entries k (y_k = fixed[cols[k], :], a_k = conf[k]).
//   * ONE WORKGROUP PER ROW, a G x G grid of threads (tx = tid % G, ty = tid / G): G = 16, 256 threads, for F > ALS_ONE_WAVE_MAX_F,
//     and G = 8, ONE WAVE, below (measured, DESIGN.md section 30: at F = 32 one wave takes 0.61 of the 256-thread time, at F = 64
//     1.32 of it).  F is rounded up to FB = G R (R = 1, 2, 4, 8: one instantiation each) and thread (ty, tx) owns the elements
//     (ty + G a, tx + G b) of A, a, b < R, IN REGISTERS.  Only the blocks a >= b are kept (the lower triangle and the diagonal
//     blocks): R (R + 1) / 2 accumulators per thread, 36 at F = 128.  Strided ownership: at G = 16 a wave reads 4 distinct words
//     for its rows (broadcast) and 16 consecutive ones for its columns.
//   * ACCUMULATE: the row's entries are staged ALS_T = 16 at a time as a zero-padded [16, FB] tile in LDS (16-byte loads where the
//     pointer and ld allow them, scalar ones otherwise: copies, the bits do not depend on it); an ABSENT entry (column outside
//     [0, n_fixed)) is staged as a zero row with confidence 0 and its column is never turned into an address.  Per staged entry
//     every thread does R products a_k y_i and R (R + 1) / 2 fused multiply-adds; threads tid < FB add (1 + a_k) y_i to b_i.  In a
//     diagonal block the thread above the diagonal forms (a_k y_j) y_i, the bits of its mirror image: the matrix is symmetric bit
//     for bit.  Entries are taken in their order: one fixed summation order.
//   * PARTIALS: the same accumulation over the entries of one part, one workgroup per part; the full symmetric [F, F] sum and the
//     F sums of b leave for the workspace.  The solve kernel adds a long row's parts in ascending order instead of walking its
//     entries (it reads the lower triangle i >= j), so a row of a million entries is spread over hundreds of workgroups, no atomics.
//   * CHOLESKY, right-looking, A still in registers: step k, (1) the G threads with tx == k % G put column k (rows >= k) into
//     LDS, barrier, (2) threads i in [k, FB) divide it by sqrtf(pivot) into column k of L (LDS, column-major at the odd stride
//     FB + 1), barrier, (3) every thread reads its R row and R column values of that column and updates its blocks b >= k / G.
//     Two barriers a step (of one wave with itself at G = 8), 2 R LDS reads and at most R (R + 1) / 2 fmas per thread and step.
//     sqrtf and the division are the correctly rounded ones.  A pivot that is not > 0 (NaN included) raises a flag: the whole
//     output row becomes NaN.
//   * SOLVES by wave 0, lane l holding the elements l and l + 64 of the right-hand side: column-oriented forward substitution
//     (column k of L is contiguous) and backward substitution (row k of L at stride FB + 1: odd, conflict-free), the pivot element
//     broadcast with a shuffle.  No barrier inside.
//   * A row without a present entry (and without parts) writes F zeros and leaves before any of this.
//   * LDS: 4 (FB (FB + 1) + 16 FB + 2 FB + 72) bytes: 73.8 KiB at FB = 128 (two workgroups per CU in 160 KiB), 21.0 KiB at 64, 6.7 KiB
//     at 32, 2.5 KiB at 16, 1.1 KiB at 8.  No atomics, no workspace beside the partials: two runs give the same bits.
#include "ebn_common.h"

#define ALS_T 16         // entries of a staged tile
#ifndef ALS_ONE_WAVE_MAX_F
#define ALS_ONE_WAVE_MAX_F 32  // rows of at most this many factors (<= 64) go to ONE wave as an 8 x 8 grid of lanes; 0: never
#endif
static_assert(ALS_ONE_WAVE_MAX_F >= 0 && ALS_ONE_WAVE_MAX_F <= 64, "an 8 x 8 grid of lanes with R <= 8 covers F <= 64");

static_assert(EBN_ALS_MAX_F == 128, "R = 8 is the largest instantiation: 16 R >= F");

namespace {

struct AlsArgs {
  const float* fixed;
  int64_t n_fixed, ld;
  const float* gram;
  int64_t ldg;
  const int64_t* indptr;  // solve: [n_solve + 1]; partials: nullptr
  const int32_t* cols;
  const float* conf;
  int64_t nnz;
  float reg;
  const int64_t* row_parts;  // solve: optional [n_solve + 1]
  const float* partials_in;
  int64_t n_parts;
  const int64_t* part_begin;  // partials: [n_parts]
  const int64_t* part_end;
  float* partials_out;
  float* out;
  int64_t ldo;
  int32_t F;
};

static __device__ __forceinline__ int64_t als_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <int R, int G>
struct AlsLds {
  static constexpr int FB = G * R, LD = FB + 1;
  static constexpr int L = 0, Y = L + FB * LD, COL = Y + ALS_T * FB, B = COL + FB, W = B + FB, ROW = W + 2 * ALS_T, FLAG = ROW + 2 * ALS_T;  // W / ROW: two tiles
  static constexpr int FLOATS = FLAG + 8;
};

// acc[a][b] (a >= b) += sum over the entries [k0, k1) of a_k y_i y_j; bsum += sum (1 + a_k) y_tid (threads tid < FB).
// Returns whether an entry was present.  Every thread of the workgroup calls it (barriers inside).
template <int R, int G, bool VEC>
static __device__ __forceinline__ bool als_accumulate(const AlsArgs& g, float* lds, int64_t k0, int64_t k1, float (&acc)[R][R], float& bsum) {
  using S = AlsLds<R, G>;
  constexpr int FB = S::FB;
  float* sY = lds + S::Y;
  const int tid = threadIdx.x, tx = tid % G, ty = tid / G;
  const int F = g.F;
  int any = 0, parity = 0;
#pragma unroll 1
  for (int64_t base = k0; base < k1; base += ALS_T, parity ^= 1) {
    // rows and confidences alternate between two slots: a tile's are written while other waves still read the previous tile's
    float* sW = lds + S::W + parity * ALS_T;
    int32_t* sRow = reinterpret_cast<int32_t*>(lds + S::ROW) + parity * ALS_T;
    const int nt = k1 - base < ALS_T ? static_cast<int>(k1 - base) : ALS_T;
    int present = 0;
    if (tid < ALS_T) {
      int32_t row = -1;
      float w = 0.0f;
      if (tid < nt) {
        const int32_t c = g.cols[base + tid];
        if (c >= 0 && c < g.n_fixed) {
          row = c;
          w = g.conf[base + tid];
          present = 1;
        }
      }
      sRow[tid] = row;
      sW[tid] = w;
    }
    any |= __syncthreads_or(present);  // also: every wave is done with the previous tile's rows in sY
    for (int idx = tid; idx < nt * (FB / 4); idx += G * G) {
      const int t = idx / (FB / 4), c = (idx - t * (FB / 4)) * 4;
      const int32_t row = sRow[t];
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (row >= 0) {
        const float* __restrict__ src = g.fixed + static_cast<int64_t>(row) * g.ld;
        if (VEC && c + 4 <= F) {
          v = *reinterpret_cast<const float4*>(src + c);
        } else {
          if (c < F) v.x = src[c];
          if (c + 1 < F) v.y = src[c + 1];
          if (c + 2 < F) v.z = src[c + 2];
          if (c + 3 < F) v.w = src[c + 3];
        }
      }
      *reinterpret_cast<float4*>(sY + t * FB + c) = v;
    }
    __syncthreads();
#pragma unroll 2
    for (int t = 0; t < nt; ++t) {
      const float w = sW[t];
      const float* __restrict__ y = sY + t * FB;
      float yi[R], yj[R], wyi[R];
#pragma unroll
      for (int a = 0; a < R; ++a) {
        yi[a] = y[ty + G * a];
        yj[a] = y[tx + G * a];
        wyi[a] = w * yi[a];
      }
#pragma unroll
      for (int a = 0; a < R; ++a) {
#pragma unroll
        for (int b = 0; b < a; ++b) acc[a][b] = fmaf(wyi[a], yj[b], acc[a][b]);
        // the diagonal block: above the diagonal the mirrored product (a_k y_j) y_i, so that A[i][j] and A[j][i] are the same bits
        acc[a][a] = ty >= tx ? fmaf(wyi[a], yj[a], acc[a][a]) : fmaf(w * yj[a], yi[a], acc[a][a]);
      }
      if (tid < FB) bsum = fmaf(1.0f + w, y[tid], bsum);
    }
  }
  return any != 0;
}

template <int R, int G, bool VEC>
static __global__ __launch_bounds__(G * G) void als_partials_kernel(AlsArgs g) {
  extern __shared__ float4 als_lds4[];
  float* lds = reinterpret_cast<float*>(als_lds4);
  const int tid = threadIdx.x, tx = tid % G, ty = tid / G;
  const int F = g.F;
  const int64_t p = blockIdx.x;
  const int64_t k0 = als_clamp(g.part_begin[p], g.nnz), k1 = als_clamp(g.part_end[p], g.nnz);
  float acc[R][R];
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int b = 0; b < R; ++b) acc[a][b] = 0.0f;
  float bsum = 0.0f;
  als_accumulate<R, G, VEC>(g, lds, k0, k1, acc, bsum);
  float* __restrict__ dst = g.partials_out + p * (static_cast<int64_t>(F) * (F + 1));
#pragma unroll
  for (int a = 0; a < R; ++a) {
    const int i = ty + G * a;
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      const int j = tx + G * b;
      if (i < F && j < F) {
        dst[i * F + j] = acc[a][b];
        if (b < a) dst[j * F + i] = acc[a][b];  // the mirror image; a diagonal block holds both triangles itself
      }
    }
  }
  if (tid < F) dst[F * F + tid] = bsum;
}

template <int R, int G, bool VEC>
static __global__ __launch_bounds__(G * G) void als_solve_kernel(AlsArgs g) {
  using S = AlsLds<R, G>;
  constexpr int FB = S::FB, LD = S::LD;
  extern __shared__ float4 als_lds4[];
  float* lds = reinterpret_cast<float*>(als_lds4);
  float* sL = lds + S::L;
  float* sCol = lds + S::COL;
  float* sB = lds + S::B;
  int32_t* sFlag = reinterpret_cast<int32_t*>(lds + S::FLAG);
  const int tid = threadIdx.x, tx = tid % G, ty = tid / G;
  const int F = g.F;
  const int64_t r = blockIdx.x;
  float* __restrict__ out = g.out + r * g.ldo;
  float acc[R][R];
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int b = 0; b < R; ++b) acc[a][b] = 0.0f;
  float bsum = 0.0f;
  if (tid == 0) sFlag[0] = 0;
  // ---- A and b: the sum of the row's parts, or a walk of its entries
  int64_t p0 = 0, p1 = 0;
  if (g.row_parts != nullptr) {
    p0 = als_clamp(g.row_parts[r], g.n_parts);
    p1 = als_clamp(g.row_parts[r + 1], g.n_parts);
  }
  if (p0 < p1) {
    const int64_t stride = static_cast<int64_t>(F) * (F + 1);
#pragma unroll 1
    for (int64_t p = p0; p < p1; ++p) {
      const float* __restrict__ src = g.partials_in + p * stride;
#pragma unroll
      for (int a = 0; a < R; ++a) {
        const int i = ty + G * a;
#pragma unroll
        for (int b = 0; b <= a; ++b) {
          const int j = tx + G * b;
          if (i < F && j < F && i >= j) acc[a][b] += src[i * F + j];
        }
      }
      if (tid < F) bsum += src[F * F + tid];
    }
  } else {
    const int64_t k0 = als_clamp(g.indptr[r], g.nnz), k1 = als_clamp(g.indptr[r + 1], g.nnz);
    if (!als_accumulate<R, G, VEC>(g, lds, k0, k1, acc, bsum)) {  // uniform: no present entry
      if (tid < F) out[tid] = 0.0f;
      return;
    }
  }
  // ---- + gram + reg I (elements inside F; the rest of the FB x FB frame stays 0 and is never factorised)
#pragma unroll
  for (int a = 0; a < R; ++a) {
    const int i = ty + G * a;
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      const int j = tx + G * b;
      if (i < F && j < F && i >= j) {
        acc[a][b] += g.gram[i * g.ldg + j];
        if (i == j) acc[a][b] += g.reg;
      }
    }
  }
  if (tid < FB) sB[tid] = bsum;
  // ---- right-looking Cholesky: A in registers, column k of L through LDS
#pragma unroll 1
  for (int k = 0; k < F; ++k) {
    const int kb = k / G, kx = k % G;
    if (tx == kx) {
#pragma unroll
      for (int b = 0; b < R; ++b) {
        if (b == kb) {
#pragma unroll
          for (int a = b; a < R; ++a) {
            const int i = ty + G * a;
            if (i >= k) sCol[i] = acc[a][b];
          }
        }
      }
    }
    __syncthreads();
    if (tid >= k && tid < FB) {
      const float pivot = sCol[k];
      if (tid == k && !(pivot > 0.0f)) sFlag[0] = 1;
      const float d = sqrtf(pivot);
      sL[k * LD + tid] = tid == k ? d : sCol[tid] / d;
    }
    __syncthreads();
    const float* __restrict__ col = sL + k * LD;
    float li[R], lj[R];
#pragma unroll
    for (int a = 0; a < R; ++a) {
      li[a] = col[ty + G * a];  // rows / columns below k of this column were never written: they only reach elements that are done
      lj[a] = col[tx + G * a];
    }
#pragma unroll
    for (int b = 0; b < R; ++b) {
      if (b >= kb) {
#pragma unroll
        for (int a = b; a < R; ++a) acc[a][b] = fmaf(-li[a], lj[b], acc[a][b]);
      }
    }
  }
  __syncthreads();  // sB and the flag
  if (tid >= EBN_WAVE) return;
  // ---- L z = b, then L^T x = z: wave 0, lane l holds the elements l and l + 64
  const int lane = tid;
  const bool bad = sFlag[0] != 0;
  float v0 = lane < FB ? sB[lane] : 0.0f, v1 = FB > 64 ? sB[(lane + 64) % FB] : 0.0f;
#pragma unroll 1
  for (int k = 0; k < F; ++k) {
    const float* __restrict__ col = sL + k * LD;
    const float bk = __shfl(k < 64 ? v0 : v1, k & 63, EBN_WAVE);
    const float z = bk / col[k];
    if (k < 64) {
      if (lane == k) v0 = z;
      else if (lane > k && lane < F) v0 = fmaf(-col[lane], z, v0);
    } else if (lane + 64 == k) {
      v1 = z;
    }
    if (FB > 64 && lane + 64 > k && lane + 64 < F) v1 = fmaf(-col[lane + 64], z, v1);
  }
#pragma unroll 1
  for (int k = F - 1; k >= 0; --k) {
    const float zk = __shfl(k < 64 ? v0 : v1, k & 63, EBN_WAVE);
    const float x = zk / sL[k * LD + k];
    if (k < 64) {
      if (lane == k) v0 = x;
    } else {
      if (lane + 64 == k) v1 = x;
      else if (lane + 64 < k) v1 = fmaf(-sL[(lane + 64) * LD + k], x, v1);
    }
    if (lane < k && lane < 64) v0 = fmaf(-sL[lane * LD + k], x, v0);
  }
  const float nan = __int_as_float(0x7FC00000);
  if (lane < F) out[lane] = bad ? nan : v0;
  if (FB > 64 && lane + 64 < F) out[lane + 64] = bad ? nan : v1;
}

static inline bool als_vec(const float* p, int64_t ld) { return ebn_aligned16(p) && (ld % 4) == 0; }

template <int R, int G, bool VEC>
static int als_launch(bool solve, const AlsArgs& g, int64_t blocks, hipStream_t s) {
  const size_t lds = static_cast<size_t>(AlsLds<R, G>::FLOATS) * sizeof(float);
  if (solve) {
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(als_solve_kernel<R, G, VEC>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess) {
      (void)hipGetLastError();
      return EBN_ERR_UNSUPPORTED;
    }
    EBN_LAUNCH((als_solve_kernel<R, G, VEC>), dim3(static_cast<unsigned>(blocks)), dim3(G * G), lds, s, g);
  } else {
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(als_partials_kernel<R, G, VEC>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess) {
      (void)hipGetLastError();
      return EBN_ERR_UNSUPPORTED;
    }
    EBN_LAUNCH((als_partials_kernel<R, G, VEC>), dim3(static_cast<unsigned>(blocks)), dim3(G * G), lds, s, g);
  }
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

static int als_dispatch(bool solve, const AlsArgs& g, int64_t blocks, hipStream_t s) {
  const bool vec = g.fixed == nullptr || als_vec(g.fixed, g.ld);
#define ALS_CASE(R, G) return vec ? als_launch<R, G, true>(solve, g, blocks, s) : als_launch<R, G, false>(solve, g, blocks, s)
  if (g.F <= ALS_ONE_WAVE_MAX_F) {  // one wave per row, an 8 x 8 grid of lanes
    if (g.F <= 8) ALS_CASE(1, 8);
    if (g.F <= 16) ALS_CASE(2, 8);
    if (g.F <= 32) ALS_CASE(4, 8);
    ALS_CASE(8, 8);
  }
  if (g.F <= 16) ALS_CASE(1, 16);
  if (g.F <= 32) ALS_CASE(2, 16);
  if (g.F <= 64) ALS_CASE(4, 16);
  ALS_CASE(8, 16);
#undef ALS_CASE
}

}  // namespace

extern "C" int ebn_als_solve_f32(const float* fixed, int64_t n_fixed, int64_t F, int64_t ld, const float* gram, int64_t ldg,
                                 const int64_t* indptr, const int32_t* cols, const float* conf, int64_t n_solve, int64_t nnz, float reg,
                                 const int64_t* row_parts, const float* partials, int64_t n_parts, float* out, int64_t ldo,
                                 ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_fixed, F, ld, ldg) && ebn_dim_ok(n_solve, nnz, n_parts, ldo), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(F >= 1 && ld >= F && ldg >= F && ldo >= F, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(reg > 0.0f && reg <= 3.4028234664e38f, EBN_ERR_BAD_ARG);  // finite and > 0 (a NaN fails both)
  EBN_REQUIRE(n_parts == 0 || partials != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_solve == 0 || (gram != nullptr && indptr != nullptr && out != nullptr), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_solve == 0 || ((nnz == 0 || (cols != nullptr && conf != nullptr)) && (n_fixed == 0 || nnz == 0 || fixed != nullptr)),
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE(F <= EBN_ALS_MAX_F, EBN_ERR_UNSUPPORTED);
  if (n_solve == 0) return EBN_OK;
  AlsArgs g{};
  g.fixed = fixed;
  g.n_fixed = n_fixed;
  g.ld = ld;
  g.gram = gram;
  g.ldg = ldg;
  g.indptr = indptr;
  g.cols = cols;
  g.conf = conf;
  g.nnz = nnz;
  g.reg = reg;
  g.row_parts = n_parts > 0 ? row_parts : nullptr;
  g.partials_in = partials;
  g.n_parts = n_parts;
  g.out = out;
  g.ldo = ldo;
  g.F = static_cast<int32_t>(F);
  return als_dispatch(true, g, n_solve, ebn_stream(stream));
}

extern "C" int ebn_als_partials_f32(const float* fixed, int64_t n_fixed, int64_t F, int64_t ld, const int32_t* cols, const float* conf,
                                    int64_t nnz, const int64_t* part_begin, const int64_t* part_end, int64_t n_parts, float* partials,
                                    ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_fixed, F, ld, nnz) && ebn_dim_ok(n_parts), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(F >= 1 && ld >= F, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_parts == 0 || (part_begin != nullptr && part_end != nullptr && partials != nullptr), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_parts == 0 || ((nnz == 0 || (cols != nullptr && conf != nullptr)) && (n_fixed == 0 || nnz == 0 || fixed != nullptr)),
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE(F <= EBN_ALS_MAX_F, EBN_ERR_UNSUPPORTED);
  if (n_parts == 0) return EBN_OK;
  AlsArgs g{};
  g.fixed = fixed;
  g.n_fixed = n_fixed;
  g.ld = ld;
  g.cols = cols;
  g.conf = conf;
  g.nnz = nnz;
  g.part_begin = part_begin;
  g.part_end = part_end;
  g.partials_out = partials;
  g.n_parts = n_parts;
  g.F = static_cast<int32_t>(F);
  return als_dispatch(false, g, n_parts, ebn_stream(stream));
}
