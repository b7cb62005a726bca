// EASE^R baseline (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", WWW 2019; contract in include/ebnerd_hip.h): the
// item-to-item ridge regression in closed form,  G = X^T X,  P = (G + reg I)^{-1},  B[i, j] = -P[i, j] / P[j, j] (i != j), B[j, j] = 0.
//   * GRAM: one 256-thread workgroup per user row.  The m (m + 1) / 2 pairs (p >= q) of the row's entries are spread over the threads
//     by their flat index t = p (p + 1) / 2 + q (p from a float square root, corrected to the exact integer); each pair whose two
//     columns are present adds 1 to G[max, min] with an INTEGER global atomic: integer sums commute, so two runs give the same bits.
//     A row of m entries costs m (m + 1) / 2 atomics; m is not capped.  The lower triangle is zeroed by a launch of its own first.
//   * SYSTEM / MIRROR: 32 x 32 tiles of the lower triangle pass through LDS and leave twice, as they are and transposed: every
//     global access runs along a row.  The int32 form converts the counts (exact up to 2^24: above it a flag is raised) and adds
//     reg on the diagonal; the fp32 form is the closing step of the inverse ((i, j) and (j, i) get the same bits).
//   * INVERT: a host loop of launches on one stream, no synchronisation and no host read in between.  With L kept in the
//     workspace (Lw) and NB the block size:
//       1. blocked right-looking Cholesky.  Step k: ease_diag_kernel factorises the diagonal block A_kk = L_kk L_kk^T in LDS (ONE
//          workgroup, the fixed-order right-looking scheme of ebn_als.hip, correctly rounded sqrtf and division) and, in the same
//          sweep over its columns, inverts the factor: W_k = L_kk^{-1} by forward substitution on the identity, row j divided by the
//          pivot's root in step j and subtracted from the rows below.  The panel below is one GEMM, Lw_ik = A_ik W_k^T; the trailing
//          update A_22 -= L_21 L_21^T runs in column strips of EASE_STRIP that start at the diagonal (rows c0 .. n of the strip
//          [c0, c1)): the blocks above the diagonal are not touched beyond a strip's own square.
//       2. Z = L^{-1} in A (zeroed first), right-looking over block rows: row k holds -sum_{j < k} L_kj Z_j when its turn comes;
//          Z_k = W_k (that), Z_kk = W_k, and the rows below take -L_ik Z_k in one GEMM of K = NB.
//       3. P = Z^T Z into Lw in column strips (only rows >= c0 of a strip: Z is lower triangular, its upper triangle holds exact
//          zeros), then mirrored into A.
//     Every product runs on ebn_gemm_f32 without a workspace (no split-K): one fixed summation order per shape.  A pivot that is
//     not > 0 (NaN included) puts its global index + 1 into *info (the first one wins: launches on a stream are ordered) and NaN /
//     inf into everything downstream; nothing faults and nothing waits for the host.  A last block of nbk < NB rows is simply cut
//     off (the steps of an identity tail would change nothing): no row or column outside [0, n) is read or written.
//     LDS of the diagonal kernel: 2 NB (NB + 1) floats: 129 KiB at NB = 128, 32.5 KiB at 64, 8.3 KiB at 32.
//   * WEIGHTS: two launches -- every off-diagonal element -P[i, j] / P[j, j] (the diagonal is only READ here, so B == P is fine),
//     then +0.0 on the diagonal.
//   * SCORES: ebn_cv_scores_f32's staging.  256-item workgroups; one lane per item finds its list and history; then one wave per
//     item: lane s takes the history entries s, s + 64, ... in order (fmaf(w_j, B[h_j, c], acc)); a butterfly (xor 32 .. 1) folds the
//     lanes.  Fixed order, no atomics, no workspace.
// There is no floating-point atomic in this file.
#include <type_traits>

#include "ebn_common.h"

#define EASE_T 256        // threads of the element-wise, gram and score workgroups
#define EASE_DT 512       // threads of the diagonal-block workgroup: a 16 x 32 grid (tx = tid % 16 columns, ty = tid / 16 rows)
#define EASE_TILE 32      // tile edge of the system / mirror kernel
#define EASE_STRIP 1024   // columns of one strip of the trailing update and of Z^T Z
#define EASE_GW 64        // lanes of one item in the scores kernel (a wave)
#ifndef EASE_NB
#define EASE_NB 128       // block size of ebn_ease_invert_f32, measured at ease-c1: 32 / 64 / 128 take
                          // 38.5 / 28.2 / 27.9 ms at n = 8192 and 223.7 / 145.5 / 115.5 ms at n = 16384
#endif
#define EASE_NB_MAX 128

static_assert(EASE_NB == 32 || EASE_NB == 64 || EASE_NB == 128, "the diagonal kernel has these three instantiations");
static_assert(EASE_STRIP % EASE_NB_MAX == 0 && EBN_EASE_MAX_ITEMS / EASE_TILE <= 65535, "strips start on block boundaries; tiles fit gridDim.y");
static_assert(EASE_T % EASE_GW == 0 && EBN_WAVE == EASE_GW, "one wave per item");

namespace {

__device__ __forceinline__ int64_t ease_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- gram ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EASE_T) void ease_zero_lower_i32_kernel(int32_t* __restrict__ G, int64_t ldg) {
  const int64_t i = blockIdx.y;  // one row of the grid per matrix row
  for (int64_t j = static_cast<int64_t>(blockIdx.x) * EASE_T + threadIdx.x; j <= i; j += static_cast<int64_t>(gridDim.x) * EASE_T) G[i * ldg + j] = 0;
}

__global__ __launch_bounds__(EASE_T) void ease_gram_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ cols, int64_t nnz,
                                                           int64_t n_items, int32_t* __restrict__ G, int64_t ldg) {
  const int64_t u = blockIdx.x;
  const int64_t b = ease_clamp(indptr[u], nnz), e = ease_clamp(indptr[u + 1], nnz);
  if (e <= b) return;
  const int64_t m = e - b, pairs = m * (m + 1) / 2;  // m <= 2^31 - 1: below 2^62
  for (int64_t t = threadIdx.x; t < pairs; t += EASE_T) {
    int64_t p = static_cast<int64_t>((sqrtf(8.0f * static_cast<float>(t) + 1.0f) - 1.0f) * 0.5f);
    p = p < 0 ? 0 : (p >= m ? m - 1 : p);
    while (p * (p + 1) / 2 > t) --p;
    while ((p + 1) * (p + 2) / 2 <= t) ++p;
    const int64_t q = t - p * (p + 1) / 2;  // 0 <= q <= p < m
    const int64_t ci = cols[b + p], cj = cols[b + q];
    if (ci >= 0 && ci < n_items && cj >= 0 && cj < n_items) {
      const int64_t hi = ci > cj ? ci : cj, lo = ci > cj ? cj : ci;
      atomicAdd(&G[hi * ldg + lo], 1);
    }
  }
}

// ---- system / mirror: dst[i, j] = dst[j, i] = value(src[max(i, j), min(i, j)]) -----------------------------------------------------
template <typename T>
__global__ __launch_bounds__(EASE_T) void ease_sym_kernel(const T* __restrict__ src, int64_t lds_, int64_t n, float reg, float* __restrict__ dst,
                                                          int64_t ldd, int32_t* __restrict__ flag) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  __shared__ float tile[EASE_TILE][EASE_TILE + 1];
  const int tx = threadIdx.x % EASE_TILE, ty = threadIdx.x / EASE_TILE;
  const int64_t i0 = static_cast<int64_t>(bi) * EASE_TILE, j0 = static_cast<int64_t>(bj) * EASE_TILE;
  bool over = false;
  for (int r = ty; r < EASE_TILE; r += EASE_T / EASE_TILE) {
    const int64_t i = i0 + r, j = j0 + tx;
    float v = 0.0f;
    if (i < n && j <= i) {  // j <= i < n
      const T s = src[i * lds_ + j];
      if constexpr (std::is_same<T, int32_t>::value) {
        over = over || s > (1 << 24);
        v = static_cast<float>(s);
        if (i == j) v += reg;
      } else {
        v = static_cast<float>(s);
      }
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < EASE_TILE; r += EASE_T / EASE_TILE) {
    const int64_t i = i0 + r, j = j0 + tx;
    if (i < n && j < n) dst[i * ldd + j] = (bi != bj || tx <= r) ? tile[r][tx] : tile[tx][r];
    if (bi != bj) {
      const int64_t ti = j0 + r, tj = i0 + tx;  // the transposed tile
      if (ti < n && tj < n) dst[ti * ldd + tj] = tile[tx][r];
    }
  }
  if (over) *flag = 1;  // plain vector stores of the same value: only ever set
}

// ---- invert --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EASE_T) void ease_fill_kernel(float* __restrict__ A, int64_t lda, int64_t rows, int64_t cols, float v) {
  const int64_t total = rows * cols;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * EASE_T + threadIdx.x; t < total; t += static_cast<int64_t>(gridDim.x) * EASE_T) {
    const int64_t i = t / cols;
    A[i * lda + (t - i * cols)] = v;
  }
}

__global__ __launch_bounds__(EASE_T) void ease_copy_kernel(const float* __restrict__ src, int64_t lds_, float* __restrict__ dst, int64_t ldd,
                                                           int64_t rows, int64_t cols) {
  const int64_t total = rows * cols;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * EASE_T + threadIdx.x; t < total; t += static_cast<int64_t>(gridDim.x) * EASE_T) {
    const int64_t i = t / cols, j = t - i * cols;
    dst[i * ldd + j] = src[i * lds_ + j];
  }
}

__global__ void ease_set_i32_kernel(int32_t* p, int32_t v) { *p = v; }

// The diagonal block [k0, k0 + nbk) of A (lower triangle read): L in LDS by right-looking Cholesky, W = L^{-1} beside it; W leaves as
// an [nbk, nbk] block at row stride NB with zeros above the diagonal.  L's diagonal is never stored: only its roots d are used.
template <int NB>
__global__ __launch_bounds__(EASE_DT) void ease_diag_kernel(const float* __restrict__ A, int64_t lda, int64_t k0, int nbk, float* __restrict__ W,
                                                            int32_t* __restrict__ info) {
  constexpr int LD = NB + 1;
  extern __shared__ __attribute__((aligned(16))) float ease_lds[];
  float* S = ease_lds;
  float* Wm = ease_lds + NB * LD;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  for (int idx = tid; idx < nbk * nbk; idx += EASE_DT) {
    const int i = idx / nbk, c = idx - i * nbk;
    S[i * LD + c] = c <= i ? A[(k0 + i) * lda + k0 + c] : 0.0f;
    Wm[i * LD + c] = i == c ? 1.0f : 0.0f;
  }
  __syncthreads();
  int32_t bad = 0;
#pragma unroll 1
  for (int j = 0; j < nbk; ++j) {
    const float pivot = S[j * LD + j];  // never overwritten
    if (!(pivot > 0.0f) && bad == 0) bad = static_cast<int32_t>(k0 + j + 1);
    const float d = sqrtf(pivot);
    for (int i = j + 1 + tid; i < nbk; i += EASE_DT) S[i * LD + j] = S[i * LD + j] / d;
    for (int c = tid; c <= j; c += EASE_DT) Wm[j * LD + c] = Wm[j * LD + c] / d;
    __syncthreads();
    for (int i = j + 1 + ty; i < nbk; i += EASE_DT / 16) {
      const float lij = S[i * LD + j];
      for (int c = j + 1 + tx; c <= i; c += 16) S[i * LD + c] = fmaf(-lij, S[c * LD + j], S[i * LD + c]);
      for (int c = tx; c <= j; c += 16) Wm[i * LD + c] = fmaf(-lij, Wm[j * LD + c], Wm[i * LD + c]);
    }
    __syncthreads();
  }
  for (int idx = tid; idx < nbk * nbk; idx += EASE_DT) {
    const int i = idx / nbk, c = idx - i * nbk;
    W[i * NB + c] = c <= i ? Wm[i * LD + c] : 0.0f;
  }
  if (tid == 0 && bad != 0 && *info == 0) *info = bad;
}

template <int NB>
int ease_diag_launch(const float* A, int64_t lda, int64_t k0, int nbk, float* W, int32_t* info, hipStream_t s) {
  const size_t lds = static_cast<size_t>(2) * NB * (NB + 1) * sizeof(float);
  // above the 64 KiB a kernel may use without asking (NB = 128); set per call: the attribute belongs to the current device
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(&ease_diag_kernel<NB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return EBN_ERR_UNSUPPORTED;
  }
  EBN_LAUNCH(ease_diag_kernel<NB>, dim3(1), dim3(EASE_DT), lds, s, A, lda, k0, nbk, W, info);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

inline int64_t ease_ldw(int64_t n) { return (n + 3) / 4 * 4; }
inline unsigned ease_grid(int64_t total) {
  const int64_t g = ebn_ceil_div(total, EASE_T);
  return static_cast<unsigned>(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

#define EASE_TRY(call)          \
  do {                          \
    const int rc__ = (call);    \
    if (rc__ != EBN_OK) return rc__; \
  } while (0)

int ease_copy(const float* src, int64_t lds_, float* dst, int64_t ldd, int64_t rows, int64_t cols, hipStream_t s) {
  EBN_LAUNCH(ease_copy_kernel, dim3(ease_grid(rows * cols)), dim3(EASE_T), 0, s, src, lds_, dst, ldd, rows, cols);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

int ease_invert(float* A, int64_t lda, int64_t n, float* work, int32_t* info, int nb, ebn_stream_t stream) {
  hipStream_t s = ebn_stream(stream);
  const int64_t ldw = ease_ldw(n), n_blocks = ebn_ceil_div(n, nb);
  float* Lw = work;                                   // [n, ldw]: L's panels, later P
  float* Wb = Lw + n * ldw;                           // [n_blocks][nb, nb]: the inverted diagonal factors
  float* T = Wb + n_blocks * nb * nb;                 // [nb, ldw]: one block row of Z on its way
  EBN_LAUNCH(ease_set_i32_kernel, dim3(1), dim3(1), 0, s, info, 0);
  EBN_CHECK_LAUNCH();
  // ---- 1. A = L L^T
  for (int64_t k = 0; k < n_blocks; ++k) {
    const int64_t k0 = k * nb, k1 = k0 + nb < n ? k0 + nb : n, nbk = k1 - k0;
    float* Wk = Wb + k * nb * nb;
    if (nb == 32) EASE_TRY(ease_diag_launch<32>(A, lda, k0, static_cast<int>(nbk), Wk, info, s));
    else if (nb == 64) EASE_TRY(ease_diag_launch<64>(A, lda, k0, static_cast<int>(nbk), Wk, info, s));
    else EASE_TRY(ease_diag_launch<128>(A, lda, k0, static_cast<int>(nbk), Wk, info, s));
    if (k1 == n) break;
    float* panel = Lw + k1 * ldw + k0;  // L[k1 .. n, k0 .. k1)
    EASE_TRY(ebn_gemm_f32(0, 1, n - k1, nbk, nbk, 1.0f, A + k1 * lda + k0, lda, Wk, nb, 0.0f, panel, ldw, stream));
    for (int64_t c0 = k1; c0 < n; c0 += EASE_STRIP) {
      const int64_t c1 = c0 + EASE_STRIP < n ? c0 + EASE_STRIP : n;
      const float* rows = Lw + c0 * ldw + k0;
      EASE_TRY(ebn_gemm_f32(0, 1, n - c0, c1 - c0, nbk, -1.0f, rows, ldw, rows, ldw, 1.0f, A + c0 * lda + c0, lda, stream));
    }
  }
  // ---- 2. Z = L^{-1} in A
  EBN_LAUNCH(ease_fill_kernel, dim3(ease_grid(n * n)), dim3(EASE_T), 0, s, A, lda, n, n, 0.0f);
  EBN_CHECK_LAUNCH();
  for (int64_t k = 0; k < n_blocks; ++k) {
    const int64_t k0 = k * nb, k1 = k0 + nb < n ? k0 + nb : n, nbk = k1 - k0;
    const float* Wk = Wb + k * nb * nb;
    if (k0 > 0) {
      EASE_TRY(ebn_gemm_f32(0, 0, nbk, k0, nbk, 1.0f, Wk, nb, A + k0 * lda, lda, 0.0f, T, ldw, stream));
      EASE_TRY(ease_copy(T, ldw, A + k0 * lda, lda, nbk, k0, s));
    }
    EASE_TRY(ease_copy(Wk, nb, A + k0 * lda + k0, lda, nbk, nbk, s));
    if (k1 < n) EASE_TRY(ebn_gemm_f32(0, 0, n - k1, k1, nbk, -1.0f, Lw + k1 * ldw + k0, ldw, A + k0 * lda, lda, 1.0f, A + k1 * lda, lda, stream));
  }
  // ---- 3. P = Z^T Z: the lower part of every column strip into Lw, then both triangles into A
  for (int64_t c0 = 0; c0 < n; c0 += EASE_STRIP) {
    const int64_t c1 = c0 + EASE_STRIP < n ? c0 + EASE_STRIP : n;
    const float* z = A + c0 * lda + c0;
    EASE_TRY(ebn_gemm_f32(1, 0, n - c0, c1 - c0, n - c0, 1.0f, z, lda, z, lda, 0.0f, Lw + c0 * ldw + c0, ldw, stream));
  }
  const unsigned tiles = static_cast<unsigned>(ebn_ceil_div(n, EASE_TILE));
  EBN_LAUNCH(ease_sym_kernel<float>, dim3(tiles, tiles), dim3(EASE_T), 0, s, Lw, ldw, n, 0.0f, A, lda, static_cast<int32_t*>(nullptr));
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

int64_t ease_workspace_floats(int64_t n, int nb) {
  const int64_t ldw = ease_ldw(n);
  return n * ldw + ebn_ceil_div(n, nb) * nb * nb + nb * ldw;
}

// ---- weights -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EASE_T) void ease_weights_kernel(const float* P, int64_t ldp, int64_t n, float* B, int64_t ldb) {
  const int64_t i = blockIdx.y;
  for (int64_t j = static_cast<int64_t>(blockIdx.x) * EASE_T + threadIdx.x; j < n; j += static_cast<int64_t>(gridDim.x) * EASE_T)
    if (j != i) B[i * ldb + j] = -(P[i * ldp + j] / P[j * ldp + j]);  // the diagonal is read here and written by the next launch
}

__global__ __launch_bounds__(EASE_T) void ease_zero_diag_kernel(float* __restrict__ B, int64_t ldb, int64_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * EASE_T + threadIdx.x;
  if (i < n) B[i * ldb + i] = 0.0f;
}

// ---- scores --------------------------------------------------------------------------------------------------------------------
// first position in [lo, hi) whose value is above key (hi if none)
__device__ __forceinline__ int64_t ease_upper_bound(const int64_t* __restrict__ v, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The list of element i = i0 + threadIdx.x among offsets [n + 1]: #{ k in [0, n] : offsets[k] <= i } - 1, in [-1, n] (cv_list_of of
// ebn_covisit.hip: one uniform search per workgroup, EASE_T staged boundaries, a fallback search behind a run of empty lists).
__device__ __forceinline__ int64_t ease_list_of(const int64_t* __restrict__ offsets, int64_t n, int64_t i0, int64_t* s_bound) {
  const int t = threadIdx.x;
  const int64_t i = i0 + t;
  const int64_t base = ease_upper_bound(offsets, 0, n + 1, i0);
  const int64_t q = base + t;
  s_bound[t] = q <= n ? offsets[q] : INT64_MAX;
  __syncthreads();
  int c = 0;
#pragma unroll
  for (int step = EASE_T / 2; step > 0; step >>= 1) c += s_bound[c + step - 1] <= i ? step : 0;
  c += s_bound[c] <= i ? 1 : 0;
  int64_t l = base + c;
  if (c == EASE_T && l <= n) l = ease_upper_bound(offsets, l, n + 1, i);
  return l - 1;
}

__global__ __launch_bounds__(EASE_T) void ease_scores_kernel(const float* __restrict__ B, int64_t n_items, int64_t ldb,
                                                             const int32_t* __restrict__ hist_rows, const float* __restrict__ hist_weights,
                                                             const int64_t* __restrict__ hist_offsets, int64_t n_hists, int64_t n_hist_items,
                                                             const int32_t* __restrict__ list_hist, const int32_t* __restrict__ cand_rows,
                                                             const int64_t* __restrict__ cand_offsets, int64_t n_lists, int64_t n_cand_items,
                                                             float* __restrict__ scores) {
  __shared__ int64_t s_bound[EASE_T];
  __shared__ int32_t s_hb[EASE_T], s_he[EASE_T], s_c[EASE_T];  // the item's history extent (empty: nothing to score) and row
  __shared__ float s_score[EASE_T];
  const int t = threadIdx.x;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * EASE_T, i = i0 + t;
  // ---- phase 1: one lane per item
  int64_t l = ease_list_of(cand_offsets, n_lists, i0, s_bound);
  l = l < 0 ? 0 : (l >= n_lists ? n_lists - 1 : l);  // never an address past list_hist
  int32_t hb = 0, he = 0, hc = 0;
  if (i < n_cand_items) {
    const int64_t u = list_hist != nullptr ? static_cast<int64_t>(list_hist[l]) : l;
    const int64_t c = cand_rows[i];
    if (u >= 0 && u < n_hists && c >= 0 && c < n_items) {
      hb = static_cast<int32_t>(ease_clamp(hist_offsets[u], n_hist_items));  // <= EBN_DIM_MAX
      he = static_cast<int32_t>(ease_clamp(hist_offsets[u + 1], n_hist_items));
      hc = static_cast<int32_t>(c);
    }
  }
  s_hb[t] = hb;
  s_he[t] = he;
  s_c[t] = hc;
  __syncthreads();
  // ---- phase 2: one wave per item
  const int sub = t & (EASE_GW - 1), grp = t / EASE_GW;
  const int64_t left = n_cand_items - i0;
  const int n_live = left < EASE_T ? static_cast<int>(left) : EASE_T;
#pragma unroll 1
  for (int r0 = 0; r0 < n_live; r0 += EASE_T / EASE_GW) {
    const int it = r0 + grp;  // items past n_live hold an empty extent
    const int32_t b = s_hb[it], e = s_he[it], c = s_c[it];
    float acc = 0.0f;
    bool any = false;
    for (int32_t j = b + sub; j < e; j += EASE_GW) {
      const int64_t h = hist_rows[j];
      if (h >= 0 && h < n_items) {
        any = true;
        const float v = B[h * ldb + c];
        acc = hist_weights != nullptr ? fmaf(hist_weights[j], v, acc) : acc + v;
      }
    }
#pragma unroll
    for (int off = EASE_GW / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, EBN_WAVE);
    const bool scored = __ballot(any) != 0ull;  // no present entry: exact +0
    if (sub == 0) s_score[it] = scored ? acc : 0.0f;
  }
  __syncthreads();
  if (i < n_cand_items) scores[i] = s_score[t];
}

inline bool ease_finite(float v) { return v >= -3.4028234664e38f && v <= 3.4028234664e38f; }  // a NaN fails both

}  // namespace

extern "C" int ebn_ease_block(void) { return EASE_NB; }

extern "C" int64_t ebn_ease_workspace_floats(int64_t n) {
  if (n < 0 || n > EBN_EASE_MAX_ITEMS) return 0;
  return ease_workspace_floats(n, EASE_NB_MAX);  // the largest of the three block sizes: enough for each
}

extern "C" int ebn_ease_gram_i32(const int64_t* indptr, const int32_t* cols, int64_t n_users, int64_t nnz, int64_t n_items, int32_t* G,
                                 int64_t ldg, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_users, nnz, n_items, ldg) && ldg >= n_items, EBN_ERR_BAD_ARG);
  EBN_REQUIRE((n_items == 0 || G != nullptr) && (n_users == 0 || indptr != nullptr) && (nnz == 0 || cols != nullptr), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_items <= EBN_EASE_MAX_ITEMS, EBN_ERR_UNSUPPORTED);
  if (n_items == 0) return EBN_OK;
  hipStream_t s = ebn_stream(stream);
  const int64_t across = ebn_ceil_div(n_items, EASE_T);
  EBN_LAUNCH(ease_zero_lower_i32_kernel, dim3(static_cast<unsigned>(across < 16 ? across : 16), static_cast<unsigned>(n_items)), dim3(EASE_T), 0, s, G,
             ldg);
  EBN_CHECK_LAUNCH();
  if (n_users == 0 || nnz == 0) return EBN_OK;
  EBN_LAUNCH(ease_gram_kernel, dim3(static_cast<unsigned>(n_users)), dim3(EASE_T), 0, s, indptr, cols, nnz, n_items, G, ldg);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ease_system_f32(const int32_t* G, int64_t ldg, int64_t n, float reg, float* A, int64_t lda, int32_t* flag,
                                   ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n, ldg, lda) && ldg >= n && lda >= n && ease_finite(reg), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n == 0 || (G != nullptr && A != nullptr && flag != nullptr), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n <= EBN_EASE_MAX_ITEMS, EBN_ERR_UNSUPPORTED);
  if (n == 0) return EBN_OK;
  const unsigned tiles = static_cast<unsigned>(ebn_ceil_div(n, EASE_TILE));
  EBN_LAUNCH(ease_sym_kernel<int32_t>, dim3(tiles, tiles), dim3(EASE_T), 0, ebn_stream(stream), G, ldg, n, reg, A, lda, flag);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ease_invert_nb_f32(float* A, int64_t lda, int64_t n, float* work, int64_t work_floats, int32_t* info, int32_t nb,
                                      ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n, lda) && lda >= n && A != nullptr && work != nullptr && info != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(nb == 32 || nb == 64 || nb == 128, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n <= EBN_EASE_MAX_ITEMS && work_floats >= ease_workspace_floats(n, nb), EBN_ERR_UNSUPPORTED);
  if (n == 0) return EBN_OK;
  return ease_invert(A, lda, n, work, info, nb, stream);
}

extern "C" int ebn_ease_invert_f32(float* A, int64_t lda, int64_t n, float* work, int64_t work_floats, int32_t* info, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n, lda) && lda >= n && A != nullptr && work != nullptr && info != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n <= EBN_EASE_MAX_ITEMS && work_floats >= ebn_ease_workspace_floats(n), EBN_ERR_UNSUPPORTED);
  if (n == 0) return EBN_OK;
  return ease_invert(A, lda, n, work, info, EASE_NB, stream);
}

extern "C" int ebn_ease_weights_f32(const float* P, int64_t ldp, int64_t n, float* B, int64_t ldb, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n, ldp, ldb) && ldp >= n && ldb >= n, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n == 0 || (P != nullptr && B != nullptr), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n <= EBN_EASE_MAX_ITEMS, EBN_ERR_UNSUPPORTED);
  if (n == 0) return EBN_OK;
  hipStream_t s = ebn_stream(stream);
  const int64_t across = ebn_ceil_div(n, EASE_T);
  EBN_LAUNCH(ease_weights_kernel, dim3(static_cast<unsigned>(across < 16 ? across : 16), static_cast<unsigned>(n)), dim3(EASE_T), 0, s, P, ldp, n, B,
             ldb);
  EBN_CHECK_LAUNCH();
  EBN_LAUNCH(ease_zero_diag_kernel, dim3(static_cast<unsigned>(across)), dim3(EASE_T), 0, s, B, ldb, n);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_ease_scores_f32(const float* B, int64_t n_items, int64_t ldb, const int32_t* hist_rows, const float* hist_weights,
                                   const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items, const int32_t* list_hist,
                                   const int32_t* cand_rows, const int64_t* cand_offsets, int64_t n_lists, int64_t n_cand_items, float* scores,
                                   ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(n_items, ldb, n_hists, n_hist_items) && ebn_dim_ok(n_lists, n_cand_items) && ldb >= n_items, EBN_ERR_BAD_ARG);
  EBN_REQUIRE((n_cand_items == 0 || n_lists >= 1) && (n_hist_items == 0 || n_hists >= 1), EBN_ERR_BAD_ARG);
  if (n_cand_items == 0) return EBN_OK;
  EBN_REQUIRE(cand_rows != nullptr && cand_offsets != nullptr && scores != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE((n_items == 0 || B != nullptr) && (n_hists == 0 || hist_offsets != nullptr) && (n_hist_items == 0 || hist_rows != nullptr),
              EBN_ERR_BAD_ARG);
  EBN_LAUNCH(ease_scores_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(n_cand_items, EASE_T))), dim3(EASE_T), 0, ebn_stream(stream), B, n_items,
             ldb, hist_rows, hist_weights, hist_offsets, n_hists, n_hist_items, list_hist, cand_rows, cand_offsets, n_lists, n_cand_items, scores);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
