// NAML (reference naml.py, layers.py:55-81): the two categorical views of the news encoder and the view-level AttLayer2.
//
// The four views of an article live view-major in one buffer, Vw [n_views, N, F] (view v of article n at row v*N + n), so the
// title / body poolings write Vw[0] / Vw[1] contiguously and the view attention's x.W is one GEMM over n_views*N rows.
//
// Categorical views (vert, subvert; naml.py _build_vertencoder / _build_subvertencoder), both in one launch (grid.y = view):
//   e_n = table[ids[n]] (K floats; an id outside [0, n_rows) reads a zero row and sets *oob_flag);
//   out[n, f] = relu(sum_k e_n[k] W[k, f] + b[f]),  Wb [K+1, F] = the Dense kernel rows, then the bias row.
// K is small and arbitrary (vert_emb_dim = 10): the contraction runs on the VALU, k ascending.
// Backward, with dY = dout * (out > 0) (the ReLU gate read back from the forward's output):
//   launch 1, per slice of CV_BWD_ROWS articles: partial [dW ; db] of the slice (rows ascending) and de[n, k] = dY_n . W_k;
//   launch 2: dWb = sum of the slices (ascending), dtable[r, k] = sum of de[n, k] over the articles n with ids[n] == r
//   (ascending n).  Fixed summation orders, no atomics: the same bits on every run.
//
// View attention (AttLayer2 over the n_views rows of each article, one wave per article):
//   U <- tanh(U + b) in place (U = Vw.Wa from ebn_gemm_f32, row v*N + n);  a_v = exp(U_v . q) (no max-subtraction);
//   w_v = a_v / (sum_v a + 1e-7);  news[n] = sum_v w_v Vw[v, n].
// Backward: dw_v = dnews_n . Vw[v, n], de_v = w_v (dw_v - sum_u w_u dw_u), dVw[v, n] = w_v dnews_n (the direct term); the rest
// (d(pre-tanh), dq, db, dWa and dpre.Wa^T) is ebn_attpool_bwd_dpre_f32 over the n_views*N rows and two GEMMs.
#include "ebn_common.h"

namespace {

constexpr int CV_THREADS = 256;
constexpr int CV_FWD_ROWS = 16;  // articles per forward workgroup
constexpr int CV_BWD_ROWS = 32;  // articles per backward slice
constexpr int CV_MAX_K = 256;
constexpr int NAML_MAX_F = 65536;
constexpr int VA_WAVES = 4;
constexpr int VA_MAX_VIEWS = 8;
constexpr float KERAS_EPS = 1e-7f;  // K.epsilon(), layers.py:75-77

struct CatView {
  const int32_t* ids;
  const float* table;  // [n_rows, K]
  int64_t n_rows;
  int32_t K;
  const float* Wb;     // [K + 1, F]
  float* out;          // [N, F]
  const float* dout;   // [N, F]
  float* dWb;          // [K + 1, F]
  float* dtable;       // [n_rows, K]
  float* part;         // [n_slices, K + 1, F]
  float* de;           // [N, K]
};

struct CatArgs {
  CatView v[2];
  int64_t N;
  int32_t F;
  int64_t n_slices;
  int32_t* oob_flag;
};

template <int ROWS>
__device__ __forceinline__ void gather_slice(const CatView& v, int64_t n0, int rows, float* es, int32_t* oob_flag) {
  const int K = v.K;
  for (int i = threadIdx.x; i < ROWS * K; i += CV_THREADS) {
    const int r = i / K, k = i - r * K;
    float val = 0.f;
    if (r < rows) {
      const int32_t id = v.ids[n0 + r];
      if (id >= 0 && id < v.n_rows) {
        val = v.table[static_cast<int64_t>(id) * K + k];
      } else if (k == 0 && oob_flag != nullptr) {
        *oob_flag = 1;
      }
    }
    es[i] = val;
  }
}

__global__ __launch_bounds__(CV_THREADS) void catview_fwd_kernel(CatArgs a) {
  __shared__ float es[CV_FWD_ROWS * CV_MAX_K];
  const CatView& v = a.v[blockIdx.y];
  const int K = v.K, F = a.F;
  const int64_t n0 = static_cast<int64_t>(blockIdx.x) * CV_FWD_ROWS;
  const int rows = static_cast<int>(a.N - n0 < CV_FWD_ROWS ? a.N - n0 : CV_FWD_ROWS);
  gather_slice<CV_FWD_ROWS>(v, n0, rows, es, a.oob_flag);
  __syncthreads();
  for (int f = threadIdx.x; f < F; f += CV_THREADS) {
    float acc[CV_FWD_ROWS];
#pragma unroll
    for (int r = 0; r < CV_FWD_ROWS; ++r) acc[r] = 0.f;
    for (int k = 0; k < K; ++k) {
      const float wk = v.Wb[static_cast<int64_t>(k) * F + f];
#pragma unroll
      for (int r = 0; r < CV_FWD_ROWS; ++r) acc[r] = fmaf(es[r * K + k], wk, acc[r]);
    }
    const float bf = v.Wb[static_cast<int64_t>(K) * F + f];
#pragma unroll
    for (int r = 0; r < CV_FWD_ROWS; ++r) {
      if (r < rows) {
        const float y = acc[r] + bf;
        v.out[(n0 + r) * F + f] = y > 0.f ? y : 0.f;
      }
    }
  }
}

__global__ __launch_bounds__(CV_THREADS) void catview_bwd_part_kernel(CatArgs a) {
  __shared__ float es[CV_BWD_ROWS * CV_MAX_K];
  const CatView& v = a.v[blockIdx.y];
  const int K = v.K, F = a.F;
  const int64_t s = blockIdx.x;
  const int64_t n0 = s * CV_BWD_ROWS;
  const int rows = static_cast<int>(a.N - n0 < CV_BWD_ROWS ? a.N - n0 : CV_BWD_ROWS);
  gather_slice<CV_BWD_ROWS>(v, n0, rows, es, nullptr);
  __syncthreads();
  float* part = v.part + s * (static_cast<int64_t>(K) + 1) * F;
  for (int f = threadIdx.x; f < F; f += CV_THREADS) {
    float dy[CV_BWD_ROWS];
#pragma unroll
    for (int r = 0; r < CV_BWD_ROWS; ++r) {
      float g = 0.f;
      if (r < rows) {
        const int64_t i = (n0 + r) * F + f;
        g = v.out[i] > 0.f ? v.dout[i] : 0.f;
      }
      dy[r] = g;
    }
    for (int k = 0; k < K; ++k) {
      float acc = 0.f;
#pragma unroll
      for (int r = 0; r < CV_BWD_ROWS; ++r) acc = fmaf(es[r * K + k], dy[r], acc);
      part[static_cast<int64_t>(k) * F + f] = acc;
    }
    float db = 0.f;
#pragma unroll
    for (int r = 0; r < CV_BWD_ROWS; ++r) db += dy[r];
    part[static_cast<int64_t>(K) * F + f] = db;
  }
  // de[n, k] = dY_n . W_k: one wave per (article, k) pair, lanes strided over f, then the wave's butterfly
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = wave; p < rows * K; p += CV_THREADS / 64) {
    const int r = p / K, k = p - r * K;
    const int64_t n = n0 + r;
    const float* wk = v.Wb + static_cast<int64_t>(k) * F;
    float acc = 0.f;
    for (int f = lane; f < F; f += 64) {
      const int64_t i = n * F + f;
      acc = fmaf(v.out[i] > 0.f ? v.dout[i] : 0.f, wk[f], acc);
    }
    acc = ebn_wave_sum(acc);
    if (lane == 0) v.de[n * K + k] = acc;
  }
}

__global__ __launch_bounds__(CV_THREADS) void catview_bwd_finish_kernel(CatArgs a) {
  const CatView& v = a.v[blockIdx.y];
  const int K = v.K;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * CV_THREADS + threadIdx.x;
  const int64_t n_wb = (static_cast<int64_t>(K) + 1) * a.F;
  if (i < n_wb) {
    float acc = 0.f;
    for (int64_t s = 0; s < a.n_slices; ++s) acc += v.part[s * n_wb + i];
    v.dWb[i] = acc;
  }
  if (i < v.n_rows * K) {
    const int64_t r = i / K;
    const int k = static_cast<int>(i - r * K);
    float acc = 0.f;
    for (int64_t n = 0; n < a.N; ++n)
      if (v.ids[n] == r) acc += v.de[n * K + k];
    v.dtable[i] = acc;
  }
}

__global__ __launch_bounds__(VA_WAVES * 64) void viewatt_fwd_kernel(float* __restrict__ U, const float* __restrict__ b,
                                                                    const float* __restrict__ q, const float* __restrict__ Vw,
                                                                    float* __restrict__ w, float* __restrict__ news, int64_t N,
                                                                    int nv, int F, int A) {
  const int lane = threadIdx.x & 63;
  const int64_t n = static_cast<int64_t>(blockIdx.x) * VA_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;
  float wv[VA_MAX_VIEWS];
  float sum = 0.f;
#pragma unroll
  for (int v = 0; v < VA_MAX_VIEWS; ++v) {
    wv[v] = 0.f;
    if (v < nv) {
      float* urow = U + (v * N + n) * A;
      float part = 0.f;
      for (int k = lane; k < A; k += 64) {
        const float u = tanhf(urow[k] + b[k]);
        urow[k] = u;
        part = fmaf(u, q[k], part);
      }
      wv[v] = expf(ebn_wave_sum(part));
      sum += wv[v];
    }
  }
  sum += KERAS_EPS;
#pragma unroll
  for (int v = 0; v < VA_MAX_VIEWS; ++v) {
    if (v < nv) {
      wv[v] = wv[v] / sum;
      if (lane == 0) w[v * N + n] = wv[v];
    }
  }
  for (int f = lane; f < F; f += 64) {
    float acc = 0.f;
#pragma unroll
    for (int v = 0; v < VA_MAX_VIEWS; ++v)
      if (v < nv) acc = fmaf(wv[v], Vw[(v * N + n) * F + f], acc);
    news[n * F + f] = acc;
  }
}

__global__ __launch_bounds__(VA_WAVES * 64) void viewatt_bwd_kernel(const float* __restrict__ Vw, const float* __restrict__ w,
                                                                    const float* __restrict__ dnews, float* __restrict__ dVw,
                                                                    float* __restrict__ de, int64_t N, int nv, int F) {
  const int lane = threadIdx.x & 63;
  const int64_t n = static_cast<int64_t>(blockIdx.x) * VA_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* dn = dnews + n * F;
  float wv[VA_MAX_VIEWS], dw[VA_MAX_VIEWS];
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < VA_MAX_VIEWS; ++v) {
    wv[v] = 0.f;
    dw[v] = 0.f;
    if (v < nv) {
      const float* x = Vw + (v * N + n) * F;
      float part = 0.f;
      for (int f = lane; f < F; f += 64) part = fmaf(dn[f], x[f], part);
      wv[v] = w[v * N + n];
      dw[v] = ebn_wave_sum(part);
      s = fmaf(wv[v], dw[v], s);
    }
  }
#pragma unroll
  for (int v = 0; v < VA_MAX_VIEWS; ++v)
    if (v < nv && lane == 0) de[v * N + n] = wv[v] * (dw[v] - s);
  for (int f = lane; f < F; f += 64) {
    const float g = dn[f];
#pragma unroll
    for (int v = 0; v < VA_MAX_VIEWS; ++v)
      if (v < nv) dVw[(v * N + n) * F + f] = wv[v] * g;
  }
}

int catview_check(int64_t N, int32_t F, int64_t rows0, int32_t K0, int64_t rows1, int32_t K1) {
  EBN_REQUIRE(N >= 0 && F > 0 && rows0 > 0 && rows1 > 0 && K0 > 0 && K1 > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(N <= EBN_DIM_MAX && F <= NAML_MAX_F && K0 <= CV_MAX_K && K1 <= CV_MAX_K && rows0 <= EBN_DIM_MAX &&
                  rows1 <= EBN_DIM_MAX,
              EBN_ERR_UNSUPPORTED);
  // every element index of out / dout / de / the tables stays far below 2^62
  EBN_REQUIRE(ebn_sat_mul(N, F) < (int64_t(1) << 40) && ebn_sat_mul(rows0, K0) < (int64_t(1) << 40) &&
                  ebn_sat_mul(rows1, K1) < (int64_t(1) << 40),
              EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

CatView cat_view(const int32_t* ids, const float* table, int64_t n_rows, int32_t K, const float* Wb) {
  CatView v{};
  v.ids = ids;
  v.table = table;
  v.n_rows = n_rows;
  v.K = K;
  v.Wb = Wb;
  return v;
}

int viewatt_check(int64_t N, int32_t n_views, int32_t F) {
  EBN_REQUIRE(N >= 0 && n_views > 0 && F > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_views <= VA_MAX_VIEWS && F <= NAML_MAX_F && N <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(ebn_sat_mul(ebn_sat_mul(N, n_views), F) < (int64_t(1) << 40), EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

}  // namespace

extern "C" int64_t ebn_naml_catview_partials_len(int64_t N, int32_t K0, int32_t K1, int32_t F) {
  if (!ebn_dim_ok(N, K0, K1, F) || K0 > CV_MAX_K || K1 > CV_MAX_K) return 0;
  const int64_t slices = ebn_ceil_div(N, CV_BWD_ROWS);
  return ebn_sat_add(ebn_sat_mul(ebn_sat_mul(slices, static_cast<int64_t>(K0) + K1 + 2), F), ebn_sat_mul(N, static_cast<int64_t>(K0) + K1));
}

extern "C" int ebn_naml_catview_fwd_f32(const int32_t* ids0, const float* table0, int64_t rows0, int32_t K0, const float* Wb0,
                                        float* out0, const int32_t* ids1, const float* table1, int64_t rows1, int32_t K1,
                                        const float* Wb1, float* out1, int64_t N, int32_t F, int32_t* oob_flag,
                                        ebn_stream_t stream) {
  EBN_REQUIRE(ids0 && table0 && Wb0 && out0 && ids1 && table1 && Wb1 && out1, EBN_ERR_BAD_ARG);
  const int rc = catview_check(N, F, rows0, K0, rows1, K1);
  if (rc != EBN_OK) return rc;
  if (N == 0) return EBN_OK;
  CatArgs a{};
  a.v[0] = cat_view(ids0, table0, rows0, K0, Wb0);
  a.v[1] = cat_view(ids1, table1, rows1, K1, Wb1);
  a.v[0].out = out0;
  a.v[1].out = out1;
  a.N = N;
  a.F = F;
  a.oob_flag = oob_flag;
  EBN_LAUNCH(catview_fwd_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(N, CV_FWD_ROWS)), 2), dim3(CV_THREADS), 0,
             ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_naml_catview_bwd_f32(const int32_t* ids0, const float* table0, int64_t rows0, int32_t K0, const float* Wb0,
                                        const float* out0, const float* dout0, float* dWb0, float* dtable0, const int32_t* ids1,
                                        const float* table1, int64_t rows1, int32_t K1, const float* Wb1, const float* out1,
                                        const float* dout1, float* dWb1, float* dtable1, float* partials,
                                        int64_t partials_len, int64_t N, int32_t F, ebn_stream_t stream) {
  EBN_REQUIRE(ids0 && table0 && Wb0 && out0 && dout0 && dWb0 && dtable0 && ids1 && table1 && Wb1 && out1 && dout1 && dWb1 &&
                  dtable1 && partials,
              EBN_ERR_BAD_ARG);
  const int rc = catview_check(N, F, rows0, K0, rows1, K1);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(partials_len >= ebn_naml_catview_partials_len(N, K0, K1, F), EBN_ERR_BAD_ARG);
  CatArgs a{};
  a.v[0] = cat_view(ids0, table0, rows0, K0, Wb0);
  a.v[1] = cat_view(ids1, table1, rows1, K1, Wb1);
  a.v[0].out = const_cast<float*>(out0);
  a.v[1].out = const_cast<float*>(out1);
  a.v[0].dout = dout0;
  a.v[1].dout = dout1;
  a.v[0].dWb = dWb0;
  a.v[1].dWb = dWb1;
  a.v[0].dtable = dtable0;
  a.v[1].dtable = dtable1;
  a.N = N;
  a.F = F;
  a.n_slices = ebn_ceil_div(N, CV_BWD_ROWS);
  a.v[0].part = partials;
  a.v[0].de = a.v[0].part + a.n_slices * (static_cast<int64_t>(K0) + 1) * F;
  a.v[1].part = a.v[0].de + N * K0;
  a.v[1].de = a.v[1].part + a.n_slices * (static_cast<int64_t>(K1) + 1) * F;
  hipStream_t s = ebn_stream(stream);
  if (N > 0) {
    EBN_LAUNCH(catview_bwd_part_kernel, dim3(static_cast<uint32_t>(a.n_slices), 2), dim3(CV_THREADS), 0, s, a);
    EBN_CHECK_LAUNCH();
  }
  // N == 0 still writes the (zero) gradients: the finishing pass sums no slice and no article
  int64_t most = 0;
  for (int v = 0; v < 2; ++v) {
    const int64_t n_wb = (static_cast<int64_t>(a.v[v].K) + 1) * F, n_tab = a.v[v].n_rows * a.v[v].K;
    most = n_wb > most ? n_wb : most;
    most = n_tab > most ? n_tab : most;
  }
  EBN_REQUIRE(ebn_ceil_div(most, CV_THREADS) <= INT32_MAX, EBN_ERR_UNSUPPORTED);
  EBN_LAUNCH(catview_bwd_finish_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(most, CV_THREADS)), 2), dim3(CV_THREADS), 0, s,
             a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_naml_viewatt_fwd_f32(float* U, const float* b, const float* q, const float* Vw, float* w, float* news,
                                        int64_t N, int32_t n_views, int32_t F, int32_t A, ebn_stream_t stream) {
  EBN_REQUIRE(U && b && q && Vw && w && news, EBN_ERR_BAD_ARG);
  const int rc = viewatt_check(N, n_views, F);
  if (rc != EBN_OK) return rc;
  EBN_REQUIRE(A > 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(A <= NAML_MAX_F && ebn_sat_mul(ebn_sat_mul(N, n_views), A) < (int64_t(1) << 40), EBN_ERR_UNSUPPORTED);
  if (N == 0) return EBN_OK;
  EBN_LAUNCH(viewatt_fwd_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(N, VA_WAVES))), dim3(VA_WAVES * 64), 0,
             ebn_stream(stream), U, b, q, Vw, w, news, N, n_views, F, A);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_naml_viewatt_bwd_f32(const float* Vw, const float* w, const float* dnews, float* dVw, float* de, int64_t N,
                                        int32_t n_views, int32_t F, ebn_stream_t stream) {
  EBN_REQUIRE(Vw && w && dnews && dVw && de, EBN_ERR_BAD_ARG);
  const int rc = viewatt_check(N, n_views, F);
  if (rc != EBN_OK) return rc;
  if (N == 0) return EBN_OK;
  EBN_LAUNCH(viewatt_bwd_kernel, dim3(static_cast<uint32_t>(ebn_ceil_div(N, VA_WAVES))), dim3(VA_WAVES * 64), 0,
             ebn_stream(stream), Vw, w, dnews, dVw, de, N, n_views, F);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
