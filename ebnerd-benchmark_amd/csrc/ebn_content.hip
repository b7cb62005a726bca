// Content-similarity baselines over a table of unit rows T (contract in include/ebnerd_hip.h): the decay-weighted centroid of a user's
// click history against each candidate, and the candidate's nearest history article (item-kNN, k = 1).  Both are gathers of whole
// table rows; nothing but the scores (and one profile row per user) is written.
//   * COLUMNS: in every kernel lane t of a wave owns the 16-byte chunks (k * 64 + t) of a row, k < ceil(D / 256) <= CS_CHUNKS, so a
//     wave covers a row of up to EBN_CS_MAX_D floats with at most 4 loads per lane.  A chunk is ONE 16-byte load where the row starts
//     on 16 bytes (pointer and ld) and the chunk lies inside D, and up to four 4-byte loads otherwise: the ownership, and with it
//     the order of every sum, is the same in both forms, so the bits do not depend on ld or on the alignment.  Columns >= D are never
//     read; they enter the sums as +0.
//   * ROWS: a wave reads the row numbers (and weights) of its next 64 entries with one coalesced load, one entry per lane, and
//     walks the PRESENT ones (a ballot) by broadcast: an absent entry costs nothing and its row never becomes an address; the next
//     present row is loaded before the current one is consumed.
//   * profiles: one workgroup per history.  Its 4 waves take the history's entries round-robin (entry j goes to wave j mod 4) and
//     each keeps its partial sum in registers; the partials are added through LDS in wave order, then thread t owns columns t,
//     t + 256, ...: squared norm by a wave sum and a sum over the waves in wave order, one division per element.
//   * centroid scores: one wave per list, 4 lists per workgroup, no barrier.  The profile row sits in registers (at most 16 floats per
//     lane) and is read once per list; per candidate one row gather, a 64-lane butterfly sum, and the score parked in the lane
//     of the candidate's slot, so that 64 scores leave in one coalesced store.
//   * nearest: one workgroup per list.  CS_NT candidate rows are staged in LDS (zero rows for absent candidates, zero columns up to
//     the next multiple of 256, so the inner loop has no column predicate); every wave streams its share of the history rows from
//     global memory once per tile, holds 16 partial dots per lane and reduces them with a HALVING butterfly (8 + 4 + 2 + 1 + 1 + 1
//     shuffles instead of 16 x 6: after it lanes 4c .. 4c + 3 hold candidate c's dot), keeps a running max of w * dot per candidate,
//     and the four waves' maxima are combined through LDS.  Lists longer than a tile loop over tiles, histories over batches.
//   * no atomics, no workspace, fixed summation orders: two runs give the same bits.
#include "ebn_common.h"

#define CS_THREADS 256
#define CS_WAVES 4    // waves of a workgroup; a history's entries go round-robin over them
#define CS_CHUNKS 4   // 16-byte chunks per lane and row: 4 * 64 lanes * 4 floats = EBN_CS_MAX_D
#define CS_NT 16      // candidate rows of one LDS tile of the nearest kernel (16 x 1024 x 4 B = 64 KiB at EBN_CS_MAX_D)

static_assert(CS_CHUNKS * EBN_WAVE * 4 == EBN_CS_MAX_D, "a wave covers a row of EBN_CS_MAX_D floats");
static_assert(CS_THREADS == CS_WAVES * EBN_WAVE && CS_NT == 16, "cs_reduce16 folds exactly 16 partials");

// columns c .. c + 3 of a row; 0 for columns >= D, which are not read
template <bool VEC>
static __device__ __forceinline__ float4 cs_load4(const float* __restrict__ row, int c, int D) {
  if (VEC && c + 4 <= D) return *reinterpret_cast<const float4*>(row + c);
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (c < D) v.x = row[c];
  if (c + 1 < D) v.y = row[c + 1];
  if (c + 2 < D) v.z = row[c + 2];
  if (c + 3 < D) v.w = row[c + 3];
  return v;
}

template <bool VEC>
static __device__ __forceinline__ void cs_load_row(const float* __restrict__ row, int lane, int nk, int D, float4 (&v)[CS_CHUNKS]) {
#pragma unroll
  for (int k = 0; k < CS_CHUNKS; ++k)
    v[k] = k < nk ? cs_load4<VEC>(row, (k * EBN_WAVE + lane) * 4, D) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

static __device__ __forceinline__ float cs_dot4(float4 a, float4 b, float s) {
  s = fmaf(a.x, b.x, s);
  s = fmaf(a.y, b.y, s);
  s = fmaf(a.z, b.z, s);
  return fmaf(a.w, b.w, s);
}

static __device__ __forceinline__ int64_t cs_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Entries first, first + step, ... below `end` of rows[] / weights[]: consume(row chunks, weight) for every PRESENT one, in order.
// Wave-uniform control flow throughout (first, step, end are the same in every lane).
template <bool VEC, class F>
static __device__ __forceinline__ void cs_stream_rows(const float* __restrict__ table, int64_t n_rows, int D, int64_t ld, int nk,
                                                      const int32_t* __restrict__ rows, const float* __restrict__ weights,
                                                      int64_t first, int64_t step, int64_t end, int lane, F&& consume) {
  for (int64_t j0 = first; j0 < end; j0 += step * EBN_WAVE) {
    const int64_t j = j0 + step * lane;
    int32_t my_r = -1;
    float my_w = 1.0f;
    if (j < end) {
      my_r = rows[j];
      if (weights != nullptr) my_w = weights[j];
    }
    uint64_t present = __ballot(my_r >= 0 && my_r < n_rows);
    if (present == 0) continue;
    float4 cur[CS_CHUNKS], nxt[CS_CHUNKS];
    int t = __ffsll(static_cast<unsigned long long>(present)) - 1;
    present &= present - 1;
    float w_nxt = __shfl(my_w, t, EBN_WAVE);
    cs_load_row<VEC>(table + static_cast<int64_t>(__shfl(my_r, t, EBN_WAVE)) * ld, lane, nk, D, nxt);
    for (;;) {
      const float w_cur = w_nxt;
#pragma unroll
      for (int k = 0; k < CS_CHUNKS; ++k) cur[k] = nxt[k];
      const bool more = present != 0;
      if (more) {  // the next present row is on its way while this one is consumed
        t = __ffsll(static_cast<unsigned long long>(present)) - 1;
        present &= present - 1;
        w_nxt = __shfl(my_w, t, EBN_WAVE);
        cs_load_row<VEC>(table + static_cast<int64_t>(__shfl(my_r, t, EBN_WAVE)) * ld, lane, nk, D, nxt);
      }
      consume(cur, w_cur);
      if (!more) break;
    }
  }
}

// ---- profiles ------------------------------------------------------------------------------------------------------------------
template <bool VEC>
static __global__ __launch_bounds__(CS_THREADS) void cs_profiles_kernel(const float* __restrict__ table, int64_t n_rows, int D, int64_t ld,
                                                                        const int32_t* __restrict__ hist_rows,
                                                                        const float* __restrict__ hist_weights,
                                                                        const int64_t* __restrict__ hist_offsets, int64_t n_hist_items,
                                                                        float* __restrict__ profiles, int64_t ldp) {
  __shared__ float4 s_part[CS_WAVES][EBN_CS_MAX_D / 4];
  __shared__ float s_red[CS_WAVES];
  const int tid = threadIdx.x, lane = tid & (EBN_WAVE - 1), wave = tid / EBN_WAVE;
  const int nk = (D + 4 * EBN_WAVE - 1) / (4 * EBN_WAVE);
  const int64_t u = blockIdx.x;
  const int64_t hb = cs_clamp(hist_offsets[u], n_hist_items), he = cs_clamp(hist_offsets[u + 1], n_hist_items);
  float4 acc[CS_CHUNKS];
#pragma unroll
  for (int k = 0; k < CS_CHUNKS; ++k) acc[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  cs_stream_rows<VEC>(table, n_rows, D, ld, nk, hist_rows, hist_weights, hb + wave, CS_WAVES, he, lane,
                      [&](const float4 (&row)[CS_CHUNKS], float w) {
#pragma unroll
                        for (int k = 0; k < CS_CHUNKS; ++k) {
                          acc[k].x = fmaf(w, row[k].x, acc[k].x);
                          acc[k].y = fmaf(w, row[k].y, acc[k].y);
                          acc[k].z = fmaf(w, row[k].z, acc[k].z);
                          acc[k].w = fmaf(w, row[k].w, acc[k].w);
                        }
                      });
#pragma unroll
  for (int k = 0; k < CS_CHUNKS; ++k)
    if (k < nk) s_part[wave][k * EBN_WAVE + lane] = acc[k];
  __syncthreads();
  // thread tid owns columns tid, tid + 256, ...: the waves' partials in wave order
  float p[CS_CHUNKS], ss = 0.0f;
#pragma unroll
  for (int k = 0; k < CS_CHUNKS; ++k) {
    const int c = k * CS_THREADS + tid;
    p[k] = 0.0f;
    if (c < D) {
      const float* part = reinterpret_cast<const float*>(&s_part[0][0]);
      p[k] = ((part[c] + part[EBN_CS_MAX_D + c]) + part[2 * EBN_CS_MAX_D + c]) + part[3 * EBN_CS_MAX_D + c];
      ss = fmaf(p[k], p[k], ss);
    }
  }
  ss = ebn_wave_sum(ss);
  if (lane == 0) s_red[wave] = ss;
  __syncthreads();
  const float norm = sqrtf(((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]);
  float* __restrict__ out = profiles + u * ldp;
#pragma unroll
  for (int k = 0; k < CS_CHUNKS; ++k) {
    const int c = k * CS_THREADS + tid;
    if (c < D) out[c] = norm > 0.0f ? p[k] / norm : 0.0f;
  }
}

// ---- centroid scores -----------------------------------------------------------------------------------------------------------
template <bool VEC>
static __global__ __launch_bounds__(CS_THREADS) void cs_centroid_kernel(const float* __restrict__ table, int64_t n_rows, int D, int64_t ld,
                                                                        const float* __restrict__ profiles, int64_t n_hists, int64_t ldp,
                                                                        const int32_t* __restrict__ list_hist,
                                                                        const int32_t* __restrict__ cand_rows,
                                                                        const int64_t* __restrict__ cand_offsets, int64_t n_lists,
                                                                        int64_t n_cand_items, float* __restrict__ scores) {
  const int lane = threadIdx.x & (EBN_WAVE - 1), wave = threadIdx.x / EBN_WAVE;
  const int nk = (D + 4 * EBN_WAVE - 1) / (4 * EBN_WAVE);
  const int64_t l = static_cast<int64_t>(blockIdx.x) * CS_WAVES + wave;
  if (l >= n_lists) return;  // no barrier in this kernel
  const int64_t b = cs_clamp(cand_offsets[l], n_cand_items), e = cs_clamp(cand_offsets[l + 1], n_cand_items);
  if (b >= e) return;
  const int64_t u = list_hist != nullptr ? static_cast<int64_t>(list_hist[l]) : l;
  const bool has_profile = u >= 0 && u < n_hists;
  float4 p[CS_CHUNKS];
#pragma unroll
  for (int k = 0; k < CS_CHUNKS; ++k) p[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (has_profile) cs_load_row<VEC>(profiles + u * ldp, lane, nk, D, p);
  for (int64_t i0 = b; i0 < e; i0 += EBN_WAVE) {
    const int64_t i = i0 + lane;
    const int32_t my_r = i < e ? cand_rows[i] : -1;
    const bool my_ok = has_profile && my_r >= 0 && my_r < n_rows;
    float my_s = 0.0f;
    uint64_t present = __ballot(my_ok);
    if (present != 0) {
      float4 cur[CS_CHUNKS], nxt[CS_CHUNKS];
      int t_nxt = __ffsll(static_cast<unsigned long long>(present)) - 1;
      present &= present - 1;
      cs_load_row<VEC>(table + static_cast<int64_t>(__shfl(my_r, t_nxt, EBN_WAVE)) * ld, lane, nk, D, nxt);
      for (;;) {
        const int t = t_nxt;
#pragma unroll
        for (int k = 0; k < CS_CHUNKS; ++k) cur[k] = nxt[k];
        const bool more = present != 0;
        if (more) {
          t_nxt = __ffsll(static_cast<unsigned long long>(present)) - 1;
          present &= present - 1;
          cs_load_row<VEC>(table + static_cast<int64_t>(__shfl(my_r, t_nxt, EBN_WAVE)) * ld, lane, nk, D, nxt);
        }
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < CS_CHUNKS; ++k) s = cs_dot4(p[k], cur[k], s);
        s = ebn_wave_sum(s);
        if (lane == t) my_s = s;
        if (!more) break;
      }
    }
    if (i < e) scores[i] = my_ok ? my_s : 0.0f;
  }
}

// ---- nearest -------------------------------------------------------------------------------------------------------------------
// s[i] (+)= the partner's s[i + N] or s[i], so that the lanes with bit `off` clear keep the lower N partials and the others the upper N
template <int N>
static __device__ __forceinline__ void cs_fold(float (&s)[CS_NT], bool upper, int off) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float send = upper ? s[i] : s[i + N], keep = upper ? s[i + N] : s[i];
    s[i] = keep + __shfl_xor(send, off, EBN_WAVE);
  }
}

// 16 per-lane partials -> the 64-lane sum of partial (lane >> 2), in every lane, with 17 shuffles
static __device__ __forceinline__ float cs_reduce16(float (&s)[CS_NT], int lane) {
  cs_fold<8>(s, (lane & 32) != 0, 32);
  cs_fold<4>(s, (lane & 16) != 0, 16);
  cs_fold<2>(s, (lane & 8) != 0, 8);
  cs_fold<1>(s, (lane & 4) != 0, 4);
  s[0] += __shfl_xor(s[0], 2, EBN_WAVE);
  s[0] += __shfl_xor(s[0], 1, EBN_WAVE);
  return s[0];
}

template <bool VEC>
static __global__ __launch_bounds__(CS_THREADS) void cs_nearest_kernel(const float* __restrict__ table, int64_t n_rows, int D, int64_t ld,
                                                                       const int32_t* __restrict__ hist_rows,
                                                                       const float* __restrict__ hist_weights,
                                                                       const int64_t* __restrict__ hist_offsets, int64_t n_hists,
                                                                       int64_t n_hist_items, const int32_t* __restrict__ list_hist,
                                                                       const int32_t* __restrict__ cand_rows,
                                                                       const int64_t* __restrict__ cand_offsets, int64_t n_cand_items,
                                                                       float* __restrict__ scores) {
  extern __shared__ float4 s_tile[];  // [CS_NT][nk * 64] chunks; after a tile's history pass its first 64 floats hold the waves' maxima
  const int tid = threadIdx.x, lane = tid & (EBN_WAVE - 1), wave = tid / EBN_WAVE;
  const int nk = (D + 4 * EBN_WAVE - 1) / (4 * EBN_WAVE);
  const int pitch = nk * EBN_WAVE;  // chunks per staged row
  const int64_t l = blockIdx.x;
  const int64_t b = cs_clamp(cand_offsets[l], n_cand_items), e = cs_clamp(cand_offsets[l + 1], n_cand_items);
  if (b >= e) return;  // the whole workgroup
  const int64_t u = list_hist != nullptr ? static_cast<int64_t>(list_hist[l]) : l;
  int64_t hb = 0, he = 0;
  if (u >= 0 && u < n_hists) {
    hb = cs_clamp(hist_offsets[u], n_hist_items);
    he = cs_clamp(hist_offsets[u + 1], n_hist_items);
  }
  if (hb >= he) {  // no history: every score is 0 and no row is read
    for (int64_t i = b + tid; i < e; i += CS_THREADS) scores[i] = 0.0f;
    return;
  }
  for (int64_t i0 = b; i0 < e; i0 += CS_NT) {
    const int nc = e - i0 < CS_NT ? static_cast<int>(e - i0) : CS_NT;
    for (int c = wave; c < nc; c += CS_WAVES) {  // stage: one wave per candidate row
      const int32_t r = cand_rows[i0 + c];
      const bool ok = r >= 0 && r < n_rows;
      float4 v[CS_CHUNKS];
#pragma unroll
      for (int k = 0; k < CS_CHUNKS; ++k) v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (ok) cs_load_row<VEC>(table + static_cast<int64_t>(r) * ld, lane, nk, D, v);
#pragma unroll
      for (int k = 0; k < CS_CHUNKS; ++k)
        if (k < nk) s_tile[c * pitch + k * EBN_WAVE + lane] = v[k];
    }
    __syncthreads();
    float best = -INFINITY;  // of candidate (lane >> 2), over this wave's history rows
    cs_stream_rows<VEC>(table, n_rows, D, ld, nk, hist_rows, hist_weights, hb + wave, CS_WAVES, he, lane,
                        [&](const float4 (&row)[CS_CHUNKS], float w) {
                          float s[CS_NT];
#pragma unroll
                          for (int c = 0; c < CS_NT; ++c) s[c] = 0.0f;
#pragma unroll
                          for (int k = 0; k < CS_CHUNKS; ++k) {
                            if (k < nk) {
#pragma unroll
                              for (int c = 0; c < CS_NT; ++c)
                                if (c < nc) s[c] = cs_dot4(row[k], s_tile[c * pitch + k * EBN_WAVE + lane], s[c]);
                            }
                          }
                          best = fmaxf(best, w * cs_reduce16(s, lane));
                        });
    __syncthreads();  // every wave is done with the tile: its head now carries the maxima
    float* s_best = reinterpret_cast<float*>(s_tile);
    if ((lane & 3) == 0) s_best[wave * CS_NT + (lane >> 2)] = best;
    __syncthreads();
    if (tid < nc) {
      const float m = fmaxf(fmaxf(s_best[tid], s_best[CS_NT + tid]), fmaxf(s_best[2 * CS_NT + tid], s_best[3 * CS_NT + tid]));
      const int32_t r = cand_rows[i0 + tid];
      scores[i0 + tid] = (r >= 0 && r < n_rows && m > -INFINITY) ? m : 0.0f;  // -inf: the history has no present entry
    }
    __syncthreads();  // before the next tile overwrites the maxima
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
static inline bool cs_vec(const float* p, int64_t ld) { return ebn_aligned16(p) && (ld % 4) == 0; }

extern "C" int ebn_cs_profiles_f32(const float* table, int64_t n_rows, int64_t D, int64_t ld, const int32_t* hist_rows,
                                   const float* hist_weights, const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items,
                                   float* profiles, int64_t ldp, ebn_stream_t stream) {
  EBN_REQUIRE(D >= 1 && ld >= D && ldp >= D && ebn_dim_ok(n_rows, n_hists, n_hist_items) && ebn_dim_ok(D, ld, ldp), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_hist_items == 0 || n_hists >= 1, EBN_ERR_BAD_ARG);  // an entry belongs to a history
  EBN_REQUIRE(D <= EBN_CS_MAX_D, EBN_ERR_UNSUPPORTED);
  if (n_hists == 0) return EBN_OK;
  EBN_REQUIRE(hist_offsets != nullptr && profiles != nullptr && (n_hist_items == 0 || hist_rows != nullptr), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_rows == 0 || table != nullptr, EBN_ERR_BAD_ARG);
  const dim3 grid(static_cast<unsigned>(n_hists)), block(CS_THREADS);
  const int d = static_cast<int>(D);
  if (cs_vec(table, ld))
    EBN_LAUNCH(cs_profiles_kernel<true>, grid, block, 0, ebn_stream(stream), table, n_rows, d, ld, hist_rows, hist_weights, hist_offsets,
               n_hist_items, profiles, ldp);
  else
    EBN_LAUNCH(cs_profiles_kernel<false>, grid, block, 0, ebn_stream(stream), table, n_rows, d, ld, hist_rows, hist_weights, hist_offsets,
               n_hist_items, profiles, ldp);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_cs_centroid_scores_f32(const float* table, int64_t n_rows, int64_t D, int64_t ld, const float* profiles, int64_t n_hists,
                                          int64_t ldp, const int32_t* list_hist, const int32_t* cand_rows, const int64_t* cand_offsets,
                                          int64_t n_lists, int64_t n_cand_items, float* scores, ebn_stream_t stream) {
  EBN_REQUIRE(D >= 1 && ld >= D && ldp >= D && ebn_dim_ok(n_rows, n_hists, n_lists, n_cand_items) && ebn_dim_ok(D, ld, ldp),
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE(n_cand_items == 0 || n_lists >= 1, EBN_ERR_BAD_ARG);  // an item belongs to a list
  EBN_REQUIRE(D <= EBN_CS_MAX_D, EBN_ERR_UNSUPPORTED);
  if (n_cand_items == 0) return EBN_OK;
  EBN_REQUIRE(cand_rows != nullptr && cand_offsets != nullptr && scores != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE((n_rows == 0 || table != nullptr) && (n_hists == 0 || profiles != nullptr), EBN_ERR_BAD_ARG);
  const dim3 grid(static_cast<unsigned>(ebn_ceil_div(n_lists, CS_WAVES))), block(CS_THREADS);
  const int d = static_cast<int>(D);
  if (cs_vec(table, ld) && cs_vec(profiles, ldp))
    EBN_LAUNCH(cs_centroid_kernel<true>, grid, block, 0, ebn_stream(stream), table, n_rows, d, ld, profiles, n_hists, ldp, list_hist,
               cand_rows, cand_offsets, n_lists, n_cand_items, scores);
  else
    EBN_LAUNCH(cs_centroid_kernel<false>, grid, block, 0, ebn_stream(stream), table, n_rows, d, ld, profiles, n_hists, ldp, list_hist,
               cand_rows, cand_offsets, n_lists, n_cand_items, scores);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_cs_nearest_scores_f32(const float* table, int64_t n_rows, int64_t D, int64_t ld, const int32_t* hist_rows,
                                         const float* hist_weights, const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items,
                                         const int32_t* list_hist, const int32_t* cand_rows, const int64_t* cand_offsets, int64_t n_lists,
                                         int64_t n_cand_items, float* scores, ebn_stream_t stream) {
  EBN_REQUIRE(D >= 1 && ld >= D && ebn_dim_ok(n_rows, n_hists, n_hist_items) && ebn_dim_ok(n_lists, n_cand_items, D, ld), EBN_ERR_BAD_ARG);
  EBN_REQUIRE((n_cand_items == 0 || n_lists >= 1) && (n_hist_items == 0 || n_hists >= 1), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(D <= EBN_CS_MAX_D, EBN_ERR_UNSUPPORTED);
  if (n_cand_items == 0) return EBN_OK;
  EBN_REQUIRE(cand_rows != nullptr && cand_offsets != nullptr && scores != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE((n_rows == 0 || table != nullptr) && (n_hists == 0 || hist_offsets != nullptr) && (n_hist_items == 0 || hist_rows != nullptr),
              EBN_ERR_BAD_ARG);
  const dim3 grid(static_cast<unsigned>(n_lists)), block(CS_THREADS);
  const int d = static_cast<int>(D);
  const size_t lds = static_cast<size_t>(CS_NT) * static_cast<size_t>(ebn_ceil_div(D, 4 * EBN_WAVE)) * EBN_WAVE * sizeof(float4);  // <= 64 KiB
  if (cs_vec(table, ld))
    EBN_LAUNCH(cs_nearest_kernel<true>, grid, block, lds, ebn_stream(stream), table, n_rows, d, ld, hist_rows, hist_weights, hist_offsets,
               n_hists, n_hist_items, list_hist, cand_rows, cand_offsets, n_cand_items, scores);
  else
    EBN_LAUNCH(cs_nearest_kernel<false>, grid, block, lds, ebn_stream(stream), table, n_rows, d, ld, hist_rows, hist_weights, hist_offsets,
               n_hists, n_hist_items, list_hist, cand_rows, cand_offsets, n_cand_items, scores);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
