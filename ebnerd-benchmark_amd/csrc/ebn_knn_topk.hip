// History-kNN top-N lists and clicked-article ranks over the WHOLE catalogue (contract in include/ebnerd_hip.h): the second outlet of
// the history-kNN baseline, beside the in-view scores of ebn_knn.hip.
//
//   score(u, c) = item_scale[c] * sum of the sims of u's neighbours whose set holds c
//
// ebn_knn_scores_f32 binary-searches every (candidate, neighbour) pair: right for 10 in-view items, hopeless for a 125 000-row
// catalogue per user.  Here the walk goes the other way, over the neighbours' SETS: a user touches at most k_nbr * |set| rows.  A
// 256-thread workgroup per (user, split) stages the neighbour row once and walks ranges of KNT_R catalogue rows, every wave on its
// own quarter of the range (ebn_knn_tile.h: the chain of a score, its order and its rounding are there, once).  Then the wave scans
// the TOUCHED BITS of its tile -- a few dozen rows of thousands -- and
//   * ebn_knn_topk_f32 keeps its own sorted list of k <= 64 entries in registers (ebn_topk_list.h), the four lists are merged by
//     wave 0 through 1.5 KiB of LDS at the end, and the lists of the splits by topk_merge_kernel;
//   * ebn_knn_target_rank_f32 first follows the target's own chain -- one thread per neighbour slot looks the target's row up in
//     that neighbour's set, thread 0 folds the hits in list order with knt_step and closes with knt_close: the tile's bits -- and
//     then counts in the same walk.
// No floating-point atomics anywhere; the integer ones (LDS bit masks) do not depend on order.  Bit-identical for every n_splits,
// from run to run and whoever shares the launch.
#include "ebn_knn_tile.h"
#include "ebn_topk_list.h"

namespace {

constexpr int KNK_MERGE_FLOATS = 2 * 3 * 64;          // the lists of waves 1 .. 3: score[3][64] | position[3][64]
constexpr int KNR_OWN_FLOATS = KNT_NBR + 16;          // found[512] | misc
static_assert(TK_MAX_SPLITS == KNT_MAX_SPLITS, "the merge launch holds one split per lane");

struct KnnTopkArgs : KnnTileArgs {
  int32_t* out_pos;
  float* out_score;
  int32_t* part_pos;  // [n_splits, U, k] (n_splits > 1)
  float* part_score;
  int32_t k;
};

struct KnnRankArgs : KnnTileArgs {
  const int32_t* target_pos;
  int32_t* out_rank;
  int32_t* out_count;
  float* out_score;
  int32_t* part;  // [2, n_splits, U]: admissible, ahead (n_splits > 1)
  float* part_t;  // [U]: the target score, NaN = no rank
  const int32_t* row_of_pos;  // [M]: the inverse of cand_pos (cand_pos != NULL), written by knn_row_of_pos_kernel
};

inline size_t knn_topk_lds_bytes() { return static_cast<size_t>(KNT_TILE_FLOATS + KNK_MERGE_FLOATS) * 4; }
inline size_t knn_rank_lds_bytes() { return static_cast<size_t>(KNT_TILE_FLOATS + KNR_OWN_FLOATS) * 4; }
static_assert((KNT_TILE_FLOATS + KNT_NBR + 16) * 4 <= 64 * 1024, "no kernel asks for more LDS than a launch may use as it is");

__global__ __launch_bounds__(KNT_THREADS, 2) void knn_topk_kernel(KnnTopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const KnnTile t = knt_tile(smem, wave);
  float* ms = t.own;
  int* mp = reinterpret_cast<int*>(t.own + 3 * 64);
  const int64_t u = blockIdx.x;
  const int split = blockIdx.y, k = a.k;

  const bool any = knt_stage(a, t, knt_history(a, u), tid);
  int wlo, whi;
  knt_window(a, u, wlo, whi);
  int64_t g_beg, g_end;
  knt_span(a, split, g_beg, g_end);

  float es = -INFINITY;  // slot `lane` of this wave's list
  int ep = TK_EMPTY;
  bool oob = false, nan = false;
  if (any) {  // a user without neighbours touches nothing
    for (int64_t g = g_beg; g < g_end; ++g) {
      int32_t r0, r1;
      if (!knt_fill_range(a, t, smem, u, g, tid, r0, r1)) continue;
      for (int wb = 0; wb < KNT_WWORDS; wb += 64) {
        const int wi = wb + lane;
        unsigned rest = wi < KNT_WWORDS ? t.touched[wi] : 0u;
        while (__ballot(rest != 0u) != 0ull) {  // every lane takes the next touched row of its word
          int pos = 0;
          float s = 0.f;
          bool ok = false;
          if (rest != 0u) {
            const int b = __builtin_ctz(rest);
            rest &= rest - 1u;
            ok = knt_admissible(a, t, r0, wi * 32 + b, wlo, whi, pos, s, oob, nan);
          }
          if (__ballot(ok) != 0ull) topk_wave_offer(es, ep, k, lane, ok, s, pos);
        }
      }
    }
  }
  if (oob) a.flags[0] = 1;
  if (nan) a.flags[1] = 1;

  // the lists of waves 1 .. 3 into wave 0's
  if (wave > 0 && lane < k) {
    ms[(wave - 1) * 64 + lane] = es;
    mp[(wave - 1) * 64 + lane] = ep;
  }
  __syncthreads();
  if (wave != 0) return;
  for (int w = 0; w < 3; ++w) {
    const float s = lane < k ? ms[w * 64 + lane] : 0.f;
    const int pos = lane < k ? mp[w * 64 + lane] : TK_EMPTY;
    topk_wave_offer(es, ep, k, lane, pos != TK_EMPTY, s, pos);
  }
  if (lane < k) {
    if (a.n_splits == 1) {
      const bool empty = ep == TK_EMPTY;
      a.out_pos[u * k + lane] = empty ? -1 : ep;
      a.out_score[u * k + lane] = empty ? -INFINITY : es;
    } else {
      const int64_t o = (static_cast<int64_t>(split) * a.U + u) * k + lane;
      a.part_pos[o] = ep;
      a.part_score[o] = es;
    }
  }
}

__device__ __forceinline__ void knr_write(const KnnRankArgs& a, int64_t u, int count, int ahead, float t) {
  const bool ranked = t == t;
  a.out_rank[u] = ranked ? 1 + ahead : 0;
  a.out_count[u] = count;
  a.out_score[u] = ranked ? t : -INFINITY;
}

__global__ __launch_bounds__(KNT_THREADS, 2) void knn_rank_kernel(KnnRankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const KnnTile t = knt_tile(smem, wave);
  int* s_f = reinterpret_cast<int*>(t.own);  // [KNT_NBR]: neighbour j's set holds the target's row
  int* s_misc = s_f + KNT_NBR;               // [1] the target's row is excluded, [2] its position or -1, [4 .. 11] the waves' counts
  float* s_t = reinterpret_cast<float*>(s_misc + 3);
  const int64_t u = blockIdx.x;
  const int split = blockIdx.y;

  if (tid == 0) s_misc[1] = 0;
  const bool any_nbr = knt_stage(a, t, knt_history(a, u), tid);  // ends with a barrier
  int wlo, whi;
  knt_window(a, u, wlo, whi);
  int64_t g_beg, g_end;
  knt_span(a, split, g_beg, g_end);
  bool oob = false, nan = false;

  // ---- the target: its row, then its chain in list order
  int tp = a.target_pos[u];
  if (static_cast<int64_t>(tp) >= a.M) {
    oob = true;
    tp = -1;
  }
  if (tp < wlo || tp >= whi) tp = -1;  // also tp < 0
  if (!any_nbr) tp = -1;               // nothing is touched
  int trow = tp;  // without cand_pos the position is the row
  if (tp >= 0 && a.cand_pos != nullptr) {  // through the inverse map; a slot no row wrote holds anything: checked against cand_pos
    const int r = a.row_of_pos[tp];
    trow = (r >= 0 && r < a.n_rows && a.cand_pos[r] == tp) ? r : -1;
  }
  if (trow >= 0) {
    for (int x = tid; x < a.X; x += KNT_THREADS)
      if (a.exclude[u * a.X + x] == trow) s_misc[1] = 1;
  }
  __syncthreads();
  const bool chase = trow >= 0 && s_misc[1] == 0;
  if (chase) {
    for (int j = tid; j < a.k_nbr; j += KNT_THREADS) {
      const int32_t lo = t.nb_lo[j], hi = t.nb_hi[j];
      const int32_t at = knt_lower_bound(a.s_items, lo, hi, trow);
      s_f[j] = (at < hi && a.s_items[at] == trow) ? 1 : 0;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float acc = 0.f;
    bool any = false;
    if (chase) {
      for (int j = 0; j < a.k_nbr; ++j) {
        if (s_f[j] == 0) continue;
        acc = any ? knt_step(acc, t.nb_sim[j]) : t.nb_sim[j];
        any = true;
      }
    }
    float tt = __builtin_nanf("");
    if (any) {
      const float v = knt_close(a, acc, trow);
      if (v != v) nan = true;  // admissible but for the NaN
      else tt = v;
    }
    s_t[0] = tt;
    s_misc[2] = tt == tt ? tp : -1;
  }
  __syncthreads();
  const float tt = s_t[0];
  const int ttp = s_misc[2];

  // ---- the walk
  int n_adm = 0, n_ahd = 0;
  if (any_nbr) {
    for (int64_t g = g_beg; g < g_end; ++g) {
      int32_t r0, r1;
      if (!knt_fill_range(a, t, smem, u, g, tid, r0, r1)) continue;
      for (int wi = lane; wi < KNT_WWORDS; wi += 64) {
        unsigned rest = t.touched[wi];
        while (rest != 0u) {
          const int b = __builtin_ctz(rest);
          rest &= rest - 1u;
          int pos = 0;
          float s = 0.f;
          if (knt_admissible(a, t, r0, wi * 32 + b, wlo, whi, pos, s, oob, nan)) {
            ++n_adm;
            n_ahd += (s > tt || (s == tt && pos < ttp)) ? 1 : 0;
          }
        }
      }
    }
  }
  if (oob) a.flags[0] = 1;
  if (nan) a.flags[1] = 1;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_adm += __shfl_xor(n_adm, off, 64);
    n_ahd += __shfl_xor(n_ahd, off, 64);
  }
  if (lane == 0) {
    s_misc[4 + wave] = n_adm;
    s_misc[8 + wave] = n_ahd;
  }
  __syncthreads();
  if (tid == 0) {
    const int count = s_misc[4] + s_misc[5] + s_misc[6] + s_misc[7];
    const int ahead = s_misc[8] + s_misc[9] + s_misc[10] + s_misc[11];
    if (a.n_splits == 1) {
      knr_write(a, u, count, ahead, tt);
    } else {
      a.part[static_cast<int64_t>(split) * a.U + u] = count;
      a.part[(static_cast<int64_t>(a.n_splits) + split) * a.U + u] = ahead;
      if (split == 0) a.part_t[u] = tt;
    }
  }
}

// the inverse of cand_pos, once per call: row_of_pos[cand_pos[r]] = r for the positions inside [0, M).  The other slots are left as
// they are -- a reader checks cand_pos[row_of_pos[p]] == p -- so one launch does, without a fill ahead of it
__global__ __launch_bounds__(256) void knn_row_of_pos_kernel(const int32_t* __restrict__ cand_pos, int64_t n_rows, int64_t M,
                                                             int32_t* __restrict__ row_of_pos) {
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; r < n_rows; r += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t p = cand_pos[r];
    if (p >= 0 && p < M) row_of_pos[p] = static_cast<int32_t>(r);
  }
}

// adds the n_splits partial counts of a user: integer sums, any order gives the same
__global__ __launch_bounds__(256) void knn_rank_merge_kernel(KnnRankArgs a) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (u >= a.U) return;
  int count = 0, ahead = 0;
  for (int s = 0; s < a.n_splits; ++s) {
    count += a.part[static_cast<int64_t>(s) * a.U + u];
    ahead += a.part[(static_cast<int64_t>(a.n_splits) + s) * a.U + u];
  }
  knr_write(a, u, count, ahead, a.part_t[u]);
}

// an empty index or no candidate position: nobody has a rank; a target position >= M is still reported
__global__ __launch_bounds__(256) void knn_rank_empty_kernel(const int32_t* __restrict__ target_pos, int64_t M, int32_t* __restrict__ out_rank,
                                                             int32_t* __restrict__ out_count, float* __restrict__ out_score,
                                                             int32_t* __restrict__ flags, int64_t U) {
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; u < U; u += static_cast<int64_t>(gridDim.x) * 256) {
    if (static_cast<int64_t>(target_pos[u]) >= M) flags[0] = 1;
    out_rank[u] = 0;
    out_count[u] = 0;
    out_score[u] = -INFINITY;
  }
}

// what both entry points check first, in this order
int knn_topk_check(int64_t n_seqs, int64_t nnz_s, int64_t n_rows, int64_t n_hists, int32_t k_nbr, const int32_t* cand_pos, int64_t M, int32_t X,
                   int32_t k, int32_t n_splits, int64_t workspace_bytes, int64_t U) {
  EBN_REQUIRE(ebn_dim_ok(n_seqs, nnz_s, n_rows, n_hists) && ebn_dim_ok(M, U) && X >= 0 && n_splits >= 0 && workspace_bytes >= 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(k_nbr >= 1 && (cand_pos != nullptr || M == n_rows), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(k >= 1 && k <= TK_MAX_K && X <= TK_MAX_X && k_nbr <= EBN_KNN_MAX_K, EBN_ERR_UNSUPPORTED);
  return EBN_OK;
}

void knn_tile_args(KnnTileArgs& a, const int64_t* s_indptr, const int32_t* s_items, int64_t n_seqs, int64_t nnz_s, int64_t n_rows,
                   const float* item_scale, const int32_t* nbr_seq, const float* nbr_sim, int64_t n_hists, int32_t k_nbr,
                   const int32_t* user_hist, const int32_t* cand_pos, int64_t M, const int32_t* window, const int32_t* exclude, int32_t X,
                   int32_t* flags, int64_t U) {
  a.s_indptr = s_indptr;
  a.s_items = s_items;
  a.item_scale = item_scale;
  a.nbr_seq = nbr_seq;
  a.nbr_sim = nbr_sim;
  a.user_hist = user_hist;
  a.cand_pos = cand_pos;
  a.window = window;
  a.exclude = exclude;
  a.flags = flags;
  a.n_seqs = n_seqs;
  a.nnz_s = nnz_s;
  a.n_rows = n_rows;
  a.n_hists = n_hists;
  a.M = M;
  a.U = U;
  a.k_nbr = k_nbr;
  a.X = exclude != nullptr ? X : 0;
}

// the operands a launch reads
bool knn_operands_ok(const KnnTileArgs& a) {
  return a.s_indptr != nullptr && a.s_items != nullptr && (a.n_hists == 0 || (a.nbr_seq != nullptr && a.nbr_sim != nullptr));
}

}  // namespace

extern "C" int64_t ebn_knn_topk_range(void) { return KNT_R; }

extern "C" int ebn_knn_topk_auto_splits(int64_t n_users, int64_t n_rows) {
  if (!ebn_dim_ok(n_users, n_rows) || n_users == 0 || n_rows == 0) return 1;
  return knt_resolve_splits(n_users, n_rows, 0);
}

extern "C" int64_t ebn_knn_topk_workspace_bytes(int64_t n_users, int32_t k, int32_t n_splits) {
  return ebn_topk_workspace_bytes(n_users, k, n_splits);  // the partial lists are ebn_topk_score_f32's
}

extern "C" int64_t ebn_knn_target_rank_workspace_bytes(int64_t n_users, int32_t n_splits, int64_t n_positions) {
  if (!ebn_dim_ok(n_users, n_positions) || n_splits < 1) return 0;
  if (n_users == 0) return 16;
  // [M] int32: the inverse of cand_pos (n_positions = M with a cand_pos, else 0); then, for more than one split (one writes the
  // outputs directly), [2, s, U] int32 partial counts and [U] float target scores
  const int64_t s = n_splits > KNT_MAX_SPLITS ? KNT_MAX_SPLITS : n_splits;
  const int64_t parts = n_splits == 1 ? 0 : ebn_sat_add(ebn_sat_mul(2 * s, n_users), n_users);
  return ebn_sat_add(ebn_sat_mul(ebn_sat_add(parts, n_positions), 4), 16);
}

extern "C" int ebn_knn_topk_f32(const int64_t* s_indptr, const int32_t* s_items, int64_t n_seqs, int64_t nnz_s, int64_t n_rows,
                                const float* item_scale, const int32_t* nbr_seq, const float* nbr_sim, int64_t n_hists, int32_t k_nbr,
                                const int32_t* user_hist, const int32_t* cand_pos, int64_t M, const int32_t* window, const int32_t* exclude,
                                int32_t X, int32_t k, int32_t n_splits, int32_t* out_pos, float* out_score, int32_t* flags, void* workspace,
                                int64_t workspace_bytes, int64_t U, ebn_stream_t stream) {
  const int rc0 = knn_topk_check(n_seqs, nnz_s, n_rows, n_hists, k_nbr, cand_pos, M, X, k, n_splits, workspace_bytes, U);
  if (rc0 != EBN_OK) return rc0;
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(out_pos != nullptr && out_score != nullptr && flags != nullptr, EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (n_rows == 0 || n_seqs == 0 || nnz_s == 0 || M == 0) return topk_launch_fill_empty(out_pos, out_score, U, k, s);
  KnnTopkArgs a;
  knn_tile_args(a, s_indptr, s_items, n_seqs, nnz_s, n_rows, item_scale, nbr_seq, nbr_sim, n_hists, k_nbr, user_hist, cand_pos, M, window,
                exclude, X, flags, U);
  a.k = k;
  a.out_pos = out_pos;
  a.out_score = out_score;
  EBN_REQUIRE(knn_operands_ok(a), EBN_ERR_BAD_ARG);
  const int splits = knt_resolve_splits(U, n_rows, n_splits);
  a.n_splits = splits;
  a.ranges_per_split = static_cast<int32_t>(ebn_ceil_div(ebn_ceil_div(n_rows, KNT_R), splits));
  TopkList l;
  l.exclude = nullptr;
  l.out_pos = out_pos;
  l.out_score = out_score;
  l.flags = flags;
  l.U = U;
  l.X = 0;
  l.k = k;
  l.mode = 0;  // the kept values are written as they are
  l.n_splits = splits;
  const int rc = topk_bind_workspace(l, splits, workspace, workspace_bytes);
  if (rc != EBN_OK) return rc;
  a.part_pos = l.part_pos;
  a.part_score = l.part_score;
  const dim3 grid(static_cast<unsigned>(U), static_cast<unsigned>(splits)), block(KNT_THREADS);
  EBN_LAUNCH(knn_topk_kernel, grid, block, knn_topk_lds_bytes(), s, a);
  EBN_CHECK_LAUNCH();
  if (splits > 1) return topk_launch_merge(l, s);
  return EBN_OK;
}

extern "C" int ebn_knn_target_rank_f32(const int64_t* s_indptr, const int32_t* s_items, int64_t n_seqs, int64_t nnz_s, int64_t n_rows,
                                       const float* item_scale, const int32_t* nbr_seq, const float* nbr_sim, int64_t n_hists,
                                       int32_t k_nbr, const int32_t* user_hist, const int32_t* cand_pos, int64_t M,
                                       const int32_t* target_pos, const int32_t* window, const int32_t* exclude, int32_t X,
                                       int32_t n_splits, int32_t* out_rank, int32_t* out_count, float* out_score, int32_t* flags,
                                       void* workspace, int64_t workspace_bytes, int64_t U, ebn_stream_t stream) {
  const int rc0 = knn_topk_check(n_seqs, nnz_s, n_rows, n_hists, k_nbr, cand_pos, M, X, 1, n_splits, workspace_bytes, U);
  if (rc0 != EBN_OK) return rc0;
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(target_pos != nullptr && out_rank != nullptr && out_count != nullptr && out_score != nullptr && flags != nullptr,
              EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (n_rows == 0 || n_seqs == 0 || nnz_s == 0 || M == 0) {
    const int64_t blocks = ebn_ceil_div(U, 256);
    EBN_LAUNCH(knn_rank_empty_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, target_pos, M, out_rank,
               out_count, out_score, flags, U);
    EBN_CHECK_LAUNCH();
    return EBN_OK;
  }
  KnnRankArgs a;
  knn_tile_args(a, s_indptr, s_items, n_seqs, nnz_s, n_rows, item_scale, nbr_seq, nbr_sim, n_hists, k_nbr, user_hist, cand_pos, M, window,
                exclude, X, flags, U);
  a.target_pos = target_pos;
  a.out_rank = out_rank;
  a.out_count = out_count;
  a.out_score = out_score;
  a.part = nullptr;
  a.part_t = nullptr;
  EBN_REQUIRE(knn_operands_ok(a), EBN_ERR_BAD_ARG);
  const int splits = knt_resolve_splits(U, n_rows, n_splits);
  a.n_splits = splits;
  a.ranges_per_split = static_cast<int32_t>(ebn_ceil_div(ebn_ceil_div(n_rows, KNT_R), splits));
  a.row_of_pos = nullptr;
  if (splits > 1 || cand_pos != nullptr) {
    const int64_t need = ebn_knn_target_rank_workspace_bytes(U, splits, cand_pos != nullptr ? M : 0);
    EBN_REQUIRE(workspace != nullptr && workspace_bytes >= need, EBN_ERR_BAD_ARG);
    EBN_REQUIRE(ebn_aligned16(workspace), EBN_ERR_ALIGN);
    int32_t* w = static_cast<int32_t*>(workspace);
    if (cand_pos != nullptr) {
      a.row_of_pos = w;
      w += M;
    }
    if (splits > 1) {
      a.part = w;
      a.part_t = reinterpret_cast<float*>(w + 2 * static_cast<int64_t>(splits) * U);
    }
  }
  if (cand_pos != nullptr) {
    const int64_t blocks = ebn_ceil_div(n_rows, 256);
    EBN_LAUNCH(knn_row_of_pos_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, cand_pos, n_rows, M,
               static_cast<int32_t*>(workspace));
    EBN_CHECK_LAUNCH();
  }
  const dim3 grid(static_cast<unsigned>(U), static_cast<unsigned>(splits)), block(KNT_THREADS);
  EBN_LAUNCH(knn_rank_kernel, grid, block, knn_rank_lds_bytes(), s, a);
  EBN_CHECK_LAUNCH();
  if (splits > 1) {
    EBN_LAUNCH(knn_rank_merge_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(U, 256))), dim3(256), 0, s, a);
    EBN_CHECK_LAUNCH();
  }
  return EBN_OK;
}
