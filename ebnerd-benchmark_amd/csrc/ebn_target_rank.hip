// Full-catalogue rank of one target candidate per user: the GEMM of ebn_topk.hip with a counting epilogue in place of the selection
// (the accuracy side of examples/beyond_accuracy/make_beyond_accuracy.ipynb, cell "Your Model": where does the clicked article
// stand in the list the top-N is drawn from).
//
//   s(u, c) = users[u, :] . news_all[cand_rows[c], :]      (exact fp32: v_mfma_f32_32x32x2_f32, an fma chain over F in k order)
//   count[u] = #{admissible c}      rank[u] = 1 + #{admissible c != target : s(u, c) > t or (s(u, c) == t and c < target_pos[u])}
//
// with t = s(u, target_pos[u]): the target's index + 1 in the total order of ebn_topk_score_f32 (score descending, then position
// ascending).  The operand staging (registers -> XOR-swizzled float4 image, 16-deep slabs, two LDS buffers, one barrier per slab)
// and the MFMA step are topk_score_kernel's own -- walk_run and walk_mma of ebn_catalogue_walk.h, which both kernels call: an
// accumulator element is the same fma chain, so s(u, c) has the bits ebn_topk_score_f32 gives the pair.  A 256-thread workgroup
// owns 128 users and walks its range of 128-candidate tiles, the four waves stacked along the users.
//
// Target tile.  Before the walk the workgroup needs its users' t.  It runs the slab pipeline once over a tile whose candidate
// operand row i is the catalogue row of user i's target: the diagonal of the 128 x 128 product is t.  Wave w's diagonal lies in
// its MFMA tile j == w only, so it issues a quarter of the MFMAs; lane (kl, il) finds row il's element in register
// (il & 3) + 4 (il >> 3) when kl == (il >> 2) & 1.  Every split of the candidates repeats the target tile -- t is the same bits
// in all of them.  A target that is no position, outside its user's window, of a row outside the table, excluded or NaN leaves
// t = NaN and position -1 in LDS: no compare against it is ever true, and the user's rank is 0.
//
// Counting epilogue, per tile and wave: no queue and no list.  Per element the compares s > t, s == t, s == s and c < target (and
// the window compare of the WINDOWED form when the tile is not inside every window of the wave) give two lane masks, "admissible"
// and "ahead of the row's target"; the C column is lane & 31, so the low and the high 32 bits of a __ballot are the two user rows
// of the lane halves.  Their popcounts over the four MFMA tiles are wave-uniform and go into the rows' two LDS counters with one
// ds_add of four lanes per accumulator register (the GEMM leaves no registers for 64 counters; a row belongs to one wave, so the
// counters need no barrier).  Integer sums: the order is free, so the counts do not depend on the split, the run or the other
// users.  More than one split: each writes its two partial counts per user to the workspace and a second launch adds them -- no
// atomics on global memory.
//
// Exclusion: a per-tile [128 users x 128 candidates] bit matrix in LDS (2 KB), built by the whole workgroup ahead of the
// tile's slabs.  The tile's 128 catalogue rows are chained into a 256-bucket hash (row & 255: ds_wrxchg on the bucket head,
// the old head is the entry's successor); then two threads per user walk that user's X exclusion rows (X <= 32: staged once per
// workgroup in LDS, padded with -1; larger X: read through the cache), follow the bucket of each and set the bit of every
// column that holds the row -- duplicates included.  That is 128 X probes per tile instead of 128 x 128 x X compares, one
// more barrier per tile, and one ds_read_b128 per accumulator register in the epilogue.  X == 0 skips all of it.  The first
// version compared every element against the X rows directly; DESIGN.md has both measured costs.
//
// WINDOWED: the tile-span logic of topk_score_kernel<true>, from the same header -- the workgroup's union picks the tiles, the
// wave's union gates its MFMAs, the wave's intersection frees a tile of the per-element window compare.
#include "ebn_catalogue_walk.h"
#include "ebn_topk_list.h"

namespace {

constexpr int TR_MAX_F = 8192;
constexpr int TR_X_LDS = 32;       // exclusion lists up to this length are staged in LDS

struct RankArgs {
  const float* users;
  const float* news;
  const int32_t* cand_rows;
  const int32_t* target_pos;
  const int32_t* window;  // [U, 2] (lo, hi) candidate positions; the WINDOWED instantiation only
  const int32_t* exclude;
  int32_t* out_rank;
  int32_t* out_count;
  float* out_score;
  int32_t* flags;
  int32_t* part;   // [2, n_splits, U]: admissible, ahead (n_splits > 1)
  float* part_t;   // [U]: the target score, NaN = no rank
  int64_t U, M, n_rows;
  int32_t F, X, XP, mode, n_splits, tiles_per_split;
};

// dynamic LDS layout (floats) behind the operand images: candrow[128] | t[128] | target position[128] | lo[128] | hi[128] |
// admissible[128] | ahead[128] | bucket head[256] | successor[128] | excluded bits [128][4] | exclude [128][XP]
constexpr int TR_BUCKETS = 256;
static_assert(TR_BUCKETS == TK_THREADS && TK_TILES == 4, "one bucket head per thread; four words of excluded bits per row");
inline int64_t rank_lds_bytes(int xp_lds) { return static_cast<int64_t>(TK_IMAGE_FLOATS + 14 * TK_BM + TK_BM * xp_lds) * 4; }

__device__ __forceinline__ void rank_write(const RankArgs& a, int64_t u, int count, int ahead, float t) {
  const bool ranked = t == t;
  a.out_rank[u] = ranked ? 1 + ahead : 0;
  a.out_count[u] = count;
  a.out_score[u] = ranked ? topk_act(t, a.mode) : -INFINITY;
}

template <bool WINDOWED>
__global__ __launch_bounds__(TK_THREADS, 2) void target_rank_kernel(RankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = lane >> 5, il = lane & 31;
  const int F = a.F, X = a.X, XP = a.XP;
  const int64_t u0 = static_cast<int64_t>(blockIdx.x) * TK_BM;
  const int split = blockIdx.y;
  const WalkImages im = walk_images(smem);
  float *As = im.As, *Bs = im.Bs;
  // every exchange through these is across a barrier: plain pointers, LDS loads
  int* candrow = reinterpret_cast<int*>(im.own);
  float* tsc = im.own + TK_BM;
  int* tps = reinterpret_cast<int*>(im.own + 2 * TK_BM);
  int* win_lo = reinterpret_cast<int*>(im.own + 3 * TK_BM);
  int* win_hi = win_lo + TK_BM;
  int* lcnt = reinterpret_cast<int*>(im.own + 5 * TK_BM);       // admissible[128] | ahead[128]
  int* head = lcnt + 2 * TK_BM;                                 // of the buckets: a column of the tile, -1 = empty
  int* nxt = head + TR_BUCKETS;                                 // a column's successor in its bucket
  unsigned* exbits = reinterpret_cast<unsigned*>(nxt + TK_BN);  // bit (c & 31) of [row][c >> 5]: column c is excluded for the row
  int* exl = reinterpret_cast<int*>(exbits + 4 * TK_BM);
  const bool ex_lds = X > 0 && X <= TR_X_LDS;

  const WalkSlab sl = walk_slab(tid);
  const float* pa[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) pa[i] = a.users + walk_slab_user(u0, a.U, tid, i) * F + sl.kq4;
  bool saw_nan = false;
  unsigned long long nan_mask = 0ull;

  int64_t t_beg, t_end;
  walk_span(a.M, TK_BN, split, a.tiles_per_split, t_beg, t_end);

  // the users' clamped ranges (not WINDOWED: [0, M); a row past the last user: [0, 0)) and the target's row of the catalogue
  if (tid < TK_BM) {
    const int64_t u = u0 + tid;
    int lo = 0, hi = 0, tp = -1, trow = -1;
    if (u < a.U) {
      hi = static_cast<int>(a.M);  // M <= INT32_MAX
      if constexpr (WINDOWED) walk_clamp(a.window, u, a.M, lo, hi);
      trow = walk_target_row(a, u, lo, hi);
      if (trow >= 0) tp = a.target_pos[u];
    }
    win_lo[tid] = lo;
    win_hi[tid] = hi;
    tps[tid] = tp;
    candrow[tid] = trow;
    lcnt[tid] = 0;
    lcnt[TK_BM + tid] = 0;
  }
  if (ex_lds) {
    for (int i = tid; i < TK_BM * XP; i += TK_THREADS) {
      const int rl = i / XP, x = i - rl * XP;
      const int64_t u = u0 + rl;
      exl[i] = (u < a.U && x < X) ? a.exclude[u * X + x] : -1;
    }
  }
  __syncthreads();

  // WINDOWED: the workgroup's union picks the tiles
  WalkSpans sp;
  if constexpr (WINDOWED) {
    sp = walk_spans_table(win_lo, win_hi, u0, a.U, wave, lane);
    walk_span(sp, TK_BN, split, a.n_splits, t_beg, t_end);
  }

  // the candidate operand rows of the tile whose catalogue rows candrow[] holds (behind a barrier)
  const float* pb[2];
  auto point_b = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = candrow[walk_slab_row(tid, i)];
      pb[i] = a.news + static_cast<int64_t>(r > 0 ? r : 0) * F + sl.kq4;
    }
  };

  // ---- target tile: candidate operand row i = the target row of user i; wave w's diagonal is in its MFMA tile j == w
  {
    point_b();
    f32x16 acc_t;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_t[r] = 0.f;
    auto mma_diag = [&](int buf) {
      const float* as = As + buf * TK_TILE_FLOATS + (wave * 32 + il) * 16;
      const float* bs = Bs + buf * TK_TILE_FLOATS + (wave * 32 + il) * 16;
#pragma unroll
      for (int j8 = 0; j8 < TK_BK / 8; ++j8) {
        const int q = walk_quad(j8, kl, il);
        float av[4], bv[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) av[w] = as[q + w];
#pragma unroll
        for (int w = 0; w < 4; ++w) bv[w] = bs[q + w];
#pragma unroll
        for (int w = 0; w < 4; ++w) acc_t = __builtin_amdgcn_mfma_f32_32x32x2f32(av[w], bv[w], acc_t, 0, 0, 0);
      }
    };
    walk_run(As, Bs, sl, pa, pb, nullptr, F, true, mma_diag);
    // C/D map of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if ((r & 3) + 8 * (r >> 2) + 4 * kl == il) tsc[wave * 32 + il] = acc_t[r];
    __syncthreads();
    if (tid < TK_BM) {
      const float t = tsc[tid];
      if (tps[tid] >= 0 && t != t) {  // a NaN inside the user's window: no rank
        saw_nan = true;
        tps[tid] = -1;
      }
      if (tps[tid] < 0) tsc[tid] = __builtin_nanf("");
    }
    // the walk's first barrier publishes t and the positions; a workgroup without tiles reads them behind the barrier below
  }

  const int rbase = wave * 32 + 4 * kl;

  for (int64_t t = t_beg; t < t_end; ++t) {
    const int64_t n0 = t * TK_BN;
    __syncthreads();  // every wave is done with the previous tile's candrow
    walk_rows<WINDOWED>(a, sp, n0, TK_BN, tid, candrow);
    if (X > 0) {
      head[tid] = -1;  // TR_BUCKETS == TK_THREADS
      exbits[tid] = 0u;
      exbits[tid + TK_THREADS] = 0u;
    }
    __syncthreads();
    point_b();
    if (X > 0) {  // the tile's excluded bits; the slab pipeline's first barrier publishes them
      if (tid < TK_BN) {
        const int row = candrow[tid];
        if (row >= 0) nxt[tid] = atomicExch(&head[row & (TR_BUCKETS - 1)], tid);
      }
      __syncthreads();
      const int rl = tid >> 1;  // two threads per user, every other exclusion row each
      const int64_t u = u0 + rl;
      auto probe = [&](int ev) {
        if (ev < 0) return;  // the padding, and entries that match nothing
        for (int col = head[ev & (TR_BUCKETS - 1)]; col >= 0; col = nxt[col])
          if (candrow[col] == ev) atomicOr(&exbits[rl * 4 + (col >> 5)], 1u << (col & 31));
      };
      if (ex_lds) {
        for (int x = tid & 1; x < XP; x += 2) probe(exl[rl * XP + x]);
      } else if (u < a.U) {
        for (int x = tid & 1; x < X; x += 2) probe(a.exclude[u * X + x]);
      }
    }

    // WINDOWED: a wave none of whose users' windows meets the tile fills the operand images and takes the barriers, nothing else
    const bool wave_on = !WINDOWED || walk_meets(sp, n0, TK_BN);
    f32x16 acc[TK_TILES];
    walk_zero(acc);
    walk_run(As, Bs, sl, pa, pb, nullptr, F, wave_on, [&](int buf) { walk_mma<true>(As, Bs, buf, wave, kl, il, acc); });
    if (!wave_on) continue;

    // ---- counting.  Column = lane & 31 of MFMA tile j, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    // WINDOWED: the column must lie in the row's window as well -- unless the tile is inside every window of this wave's users
    const bool gated = WINDOWED && walk_gated(sp, n0, TK_BN);
    const int c0 = static_cast<int>(n0) + il;  // this lane's column of MFMA tile 0
    int crow[TK_TILES];
#pragma unroll
    for (int j = 0; j < TK_TILES; ++j) crow[j] = candrow[32 * j + il];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = rbase + (r & 3) + 8 * (r >> 2);
      const float tt = tsc[rl];
      const int tp = tps[rl];
      WalkGate g;
      if constexpr (WINDOWED) {
        if (gated) g = walk_gate(win_lo[rl], win_hi[rl]);
      }
      bool hit[TK_TILES];
      {
        uint4 xb = make_uint4(0u, 0u, 0u, 0u);
        if (X > 0) xb = *reinterpret_cast<const uint4*>(&exbits[rl * 4]);
        hit[0] = (xb.x >> il) & 1u;
        hit[1] = (xb.y >> il) & 1u;
        hit[2] = (xb.z >> il) & 1u;
        hit[3] = (xb.w >> il) & 1u;
      }
      int n_adm[2] = {0, 0}, n_ahd[2] = {0, 0};  // of the rows of lane half 0 and 1: wave-uniform
#pragma unroll
      for (int j = 0; j < TK_TILES; ++j) {
        const float s = acc[j][r];
        const bool inside = crow[j] >= 0 && (!WINDOWED || g.pass(c0 + 32 * j));
        nan_mask |= __ballot(inside && s != s);
        const bool adm = inside && s == s && !hit[j];
        const unsigned long long m_adm = __ballot(adm);
        const unsigned long long m_ahd = __ballot(adm && (s > tt || (s == tt && c0 + 32 * j < tp)));
        n_adm[0] += __popc(static_cast<unsigned>(m_adm));
        n_adm[1] += __popc(static_cast<unsigned>(m_adm >> 32));
        n_ahd[0] += __popc(static_cast<unsigned>(m_ahd));
        n_ahd[1] += __popc(static_cast<unsigned>(m_ahd >> 32));
      }
      if (lane < 4) {  // lane 0 / 1: admissible of the two rows, lane 2 / 3: ahead
        const int v = lane == 0 ? n_adm[0] : lane == 1 ? n_adm[1] : lane == 2 ? n_ahd[0] : n_ahd[1];
        atomicAdd(&lcnt[(lane >> 1) * TK_BM + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane & 1)], v);
      }
    }
  }

  if (saw_nan || nan_mask != 0ull) a.flags[1] = 1;
  __syncthreads();  // t and the counters, also for a workgroup that had no tile to walk
  if (tid < TK_BM) {
    const int64_t u = u0 + tid;
    if (u < a.U) {
      if (a.n_splits == 1) {
        rank_write(a, u, lcnt[tid], lcnt[TK_BM + tid], tsc[tid]);
      } else {
        a.part[static_cast<int64_t>(split) * a.U + u] = lcnt[tid];
        a.part[(static_cast<int64_t>(a.n_splits) + split) * a.U + u] = lcnt[TK_BM + tid];
        if (split == 0) a.part_t[u] = tsc[tid];
      }
    }
  }
}

// adds the n_splits partial counts of a user: integer sums, any order gives the same
__global__ __launch_bounds__(256) void target_rank_merge_kernel(RankArgs a) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (u >= a.U) return;
  int count = 0, ahead = 0;
  for (int s = 0; s < a.n_splits; ++s) {
    count += a.part[static_cast<int64_t>(s) * a.U + u];
    ahead += a.part[(static_cast<int64_t>(a.n_splits) + s) * a.U + u];
  }
  rank_write(a, u, count, ahead, a.part_t[u]);
}

// M == 0: nobody has a rank; a target position >= M = 0 is still reported
__global__ __launch_bounds__(256) void target_rank_empty_kernel(const int32_t* __restrict__ target_pos, int32_t* __restrict__ out_rank,
                                                                int32_t* __restrict__ out_count, float* __restrict__ out_score,
                                                                int32_t* __restrict__ flags, int64_t U) {
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; u < U; u += static_cast<int64_t>(gridDim.x) * 256) {
    if (target_pos[u] >= 0) flags[0] = 1;
    out_rank[u] = 0;
    out_count[u] = 0;
    out_score[u] = -INFINITY;
  }
}

}  // namespace

extern "C" int64_t ebn_target_rank_workspace_bytes(int64_t n_users, int32_t n_splits) {
  if (!ebn_dim_ok(n_users) || n_splits < 1) return 0;
  if (n_splits == 1 || n_users == 0) return 16;  // one split writes the outputs directly
  const int64_t s = n_splits > TK_MAX_SPLITS ? TK_MAX_SPLITS : n_splits;
  // [2, s, U] int32 partial counts, [U] float target scores
  return ebn_sat_add(ebn_sat_mul(ebn_sat_add(ebn_sat_mul(2 * s, n_users), n_users), 4), 16);
}

extern "C" int ebn_target_rank_f32(const float* users, const float* news_all, int64_t n_rows, const int32_t* cand_rows, int64_t M,
                                   const int32_t* target_pos, const int32_t* window, const int32_t* exclude, int32_t X, int32_t mode,
                                   int32_t n_splits, int32_t* out_rank, int32_t* out_count, float* out_score, int32_t* flags,
                                   void* workspace, int64_t workspace_bytes, int64_t U, int32_t F, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(U, M, n_rows) && F >= 0 && X >= 0 && n_splits >= 0 && workspace_bytes >= 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(mode == 0 || mode == 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(X <= TK_MAX_X && F >= 4 && F % 4 == 0 && F <= TR_MAX_F, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(cand_rows != nullptr || M == n_rows, EBN_ERR_BAD_ARG);
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(target_pos != nullptr && out_rank != nullptr && out_count != nullptr && out_score != nullptr && flags != nullptr,
              EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (M == 0) {
    const int64_t blocks = ebn_ceil_div(U, 256);
    EBN_LAUNCH(target_rank_empty_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, target_pos, out_rank,
               out_count, out_score, flags, U);
    EBN_CHECK_LAUNCH();
    return EBN_OK;
  }
  EBN_REQUIRE(users != nullptr && news_all != nullptr && n_rows >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_aligned16(users) && ebn_aligned16(news_all), EBN_ERR_ALIGN);
  if (exclude == nullptr) X = 0;
  const int splits = walk_resolve_splits(U, M, TK_BN, n_splits);
  const int64_t user_tiles = ebn_ceil_div(U, TK_BM);
  EBN_REQUIRE(user_tiles <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  RankArgs a;
  a.users = users;
  a.news = news_all;
  a.cand_rows = cand_rows;
  a.target_pos = target_pos;
  a.window = window;
  a.exclude = exclude;
  a.out_rank = out_rank;
  a.out_count = out_count;
  a.out_score = out_score;
  a.flags = flags;
  a.part = nullptr;
  a.part_t = nullptr;
  a.U = U;
  a.M = M;
  a.n_rows = n_rows;
  a.F = F;
  a.X = X;
  a.XP = (X + 3) / 4 * 4;
  a.mode = mode;
  a.n_splits = splits;
  a.tiles_per_split = walk_units_per_split(M, TK_BN, splits);
  if (splits > 1) {
    const int64_t need = ebn_target_rank_workspace_bytes(U, splits);
    EBN_REQUIRE(workspace != nullptr && workspace_bytes >= need, EBN_ERR_BAD_ARG);
    EBN_REQUIRE(ebn_aligned16(workspace), EBN_ERR_ALIGN);
    a.part = static_cast<int32_t*>(workspace);
    a.part_t = reinterpret_cast<float*>(a.part + 2 * static_cast<int64_t>(splits) * U);
  }
  const size_t lds = static_cast<size_t>(rank_lds_bytes(X <= TR_X_LDS ? a.XP : 0));
  const dim3 grid(static_cast<unsigned>(user_tiles), static_cast<unsigned>(splits));
  if (window != nullptr) {
    EBN_LAUNCH(target_rank_kernel<true>, grid, dim3(TK_THREADS), lds, s, a);
  } else {
    EBN_LAUNCH(target_rank_kernel<false>, grid, dim3(TK_THREADS), lds, s, a);
  }
  EBN_CHECK_LAUNCH();
  if (splits > 1) {
    EBN_LAUNCH(target_rank_merge_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(U, 256))), dim3(256), 0, s, a);
    EBN_CHECK_LAUNCH();
  }
  return EBN_OK;
}
