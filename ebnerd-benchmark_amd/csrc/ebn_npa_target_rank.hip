// Full-catalogue rank of one target candidate per user for NPA: the two GEMMs and the softmax pooling of ebn_npa_topk.hip with a
// counting epilogue in place of the selection (what ebn_target_rank.hip is to ebn_topk.hip).  Per (user u, candidate row) pair
//
//   s_l = Q[u] . Ua_all[row, l]     w = softmax_l(s)     d_l = users[u] . Vd_all[row, l]     s(u, c) = (sum_l e_l d_l) / (sum_l e_l)
//   count[u] = #{admissible c}      rank[u] = 1 + #{admissible c : s(u, c) > t or (s(u, c) == t and c < target_pos[u])}
//
// with t = s(u, target_pos[u]): the target's index + 1 in the total order of ebn_npa_topk_score_f32 (score descending, then position
// ascending).  The step body -- operand staging, both GEMM phases, the in-lane reductions over the 16 registers, the cross-half adds
// and the division -- is npa_topk_kernel's: both call npa_pooled of ebn_catalogue_walk.h, so s(u, c) has the bits that kernel gives
// the pair.
//
// Counting epilogue.  In the 32x32 C layout a lane holds ONE user's column for the whole walk (user = lane & 31 of the wave's 32), so
// the user's t, target position and window sit in registers and the two counters -- admissible, ahead of the target -- are two
// VGPRs per lane: lane half kl counts candidates kl and kl + 2 of each step, the halves are added once at the end.  No queue, no
// list, no ballot, no LDS counters.  Per element: s > t, s == t && c < target, s == s, the window compare and the exclusion.
//
// Exclusion.  Every candidate is tested, not only survivors: a lane compares the catalogue rows of its two candidates of the step
// (wave-uniform in candrow[]) against its user's X rows -- 2 X integer compares per lane and step next to (A + F) / 2 * 4 MFMAs.
// Lists of X <= 32 are staged once per workgroup in LDS (int4 per four entries, users along the lanes: no bank conflict), padded
// with -1; longer ones are read through the cache.
//
// Target pass.  Every range needs t before its walk, with the pair's exact bits.  A first launch (one workgroup per 128 users) runs
// the same step body over steps whose candidates are the targets of 4 (2) of the workgroup's users; only the owner's column keeps
// its value, so only the wave that owns the step's users issues MFMAs (the others stage and take the barriers).  It writes t [U] to
// the workspace, NaN for "no rank": a target that is no position, outside its user's window, of a row outside the table, excluded
// or NaN.  No compare against a NaN t is ever true, so such a user's rank is 0.  The pass costs 128 / M of the walk's steps.
//
// WINDOWED: the union of the workgroup's windows picks the steps it walks (n_splits ranges divide those), the union of a wave's
// windows gates its MFMAs, a step inside every window of the wave skips the per-element window compare.
//
// Each range writes its two partial counts per user to the workspace and a last small launch adds them (integer sums: any order
// gives the same) and writes the three outputs -- no atomics on global memory.
#include "ebn_catalogue_walk.h"
#include "ebn_topk_list.h"

namespace {

constexpr int NR_MAX_L = 64, NR_MAX_A = 1024, NR_MAX_F = 4096;
constexpr int NR_X_LDS = 32;              // exclusion lists up to this length are staged in LDS

struct NpaRankArgs {
  const float* users;  // [U, F]
  const float* Q;      // [U, A]
  const float* Ua;     // [n_rows, L, A]
  const float* Vd;     // [n_rows, L, F]
  const int32_t* cand_rows;
  const int32_t* target_pos;
  const int32_t* window;  // [U, 2] or NULL
  const int32_t* exclude;
  int32_t* out_rank;
  int32_t* out_count;
  float* out_score;
  int32_t* flags;
  float* t;       // [U]: the target score, NaN = no rank
  int32_t* part;  // [2, n_splits, U]: admissible, ahead
  int64_t U, M, n_rows;
  int32_t L, F, A, X, XP, mode, n_splits, steps_per_split;
};

// dynamic LDS layout (floats) behind the operand images: candrow[128] | target row[128] | wave unions[16] | exclude [XP / 4][128] int4
inline int64_t npa_rank_lds_bytes(int xp_lds) { return static_cast<int64_t>(TK_IMAGE_FLOATS + 2 * TK_BM + 16 + TK_BM * xp_lds) * 4; }

// LT: row tiles of one candidate (1: L <= 32, 2: L <= 64).  TPASS: the target pass (then WINDOWED is false: the window is looked
// at once per user, at run time)
template <int LT, bool WINDOWED, bool TPASS>
__global__ __launch_bounds__(TK_THREADS, 2) void npa_rank_kernel(NpaRankArgs a) {
  constexpr int CPS = TK_TILES / LT;  // candidates of a step
  static_assert(!(WINDOWED && TPASS), "the target pass has no windowed form");
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = lane >> 5, il = lane & 31;
  const int X = a.X;
  const int64_t u0 = static_cast<int64_t>(blockIdx.x) * TK_BM;
  const int split = blockIdx.y;
  const WalkImages im = walk_images(smem);
  float *Ts = im.As, *Us = im.Bs;  // token rows | users
  // every exchange through these is across a barrier: plain pointers, LDS loads
  int* candrow = reinterpret_cast<int*>(im.own);
  int* trow = candrow + TK_BM;  // TPASS: the catalogue row of user i's target, -1 = no rank
  int* wun = trow + TK_BM;      // WINDOWED: (lo, hi) of the four waves' unions
  const int4* exl = reinterpret_cast<const int4*>(wun + 16);
  const bool ex_lds = X > 0 && X <= NR_X_LDS;

  const NpaThread th = npa_thread<LT>(a, u0, tid);
  bool saw_nan = false;

  // ---- this lane's user: column il of the wave's tile
  const int rl = wave * 32 + il;
  const int64_t ul = u0 + rl;
  const bool live = ul < a.U;
  const int64_t uc = live ? ul : a.U - 1;
  int lo = 0, hi = static_cast<int>(a.M);  // M <= INT32_MAX; a column past the last user repeats the last user, window included
  if constexpr (WINDOWED) walk_clamp(a.window, uc, a.M, lo, hi);
  float tt = __builtin_nanf("");
  int tp = -1;
  if constexpr (!TPASS) {
    tt = a.t[uc];  // NaN: no compare against it is ever true
    tp = a.target_pos[uc];
  }

  int64_t t_beg, t_end;
  WalkSpans sp;
  if constexpr (TPASS) {
    // the users' targets: position -> catalogue row, -1 when the target can have no rank
    if (tid < TK_BM) {
      const int64_t u = u0 + tid;
      int row = -1;
      if (u < a.U) {
        int wl = 0, wh = static_cast<int>(a.M);
        if (a.window != nullptr) walk_clamp(a.window, u, a.M, wl, wh);
        row = walk_target_row(a, u, wl, wh);
      }
      trow[tid] = row;
    }
    const int64_t left = a.U - u0;
    t_beg = 0;
    t_end = ((left < TK_BM ? left : TK_BM) + CPS - 1) / CPS;
  } else {
    if (ex_lds) {  // [XP / 4][128] int4, padded with -1
      int* exw = reinterpret_cast<int*>(wun + 16);
      for (int i = tid; i < TK_BM * a.XP; i += TK_THREADS) {
        const int x = i / TK_BM, r = i - x * TK_BM;
        const int64_t u = u0 + r;
        exw[((x >> 2) * TK_BM + r) * 4 + (x & 3)] = (u < a.U && x < X) ? a.exclude[u * X + x] : -1;
      }
    }
    walk_span(a.M, CPS, split, a.steps_per_split, t_beg, t_end);
    if constexpr (WINDOWED) {  // the workgroup's union picks the steps
      sp = walk_spans_lane(lo, hi, live, wun, wave, lane);
      walk_span(sp, CPS, split, a.n_splits, t_beg, t_end);
    }
  }

  int n_adm = 0, n_ahd = 0;  // of this lane's user, over the candidates kl and kl + 2 of every step

  for (int64_t t = t_beg; t < t_end; ++t) {
    const int64_t n0 = t * CPS;
    __syncthreads();  // every wave is done with the previous step's candrow (and the prologue's LDS is written)
    if constexpr (TPASS) {
      if (tid < CPS) candrow[tid] = trow[n0 + tid];  // user n0 + tid of the workgroup owns this candidate
    } else {
      walk_rows<WINDOWED>(a, sp, n0, CPS, tid, candrow);
    }
    __syncthreads();

    // a wave with nothing to count in this step fills the operand images and takes the barriers, nothing else.  TPASS: the step's
    // CPS users all belong to one wave (32 % CPS == 0).  WINDOWED: none of the wave's windows meets the step.
    bool wave_on = true;
    if constexpr (TPASS) wave_on = static_cast<int>(n0) / 32 == wave;
    if constexpr (WINDOWED) wave_on = walk_meets(sp, n0, CPS);
    NpaPooled<LT> p;
    npa_pooled<LT>(a, th, Ts, Us, candrow, wave, kl, il, wave_on, p);
    if (!wave_on) continue;  // wave-uniform; the barriers of the step are all behind it

    if constexpr (TPASS) {
      // ---- the owner keeps its value: candidate c of the step is the target of the workgroup's user n0 + c
      const int own = rl - static_cast<int>(n0);
      {
        const float s0 = p.score(0), s1 = p.score(1);
        if (own == 0) tt = s0;
        if (own == 1) tt = s1;
      }
      if constexpr (CPS == 4) {
        const float s2 = p.score(2), s3 = p.score(3);
        if (own == 2) tt = s2;
        if (own == 3) tt = s3;
      }
    } else {
      // ---- counting: lane half kl takes candidates kl, kl + 2 of the step for user il.  WINDOWED: the position must lie in the
      // user's window as well -- unless the step is inside every window of this wave's users
      const WalkGate g = WINDOWED && walk_gated(sp, n0, CPS) ? walk_gate(lo, hi) : WalkGate();
      const int c0 = static_cast<int>(n0) + kl, c1 = c0 + 2;
      const int r0 = candrow[kl], r1 = CPS == 4 ? candrow[2 + kl] : -2;
      bool hit0 = false, hit1 = false;
      if (ex_lds) {
        for (int x4 = 0; x4 < a.XP / 4; ++x4) {
          const int4 e = exl[x4 * TK_BM + rl];
          hit0 |= e.x == r0 || e.y == r0 || e.z == r0 || e.w == r0;
          hit1 |= e.x == r1 || e.y == r1 || e.z == r1 || e.w == r1;
        }
      } else if (X > 0) {
        const int32_t* ex = a.exclude + uc * X;
        for (int x = 0; x < X; ++x) {
          const int e = ex[x];
          hit0 |= e == r0;
          hit1 |= e == r1;
        }
      }
      auto tally = [&](const float s, const int c, const int crow, const bool hit) {
        const bool inside = crow >= 0 && g.pass(c);
        saw_nan |= inside && s != s;
        const bool adm = inside && s == s && !hit;
        n_adm += adm ? 1 : 0;
        n_ahd += (adm && (s > tt || (s == tt && c < tp))) ? 1 : 0;
      };
      {
        const float s0 = p.score(0), s1 = p.score(1);
        tally(kl ? s1 : s0, c0, r0, hit0);
      }
      if constexpr (CPS == 4) {
        const float s2 = p.score(2), s3 = p.score(3);
        tally(kl ? s3 : s2, c1, r1, hit1);
      }
    }
  }

  if constexpr (TPASS) {
    if (kl == 0 && live) {
      const bool has = trow[rl] >= 0;  // written before the first step's barriers; a workgroup always has a step
      if (has && tt != tt) saw_nan = true;  // a NaN inside the user's window: no rank
      a.t[ul] = has ? tt : __builtin_nanf("");
    }
  } else {
    n_adm += __shfl_xor(n_adm, 32, 64);
    n_ahd += __shfl_xor(n_ahd, 32, 64);
    if (kl == 0 && live) {
      a.part[static_cast<int64_t>(split) * a.U + ul] = n_adm;
      a.part[(static_cast<int64_t>(a.n_splits) + split) * a.U + ul] = n_ahd;
    }
  }
  if (saw_nan && live) a.flags[1] = 1;
}

// adds the n_splits partial counts of a user (integer sums, any order gives the same) and writes the outputs
__global__ __launch_bounds__(256) void npa_rank_finish_kernel(NpaRankArgs a) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (u >= a.U) return;
  int count = 0, ahead = 0;
  for (int s = 0; s < a.n_splits; ++s) {
    count += a.part[static_cast<int64_t>(s) * a.U + u];
    ahead += a.part[(static_cast<int64_t>(a.n_splits) + s) * a.U + u];
  }
  const float t = a.t[u];
  const bool ranked = t == t;
  a.out_rank[u] = ranked ? 1 + ahead : 0;
  a.out_count[u] = count;
  a.out_score[u] = ranked ? topk_act(t, a.mode) : -INFINITY;
}

// M == 0: nobody has a rank; a target position >= M = 0 is still reported
__global__ __launch_bounds__(256) void npa_rank_empty_kernel(const int32_t* __restrict__ target_pos, int32_t* __restrict__ out_rank,
                                                             int32_t* __restrict__ out_count, float* __restrict__ out_score,
                                                             int32_t* __restrict__ flags, int64_t U) {
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; u < U; u += static_cast<int64_t>(gridDim.x) * 256) {
    if (target_pos[u] >= 0) flags[0] = 1;
    out_rank[u] = 0;
    out_count[u] = 0;
    out_score[u] = -INFINITY;
  }
}

template <int LT>
int npa_rank_launch(const NpaRankArgs& a, int64_t user_tiles, int splits, hipStream_t s) {
  const dim3 block(TK_THREADS);
  const unsigned tiles = static_cast<unsigned>(user_tiles);
  EBN_LAUNCH((npa_rank_kernel<LT, false, true>), dim3(tiles), block, static_cast<size_t>(npa_rank_lds_bytes(0)), s, a);
  EBN_CHECK_LAUNCH();
  const size_t lds = static_cast<size_t>(npa_rank_lds_bytes(a.X > 0 && a.X <= NR_X_LDS ? a.XP : 0));
  const dim3 grid(tiles, static_cast<unsigned>(splits));
  if (a.window != nullptr) {
    EBN_LAUNCH((npa_rank_kernel<LT, true, false>), grid, block, lds, s, a);
  } else {
    EBN_LAUNCH((npa_rank_kernel<LT, false, false>), grid, block, lds, s, a);
  }
  EBN_CHECK_LAUNCH();
  EBN_LAUNCH(npa_rank_finish_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(a.U, 256))), dim3(256), 0, s, a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

}  // namespace

extern "C" int64_t ebn_npa_target_rank_workspace_bytes(int64_t n_users, int32_t n_splits) {
  if (!ebn_dim_ok(n_users) || n_splits < 1) return 0;
  if (n_users == 0) return 16;
  const int64_t s = n_splits > TK_MAX_SPLITS ? TK_MAX_SPLITS : n_splits;
  // [U] float target scores, [2, s, U] int32 partial counts: one range needs them too (the target pass, the adding launch)
  return ebn_sat_add(ebn_sat_mul(ebn_sat_add(ebn_sat_mul(2 * s, n_users), n_users), 4), 16);
}

extern "C" int ebn_npa_target_rank_f32(const float* users, const float* Q, const float* Ua_all, const float* Vd_all, int64_t n_rows,
                                       const int32_t* cand_rows, int64_t M, const int32_t* target_pos, const int32_t* window,
                                       const int32_t* exclude, int32_t X, int32_t mode, int32_t n_splits, int32_t* out_rank,
                                       int32_t* out_count, float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes,
                                       int64_t U, int32_t L, int32_t F, int32_t A, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(U, M, n_rows) && L >= 0 && F >= 0 && A >= 0 && X >= 0 && n_splits >= 0 && workspace_bytes >= 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(mode == 0 || mode == 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(X <= TK_MAX_X && L >= 1 && L <= NR_MAX_L, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(A >= 4 && A % 4 == 0 && A <= NR_MAX_A && F >= 4 && F % 4 == 0 && F <= NR_MAX_F, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(cand_rows != nullptr || M == n_rows, EBN_ERR_BAD_ARG);
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(target_pos != nullptr && out_rank != nullptr && out_count != nullptr && out_score != nullptr && flags != nullptr,
              EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (M == 0) {
    const int64_t blocks = ebn_ceil_div(U, 256);
    EBN_LAUNCH(npa_rank_empty_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, target_pos, out_rank,
               out_count, out_score, flags, U);
    EBN_CHECK_LAUNCH();
    return EBN_OK;
  }
  EBN_REQUIRE(users != nullptr && Q != nullptr && Ua_all != nullptr && Vd_all != nullptr && n_rows >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_aligned16(users) && ebn_aligned16(Q) && ebn_aligned16(Ua_all) && ebn_aligned16(Vd_all), EBN_ERR_ALIGN);
  if (exclude == nullptr) X = 0;
  const int splits = walk_resolve_splits(U, M, npa_cands_per_step(L), n_splits);
  const int64_t user_tiles = ebn_ceil_div(U, TK_BM);
  EBN_REQUIRE(user_tiles <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  const int64_t need = ebn_npa_target_rank_workspace_bytes(U, splits);
  EBN_REQUIRE(workspace != nullptr && workspace_bytes >= need, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_aligned16(workspace), EBN_ERR_ALIGN);
  NpaRankArgs a;
  a.users = users;
  a.Q = Q;
  a.Ua = Ua_all;
  a.Vd = Vd_all;
  a.cand_rows = cand_rows;
  a.target_pos = target_pos;
  a.window = window;
  a.exclude = exclude;
  a.out_rank = out_rank;
  a.out_count = out_count;
  a.out_score = out_score;
  a.flags = flags;
  a.t = static_cast<float*>(workspace);
  a.part = reinterpret_cast<int32_t*>(a.t + U);
  a.U = U;
  a.M = M;
  a.n_rows = n_rows;
  a.L = L;
  a.F = F;
  a.A = A;
  a.X = X;
  a.XP = (X + 3) / 4 * 4;
  a.mode = mode;
  a.n_splits = splits;
  a.steps_per_split = walk_units_per_split(M, npa_cands_per_step(L), splits);
  return L <= 32 ? npa_rank_launch<1>(a, user_tiles, splits, s) : npa_rank_launch<2>(a, user_tiles, splits, s);
}
