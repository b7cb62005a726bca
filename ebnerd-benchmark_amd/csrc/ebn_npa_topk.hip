// Top-k recommendation for NPA from the once-encoded catalogue: NPA's news vector depends on the user (personalised attentive
// pooling, layers.py:312-339), so there is no [n_rows, F] catalogue to run ebn_topk.hip over.  Per (user u, candidate row) pair
//
//   s_l = Q[u] . Ua_all[row, l]            l = 0 .. L-1       (GEMM 1, K = A)
//   w   = softmax_l(s)                                        (max-subtracted; NPA has no masking: every token counts)
//   d_l = users[u] . Vd_all[row, l]                           (GEMM 2, K = F)
//   score[u, c] = sum_l w_l d_l = (sum_l e_l d_l) / (sum_l e_l),  e_l = exp(s_l - max s)
//
// Both GEMMs run on v_mfma_f32_32x32x2_f32 (exact fp32, an fma chain in k order) with the catalogue TOKENS on the row side and the
// users on the column side: in the 32x32 C layout a lane then holds ONE user's column (user = lane & 31), 16 of a candidate's 32
// token rows in its own registers (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) and the other 16 in lane ^ 32 -- the max, the sum
// and the weighted sum over L are in-register reductions plus one cross-half exchange per candidate.  Neither the [U, M, L] logits
// and dots nor the [U, M] scores reach memory.
//
// A 256-thread workgroup owns 128 users (wave w: users 32w .. 32w + 31, ONE column tile) and walks its range of candidate steps; a
// step is 128 token rows = four row tiles = four candidates (L <= 32) or two (L in 33 .. 64: a candidate is two tiles).  L is padded
// to the tile only: a padded token row is never loaded (zeros go into the LDS image, its address stays inside the row's L tokens)
// and its logit is set to -inf, weight exactly 0.  The K = A phase leaves the logits in 64 accumulator registers, they are turned
// into e_l in place, the K = F phase fills a second set of 64, and the score is reduced from the two.  Operand staging is
// ebn_topk.hip's: XOR-swizzled float4 LDS images, 16-deep slabs, two buffers, one barrier per slab.  The whole step up to the score
// is npa_pooled of ebn_catalogue_walk.h, which npa_rank_kernel (ebn_npa_target_rank.hip) calls as well; the selection (survivor
// queue, sorted insert, write-out, merge of the n_splits partial lists) is ebn_topk_list.h, shared with ebn_topk.hip.
//
// A pair's score bits depend only on the user's two rows and the catalogue row's data: every fma chain, the in-lane reduction order
// and the (commutative) cross-half add are the same whatever the candidate's position, U, M or n_splits.  Lists are bit-identical for
// every n_splits and from run to run.  The score is NOT bit-equal to ebn_pap_indexed_f32's, which pools first and dots second.
//
// Windowed form (ebn_npa_topk_score_window_f32, the WINDOWED instantiations): user u may only receive the candidate positions of
// window[u] = [lo, hi), clamped to [0, M).  A lane holds ONE user for the whole walk, so the user's clamped range sits in two
// registers (npa_rank_kernel<LT, true, false>'s arrangement; no per-row LDS table as in ebn_topk.hip).  A wave reduces its 32 ranges
// to their union [vlo, vhi) over the non-empty ones and their intersection [ilo, ihi); the workgroup's union [wlo, whi) goes through
// 8 ints of LDS behind the list plan and picks the steps the workgroup walks, dealt evenly over the n_splits ranges of ITS OWN step
// span.  A wave whose union misses a visited step stages its share of the slabs and takes the barriers -- no MFMA, no expf pass, no
// selection.  A score is offered only when its position also lies in the lane's window (one unsigned compare; a step inside the
// wave's intersection takes the plain compare), so nothing outside a window reaches the queue, the NaN flag or the lists.  The
// score is the plain form's call of npa_pooled: the same bits for the same (user rows, catalogue row) pair.
#include "ebn_catalogue_walk.h"
#include "ebn_topk_list.h"

namespace {

constexpr int NT_MAX_L = 64, NT_MAX_A = 1024, NT_MAX_F = 4096;

struct NpaTopkArgs : TopkList {
  const float* users;  // [U, F]
  const float* Q;      // [U, A]
  const float* Ua;     // [n_rows, L, A]
  const float* Vd;     // [n_rows, L, F]
  const int32_t* cand_rows;
  int64_t M, n_rows;
  int32_t L, F, A, steps_per_split;
  const int32_t* window;  // [U, 2] (lo, hi) candidate positions; the WINDOWED instantiations only
};

constexpr int NT_WINDOW_LDS_BYTES = 8 * 4;  // (lo, hi) of the four waves' unions behind the plan of ebn_topk_list.h

// LT: row tiles of one candidate (1: L <= 32, 2: L <= 64).  dynamic LDS layout: ebn_topk_list.h (WINDOWED: + wave unions[8])
template <int LT, bool WINDOWED>
__global__ __launch_bounds__(TK_THREADS, 2) void npa_topk_kernel(NpaTopkArgs a) {
  constexpr int CPS = TK_TILES / LT;  // candidates of a step
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = lane >> 5, il = lane & 31;
  const int k = a.k;
  const int64_t u0 = static_cast<int64_t>(blockIdx.x) * TK_BM;
  const int split = blockIdx.y;
  const TopkLds lds = topk_lds(smem, wave, k);
  float *Ts = lds.As, *Us = lds.Bs;  // token rows | users
  volatile float* thr = lds.thr;
  volatile int* candrow = lds.candrow;
  volatile float* qs = lds.qs;
  volatile int* qrc = lds.qrc;

  topk_list_init(lds, k, tid);
  __syncthreads();  // a range without steps (more splits than steps divide into) still writes its empty lists out

  const NpaThread th = npa_thread<LT>(a, u0, tid);
  bool saw_nan = false;

  int64_t t_beg, t_end;
  walk_span(a.M, CPS, split, a.steps_per_split, t_beg, t_end);

  // WINDOWED: this lane's user (column il of the wave's tile) and its clamped range; a column past the last user repeats the last
  // user, window included.  The workgroup's union picks the steps
  int lo = 0, hi = 0;
  WalkSpans sp;
  if constexpr (WINDOWED) {
    const int64_t ul = u0 + wave * 32 + il;
    const bool live = ul < a.U;
    walk_clamp(a.window, live ? ul : a.U - 1, a.M, lo, hi);
    volatile int* wun = lds.lps + TK_BM * k;  // the end of the plan: topk_lds_bytes(k)
    sp = walk_spans_lane(lo, hi, live, wun, wave, lane);
    walk_span(sp, CPS, split, a.n_splits, t_beg, t_end);
  }

  for (int64_t t = t_beg; t < t_end; ++t) {
    const int64_t n0 = t * CPS;
    __syncthreads();  // every wave is done with the previous step's candrow (and the lists are initialised)
    walk_rows<WINDOWED>(a, sp, n0, CPS, tid, candrow);
    __syncthreads();

    // WINDOWED: a wave none of whose users' windows meets the step fills the operand images and takes the barriers, nothing else:
    // no MFMA, no expf pass, no selection
    const bool wave_on = !WINDOWED || walk_meets(sp, n0, CPS);
    NpaPooled<LT> p;
    npa_pooled<LT>(a, th, Ts, Us, candrow, wave, kl, il, wave_on, p);
    if (!wave_on) continue;  // wave-uniform; the barriers of the step are all behind it, the drain has none

    // ---- selection: lane half kl offers candidates kl, kl + 2 of the step for user il; one compare against the user's current
    // k-th best (NaN survives on purpose, it has to reach the flag), survivors compacted into the wave's queue and drained
    const int rl = wave * 32 + il;
    const float thv = thr[rl];
    int cnt = 0;
    // WINDOWED: the position must lie in the user's window as well -- unless the step is inside every window of this wave's users
    const WalkGate g = WINDOWED && walk_gated(sp, n0, CPS) ? walk_gate(lo, hi) : WalkGate();
    const int c0 = static_cast<int>(n0);
    auto offer = [&](const float s, const int c) {
      const bool pass = !(s < thv) && (!WINDOWED || g.pass(c0 + c));
      const unsigned long long m = __ballot(pass);
      if (pass) {
        const int slot = cnt + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
        qs[slot] = s;
        qrc[slot] = (rl << 8) | c;
      }
      cnt += __popcll(m);
    };
    {
      const float s0 = p.score(0), s1 = p.score(1);
      offer(kl ? s1 : s0, kl);
    }
    if constexpr (CPS == 4) {
      const float s2 = p.score(2), s3 = p.score(3);
      offer(kl ? s3 : s2, 2 + kl);
    }
    topk_list_drain(a, lds, cnt, u0, n0, lane, saw_nan);
  }

  if (saw_nan) a.flags[1] = 1;
  topk_list_write(a, lds, u0, split, wave, lane);
}

template <int LT, bool WINDOWED>
int npa_launch(const NpaTopkArgs& a, int64_t user_tiles, int splits, hipStream_t s) {
  constexpr int extra = WINDOWED ? NT_WINDOW_LDS_BYTES : 0;
  // above the 64 KB a kernel may use without asking (k > 44); set per call: the attribute belongs to the current device
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(npa_topk_kernel<LT, WINDOWED>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(topk_lds_bytes(TK_MAX_K)) + extra) != hipSuccess) {
    (void)hipGetLastError();
    return EBN_ERR_UNSUPPORTED;
  }
  EBN_LAUNCH((npa_topk_kernel<LT, WINDOWED>), dim3(static_cast<unsigned>(user_tiles), static_cast<unsigned>(splits)), dim3(TK_THREADS),
             static_cast<size_t>(topk_lds_bytes(a.k) + extra), s, a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

}  // namespace

extern "C" int ebn_npa_topk_auto_splits(int64_t n_users, int64_t n_cand, int32_t L) {
  if (!ebn_dim_ok(n_users, n_cand) || n_users == 0 || n_cand == 0 || L < 1 || L > NT_MAX_L) return 1;
  return walk_resolve_splits(n_users, n_cand, npa_cands_per_step(L), 0);
}

namespace {

// both entry points: the checks, the plan and the launches; WINDOWED adds the window argument and 32 bytes of LDS
template <bool WINDOWED>
int npa_topk_score(const float* users, const float* Q, const float* Ua_all, const float* Vd_all, int64_t n_rows, const int32_t* cand_rows,
                   int64_t M, const int32_t* window, const int32_t* exclude, int32_t X, int32_t k, int32_t mode, int32_t n_splits,
                   int32_t* out_pos, float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U, int32_t L,
                   int32_t F, int32_t A, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(U, M, n_rows) && L >= 0 && F >= 0 && A >= 0 && X >= 0 && n_splits >= 0 && workspace_bytes >= 0, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(mode == 0 || mode == 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(k >= 1 && k <= TK_MAX_K && X <= TK_MAX_X && L >= 1 && L <= NT_MAX_L, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(A >= 4 && A % 4 == 0 && A <= NT_MAX_A && F >= 4 && F % 4 == 0 && F <= NT_MAX_F, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(cand_rows != nullptr || M == n_rows, EBN_ERR_BAD_ARG);
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(out_pos != nullptr && out_score != nullptr && flags != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(!WINDOWED || window != nullptr, EBN_ERR_BAD_ARG);
  hipStream_t s = ebn_stream(stream);
  if (M == 0) return topk_launch_fill_empty(out_pos, out_score, U, k, s);
  EBN_REQUIRE(users != nullptr && Q != nullptr && Ua_all != nullptr && Vd_all != nullptr && n_rows >= 1, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_aligned16(users) && ebn_aligned16(Q) && ebn_aligned16(Ua_all) && ebn_aligned16(Vd_all), EBN_ERR_ALIGN);
  if (exclude == nullptr) X = 0;
  const int splits = walk_resolve_splits(U, M, npa_cands_per_step(L), n_splits);
  const int64_t user_tiles = ebn_ceil_div(U, TK_BM);
  EBN_REQUIRE(user_tiles <= EBN_DIM_MAX, EBN_ERR_UNSUPPORTED);
  NpaTopkArgs a;
  a.users = users;
  a.Q = Q;
  a.Ua = Ua_all;
  a.Vd = Vd_all;
  a.cand_rows = cand_rows;
  a.window = window;
  a.exclude = exclude;
  a.out_pos = out_pos;
  a.out_score = out_score;
  a.flags = flags;
  a.U = U;
  a.M = M;
  a.n_rows = n_rows;
  a.L = L;
  a.F = F;
  a.A = A;
  a.X = X;
  a.k = k;
  a.mode = mode;
  a.n_splits = splits;
  a.steps_per_split = walk_units_per_split(M, npa_cands_per_step(L), splits);
  int rc = topk_bind_workspace(a, splits, workspace, workspace_bytes);
  if (rc != EBN_OK) return rc;
  rc = L <= 32 ? npa_launch<1, WINDOWED>(a, user_tiles, splits, s) : npa_launch<2, WINDOWED>(a, user_tiles, splits, s);
  if (rc != EBN_OK) return rc;
  if (splits > 1) return topk_launch_merge(a, s);
  return EBN_OK;
}

}  // namespace

extern "C" int ebn_npa_topk_score_f32(const float* users, const float* Q, const float* Ua_all, const float* Vd_all, int64_t n_rows,
                                      const int32_t* cand_rows, int64_t M, const int32_t* exclude, int32_t X, int32_t k, int32_t mode,
                                      int32_t n_splits, int32_t* out_pos, float* out_score, int32_t* flags, void* workspace,
                                      int64_t workspace_bytes, int64_t U, int32_t L, int32_t F, int32_t A, ebn_stream_t stream) {
  return npa_topk_score<false>(users, Q, Ua_all, Vd_all, n_rows, cand_rows, M, nullptr, exclude, X, k, mode, n_splits, out_pos, out_score,
                               flags, workspace, workspace_bytes, U, L, F, A, stream);
}

extern "C" int ebn_npa_topk_score_window_f32(const float* users, const float* Q, const float* Ua_all, const float* Vd_all, int64_t n_rows,
                                             const int32_t* cand_rows, int64_t M, const int32_t* window, const int32_t* exclude, int32_t X,
                                             int32_t k, int32_t mode, int32_t n_splits, int32_t* out_pos, float* out_score, int32_t* flags,
                                             void* workspace, int64_t workspace_bytes, int64_t U, int32_t L, int32_t F, int32_t A,
                                             ebn_stream_t stream) {
  return npa_topk_score<true>(users, Q, Ua_all, Vd_all, n_rows, cand_rows, M, window, exclude, X, k, mode, n_splits, out_pos, out_score,
                              flags, workspace, workspace_bytes, U, L, F, A, stream);
}
