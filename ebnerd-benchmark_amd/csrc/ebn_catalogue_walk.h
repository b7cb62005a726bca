// The catalogue walk shared by the fused score kernels: ebn_topk.hip and ebn_target_rank.hip (score = user . news row), and
// ebn_npa_topk.hip and ebn_npa_target_rank.hip (NPA's personalised pooling).  A 256-thread workgroup owns 128 users, four waves of
// 32, and walks its range of the candidates in units of 128 operand rows (a 128-candidate tile; an NPA step of 4 or 2 candidates'
// token rows).  What a kernel does with the scores -- a sorted list, two counters -- is its own epilogue; everything a score's bits
// depend on is in here, ONCE: a target's rank is the index of its slot in the top-k list, with that slot's score bits, because
// both kernels are built from these functions.
//
//   staging    registers -> XOR-swizzled float4 LDS image S4[mn][kq ^ ((mn >> 2) & 3)] of ebn_gemm.hip (one conflict-free
//              ds_read_b128 per four MFMA steps), 16-deep slabs, two buffers, one barrier per slab: walk_run
//   MFMA       v_mfma_f32_32x32x2_f32 (exact fp32, an fma chain in k order), the wave's own 32 rows against all 128 of the other
//              operand, 64 accumulator registers: walk_mma
//   NPA        both GEMM phases, the softmax over a candidate's tokens in registers, the pooled score: npa_pooled
//   windows    clamp, the unions and the intersection a workgroup and a wave walk by, the span of a split, the one-compare gate
//   rows       position -> catalogue row of a unit's candidates and of a user's target, with the "outside the table" flag
//   host       the number of ranges the candidates are split into
#pragma once
#include <math.h>

#include "ebn_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TK_BM = 128, TK_BN = 128, TK_BK = 16, TK_THREADS = 256;
constexpr int TK_TILES = TK_BN / 32;           // 32-row MFMA tiles of the streamed operand
constexpr int TK_MAX_SPLITS = 64;
constexpr int TK_TILE_FLOATS = TK_BM * TK_BK;  // one operand slab image

// ---- dynamic LDS: the operand images (A | B, two buffers each) come first, a kernel's own plan follows at `own`
constexpr int TK_IMAGE_FLOATS = 4 * TK_TILE_FLOATS;

struct WalkImages {
  float *As, *Bs, *own;
};

__device__ __forceinline__ WalkImages walk_images(float* smem) { return {smem, smem + 2 * TK_TILE_FLOATS, smem + TK_IMAGE_FLOATS}; }

// ---- operand staging.  A thread's two float4 of an operand slab: item v = tid + 256 i -> image row v / 4, k quarter v % 4
struct WalkSlab {
  int sdst[2];  // where the float4 goes in the swizzled image
  int kq4;      // its first k inside the slab (256 % 4 == 0: the same for both items)
};

__device__ __forceinline__ WalkSlab walk_slab(int tid) {
  WalkSlab s;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int v = tid + i * TK_THREADS, mn = v >> 2, kq = v & 3;
    s.sdst[i] = (mn * 4 + (kq ^ ((mn >> 2) & 3))) * 4;
  }
  s.kq4 = (tid & 3) * 4;
  return s;
}

__device__ __forceinline__ int walk_slab_row(int tid, int i) { return (tid + i * TK_THREADS) >> 2; }

// the user whose row item i stages: rows past the last user repeat it; what they give is never written out
__device__ __forceinline__ int64_t walk_slab_user(int64_t u0, int64_t U, int tid, int i) {
  const int64_t u = u0 + walk_slab_row(tid, i);
  return u < U ? u : U - 1;
}

__device__ __forceinline__ void walk_zero(f32x16 (&acc)[TK_TILES]) {
#pragma unroll
  for (int j = 0; j < TK_TILES; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
}

// The slab pipeline of one unit over K: image A from the rows pa[] (+ kq4 already), image B from pb[]; mma(buf) only when this
// wave has something to compute (a wave that has not still stages its share and takes the barriers).  K % 4 == 0: a float4 is all
// inside the row or all outside; an outside piece reads the row's first bytes and is zeroed.  With load_a (NPA's token rows: those
// past L are padding, load_a[i] false) image A skips the load instead: a padded row and an outside piece are zeros, never read.
template <class Mma>
__device__ __forceinline__ void walk_run(float* As, float* Bs, const WalkSlab& sl, const float* const (&pa)[2],
                                         const float* const (&pb)[2], const bool* load_a, int K, bool wave_on, Mma&& mma) {
  const int nk = (K + TK_BK - 1) / TK_BK;
  float4 ra[2], rb[2];
  auto fetch = [&](int kt) {
    const int kk = kt * TK_BK;
    const bool ok = kk + sl.kq4 < K;
    const int off = ok ? kk : -sl.kq4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (load_a == nullptr || (ok && load_a[i])) x = *reinterpret_cast<const float4*>(pa[i] + off);
      const float4 y = *reinterpret_cast<const float4*>(pb[i] + off);
      if (load_a == nullptr) x = make_float4(ok ? x.x : 0.f, ok ? x.y : 0.f, ok ? x.z : 0.f, ok ? x.w : 0.f);
      ra[i] = x;
      rb[i] = make_float4(ok ? y.x : 0.f, ok ? y.y : 0.f, ok ? y.z : 0.f, ok ? y.w : 0.f);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<float4*>(&As[buf * TK_TILE_FLOATS + sl.sdst[i]]) = ra[i];
      *reinterpret_cast<float4*>(&Bs[buf * TK_TILE_FLOATS + sl.sdst[i]]) = rb[i];
    }
  };
  fetch(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt += 2) {
    if (kt + 1 < nk) fetch(kt + 1);
    if (wave_on) mma(0);
    if (kt + 1 < nk) store(1);
    __syncthreads();
    if (kt + 1 < nk) {
      if (kt + 2 < nk) fetch(kt + 2);
      if (wave_on) mma(1);
      if (kt + 2 < nk) store(0);
      __syncthreads();
    }
  }
}

// ---- MFMA.  Lane (kl, il) reads image row il's k-quad of MFMA steps 4 j8 .. 4 j8 + 3 at float q of the row: contraction index
// k = 8 j8 + 4 kl + w, the same for both operands (rows il and 32 wave + il share the swizzle)
__device__ __forceinline__ int walk_quad(int j8, int kl, int il) { return ((2 * j8 + kl) ^ ((il >> 2) & 3)) * 4; }

// One slab: the wave's own 32 rows (image A when OWN_A -- the dense kernels' users -- else image B: NPA's users, the tokens on the
// A side) against the four 32-row tiles of the other image.  C/D map: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
template <bool OWN_A>
__device__ __forceinline__ void walk_mma(const float* As, const float* Bs, int buf, int wave, int kl, int il, f32x16 (&acc)[TK_TILES]) {
  const float* own = (OWN_A ? As : Bs) + buf * TK_TILE_FLOATS + (wave * 32 + il) * 16;
  const float* all = (OWN_A ? Bs : As) + buf * TK_TILE_FLOATS + il * 16;
#pragma unroll
  for (int j8 = 0; j8 < TK_BK / 8; ++j8) {
    const int q = walk_quad(j8, kl, il);
    float ov[4], tv[TK_TILES][4];
#pragma unroll
    for (int w = 0; w < 4; ++w) ov[w] = own[q + w];
#pragma unroll
    for (int j = 0; j < TK_TILES; ++j)
#pragma unroll
      for (int w = 0; w < 4; ++w) tv[j][w] = all[j * 32 * 16 + q + w];
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int j = 0; j < TK_TILES; ++j)
        acc[j] = OWN_A ? __builtin_amdgcn_mfma_f32_32x32x2f32(ov[w], tv[j][w], acc[j], 0, 0, 0)
                       : __builtin_amdgcn_mfma_f32_32x32x2f32(tv[j][w], ov[w], acc[j], 0, 0, 0);
  }
}

// ---- windows.  window[u] = [lo, hi) candidate positions, clamped to [0, M) (M <= INT32_MAX); an empty one is [0, 0): no
// position passes
__device__ __forceinline__ void walk_clamp(const int32_t* window, int64_t u, int64_t M, int& lo, int& hi) {
  lo = window[2 * u];
  hi = window[2 * u + 1];
  lo = lo > 0 ? lo : 0;
  hi = static_cast<int64_t>(hi) < M ? hi : static_cast<int>(M);
  if (lo >= hi) lo = hi = 0;
}

// What the walk needs of 128 windows, all wave-uniform: the union of the workgroup [wlo, whi) and of this wave [vlo, vhi) over the
// non-empty ranges (none: lo = INT32_MAX, hi = 0), the intersection of this wave [ilo, ihi) over its users below U
struct WalkSpans {
  int wlo = 0, whi = 0, vlo = 0, vhi = 0, ilo = 0, ihi = 0;
};

// the dense arrangement: the clamped ranges are a per-row LDS table (a row past the last user: [0, 0)), already behind a barrier.
// lane l: rows l and l + 64 for the workgroup, row 32 wave + (l & 31) for the wave
template <class Table>
__device__ __forceinline__ WalkSpans walk_spans_table(Table win_lo, Table win_hi, int64_t u0, int64_t U, int wave, int lane) {
  int ulo = INT32_MAX, uhi = 0, xlo = INT32_MAX, xhi = 0, nlo = 0, nhi = INT32_MAX;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int lo = win_lo[lane + 64 * i], hi = win_hi[lane + 64 * i];
    if (lo < hi) {
      ulo = lo < ulo ? lo : ulo;
      uhi = hi > uhi ? hi : uhi;
    }
  }
  {
    const int row = wave * 32 + (lane & 31);
    const int lo = win_lo[row], hi = win_hi[row];
    if (lo < hi) {
      xlo = lo;
      xhi = hi;
    }
    if (u0 + row < U) {
      nlo = lo;
      nhi = hi;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o0 = __shfl_xor(ulo, off, 64), o1 = __shfl_xor(uhi, off, 64), o2 = __shfl_xor(xlo, off, 64);
    const int o3 = __shfl_xor(xhi, off, 64), o4 = __shfl_xor(nlo, off, 64), o5 = __shfl_xor(nhi, off, 64);
    ulo = o0 < ulo ? o0 : ulo;
    uhi = o1 > uhi ? o1 : uhi;
    xlo = o2 < xlo ? o2 : xlo;
    xhi = o3 > xhi ? o3 : xhi;
    nlo = o4 > nlo ? o4 : nlo;
    nhi = o5 < nhi ? o5 : nhi;
  }
  WalkSpans s;
  s.wlo = __builtin_amdgcn_readfirstlane(ulo);
  s.whi = __builtin_amdgcn_readfirstlane(uhi);
  s.vlo = __builtin_amdgcn_readfirstlane(xlo);
  s.vhi = __builtin_amdgcn_readfirstlane(xhi);
  s.ilo = __builtin_amdgcn_readfirstlane(nlo);
  s.ihi = __builtin_amdgcn_readfirstlane(nhi);
  return s;
}

// NPA's arrangement: a lane holds ONE user for the whole walk (column lane & 31 of the wave's tile, both lane halves the same 32
// users), so its clamped range [lo, hi) sits in two registers; live: the user is below U.  The workgroup's union goes through the
// 8 ints of LDS at wun, with a barrier
template <class Unions>
__device__ __forceinline__ WalkSpans walk_spans_lane(int lo, int hi, bool live, Unions wun, int wave, int lane) {
  int xlo = INT32_MAX, xhi = 0, nlo = 0, nhi = INT32_MAX;
  if (live) {
    if (lo < hi) {
      xlo = lo;
      xhi = hi;
    }
    nlo = lo;
    nhi = hi;
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {
    const int o0 = __shfl_xor(xlo, off, 64), o1 = __shfl_xor(xhi, off, 64), o2 = __shfl_xor(nlo, off, 64), o3 = __shfl_xor(nhi, off, 64);
    xlo = o0 < xlo ? o0 : xlo;
    xhi = o1 > xhi ? o1 : xhi;
    nlo = o2 > nlo ? o2 : nlo;
    nhi = o3 < nhi ? o3 : nhi;
  }
  WalkSpans s;
  s.vlo = __builtin_amdgcn_readfirstlane(xlo);
  s.vhi = __builtin_amdgcn_readfirstlane(xhi);
  s.ilo = __builtin_amdgcn_readfirstlane(nlo);
  s.ihi = __builtin_amdgcn_readfirstlane(nhi);
  if (lane == 0) {
    wun[2 * wave] = s.vlo;
    wun[2 * wave + 1] = s.vhi;
  }
  __syncthreads();
  int wlo = INT32_MAX, whi = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int l = wun[2 * w], h = wun[2 * w + 1];
    wlo = l < wlo ? l : wlo;
    whi = h > whi ? h : whi;
  }
  s.wlo = __builtin_amdgcn_readfirstlane(wlo);
  s.whi = __builtin_amdgcn_readfirstlane(whi);
  return s;
}

// the units [t_beg, t_end) of range `split`: per_split units each, of the ceil(M / unit) there are
__device__ __forceinline__ void walk_span(int64_t M, int unit, int split, int per_split, int64_t& t_beg, int64_t& t_end) {
  const int64_t n_units = (M + unit - 1) / unit;
  t_beg = static_cast<int64_t>(split) * per_split;
  t_end = t_beg + per_split;
  t_end = t_end < n_units ? t_end : n_units;
}

// windowed: the units that meet the workgroup's union, dealt evenly over the n_splits ranges of ITS OWN span
__device__ __forceinline__ void walk_span(const WalkSpans& s, int unit, int split, int n_splits, int64_t& t_beg, int64_t& t_end) {
  const int64_t w_beg = s.wlo / unit, w_end = s.wlo < s.whi ? (static_cast<int64_t>(s.whi) + unit - 1) / unit : w_beg;
  const int64_t w_n = w_end - w_beg;
  t_beg = w_beg + w_n * split / n_splits;
  t_end = w_beg + w_n * (split + 1) / n_splits;
}

// the wave's union meets the unit [n0, n0 + n): it has something to compute
__device__ __forceinline__ bool walk_meets(const WalkSpans& s, int64_t n0, int n) { return n0 < s.vhi && n0 + n > s.vlo; }

// the unit [n0, n0 + n) is not inside every window of the wave: each position is compared against its user's window as well
__device__ __forceinline__ bool walk_gated(const WalkSpans& s, int64_t n0, int n) { return !(n0 >= s.ilo && n0 + n <= s.ihi); }

// lo <= c < hi as ONE unsigned compare: (c - lo) < (hi - lo); 0 <= lo <= hi <= M and c < 2^31, nothing wraps.  The default lets
// every position pass
struct WalkGate {
  int lo = 0;
  unsigned width = UINT32_MAX;
  __device__ __forceinline__ bool pass(int c) const { return static_cast<unsigned>(c - lo) < width; }
};

__device__ __forceinline__ WalkGate walk_gate(int lo, int hi) { return {lo, static_cast<unsigned>(hi - lo)}; }

// ---- rows.  The catalogue rows of the unit's n positions n0 .. n0 + n - 1 into candrow[] (LDS; the caller's barrier publishes
// them): -2 past the last candidate, -1 outside the table -- never turned into an address, and flags[0] is set; WINDOWED: only
// inside the workgroup's union, a visited unit also has positions outside it
template <bool WINDOWED, class Args, class Rows>
__device__ __forceinline__ void walk_rows(const Args& a, const WalkSpans& s, int64_t n0, int n, int tid, Rows candrow) {
  if (tid < n) {
    const int64_t c = n0 + tid;
    int row = -2;
    if (c < a.M) {
      const int64_t r = a.cand_rows != nullptr ? static_cast<int64_t>(a.cand_rows[c]) : c;
      if (r < 0 || r >= a.n_rows) {
        row = -1;
        if (!WINDOWED || (c >= s.wlo && c < s.whi)) a.flags[0] = 1;
      } else {
        row = static_cast<int>(r);
      }
    }
    candrow[tid] = row;
  }
}

// The catalogue row of user u's target, -1 when it can have no rank: no position (>= M sets flags[0]), outside the user's clamped
// window [lo, hi), of a row outside the table (flags[0]: it is inside this user's window), or excluded
template <class Args>
__device__ __forceinline__ int walk_target_row(const Args& a, int64_t u, int lo, int hi) {
  int p = a.target_pos[u];
  if (static_cast<int64_t>(p) >= a.M) {
    a.flags[0] = 1;
    p = -1;
  }
  if (p < lo || p >= hi) p = -1;  // also p < 0
  int row = -1;
  if (p >= 0) {
    const int64_t r = a.cand_rows != nullptr ? static_cast<int64_t>(a.cand_rows[p]) : p;
    if (r < 0 || r >= a.n_rows) {
      a.flags[0] = 1;
    } else {
      row = static_cast<int>(r);
      const int32_t* ex = a.exclude + u * a.X;
      bool hit = false;
      for (int x = 0; x < a.X; ++x) hit |= ex[x] == row;
      if (hit) row = -1;
    }
  }
  return row;
}

// ---- NPA: score(u, row) = sum_l softmax_l(Q[u] . Ua[row, l]) (users[u] . Vd[row, l]).  LT: 32-row tiles of one candidate (1:
// L <= 32, 2: L <= 64); a step is TK_TILES / LT candidates
inline int npa_cands_per_step(int32_t L) { return L <= 32 ? TK_TILES : TK_TILES / 2; }

// what a thread keeps for the whole walk: its slab items' user rows of Q and users, and which token row of the step they stage
struct NpaThread {
  WalkSlab sl;
  const float *pq[2], *pu[2];
  int tok_c[2], tok_l[2];  // candidate of the step, token of the candidate (>= L: padding)
};

template <int LT, class Args>
__device__ __forceinline__ NpaThread npa_thread(const Args& a, int64_t u0, int tid) {
  NpaThread th;
  th.sl = walk_slab(tid);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t u = walk_slab_user(u0, a.U, tid, i);
    th.pq[i] = a.Q + u * a.A + th.sl.kq4;
    th.pu[i] = a.users + u * a.F + th.sl.kq4;
    th.tok_c[i] = walk_slab_row(tid, i) / (32 * LT);
    th.tok_l[i] = walk_slab_row(tid, i) % (32 * LT);
  }
  return th;
}

// C/D map of both phases: user = lane & 31, token row of tile j = (r & 3) + 8 (r >> 2) + 4 (lane >> 5); candidate c of the step
// owns tiles c LT .. c LT + LT - 1
template <int LT>
struct NpaPooled {
  f32x16 ew[TK_TILES];      // e_l = exp(s_l - max s)
  f32x16 dv[TK_TILES];      // d_l
  float den[TK_TILES / LT];  // sum_l e_l
  // both lane halves end with the same bits: the cross-half add is commutative
  __device__ __forceinline__ float score(const int c) const {
    float num = 0.f;
#pragma unroll
    for (int lt = 0; lt < LT; ++lt)
#pragma unroll
      for (int r = 0; r < 16; ++r) num = fmaf(ew[c * LT + lt][r], dv[c * LT + lt][r], num);
    num = num + __shfl_xor(num, 32, 64);
    return num / den[c];
  }
};

// One step, candrow[] published: the K = A phase leaves the logits in 64 accumulator registers, they are turned into e_l in place
// (a padded token: logit -inf, weight exactly 0), the K = F phase fills the second 64.  All the step's barriers are in here; a wave
// that is not on computes nothing and leaves p undefined
template <int LT, class Args, class Rows>
__device__ __forceinline__ void npa_pooled(const Args& a, const NpaThread& th, float* Ts, float* Us, Rows candrow, int wave, int kl, int il,
                                           bool wave_on, NpaPooled<LT>& p) {
  constexpr int CPS = TK_TILES / LT;
  const int L = a.L;
  // token rows of this thread: a padded token points at the row's token 0 and is never loaded
  const float *pa[2], *pv[2];
  bool tok_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = candrow[th.tok_c[i]];
    tok_ok[i] = th.tok_l[i] < L;
    const int64_t tok = static_cast<int64_t>(r > 0 ? r : 0) * L + (tok_ok[i] ? th.tok_l[i] : 0);
    pa[i] = a.Ua + tok * a.A + th.sl.kq4;
    pv[i] = a.Vd + tok * a.F + th.sl.kq4;
  }
  // acc[j][r] = sum_k tokens[32 j + row(r, kl)][k] * users[32 wave + il][k]
  auto gemm = [&](const float* const(&ptok)[2], const float* const(&pusr)[2], const int K, f32x16(&acc)[TK_TILES]) {
    walk_zero(acc);
    walk_run(Ts, Us, th.sl, ptok, pusr, tok_ok, K, wave_on, [&](int buf) { walk_mma<false>(Ts, Us, buf, wave, kl, il, acc); });
  };
  gemm(pa, th.pq, a.A, p.ew);
#pragma unroll
  for (int c = 0; c < CPS; ++c) {
    if (!wave_on) {  // wave-uniform
      p.den[c] = 1.f;
      continue;
    }
    float m = -INFINITY;
#pragma unroll
    for (int lt = 0; lt < LT; ++lt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int l = lt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
        const float s = l < L ? p.ew[c * LT + lt][r] : -INFINITY;
        p.ew[c * LT + lt][r] = s;
        m = fmaxf(m, s);
      }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int lt = 0; lt < LT; ++lt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = expf(p.ew[c * LT + lt][r] - m);
        p.ew[c * LT + lt][r] = e;
        sum += e;
      }
    p.den[c] = sum + __shfl_xor(sum, 32, 64);
  }
  gemm(pv, th.pu, a.F, p.dv);
}

// ---- host.  The candidates are walked in units (a 128-candidate tile, an NPA step); n_splits ranges divide them.  Automatic: a
// few hundred workgroups (two per CU) when the users alone do not give them (n_splits == 0).  Never finer than one unit.  U, M >= 1
inline int walk_resolve_splits(int64_t U, int64_t M, int unit, int32_t n_splits) {
  const int64_t units = ebn_ceil_div(M, unit);
  int64_t s = n_splits > 0 ? n_splits : ebn_ceil_div(512, ebn_ceil_div(U, TK_BM));
  if (s > units) s = units;
  if (s > TK_MAX_SPLITS) s = TK_MAX_SPLITS;
  return static_cast<int>(s < 1 ? 1 : s);
}

inline int32_t walk_units_per_split(int64_t M, int unit, int splits) {
  return static_cast<int32_t>(ebn_ceil_div(ebn_ceil_div(M, unit), splits));
}

}  // namespace
