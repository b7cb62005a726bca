// The per-user sorted list of the fused score + top-k kernels (ebn_topk.hip: act(user . news); ebn_npa_topk.hip: NPA's personalised
// pooling): the LDS plan behind the operand images, the drain of a wave's survivor queue into the lists, the write-out, and the
// merge / fill launches.  Both kernels are 256 threads = four waves stacked along 128 users, so a user's list is only ever touched
// by ONE wave: no workgroup barrier and no atomics in here.
//
// The order is total -- score descending, then candidate position ascending -- so a list does not depend on the order in which
// survivors arrive, nor on how the candidates are split over workgroups; partial lists are merged in the same order.
#pragma once
#include "ebn_catalogue_walk.h"

namespace {

constexpr int TK_QCAP = 2 * TK_BN;     // capacity of a wave's survivor queue
constexpr int TK_MAX_K = 64, TK_MAX_X = 256;
constexpr int TK_EMPTY = INT32_MAX;    // position of an empty slot inside the kernels (sorts after every real candidate)

// what the list code needs of a call; the scoring kernels' argument blocks derive from it
struct TopkList {
  const int32_t* exclude;
  int32_t* out_pos;
  float* out_score;
  int32_t* flags;
  int32_t* part_pos;   // [n_splits, U, k] (n_splits > 1)
  float* part_score;
  int64_t U;
  int32_t X, k, mode, n_splits;
};

__device__ __forceinline__ float topk_act(float s, int mode) { return mode == 1 ? 1.0f / (1.0f + expf(-s)) : s; }

// (s0, p0) ranks strictly before (s1, p1)
__device__ __forceinline__ bool topk_before(float s0, int p0, float s1, int p1) { return s0 > s1 || (s0 == s1 && p0 < p1); }

// dynamic LDS layout (floats) behind the operand images: thr[128] | candrow[128] | queue score[4][256] | queue rowcol[4][256] | list
// score [128][k] | list pos [128][k]
struct TopkLds {
  float *As, *Bs;  // 2 buffers each
  volatile float* thr;
  volatile int* candrow;
  volatile float* qs;  // this wave's queue
  volatile int* qrc;
  volatile float* lsc;
  volatile int* lps;
};

__device__ __forceinline__ TopkLds topk_lds(float* smem, int wave, int k) {
  const WalkImages im = walk_images(smem);
  TopkLds l;
  l.As = im.As;
  l.Bs = im.Bs;
  l.thr = im.own;
  l.candrow = reinterpret_cast<volatile int*>(im.own + TK_BM);
  l.qs = im.own + TK_BM + TK_BN + wave * TK_QCAP;
  l.qrc = reinterpret_cast<volatile int*>(im.own + TK_BM + TK_BN + 4 * TK_QCAP) + wave * TK_QCAP;
  l.lsc = im.own + TK_BM + TK_BN + 8 * TK_QCAP;
  l.lps = reinterpret_cast<volatile int*>(im.own + TK_BM + TK_BN + 8 * TK_QCAP + TK_BM * k);
  return l;
}

inline int64_t topk_lds_bytes(int k) {
  return static_cast<int64_t>(TK_IMAGE_FLOATS + TK_BM + TK_BN + 8 * TK_QCAP + 2 * TK_BM * k) * 4;
}

// empty lists; the caller's next __syncthreads() publishes them
__device__ __forceinline__ void topk_list_init(const TopkLds& l, int k, int tid) {
  for (int i = tid; i < TK_BM * k; i += TK_THREADS) {
    l.lsc[i] = -INFINITY;
    l.lps[i] = TK_EMPTY;
  }
  if (tid < TK_BM) l.thr[tid] = -INFINITY;
}

// Drains the first cnt entries of this wave's queue -- score qs[i], qrc[i] = (user row of the tile << 8) | candidate column of the
// tile -- 64 at a time: each lane checks ITS entry (user / candidate in range, NaN, the current thr, the user's exclusion list), and
// what is left is inserted by the whole wave, one entry at a time: lane t holds slot t of the sorted list, the rank of the newcomer
// is a ballot popcount, the tail moves down by one lane.
__device__ __forceinline__ void topk_list_drain(const TopkList& a, const TopkLds& l, int cnt, int64_t u0, int64_t n0, int lane,
                                                bool& saw_nan) {
  const int k = a.k, X = a.X;
  for (int base = 0; base < cnt; base += 64) {
    const int idx = base + lane;
    bool ok = idx < cnt;
    const float s = ok ? l.qs[idx] : 0.f;
    const int rc = ok ? l.qrc[idx] : 0;
    const int erl = rc >> 8, ecol = rc & 255;
    const int64_t u = u0 + erl, c = n0 + ecol;
    const int crow = l.candrow[ecol];
    ok = ok && u < a.U && crow >= 0;
    if (ok && s != s) {
      saw_nan = true;
      ok = false;
    }
    ok = ok && !(s < l.thr[erl]);
    if (ok && X > 0) {
      const int32_t* ex = a.exclude + u * X;
      bool hit = false;
      for (int x = 0; x < X; ++x) hit |= ex[x] == crow;
      ok = !hit;
    }
    unsigned long long m = __ballot(ok);
    while (m != 0ull) {
      const int src = __builtin_ctzll(m);
      m &= m - 1ull;
      const float ns = __shfl(s, src, 64);
      const int nrl = __shfl(erl, src, 64);
      const int np = static_cast<int>(__shfl(static_cast<int>(c), src, 64));
      // the whole wave inserts (ns, np) into the list of row nrl: lane t holds slot t
      const bool in = lane < k;
      const float es = in ? l.lsc[nrl * k + lane] : 0.f;
      const int ep = in ? l.lps[nrl * k + lane] : 0;
      const int rank = __popcll(__ballot(in && topk_before(es, ep, ns, np)));
      const float us = __shfl_up(es, 1, 64);
      const int up = __shfl_up(ep, 1, 64);
      if (rank < k) {
        if (in && lane >= rank) {
          const float ws = lane == rank ? ns : us;
          l.lsc[nrl * k + lane] = ws;
          l.lps[nrl * k + lane] = lane == rank ? np : up;
          if (lane == k - 1) l.thr[nrl] = ws;
        }
      }
    }
  }
}

// ---- a wave-private list in REGISTERS (ebn_covisit_topk.hip, ebn_ease_topk.hip): lane t holds slot t of the sorted list of k <= 64
// entries; the same insertion as topk_list_drain's without the LDS round trip
// the whole wave inserts (ns, np) into its list: lane t holds slot t in (es, ep)
__device__ __forceinline__ void topk_wave_insert(float& es, int& ep, int k, int lane, float ns, int np) {
  const bool in = lane < k;
  const int rank = __popcll(__ballot(in && topk_before(es, ep, ns, np)));
  const float us = __shfl_up(es, 1, 64);
  const int up = __shfl_up(ep, 1, 64);
  if (in && lane >= rank) {  // rank == k: nobody
    es = lane == rank ? ns : us;
    ep = lane == rank ? np : up;
  }
}

// the lanes with ok offer (s, pos); what ranks before the list's k-th entry goes in
__device__ __forceinline__ void topk_wave_offer(float& es, int& ep, int k, int lane, bool ok, float s, int pos) {
  const float ks = __shfl(es, k - 1, 64);
  const int kp = __shfl(ep, k - 1, 64);
  unsigned long long m = __ballot(ok && topk_before(s, pos, ks, kp));
  while (m != 0ull) {
    const int src = __builtin_ctzll(m);
    m &= m - 1ull;
    topk_wave_insert(es, ep, k, lane, __shfl(s, src, 64), __shfl(pos, src, 64));
  }
}

// a wave writes the lists of its own 32 rows: lane t slot t; one split writes the outputs, more write their partial lists
__device__ __forceinline__ void topk_list_write(const TopkList& a, const TopkLds& l, int64_t u0, int split, int wave, int lane) {
  const int k = a.k;
  const bool direct = a.n_splits == 1;
  for (int rr = 0; rr < 32; ++rr) {
    const int rl = wave * 32 + rr;
    const int64_t u = u0 + rl;
    if (u >= a.U || lane >= k) continue;
    const float es = l.lsc[rl * k + lane];
    const int ep = l.lps[rl * k + lane];
    if (direct) {
      const bool empty = ep == TK_EMPTY;
      a.out_pos[u * k + lane] = empty ? -1 : ep;
      a.out_score[u * k + lane] = empty ? -INFINITY : topk_act(es, a.mode);
    } else {
      const int64_t o = (static_cast<int64_t>(split) * a.U + u) * k + lane;
      a.part_pos[o] = ep;
      a.part_score[o] = es;
    }
  }
}

// Merge of the n_splits (<= 64) sorted partial lists of a user: one wave per user, lane s holds the head of split s, k rounds of a
// wave-wide "first in the total order".  Positions of real candidates are distinct, so the winner is unique.
__global__ __launch_bounds__(256) void topk_merge_kernel(TopkList a) {
  const int lane = threadIdx.x & 63;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (u >= a.U) return;
  const int k = a.k;
  const bool has = lane < a.n_splits;
  const int64_t base = (static_cast<int64_t>(has ? lane : 0) * a.U + u) * k;
  int head = 0;
  for (int t = 0; t < k; ++t) {
    const bool live = has && head < k;
    const float s = live ? a.part_score[base + head] : -INFINITY;
    const int p = live ? a.part_pos[base + head] : TK_EMPTY;
    float bs = s;
    int bp = p;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float os = __shfl_xor(bs, off, 64);
      const int op = __shfl_xor(bp, off, 64);
      if (topk_before(os, op, bs, bp)) {
        bs = os;
        bp = op;
      }
    }
    const bool empty = bp == TK_EMPTY;
    if (!empty && live && p == bp) ++head;
    if (lane == 0) {
      a.out_pos[u * k + t] = empty ? -1 : bp;
      a.out_score[u * k + t] = empty ? -INFINITY : topk_act(bs, a.mode);
    }
  }
}

__global__ __launch_bounds__(256) void topk_fill_empty_kernel(int32_t* __restrict__ out_pos, float* __restrict__ out_score, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
    out_pos[i] = -1;
    out_score[i] = -INFINITY;
  }
}

// M == 0: every list empty
inline int topk_launch_fill_empty(int32_t* out_pos, float* out_score, int64_t U, int32_t k, hipStream_t s) {
  const int64_t n = U * k;
  const int64_t blocks = ebn_ceil_div(n, 256);
  EBN_LAUNCH(topk_fill_empty_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, out_pos, out_score, n);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

// the partial lists of splits > 1 ranges inside the caller's workspace ([splits, U, k] positions, then scores)
inline int topk_bind_workspace(TopkList& a, int splits, void* workspace, int64_t workspace_bytes) {
  a.part_pos = nullptr;
  a.part_score = nullptr;
  if (splits <= 1) return EBN_OK;
  const int64_t need = ebn_topk_workspace_bytes(a.U, a.k, splits);
  EBN_REQUIRE(workspace != nullptr && workspace_bytes >= need, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(ebn_aligned16(workspace), EBN_ERR_ALIGN);
  const int64_t n = static_cast<int64_t>(splits) * a.U * a.k;
  a.part_pos = static_cast<int32_t*>(workspace);
  a.part_score = reinterpret_cast<float*>(a.part_pos + n);
  return EBN_OK;
}

inline int topk_launch_merge(const TopkList& a, hipStream_t s) {
  EBN_LAUNCH(topk_merge_kernel, dim3(static_cast<unsigned>(ebn_ceil_div(a.U, 4))), dim3(256), 0, s, a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

}  // namespace
