// Per-impression ranking metrics over ragged lists (reference: evaluation/metrics_protocols.py, metrics/_ranking.py, metrics/_sklearn.py):
// auc, mrr, ndcg@k, logloss, rmse, accuracy, f1 of every list in ONE pass over (scores, labels, offsets), and the ranks of
// rank_predictions_by_score (utils/_python.py).  Every kernel is "a rank per candidate by counting, a few segmented sums":
//   * rank_i = 1 + #{j : s_j > s_i} + #{j < i : s_j == s_i}; scores are compared in the type given (fp32 or fp64), all other
//     arithmetic is fp64.  The host sorts with an unstable argsort, so the order INSIDE a tie group is its own: a list in which two
//     equal scores carry different labels (the only case where mrr / ndcg depend on that order) is flagged and left to the host;
//   * one workgroup owns RM_LPB consecutive lists and takes each in the cheapest form its length allows: up to 16 candidates in a
//     16-lane group (four lists per wave, cross-lane shuffles of that width), up to 64 in one wave, longer ones with the whole
//     workgroup over an LDS copy of the list (up to RM_TILE candidates) or over RM_TILE-sized tiles re-read from global memory;
//   * sums are taken in a fixed order -- lane tree, the leader's running sum in LDS, the 16 leaders of a workgroup, then a closing
//     launch over the workgroups' partials -- and never with floating-point atomics: two runs give the same bits.
#include "ebn_common.h"

#define RM_LPB 256    // lists per workgroup
#define RM_TILE 1024  // candidates of one list kept in LDS
#define RM_TBL 256    // ranks whose ndcg discount 1 / log2(rank + 1) is tabulated per workgroup
#define RM_ROWS 16    // leaders per workgroup: one per 16-lane group

struct RmPair {
  int gt, eqb, eqd, ltn;  // s_j > s_i;  s_j == s_i, j < i;  s_j == s_i, y_j != y_i;  y_j == 0, s_j < s_i
};

template <typename T>
static __device__ __forceinline__ void rm_pair(RmPair& p, T si, int yi, bool before, T sj, int yj) {
  const bool eq = sj == si;
  p.gt += sj > si;
  p.eqb += eq && before;
  p.eqd += eq && (yj != yi);
  p.ltn += (yj == 0) && (sj < si);
}

template <typename T>
struct RmSmem {
  int beg[RM_LPB], len[RM_LPB];
  double inv_log2[RM_TBL + 1];
  double red[RM_ROWS][2][EBN_RM_MAX_SLOTS];  // a list's slot sums, at its leader's row
  double acc[RM_ROWS][EBN_RM_MAX_SLOTS];     // the leader's running sum over its lists
  long long cnt[RM_ROWS][3];
  long long redi[4][3];
  unsigned long long mask[3][4];  // per wave of list numbers: group form, wave form, workgroup form
  int kind[EBN_RM_MAX_SLOTS];
  double param[EBN_RM_MAX_SLOTS];
  T ts[RM_TILE];
  uint8_t ty[RM_TILE];
};

template <int GW>
static __device__ __forceinline__ double rm_group_sum(double v) {
#pragma unroll
  for (int off = GW / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <int GW>
static __device__ __forceinline__ int rm_group_sum_i(int v) {
#pragma unroll
  for (int off = GW / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
static __device__ __forceinline__ long long rm_wave_sum_ll(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

static __device__ __forceinline__ double rm_discount(const double* tbl, int64_t rank) {
  return rank <= RM_TBL ? tbl[rank] : 1.0 / log2(static_cast<double>(rank) + 1.0);
}
static __device__ __forceinline__ int64_t rm_k(double param) { return static_cast<int64_t>(fmin(fmax(param, 0.0), 4e18)); }

// what one candidate adds to a slot's list sums
static __device__ __forceinline__ void rm_contrib(int kind, double param, bool valid, double s, int y, int64_t rank, int64_t n, int64_t w2,
                                                  const double* tbl, double& c0, double& c1) {
  c0 = 0.0, c1 = 0.0;
  if (!valid) return;
  switch (kind) {
    case EBN_RM_AUC: c0 = y ? static_cast<double>(w2) : 0.0; break;
    case EBN_RM_MRR: c0 = y ? 1.0 / static_cast<double>(rank) : 0.0; break;
    case EBN_RM_NDCG: {
      const int64_t k = rm_k(param);
      if (y && rank <= (k < n ? k : n)) c0 = rm_discount(tbl, rank);
    } break;
    case EBN_RM_LOGLOSS: {
      const double p = fmax(fmin(s, 1.0 - 10e-12), 10e-12);
      c0 = y ? log(p) : log(1.0 - p);
    } break;
    case EBN_RM_RMSE: {
      const double d = static_cast<double>(y) - s;
      c0 = d * d;
    } break;
    case EBN_RM_ACCURACY: c0 = ((s >= param) == (y != 0)) ? 1.0 : 0.0; break;
    case EBN_RM_F1: {
      const bool pred = s >= param;
      c0 = (pred && y) ? 1.0 : 0.0;
      c1 = (pred != (y != 0)) ? 1.0 : 0.0;
    } break;
    default: break;
  }
}

// a slot's value of one list from its sums
static __device__ __forceinline__ double rm_value(int kind, double param, double s0, double s1, int64_t n, int64_t np, const double* tbl) {
  const double nan = __builtin_nan("");
  const double dn = static_cast<double>(n), dp = static_cast<double>(np);
  switch (kind) {
    case EBN_RM_AUC: return (np > 0 && np < n) ? s0 / (2.0 * dp * (dn - dp)) : nan;
    case EBN_RM_MRR: return np > 0 ? s0 / dp : nan;
    case EBN_RM_NDCG: {
      int64_t m = rm_k(param);
      m = m < n ? m : n;
      m = m < np ? m : np;
      double ideal = 0.0;
      for (int64_t r = 1; r <= m; ++r) ideal += rm_discount(tbl, r);
      return s0 / ideal;  // no positive: 0 / 0
    }
    case EBN_RM_LOGLOSS: return (np > 0 && np < n) ? -(s0 / dn) : nan;
    case EBN_RM_RMSE: return sqrt(s0 / dn);
    case EBN_RM_ACCURACY: return s0 / dn;
    case EBN_RM_F1: {
      const double den = 2.0 * s0 + s1;
      return den == 0.0 ? 0.0 : 2.0 * s0 / den;
    }
    default: return nan;
  }
}

// the leader's closing step for list l: flags, counters, per-list values, running sums.  sm.red[row] holds the list's slot sums.
template <typename T>
static __device__ void rm_finish_list(RmSmem<T>& sm, int row, int64_t l, int64_t n_lists, int n_slots, int64_t n, int64_t np, bool tie, bool nonf,
                                      uint8_t* __restrict__ flags, double* __restrict__ per_list) {
  flags[l] = static_cast<uint8_t>((tie ? 1 : 0) | (nonf ? 2 : 0));
  const bool one = !(np > 0 && np < n);
  sm.cnt[row][0] += one, sm.cnt[row][1] += tie, sm.cnt[row][2] += nonf;
  for (int m = 0; m < n_slots; ++m) {
    const int kind = sm.kind[m];
    const double v = rm_value(kind, sm.param[m], sm.red[row][0][m], sm.red[row][1][m], n, np, sm.inv_log2);
    if (per_list != nullptr) per_list[static_cast<int64_t>(m) * n_lists + l] = v;
    const bool ranked = kind == EBN_RM_MRR || kind == EBN_RM_NDCG, two_class = kind == EBN_RM_AUC || kind == EBN_RM_LOGLOSS;
    if (!nonf && !(tie && ranked) && !(one && two_class)) sm.acc[row][m] += v;
  }
}

// After the pair counts of a list that sits in ONE group of GW lanes (one candidate per lane): ranks, or slot sums and the closing step.
// Every lane of the wave calls it; `mine` = this group holds a list, `leader` = its first lane.
template <typename T, bool RANKS, int GW>
static __device__ __forceinline__ void rm_group_close(RmSmem<T>& sm, int row, bool leader, bool mine, bool valid, T s, int y, const RmPair& p,
                                                      int beg, int pos, int n, int64_t l, int64_t n_lists, int n_slots,
                                                      uint8_t* __restrict__ flags, double* __restrict__ per_list, int32_t* __restrict__ ranks) {
  const bool nonf1 = valid && !isfinite(s);
  const bool tie1 = valid && (RANKS ? p.eqb > 0 : p.eqd > 0);
  const int packed = rm_group_sum_i<GW>(((valid && y) ? 1 : 0) | (tie1 ? 1 << 8 : 0) | (nonf1 ? 1 << 16 : 0));  // each count <= 64
  const int np = packed & 255;
  const bool tie = ((packed >> 8) & 255) != 0, nonf = (packed >> 16) != 0;
  const int64_t rank = 1 + static_cast<int64_t>(p.gt) + p.eqb;
  if (RANKS) {
    if (valid) ranks[beg + pos] = (tie || nonf) ? 0 : static_cast<int32_t>(rank);
    if (leader && mine) flags[l] = static_cast<uint8_t>((tie ? 1 : 0) | (nonf ? 2 : 0));
    return;
  }
  for (int m = 0; m < n_slots; ++m) {
    const int kind = sm.kind[m];
    double c0, c1;
    rm_contrib(kind, sm.param[m], valid, static_cast<double>(s), y, rank, n, 2 * static_cast<int64_t>(p.ltn) + p.eqd, sm.inv_log2, c0, c1);
    c0 = rm_group_sum<GW>(c0);
    if (kind == EBN_RM_F1) c1 = rm_group_sum<GW>(c1);
    if (leader) sm.red[row][0][m] = c0, sm.red[row][1][m] = c1;
  }
  if (leader && mine) rm_finish_list(sm, row, l, n_lists, n_slots, n, np, tie, nonf, flags, per_list);
}

// One list with the whole workgroup: candidate i0 + t per thread, every j from LDS -- the whole list when it fits there (resident),
// otherwise tile by tile, re-read from global memory for every 256 candidates.
template <typename T, bool RANKS>
static __device__ void rm_block_list(RmSmem<T>& sm, const T* __restrict__ scores, const uint8_t* __restrict__ labels, int beg, int n, bool resident,
                                     int64_t l, int64_t n_lists, int n_slots, uint8_t* __restrict__ flags, double* __restrict__ per_list,
                                     int32_t* __restrict__ ranks) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, row = wave * 4;
  if (!RANKS && lane == 0)
    for (int m = 0; m < n_slots; ++m) sm.red[row][0][m] = 0.0, sm.red[row][1][m] = 0.0;
  long long npT = 0, tieT = 0, nonfT = 0;
  if (resident) {
    for (int j = t; j < n; j += 256) sm.ts[j] = scores[beg + j], sm.ty[j] = RANKS ? 0 : (labels[beg + j] != 0);
    __syncthreads();
  }
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + t;  // n <= INT32_MAX - 256 is checked by the entry point
    const bool valid = i < n;
    T s = 0;
    int y = 0;
    if (valid) {
      s = scores[beg + i];
      if (!RANKS) y = labels[beg + i] != 0;
    }
    RmPair p = {0, 0, 0, 0};
    if (resident) {
      for (int j = 0; j < n; ++j) rm_pair(p, s, y, j < i, sm.ts[j], static_cast<int>(sm.ty[j]));
    } else {
      for (int j0 = 0; j0 < n; j0 += RM_TILE) {
        const int tn = n - j0 < RM_TILE ? n - j0 : RM_TILE;
        __syncthreads();
        for (int j = t; j < tn; j += 256) sm.ts[j] = scores[beg + j0 + j], sm.ty[j] = RANKS ? 0 : (labels[beg + j0 + j] != 0);
        __syncthreads();
        for (int j = 0; j < tn; ++j) rm_pair(p, s, y, j0 + j < i, sm.ts[j], static_cast<int>(sm.ty[j]));
      }
    }
    npT += valid && y;
    tieT += valid && (RANKS ? p.eqb > 0 : p.eqd > 0);
    nonfT += valid && !isfinite(s);
    const int64_t rank = 1 + static_cast<int64_t>(p.gt) + p.eqb;
    if (RANKS) {
      if (valid) ranks[beg + i] = static_cast<int32_t>(rank);
    } else {
      for (int m = 0; m < n_slots; ++m) {
        const int kind = sm.kind[m];
        double c0, c1;
        rm_contrib(kind, sm.param[m], valid, static_cast<double>(s), y, rank, n, 2 * static_cast<int64_t>(p.ltn) + p.eqd, sm.inv_log2, c0, c1);
        c0 = rm_group_sum<64>(c0);
        if (kind == EBN_RM_F1) c1 = rm_group_sum<64>(c1);
        if (lane == 0) sm.red[row][0][m] += c0, sm.red[row][1][m] += c1;
      }
    }
  }
  npT = rm_wave_sum_ll(npT), tieT = rm_wave_sum_ll(tieT), nonfT = rm_wave_sum_ll(nonfT);
  if (lane == 0) sm.redi[wave][0] = npT, sm.redi[wave][1] = tieT, sm.redi[wave][2] = nonfT;
  __syncthreads();
  const long long np = (sm.redi[0][0] + sm.redi[1][0]) + (sm.redi[2][0] + sm.redi[3][0]);
  const bool tie = ((sm.redi[0][1] + sm.redi[1][1]) + (sm.redi[2][1] + sm.redi[3][1])) != 0;
  const bool nonf = ((sm.redi[0][2] + sm.redi[1][2]) + (sm.redi[2][2] + sm.redi[3][2])) != 0;
  if (RANKS) {
    if (tie || nonf)
      for (int i = t; i < n; i += 256) ranks[beg + i] = 0;
    if (t == 0) flags[l] = static_cast<uint8_t>((tie ? 1 : 0) | (nonf ? 2 : 0));
  } else if (t == 0) {
    for (int m = 0; m < n_slots; ++m)
      for (int h = 0; h < 2; ++h) sm.red[0][h][m] = (sm.red[0][h][m] + sm.red[4][h][m]) + (sm.red[8][h][m] + sm.red[12][h][m]);
    rm_finish_list(sm, 0, l, n_lists, n_slots, n, np, tie, nonf, flags, per_list);
  }
  __syncthreads();  // sm.ts, sm.red and sm.redi are free for the next list
}

template <typename T, bool RANKS>
static __global__ __launch_bounds__(256) void rm_lists_kernel(const T* __restrict__ scores, const uint8_t* __restrict__ labels, int64_t n_items,
                                                              const int64_t* __restrict__ offsets, int64_t n_lists,
                                                              const int32_t* __restrict__ slot_kind, const double* __restrict__ slot_param,
                                                              int n_slots, int form, uint8_t* __restrict__ flags, double* __restrict__ per_list,
                                                              int32_t* __restrict__ ranks, double* __restrict__ part_sums,
                                                              long long* __restrict__ part_cnt) {
  __shared__ RmSmem<T> sm;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * RM_LPB;
  {
    const int64_t l = base + t;
    int beg = 0, len = 0, cls = 3;
    if (l < n_lists) {
      const int64_t o0 = offsets[l], o1 = offsets[l + 1];
      if (o0 >= 0 && o1 >= o0 && o1 <= n_items) beg = static_cast<int>(o0), len = static_cast<int>(o1 - o0);  // n_items <= INT32_MAX
      cls = form == 1 ? 2 : (len <= 16 ? 0 : (len <= 64 ? 1 : 2));
    }
    sm.beg[t] = beg, sm.len[t] = len;
    const unsigned long long m0 = __ballot(cls == 0), m1 = __ballot(cls == 1), m2 = __ballot(cls == 2);
    if (lane == 0) sm.mask[0][wave] = m0, sm.mask[1][wave] = m1, sm.mask[2][wave] = m2;
    if (!RANKS) {
      if (t < EBN_RM_MAX_SLOTS) sm.kind[t] = t < n_slots ? slot_kind[t] : -1, sm.param[t] = t < n_slots ? slot_param[t] : 0.0;
      sm.acc[t >> 4][t & 15] = 0.0;
      if (t < RM_ROWS * 3) sm.cnt[t / 3][t % 3] = 0;
      sm.inv_log2[t + 1] = 1.0 / log2(static_cast<double>(t) + 2.0);
      if (t == 0) sm.inv_log2[0] = 0.0;
    }
  }
  __syncthreads();

  // up to 16 candidates: four lists per wave, one per 16-lane group
  {
    const int g = t >> 4, gl = lane & 15, gbase = lane & 48;
    for (int it = 0; it < RM_LPB / RM_ROWS; ++it) {
      if ((sm.mask[0][it >> 2] >> ((it & 3) * 16) & 0xFFFFull) == 0) continue;  // none of these 16 lists takes this form (uniform)
      const int li = it * RM_ROWS + g;
      const bool mine = (sm.mask[0][li >> 6] >> (li & 63)) & 1;
      const int len = mine ? sm.len[li] : 0, beg = sm.beg[li];
      const bool valid = gl < len;
      T s = 0;
      int y = 0;
      if (valid) {
        s = scores[beg + gl];
        if (!RANKS) y = labels[beg + gl] != 0;
      }
      const unsigned long long ym = __ballot(y);
      RmPair p = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const T sj = __shfl(s, gbase + j, 64);
        if (j < len) rm_pair(p, s, y, j < gl, sj, static_cast<int>((ym >> (gbase + j)) & 1));
      }
      rm_group_close<T, RANKS, 16>(sm, g, gl == 0, mine, valid, s, y, p, beg, gl, len, base + li, n_lists, n_slots, flags, per_list, ranks);
    }
  }
  // 17 to 64 candidates: one wave per list
  for (unsigned long long m1 = sm.mask[1][wave]; m1 != 0; m1 &= m1 - 1) {
    const int li = wave * 64 + __builtin_ctzll(m1);
    const int len = sm.len[li], beg = sm.beg[li];
    const bool valid = lane < len;
    T s = 0;
    int y = 0;
    if (valid) {
      s = scores[beg + lane];
      if (!RANKS) y = labels[beg + lane] != 0;
    }
    const unsigned long long ym = __ballot(y);
    RmPair p = {0, 0, 0, 0};
    for (int j = 0; j < len; ++j) {
      const T sj = __shfl(s, j, 64);
      rm_pair(p, s, y, j < lane, sj, static_cast<int>((ym >> j) & 1));
    }
    rm_group_close<T, RANKS, 64>(sm, wave * 4, lane == 0, true, valid, s, y, p, beg, lane, len, base + li, n_lists, n_slots, flags, per_list, ranks);
  }
  // longer lists (form 1: every list): the whole workgroup
  __syncthreads();
  for (int w = 0; w < 4; ++w)
    for (unsigned long long m2 = sm.mask[2][w]; m2 != 0; m2 &= m2 - 1) {
      const int li = w * 64 + __builtin_ctzll(m2);
      const int len = sm.len[li];
      rm_block_list<T, RANKS>(sm, scores, labels, sm.beg[li], len, form == 0 && len <= RM_TILE, base + li, n_lists, n_slots, flags, per_list, ranks);
    }
  if (RANKS) return;
  __syncthreads();
  if (t < EBN_RM_MAX_SLOTS) {
    double a = 0.0;
    for (int r = 0; r < RM_ROWS; ++r) a += sm.acc[r][t];
    part_sums[static_cast<int64_t>(blockIdx.x) * EBN_RM_MAX_SLOTS + t] = a;
  } else if (t >= 64 && t < 67) {
    long long c = 0;
    for (int r = 0; r < RM_ROWS; ++r) c += sm.cnt[r][t - 64];
    part_cnt[static_cast<int64_t>(blockIdx.x) * 3 + (t - 64)] = c;
  }
}

// closing pass: slot t / 16 by 16 lanes, each over the workgroups b = t % 16, t % 16 + 16, ... in ascending order, then a lane tree
static __global__ __launch_bounds__(256) void rm_close_kernel(const double* __restrict__ part_sums, const long long* __restrict__ part_cnt,
                                                              int64_t n_blocks, int n_slots, double* __restrict__ sums,
                                                              int64_t* __restrict__ counters) {
  const int slot = threadIdx.x >> 4, sub = threadIdx.x & 15;
  double a = 0.0;
  long long c = 0;
  for (int64_t b = sub; b < n_blocks; b += 16) {
    a += part_sums[b * EBN_RM_MAX_SLOTS + slot];
    if (slot < 3) c += part_cnt[b * 3 + slot];
  }
  a = rm_group_sum<16>(a);
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if (sub == 0 && slot < n_slots) sums[slot] = a;
  if (sub == 0 && slot < 3) counters[slot] = c;
}

// ---- entry points ------------------------------------------------------------------------------------------------------------
static inline int64_t rm_blocks(int64_t n_lists) { return ebn_ceil_div(n_lists, RM_LPB); }
static inline int64_t rm_sums_bytes(int64_t blocks) { return blocks * EBN_RM_MAX_SLOTS * static_cast<int64_t>(sizeof(double)); }

extern "C" int64_t ebn_rank_metrics_workspace_bytes(int64_t n_lists) {
  if (!ebn_dim_ok(n_lists)) return 0;
  const int64_t blocks = rm_blocks(n_lists);
  return rm_sums_bytes(blocks) + blocks * 3 * static_cast<int64_t>(sizeof(long long));
}

// candidates are addressed with 32-bit positions inside a list; the workgroup form steps past the end by up to 255
static inline bool rm_sizes_ok(int64_t n_items, int64_t n_lists) { return ebn_dim_ok(n_items, n_lists) && n_items <= EBN_DIM_MAX - 256; }

extern "C" int ebn_rank_metrics(const void* scores, int32_t score_kind, const uint8_t* labels, int64_t n_items, const int64_t* offsets,
                                int64_t n_lists, const int32_t* slot_kind, const double* slot_param, int32_t n_slots, int32_t form, double* sums,
                                uint8_t* flags, int64_t* counters, double* per_list, void* workspace, int64_t workspace_bytes,
                                ebn_stream_t stream) {
  EBN_REQUIRE(rm_sizes_ok(n_items, n_lists) && n_slots >= 0 && n_slots <= EBN_RM_MAX_SLOTS && (form == 0 || form == 1) &&
                  (score_kind == EBN_RM_F32 || score_kind == EBN_RM_F64),
              EBN_ERR_BAD_ARG);
  if (n_lists == 0) return EBN_OK;
  EBN_REQUIRE(offsets != nullptr && flags != nullptr && counters != nullptr && workspace != nullptr &&
                  ((scores != nullptr && labels != nullptr) || n_items == 0) &&
                  ((slot_kind != nullptr && slot_param != nullptr && sums != nullptr) || n_slots == 0),
              EBN_ERR_BAD_ARG);
  EBN_REQUIRE(workspace_bytes >= ebn_rank_metrics_workspace_bytes(n_lists) && ebn_aligned16(workspace), EBN_ERR_BAD_ARG);
  const int64_t blocks = rm_blocks(n_lists);
  double* part_sums = static_cast<double*>(workspace);
  long long* part_cnt = reinterpret_cast<long long*>(static_cast<char*>(workspace) + rm_sums_bytes(blocks));
  hipStream_t s = ebn_stream(stream);
  if (score_kind == EBN_RM_F32)
    EBN_LAUNCH((rm_lists_kernel<float, false>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, static_cast<const float*>(scores), labels,
               n_items, offsets, n_lists, slot_kind, slot_param, n_slots, form, flags, per_list, nullptr, part_sums, part_cnt);
  else
    EBN_LAUNCH((rm_lists_kernel<double, false>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, static_cast<const double*>(scores), labels,
               n_items, offsets, n_lists, slot_kind, slot_param, n_slots, form, flags, per_list, nullptr, part_sums, part_cnt);
  EBN_CHECK_LAUNCH();
  EBN_LAUNCH(rm_close_kernel, dim3(1), dim3(256), 0, s, part_sums, part_cnt, blocks, n_slots, sums, counters);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_list_ranks(const void* scores, int32_t score_kind, int64_t n_items, const int64_t* offsets, int64_t n_lists, int32_t form,
                              int32_t* ranks, uint8_t* flags, ebn_stream_t stream) {
  EBN_REQUIRE(rm_sizes_ok(n_items, n_lists) && (form == 0 || form == 1) && (score_kind == EBN_RM_F32 || score_kind == EBN_RM_F64),
              EBN_ERR_BAD_ARG);
  if (n_lists == 0) return EBN_OK;
  EBN_REQUIRE(offsets != nullptr && flags != nullptr && ((scores != nullptr && ranks != nullptr) || n_items == 0), EBN_ERR_BAD_ARG);
  const int64_t blocks = rm_blocks(n_lists);
  hipStream_t s = ebn_stream(stream);
  if (score_kind == EBN_RM_F32)
    EBN_LAUNCH((rm_lists_kernel<float, true>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, static_cast<const float*>(scores), nullptr,
               n_items, offsets, n_lists, nullptr, nullptr, 0, form, flags, nullptr, ranks, nullptr, nullptr);
  else
    EBN_LAUNCH((rm_lists_kernel<double, true>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, static_cast<const double*>(scores), nullptr,
               n_items, offsets, n_lists, nullptr, nullptr, 0, form, flags, nullptr, ranks, nullptr, nullptr);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
