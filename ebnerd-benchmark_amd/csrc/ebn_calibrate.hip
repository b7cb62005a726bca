// Calibrated re-ranking of a relevance pool (Steck, "Calibrated Recommendations", RecSys 2018): greedily pick the list whose label
// distribution stays close, in KL divergence, to a target distribution -- what `Distribution` of the beyond-accuracy workflow measures
// (examples/beyond_accuracy/make_beyond_accuracy.ipynb: category, sentiment_label, topics), as MMR does for IntralistDiversity.
//
// Label table W [n_rows, C]: W[r, c] >= 0 is the share of label c in article r (one-hot, 1 / len over a list's labels, or a zero row).
// Per user: a pool of P <= 64 entries (rel[i], row[i]) and a target p [C].  With S_c the sum of the picked rows, n the number of picks,
//   q~_c = (1 - alpha) S_c / n + alpha p_c,    KL(I) = sum over c with p_c > 0 of p_c log(p_c / q~_c)
//   every round (round 0 too): the present, unpicked entry with the largest obj_i = lam rel[i] - (1 - lam) KL(I + {i});
//   larger obj first, equal obj to the smaller pool index.
//
// One wave per user, one user per workgroup: nothing is shared between users, so a user's bits depend on no other user.  Only the
// labels with p_c > 0 enter the KL, so the wave first compacts them (two ballots: label c becomes column j of the user's own list,
// in label order) and everything after works on those n_pos columns.  The pool's label rows are gathered ONCE into LDS -- the n_pos
// wanted columns of each row -- with row stride C | 1: in a round lane i walks its own row, and the 32 lanes of a ds_read_b32 group
// sit on 32 different banks (odd stride); the compacted target p and the running sums S are read at one address by all lanes (a
// broadcast).  The LDS is sized by the call (3 C + P (C | 1) floats, 33.8 KiB at the limits), so small label sets leave room for many
// waves per CU.  A round: each lane evaluates ITS OWN KL over the n_pos columns from S + its row -- a branch-free loop, the same
// instruction sequence in every lane, so two entries with the same label row get the same bits, and no incremental update whose
// cancellation would cost accuracy; then the wave-wide argmax of ebn_rerank.hip, and lanes j, j + 64 add the picked row to S.
// An absent entry's row is never turned into an address: its LDS row is zeros.
//
// ebn_label_target_f32 forms the history target p_c = sum_h w_h W[hist_row_h, c] / sum_h w_h the same way: one wave per user, lanes own
// labels c and c + 64, the history is walked in slot order (one fixed-order sum per label).
#include <math.h>

#include "ebn_common.h"

namespace {

constexpr int CAL_THREADS = 64;
constexpr int CAL_MAX_P = 64, CAL_MAX_K = 64, CAL_MAX_C = 128, CAL_MAX_H = 256;
constexpr int CAL_NONE = INT32_MAX;  // index of "no entry" in the argmax (sorts after every real entry)

struct CalArgs {
  const float* W;
  const int32_t* pool_rows;
  const float* pool_rel;
  const float* target;
  int32_t* out_sel;
  float* out_obj;
  int32_t* flags;
  int64_t n_rows, target_stride;
  int32_t C, P, k, ld;  // ld: row stride of the label rows in LDS, C | 1
  float lam, alpha;
};

__global__ __launch_bounds__(CAL_THREADS) void calibrated_rerank_kernel(CalArgs a) {
  extern __shared__ float cal_lds[];
  const int C = a.C, P = a.P, ld = a.ld;
  float* sp = cal_lds;                                      // [n_pos] the target's positive entries, in label order
  float* sS = cal_lds + C;                                  // [n_pos] sum of the picked label rows, the same columns
  int* scol = reinterpret_cast<int*>(cal_lds + 2 * C);      // [n_pos] the label of a column
  float* srows = cal_lds + 3 * C;                           // [P][ld] the pool's label rows (those columns), zeros for an absent entry

  const int lane = threadIdx.x;
  const int64_t u = blockIdx.x;

  // ---- the pool: lane i owns entry i
  int row = -1;
  float rel = -INFINITY;
  if (lane < P) {
    const int64_t r = a.pool_rows[u * P + lane];
    const float x = a.pool_rel[u * P + lane];
    const bool row_ok = r >= 0 && r < a.n_rows;
    const bool rel_ok = fabsf(x) < INFINITY;  // false for NaN
    if (!row_ok && r != -1) a.flags[0] = 1;
    if (!rel_ok && !(x == -INFINITY)) a.flags[1] = 1;
    if (row_ok && rel_ok) {
      row = static_cast<int>(r);
      rel = x;
    }
  }
  const bool present = row >= 0;

  // ---- the target (used as given, not renormalised): labels lane and lane + 64, compacted to the positive ones; S = 0
  const float* tgt = a.target + u * a.target_stride;
  const unsigned long long below = (1ull << lane) - 1ull;
  int n_pos = 0;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int c = lane + half * CAL_THREADS;
    float x = 0.0f;
    if (c < C) {
      x = tgt[c];
      const bool ok = x >= 0.0f && x < INFINITY;  // false for NaN
      if (!ok) {
        a.flags[1] = 1;
        x = 0.0f;
      }
    }
    const unsigned long long mask = __ballot(x > 0.0f);
    if (x > 0.0f) {
      const int j = n_pos + __popcll(mask & below);  // j <= c < C
      sp[j] = x;
      sS[j] = 0.0f;
      scol[j] = c;
    }
    n_pos += __popcll(mask);  // wave-uniform
  }
  __syncthreads();

  // ---- the label rows, once: the wanted columns of each pool row
  const int j0 = lane, j1 = lane + CAL_THREADS;
  const int col0 = j0 < n_pos ? scol[j0] : 0, col1 = j1 < n_pos ? scol[j1] : 0;
  for (int i = 0; i < P; ++i) {
    const int r = __shfl(row, i, 64);
    const float* src = a.W + static_cast<int64_t>(r >= 0 ? r : 0) * C;  // formed, never read when absent
    if (j0 < n_pos) srows[i * ld + j0] = r >= 0 ? src[col0] : 0.0f;
    if (j1 < n_pos) srows[i * ld + j1] = r >= 0 ? src[col1] : 0.0f;
  }
  __syncthreads();

  // ---- the greedy rounds
  const float* mine = srows + (lane < P ? lane : 0) * ld;
  const float lam = a.lam, oml = 1.0f - a.lam, alpha = a.alpha, oma = 1.0f - a.alpha;
  const int k = a.k;
  bool picked = false;
  int my_sel = -1;  // lane t keeps the pick of round t
  float my_obj = -INFINITY;
  for (int t = 0; t < k; ++t) {
    const bool cand = present && !picked;
    const float scale = oma / static_cast<float>(t + 1);  // (1 - alpha) / n with this round's pick counted
    float kl = 0.0f;
#pragma unroll 4
    for (int j = 0; j < n_pos; ++j) {  // in label order, one accumulator: the iterations' divisions and logarithms overlap
      const float pc = sp[j];
      const float q = (sS[j] + mine[j]) * scale + alpha * pc;
      kl += pc * logf(pc / q);
    }
    float obj = lam * rel - oml * kl;
    obj = obj == obj ? obj : -INFINITY;  // 0 * inf of an overflowed KL: last among the candidates, not unordered
    float bo = cand ? obj : -INFINITY;
    int bi = cand ? lane : CAL_NONE;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float oo = __shfl_xor(bo, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (oo > bo || (oo == bo && oi < bi)) {
        bo = oo;
        bi = oi;
      }
    }
    if (bi == CAL_NONE) break;  // nothing left: the list stays short (wave-uniform)
    if (lane == t) {
      my_sel = bi;
      my_obj = bo;
    }
    picked |= lane == bi;
    if (t + 1 < k) {
      __syncthreads();  // every lane is done with this round's S
      for (int j = lane; j < n_pos; j += CAL_THREADS) sS[j] += srows[bi * ld + j];
      __syncthreads();
    }
  }
  if (lane < k) {
    a.out_sel[u * k + lane] = my_sel;
    if (a.out_obj != nullptr) a.out_obj[u * k + lane] = my_obj;
  }
}

struct TargetArgs {
  const float* W;
  const int32_t* hist_rows;
  const float* hist_w;
  float* target;
  int32_t* flags;
  int64_t n_rows;
  int32_t C, H;
};

__global__ __launch_bounds__(CAL_THREADS) void label_target_kernel(TargetArgs a) {
  const int lane = threadIdx.x;
  const int64_t u = blockIdx.x;
  const int C = a.C, H = a.H;
  const int c0 = lane, c1 = lane + CAL_THREADS;
  const int32_t* hist = a.hist_rows + u * H;
  float acc0 = 0.0f, acc1 = 0.0f, wsum = 0.0f;
  bool bad = false;
  for (int h = 0; h < H; ++h) {  // slot order: one fixed-order sum per label
    const int64_t r = hist[h];
    const bool ok = r >= 0 && r < a.n_rows;
    bad |= !ok && r != -1;
    if (!ok) continue;  // wave-uniform; the row is never turned into an address
    const float w = a.hist_w != nullptr ? a.hist_w[h] : 1.0f;
    const float* src = a.W + r * C;
    if (c0 < C) acc0 += w * src[c0];
    if (c1 < C) acc1 += w * src[c1];
    wsum += w;
  }
  if (bad && lane == 0) a.flags[0] = 1;
  const bool any = wsum > 0.0f;  // no valid slot or a weight sum of 0: a zero row
  float* out = a.target + u * C;
  if (c0 < C) out[c0] = any ? acc0 / wsum : 0.0f;
  if (c1 < C) out[c1] = any ? acc1 / wsum : 0.0f;
}

}  // namespace

extern "C" int ebn_label_target_f32(const float* W, int64_t n_rows, int32_t C, const int32_t* hist_rows, int32_t H, const float* hist_w,
                                    float* target, int32_t* flags, int64_t U, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(U, n_rows), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(C >= 1 && C <= CAL_MAX_C && H >= 1 && H <= CAL_MAX_H, EBN_ERR_UNSUPPORTED);
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(hist_rows != nullptr && target != nullptr && flags != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(W != nullptr || n_rows == 0, EBN_ERR_BAD_ARG);
  TargetArgs a;
  a.W = W;
  a.hist_rows = hist_rows;
  a.hist_w = hist_w;
  a.target = target;
  a.flags = flags;
  a.n_rows = n_rows;
  a.C = C;
  a.H = H;
  // U <= 2^31 - 1: fits the grid's 32 bits
  EBN_LAUNCH(label_target_kernel, dim3(static_cast<unsigned>(U)), dim3(CAL_THREADS), 0, ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}

extern "C" int ebn_calibrated_rerank_f32(const float* W, int64_t n_rows, int32_t C, const int32_t* pool_rows, const float* pool_rel,
                                         int32_t P, const float* target, int64_t target_stride, int32_t k, float lam, float alpha,
                                         int32_t* out_sel, float* out_obj, int32_t* flags, int64_t U, ebn_stream_t stream) {
  EBN_REQUIRE(ebn_dim_ok(U, n_rows), EBN_ERR_BAD_ARG);
  EBN_REQUIRE(lam >= 0.0f && lam <= 1.0f, EBN_ERR_BAD_ARG);     // false for NaN
  EBN_REQUIRE(alpha > 0.0f && alpha < 1.0f, EBN_ERR_BAD_ARG);   // false for NaN
  EBN_REQUIRE(P >= 1 && P <= CAL_MAX_P && k >= 1 && k <= CAL_MAX_K && C >= 1 && C <= CAL_MAX_C, EBN_ERR_UNSUPPORTED);
  EBN_REQUIRE(target_stride == 0 || target_stride == C, EBN_ERR_BAD_ARG);
  if (U == 0) return EBN_OK;
  EBN_REQUIRE(pool_rows != nullptr && pool_rel != nullptr && target != nullptr && out_sel != nullptr && flags != nullptr, EBN_ERR_BAD_ARG);
  EBN_REQUIRE(W != nullptr || n_rows == 0, EBN_ERR_BAD_ARG);
  CalArgs a;
  a.W = W;
  a.pool_rows = pool_rows;
  a.pool_rel = pool_rel;
  a.target = target;
  a.out_sel = out_sel;
  a.out_obj = out_obj;
  a.flags = flags;
  a.n_rows = n_rows;
  a.target_stride = target_stride;
  a.C = C;
  a.P = P;
  a.k = k;
  a.ld = C | 1;
  a.lam = lam;
  a.alpha = alpha;
  const size_t lds_bytes = sizeof(float) * (3 * static_cast<size_t>(C) + static_cast<size_t>(P) * a.ld);  // at most 34 560
  // U <= 2^31 - 1: fits the grid's 32 bits
  EBN_LAUNCH(calibrated_rerank_kernel, dim3(static_cast<unsigned>(U)), dim3(CAL_THREADS), lds_bytes, ebn_stream(stream), a);
  EBN_CHECK_LAUNCH();
  return EBN_OK;
}
