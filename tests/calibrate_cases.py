"""Float64 restatement of the calibrated re-ranking of ebn_calibrated_rerank_f32 / ebn_label_target_f32 / calibrated_rerank() /
recommend(rerank=Calibrated(...)), and the case generators shared by tests/test_calibrate_cpu.py and tests/test_calibrate_gpu.py.
Independent of the product's host path.

The rule.  W [n_rows, C] >= 0 holds one label row per article.  Per user a pool of P entries (relevance rel[i], row row[i] of W).  An
entry is absent when its row is outside [0, n_rows) (-1 sets nothing, any other such row sets flag 0) or its relevance is not finite
(-inf sets nothing, NaN and +inf set flag 1).  The target p [C] is used as given; an entry that is negative or not finite counts as 0
and sets flag 1.  After the picks I, with S_c = sum over j in I of W[row_j, c], n = |I|, q~_c = (1 - alpha) S_c / n + alpha p_c and
KL(I) = sum over c with p_c > 0 of p_c log(p_c / q~_c), every round picks the present unpicked entry with the largest
obj_i = lam rel[i] - (1 - lam) KL(I + {i}); larger obj first, equal obj to the smaller pool index; k rounds or until nothing is left,
short lists padded with (-1, -inf).
History target: p_c = sum_h w_h W[hist_row_h, c] / sum_h w_h over the slots whose row lies in [0, n_rows) (-1 is silent, any other row
outside sets flag 0); no valid slot or a weight sum of 0 gives a zero row."""
import numpy as np

# (U, P, C, k, H): 1x1; k > P; on the 32 boundary; P and C off it; the largest k; the limits of C and H; C just past a wave
EXACT_SHAPES = [(1, 1, 1, 1, 1), (3, 3, 2, 10, 4), (5, 32, 3, 5, 20), (7, 33, 33, 10, 7), (130, 64, 64, 64, 50), (9, 64, 128, 10, 256),
                (6, 50, 65, 10, 20)]
EXACT_LAMS = [0.25, 0.5]
ROUNDED_SHAPES = [(64, 64, 64, 10, 20), (33, 50, 24, 5, 20), (64, 64, 128, 10, 50)]
ROUNDED_LAMS = [0.3, 0.7]
ALPHA = 0.01
E_LOG = 4  # ulp of logf: the HIP math documentation's table is not at hand, so 4 (it states fewer) -- see tolerance()


def shape_id(s):
    return "x".join(map(str, s))


def present_mask(rows, rel, n_rows):
    rows, rel = np.asarray(rows, dtype=np.int64), np.asarray(rel, dtype=np.float64)
    return (rows >= 0) & (rows < n_rows) & np.isfinite(rel)


def clean_target(target):
    """-> (float64 target with the negative and non-finite entries as 0, whether there was one)"""
    t = np.asarray(target, dtype=np.float64)
    bad = ~np.isfinite(t) | (t < 0)
    return np.where(bad, 0.0, t), bool(bad.any())


def kl_with_each(S, rows_w, p, n, alpha):
    """[P]: KL of the list (picks with label-row sum S) + {i}, n = its length with i counted, for every entry i"""
    pos = p > 0
    q = (1.0 - alpha) * (S[None, pos] + rows_w[:, pos]) / n + alpha * p[None, pos]
    return (p[pos] * np.log(p[pos] / q)).sum(1)


def pool_label_rows(W, rows, present):
    W = np.asarray(W, dtype=np.float64)
    return np.where(present[:, None], W[np.where(present, rows, 0)], 0.0)


def target_reference(W, hist_rows, weights=None):
    """W [n_rows, C], hist_rows [U, H], weights [H] or None -> (p [U, C] float64, flag 0)"""
    W = np.asarray(W, dtype=np.float64)
    hist_rows = np.asarray(hist_rows, dtype=np.int64)
    ok = (hist_rows >= 0) & (hist_rows < len(W))
    w = np.where(ok, 1.0 if weights is None else np.asarray(weights, dtype=np.float64)[None, :], 0.0)
    total = np.einsum("uh,uhc->uc", w, W[np.where(ok, hist_rows, 0)])
    wsum = w.sum(1, keepdims=True)
    return np.where(wsum > 0, total / np.where(wsum > 0, wsum, 1.0), 0.0), int((~ok & (hist_rows != -1)).any())


def calibrated_reference(W, rows, rel, target, k, lam, alpha=ALPHA, margins=False):
    """W [n_rows, C], rows [U, P] int, rel [U, P], target [U, C] or [C] -> sel [U, k] int32, obj [U, k] float64, flags (bad row,
    non-finite).  margins=True: also [U], the smallest lead over the rounds of the winner on the best entry left with ANOTHER
    label row (inf where there never was one)."""
    rows, rel = np.asarray(rows, dtype=np.int64), np.asarray(rel, dtype=np.float64)
    n_rows = len(W)
    U, P = rows.shape
    target, bad_target = clean_target(target)
    sel = np.full((U, k), -1, np.int32)
    out = np.full((U, k), -np.inf)
    lead = np.full(U, np.inf)
    in_range = (rows >= 0) & (rows < n_rows)
    flag0 = bool((~in_range & (rows != -1)).any())
    flag1 = bool((~np.isfinite(rel) & ~np.isneginf(rel)).any()) or bad_target
    lam = float(lam)
    for u in range(U):
        p = target[u] if target.ndim == 2 else target
        present = present_mask(rows[u], rel[u], n_rows)
        rows_w = pool_label_rows(W, rows[u], present)
        left = present.copy()
        S = np.zeros(len(p))
        for t in range(k):
            if not left.any():
                break
            obj = np.where(left, lam * np.where(left, rel[u], 0.0) - (1.0 - lam) * kl_with_each(S, rows_w, p, t + 1, alpha), -np.inf)
            best = int(np.argmax(obj))  # the first maximum: the smaller pool index
            sel[u, t], out[u, t] = best, obj[best]
            other = left & (rows_w != rows_w[best]).any(1)
            if other.any():
                lead[u] = min(lead[u], obj[best] - obj[other].max())
            left[best] = False
            S = S + rows_w[best]
    res = (sel, out, (int(flag0), int(flag1)))
    return res + (lead,) if margins else res


def tolerance(lam, C, k, alpha=ALPHA):
    """(1 - lam) B + 4 * 2^-23 for a recomputed objective, B = 2^-23 ((8 + k) + (E_LOG + 1 + C) (ln(1 / alpha) + ln max(C, 2))):
    8 + k ulp for the rounding of each q~_c argument (the k additions into S_c, the row added, 1 - alpha, the division by n, alpha p_c,
    the product and the sum: a relative error e of the argument moves the logarithm by e); E_LOG + 1 for logf and the product with
    p_c; C for the summation over the labels in any order; the last factor bounds sum |p_c log(p_c / q~_c)| since
    alpha p_c <= q~_c <= 1 and sum p_c <= 1: each term is at most p_c ln(1 / alpha) on one side and p_c ln(1 / p_c) on the other,
    and sum p_c ln(1 / p_c) <= ln C.  The 8 + k ulp enter through sum p_c <= 1.  The 4 ulp of a number below 4 cover lam and 1 - lam
    in fp32, the two products and their difference.  E_LOG = 4: the HIP math documentation's accuracy table for logf is not at
    hand; it states fewer ulp than that."""
    B = 2.0 ** -23 * ((8 + k) + (E_LOG + 1 + C) * (np.log(1.0 / alpha) + np.log(max(C, 2))))
    return (1.0 - lam) * B + 4 * 2.0 ** -23


def check_structure(W, rows, rel, sel, obj=None):
    """no repeats, no absent entry, the padding only once nothing is left (and then to the end, with -inf objectives)"""
    rows, rel = np.asarray(rows, dtype=np.int64), np.asarray(rel, dtype=np.float64)
    for u in range(rows.shape[0]):
        left = present_mask(rows[u], rel[u], len(W))
        for t, s in enumerate(np.asarray(sel[u]).tolist()):
            if s < 0:
                assert not left.any(), (u, t, "padding while entries are left")
                assert (np.asarray(sel[u][t:]) == -1).all() and (obj is None or np.isneginf(obj[u][t:]).all()), (u, t)
                break
            assert 0 <= s < rows.shape[1] and left[s], (u, t, s, "absent or repeated")
            left[s] = False


def check_greedy(W, rows, rel, target, sel, obj, lam, tol, alpha=ALPHA, users=None):
    """The greedy property of lists `sel` [U, k] (with objectives `obj`, or None): the structure above; every pick's float64
    objective, GIVEN the earlier picks of the list, within 2 tol of the best one left, and obj within tol of it.
    -> (largest shortfall against the best, largest |obj - float64|)."""
    rows, rel = np.asarray(rows, dtype=np.int64), np.asarray(rel, dtype=np.float64)
    target, _ = clean_target(target)
    check_structure(W, rows, rel, sel, obj)
    worst_gap, worst_obj = 0.0, 0.0
    for u in (range(rows.shape[0]) if users is None else users):
        p = target[u] if target.ndim == 2 else target
        present = present_mask(rows[u], rel[u], len(W))
        rows_w = pool_label_rows(W, rows[u], present)
        left = present.copy()
        S = np.zeros(len(p))
        for t, s in enumerate(np.asarray(sel[u]).tolist()):
            if s < 0:
                break
            o64 = lam * np.where(left, rel[u], 0.0) - (1.0 - lam) * kl_with_each(S, rows_w, p, t + 1, alpha)
            gap = float(o64[left].max() - o64[s])
            worst_gap = max(worst_gap, gap)
            assert gap <= 2 * tol, (u, t, s, gap, tol)
            if obj is not None:
                err = abs(float(obj[u][t]) - float(o64[s]))
                worst_obj = max(worst_obj, err)
                assert err <= tol, (u, t, s, err, tol)
            left[s] = False
            S = S + rows_w[s]
    return worst_gap, worst_obj


def relevance_order(W, rows, rel, k):
    """sel [U, k]: the present entries by descending relevance, equal relevance to the smaller pool index, -1 behind them"""
    rows, rel = np.asarray(rows, dtype=np.int64), np.asarray(rel, dtype=np.float64)
    sel = np.full((rows.shape[0], k), -1, np.int32)
    for u in range(rows.shape[0]):
        present = np.flatnonzero(present_mask(rows[u], rel[u], len(W)))
        want = present[np.argsort(-rel[u, present], kind="stable")][:k]
        sel[u, :len(want)] = want
    return sel


def label_table(n_rows, C, rng, multi=False):
    """float32 [n_rows, C]: one-hot rows, or (multi) one to three distinct labels of weight 1 / len with about 5 % zero rows"""
    W = np.zeros((n_rows, C), np.float32)
    if not multi:
        W[np.arange(n_rows), rng.integers(0, C, n_rows)] = 1.0
        return W
    for r in range(n_rows):
        if rng.random() < 0.05:
            continue
        labels = rng.choice(C, min(C, int(rng.integers(1, 4))), replace=False)
        W[r, labels] = np.float32(1.0 / len(labels))
    return W


def exact_case(U, P, C, H, seed, bad_row=False, nan_rel=False):
    """One-hot label rows over a table smaller than the pool (duplicates are frequent), relevances in multiples of 1/64 in [0, 1]
    (ties are frequent; with a dyadic lam every lam * rel is exact in fp32), an unsorted pool, about 10 % of the entries with row
    -1 (half of them with the padding's -inf relevance), user 1 (when there is one) all padding.  Histories [U, H] drawn from
    the table, about 10 % padding; user 2 (when there is one) has an empty history.  bad_row: one entry's row is n_rows
    (absent, flag 0); nan_rel: one entry's relevance is NaN (absent, flag 1).  -> W, rows, rel, hist"""
    rng = np.random.default_rng(seed)
    n_rows = max(3, (3 * P) // 4)
    W = label_table(n_rows, C, rng)
    rows = rng.integers(0, n_rows, (U, P)).astype(np.int32)
    rel = (rng.integers(0, 65, (U, P)) / 64.0).astype(np.float32)
    gone = rng.random((U, P)) < 0.1
    rows[gone] = -1
    rel[gone & (rng.random((U, P)) < 0.5)] = -np.inf
    hist = rng.integers(0, n_rows, (U, H)).astype(np.int32)
    hist[rng.random((U, H)) < 0.1] = -1
    if U > 1:
        rows[1], rel[1] = -1, -np.inf
    if U > 2:
        hist[2] = -1
    u, i = U - 1, P // 2
    if bad_row:
        rows[u, i] = n_rows
    if nan_rel:
        rel[u, (i + 1) % P] = np.nan
    return W, rows, rel, hist


def rounded_case(U, P, C, H, seed, multi=False):
    """Uniform relevances, histories and pools drawn from a table of 4 P rows (one-hot, or one to three labels per row), about
    10 % padding in the pools.  -> W, rows, rel, hist"""
    rng = np.random.default_rng(seed)
    n_rows = 4 * P
    W = label_table(n_rows, C, rng, multi)
    rows = rng.integers(0, n_rows, (U, P)).astype(np.int32)
    rel = rng.random((U, P)).astype(np.float32)
    gone = rng.random((U, P)) < 0.1
    rows[gone], rel[gone] = -1, -np.inf
    hist = rng.integers(0, n_rows, (U, H)).astype(np.int32)
    return W, rows, rel, hist


def dyadic_weights(H, rng):
    """[H] float32 weights in multiples of 1/4 whose sum is a power of two: every product, sum and the final division are exact"""
    w = rng.integers(1, 9, H) / 4.0
    total = w.sum() - w[-1]
    top = 2.0 ** np.ceil(np.log2(total + 0.25))
    w[-1] = top - total
    assert w[-1] > 0 and np.log2(w.sum()) % 1 == 0 and np.array_equal(w * 4, np.round(w * 4))
    return w.astype(np.float32)
