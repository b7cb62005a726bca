"""Float64 restatement of the greedy MMR selection of ebn_mmr_rerank_f32 / mmr_rerank() / recommend(rerank=MMR(...)), and the
case generators shared by tests/test_rerank_cpu.py and tests/test_rerank_gpu.py.  Independent of the product's host path.

The rule.  Per user a pool of P entries (relevance rel[i], row row[i] of unit [n_rows, D]).  An entry is absent when its row is
outside [0, n_rows) (-1 sets nothing, any other such row sets flag 0) or its relevance is not finite (-inf sets nothing, NaN and
+inf set flag 1).  d(i, j) = min(max(1 - u_i . u_j, 0), 2), a NaN dot product between two present entries gives 0 and sets flag 1.
Round 0 picks the present entry with the largest rel (obj = rel), round t >= 1 the present unpicked entry with the largest
obj_i = lam rel[i] + (1 - lam) min over picked j of d(i, j); larger obj first, equal obj to the smaller pool index; k rounds or
until nothing is left, short lists padded with (-1, -inf)."""
import numpy as np

# (U, P, D, k): 1x1, k > P, on the 32-tile, off the 32-tile and off a 16-deep slab, two workgroup forms with the largest k, the real width
EXACT_SHAPES = [(1, 1, 4, 1), (3, 3, 4, 10), (5, 32, 16, 5), (7, 33, 36, 10), (130, 64, 64, 64), (9, 64, 768, 10)]
EXACT_LAMS = [0.0, 0.25, 0.5, 1.0]
ROUNDED_SHAPES = [(64, 64, 768, 10), (33, 50, 36, 5)]
ROUNDED_LAMS = [0.3, 0.7]


def present_mask(rows, rel, n_rows):
    rows, rel = np.asarray(rows, dtype=np.int64), np.asarray(rel, dtype=np.float64)
    return (rows >= 0) & (rows < n_rows) & np.isfinite(rel)


def distances64(unit, rows, present):
    """float64 [P, P] distances of one pool (absent entries: zero vectors, never looked at) and whether a present pair's dot is NaN"""
    unit = np.asarray(unit, dtype=np.float64)
    vec = np.where(present[:, None], unit[np.where(present, rows, 0)], 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        dots = vec @ vec.T
    pair = present[:, None] & present[None, :] & ~np.eye(len(rows), dtype=bool)
    nan = np.isnan(dots)
    dist = np.where(nan, 0.0, np.minimum(np.maximum(1.0 - np.where(nan, 0.0, dots), 0.0), 2.0))
    return dist, bool((nan & pair).any())


def mmr_reference(unit, rows, rel, k, lam):
    """unit [n_rows, D], rows [U, P] int, rel [U, P] -> sel [U, k] int32, obj [U, k] float64, flags (bad row, non-finite)"""
    rows, rel = np.asarray(rows, dtype=np.int64), np.asarray(rel, dtype=np.float64)
    n_rows = len(unit)
    U, P = rows.shape
    sel = np.full((U, k), -1, np.int32)
    out = np.full((U, k), -np.inf)
    in_range = (rows >= 0) & (rows < n_rows)
    flag0 = bool((~in_range & (rows != -1)).any())
    flag1 = bool((~np.isfinite(rel) & ~np.isneginf(rel)).any())
    lam = float(lam)
    for u in range(U):
        present = present_mask(rows[u], rel[u], n_rows)
        dist, nan_seen = distances64(unit, rows[u], present)
        flag1 |= nan_seen
        left = present.copy()
        mind = np.full(P, np.inf)
        for t in range(k):
            if not left.any():
                break
            obj = np.where(left, rel[u] if t == 0 else lam * np.where(left, rel[u], 0.0) + (1.0 - lam) * mind, -np.inf)
            best = int(np.argmax(obj))  # the first maximum: the smaller pool index
            sel[u, t], out[u, t] = best, obj[best]
            left[best] = False
            mind = np.minimum(mind, dist[best])
    return sel, out, (int(flag0), int(flag1))


def exact_case(U, P, D, seed, bad_row=False, nan_rel=False):
    """Table entries in {0, +-0.25, +-0.5}, about 6 sqrt(D) non-zeros per row (all of them below D = 36): every product is a
    multiple of 1/16, |dot| <= D / 4 <= 192, so a dot product is a 12-bit dyadic rational, exact in fp32 in any order with or
    without fma; two rows overlap in about 36 places, so 1 - dot leaves [0, 2] on both sides at large D (and a duplicate row's
    distance is clipped to 0).  Relevances are multiples of 1/64 in [0, 1]; with lam in {0, 1/4, 1/2, 1} every objective is a
    multiple of 1/256 below 4.  The table is smaller than the pool, so duplicates and ties are frequent; the pool is unsorted;
    about 10 % of the entries have row -1 (half of them with the padding's -inf relevance), user 1 (when there is one) is all
    padding.  bad_row: one entry's row is n_rows (absent, flag 0); nan_rel: one entry's relevance is NaN (absent, flag 1)."""
    rng = np.random.default_rng(seed)
    n_rows = max(3, (3 * P) // 4)
    keep = min(1.0, 6.0 / np.sqrt(D))
    unit = (rng.choice([-0.5, -0.25, 0.25, 0.5], (n_rows, D)) * (rng.random((n_rows, D)) < keep)).astype(np.float32)
    rows = rng.integers(0, n_rows, (U, P)).astype(np.int32)
    rel = (rng.integers(0, 65, (U, P)) / 64.0).astype(np.float32)
    gone = rng.random((U, P)) < 0.1
    rows[gone] = -1
    rel[gone & (rng.random((U, P)) < 0.5)] = -np.inf
    if U > 1:
        rows[1], rel[1] = -1, -np.inf
    u, i = U - 1, P // 2
    if bad_row:
        rows[u, i] = n_rows
    if nan_rel:
        rel[u, (i + 1) % P] = np.nan
    return unit, rows, rel


def exact_unit_table(n_rows, D, rng):
    """Rows that ARE unit vectors in dyadic numbers: four entries of +-1/2 (or sixteen of +-1/4 when D >= 16, every other row).
    Normalising them divides by exactly 1, and every dot product is a multiple of 1/16 in [-1, 1]."""
    table = np.zeros((n_rows, D), np.float32)
    for r in range(n_rows):
        m, v = (16, 0.25) if D >= 16 and r % 2 else (4, 0.5)
        table[r, rng.choice(D, m, replace=False)] = rng.choice([-v, v], m)
    return table


def rounded_case(U, P, D, seed):
    """Standard-normal rows normalised in float32, uniform relevances, rows drawn from a table of 4 P rows, about 10 % padding."""
    rng = np.random.default_rng(seed)
    n_rows = 4 * P
    x = rng.standard_normal((n_rows, D)).astype(np.float32)
    unit = (x / np.sqrt((x * x).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    rows = rng.integers(0, n_rows, (U, P)).astype(np.int32)
    rel = rng.random((U, P)).astype(np.float32)
    gone = rng.random((U, P)) < 0.1
    rows[gone], rel[gone] = -1, -np.inf
    return unit, rows, rel


def tolerance(unit, lam):
    """(1 - lam) b + 4 * 2^-23: b, the fp32 summation bound gamma_D max sum |u_i u_j| of a dot product of the table's rows in any
    order (recommend_cases.summation_bound), enters through the distance; the four ulp of a number below 4 cover the rounding
    of lam and 1 - lam to fp32, of the two products and of their sum."""
    from tests.recommend_cases import summation_bound

    return (1.0 - lam) * summation_bound(unit, unit) + 4 * 2.0 ** -23


def check_greedy(unit, rows, rel, sel, obj, lam, tol):
    """The greedy property of lists `sel` [U, k] (with objectives `obj`, or None): no repeats, no absent entry, the padding only
    once nothing is left; every pick's float64 objective, GIVEN the earlier picks of the list, within 2 tol of the best one
    left, and obj within tol of it.  -> (largest shortfall against the best, largest |obj - float64|)."""
    rows, rel = np.asarray(rows, dtype=np.int64), np.asarray(rel, dtype=np.float64)
    worst_gap, worst_obj = 0.0, 0.0
    for u in range(rows.shape[0]):
        present = present_mask(rows[u], rel[u], len(unit))
        dist, _ = distances64(unit, rows[u], present)
        left = present.copy()
        mind = np.full(rows.shape[1], np.inf)
        for t, s in enumerate(np.asarray(sel[u]).tolist()):
            if s < 0:
                assert not left.any(), (u, t, "padding while entries are left")
                assert (np.asarray(sel[u][t:]) == -1).all() and (obj is None or np.isneginf(obj[u][t:]).all()), (u, t)
                break
            assert left[s], (u, t, s, "absent or repeated")
            o64 = np.where(left, rel[u], 0.0) if t == 0 else lam * np.where(left, rel[u], 0.0) + (1.0 - lam) * mind
            gap = float(o64[left].max() - o64[s])
            worst_gap = max(worst_gap, gap)
            assert gap <= 2 * tol, (u, t, s, gap, tol)
            if obj is not None:
                err = abs(float(obj[u][t]) - float(o64[s]))
                worst_obj = max(worst_obj, err)
                assert err <= tol, (u, t, s, err, tol)
            left[s] = False
            mind = np.minimum(mind, dist[s])
    return worst_gap, worst_obj
