"""Float64 restatement of ebn_topk_score_window_f32 and the window patterns shared by tests/test_recommend_window_cpu.py and
tests/test_recommend_window_gpu.py.

The rule is that of recommend_cases.topk_reference plus one condition: user u may receive candidate position c only when
max(lo_u, 0) <= c < min(hi_u, M) with (lo_u, hi_u) = window[u].  A NaN counts (flag 1) only inside the user's window; a candidate
row outside the table counts (flag 0) when it lies in the window of at least one user -- the kernel may ALSO report one that
lies in [min lo, max hi) but in nobody's window, which the tests of that flag construct explicitly."""
import numpy as np

from tests.recommend_cases import EXACT_SHAPES, SPLIT_SHAPES, integer_case, scores64, topk_reference  # noqa: F401

PATTERNS = ["all", "empty", "one", "random", "edges", "outside", "sliding"]


def clamp(window, M):
    """[U, 2] int64: the windows clamped to [0, M]; an empty one (lo >= hi after clamping) becomes [0, 0)"""
    w = np.asarray(window, dtype=np.int64).reshape(-1, 2)
    lo, hi = np.maximum(w[:, 0], 0), np.minimum(w[:, 1], M)
    empty = lo >= hi
    return np.stack([np.where(empty, 0, lo), np.where(empty, 0, hi)], 1)


def window_reference(scores, k, window, cand_rows=None, n_rows=None, exclude=None):
    """scores [U, M] float64 by candidate POSITION, window [U, 2].  -> pos [U, k] int32, score [U, k] float64, flags (row out of
    range inside somebody's window, NaN seen inside the user's window)."""
    scores = np.asarray(scores, dtype=np.float64)
    U, M = scores.shape
    w = clamp(window, M)
    rows = np.arange(M) if cand_rows is None else np.asarray(cand_rows, dtype=np.int64)
    n_rows = M if n_rows is None else n_rows
    in_range = (rows >= 0) & (rows < n_rows)
    position = np.arange(M)
    pos = np.full((U, k), -1, np.int32)
    out = np.full((U, k), -np.inf)
    nan_seen = row_bad = False
    for u in range(U):
        inside = (position >= w[u, 0]) & (position < w[u, 1])
        row_bad |= bool((inside & ~in_range).any())
        ok = inside & in_range
        nan_seen |= bool((np.isnan(scores[u]) & ok).any())
        ok &= ~np.isnan(scores[u])
        if exclude is not None:
            ok &= ~np.isin(rows, np.asarray(exclude[u]))
        cand = np.flatnonzero(ok)
        order = cand[np.argsort(-scores[u, cand], kind="stable")][:k]
        pos[u, :len(order)] = order
        out[u, :len(order)] = scores[u, order]
    return pos, out, (int(row_bad), int(nan_seen))


def windows(pattern, U, M, seed=0):
    """[U, 2] int32 windows of one pattern for a (U, M) shape"""
    rng = np.random.default_rng(seed)
    if pattern == "all":
        lo, hi = np.zeros(U, np.int64), np.full(U, M, np.int64)
    elif pattern == "empty":  # lo == hi for the even users, lo > hi for the odd ones
        lo = rng.integers(0, M + 1, U)
        hi = np.where(np.arange(U) % 2 == 0, lo, lo - 1 - rng.integers(0, 3, U))
    elif pattern == "one":
        lo = rng.integers(0, M, U)
        hi = lo + 1
    elif pattern == "random":
        a, b = rng.integers(0, M + 1, U), rng.integers(0, M + 1, U)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
    elif pattern == "edges":  # around the first tile boundary and the end of the list
        pts = np.minimum(np.array([0, 127, 128, 129, M - 1, M]), M)
        lo, hi = rng.choice(pts, U), rng.choice(pts, U)
    elif pattern == "outside":  # lo < 0 and hi > M: clamped to everything
        lo, hi = -1 - rng.integers(0, 1000, U), M + 1 + rng.integers(0, 1000, U)
    elif pattern == "sliding":  # users in order, a window of about M / 4 that slides over the list: whole tiles are skipped
        width = max(1, M // 4)
        lo = (np.arange(U) * max(M - width, 0)) // max(U - 1, 1)
        hi = lo + width
    else:
        raise ValueError(pattern)
    return np.stack([lo, hi], 1).astype(np.int32)
