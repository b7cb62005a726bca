"""Float64 restatement of the top-k selection of ebn_topk_score_f32 / recommend(), and the case generators shared by
tests/test_recommend_cpu.py and tests/test_recommend_gpu.py.

The rule: a user's admissible candidates are those whose row lies in [0, n_rows), is not in the user's exclusion list and whose
score is not NaN; they are ordered by score descending, ties by ascending candidate position (a stable argsort of -score);
the first k positions are returned, short lists padded with (-1, -inf)."""
import numpy as np

# the shapes (U, M, F, k) of the exact cases: 1x1, M < k, on the tile, off the tile in every dimension, the real width and largest k
EXACT_SHAPES = [(1, 1, 4, 1), (3, 7, 4, 10), (64, 128, 32, 1), (65, 257, 36, 10), (130, 1000, 400, 64)]
SPLIT_SHAPES = [(65, 257, 36, 10), (130, 1000, 400, 64)]
ROUNDED_SHAPES = [(256, 4096, 400, 10), (33, 500, 36, 5)]
MAX_X = 256


def topk_reference(scores, k, cand_rows=None, n_rows=None, exclude=None):
    """scores [U, M] float64 (NaN / inf allowed), one column per candidate POSITION.  cand_rows [M] (None: position == row),
    exclude [U, X] rows (None: nothing).  -> pos [U, k] int32, score [U, k] float64, flags (row out of range, NaN seen)."""
    scores = np.asarray(scores, dtype=np.float64)
    U, M = scores.shape
    rows = np.arange(M) if cand_rows is None else np.asarray(cand_rows, dtype=np.int64)
    n_rows = M if n_rows is None else n_rows
    in_range = (rows >= 0) & (rows < n_rows)
    pos = np.full((U, k), -1, np.int32)
    out = np.full((U, k), -np.inf)
    nan_seen = False
    for u in range(U):
        ok = in_range.copy()
        nan = np.isnan(scores[u]) & ok
        nan_seen |= bool(nan.any())
        ok &= ~np.isnan(scores[u])
        if exclude is not None:
            ok &= ~np.isin(rows, np.asarray(exclude[u]))
        cand = np.flatnonzero(ok)
        order = cand[np.argsort(-scores[u, cand], kind="stable")][:k]
        pos[u, :len(order)] = order
        out[u, :len(order)] = scores[u, order]
    return pos, out, (int((~in_range).any()), int(nan_seen))


def integer_case(U, M, F, seed, cand="null", exclude=None):
    """Integer-valued users / news in [-4, 4]: every partial sum of a dot product is an integer below 2^24 (F <= 8192: |sum| <=
    16 F), so fp32 accumulates it exactly in any order and ties are frequent.  cand "null": the M candidates are the rows of news;
    "subset": news has M + 5 rows and cand_rows draws M of them with replacement, shuffled (duplicates are distinct candidates).
    exclude None | "x3" (X = 3: rows of the case, -1 padding and rows past the table, which match nothing) | "all" (user 0 excludes
    the first min(256, distinct) candidate rows -- every candidate when there are that few; the others only padding)."""
    rng = np.random.default_rng(seed)
    n_rows = M if cand == "null" else M + 5
    users = rng.integers(-4, 5, (U, F)).astype(np.float32)
    news = rng.integers(-4, 5, (n_rows, F)).astype(np.float32)
    cand_rows = None if cand == "null" else rng.integers(0, n_rows, M).astype(np.int32)
    rows = np.arange(M, dtype=np.int32) if cand_rows is None else cand_rows
    ex = None
    if exclude == "x3":
        ex = rng.choice(rows, (U, 3)).astype(np.int32)
        ex[rng.random((U, 3)) < 0.3] = -1
        ex[rng.random((U, 3)) < 0.1] = n_rows + 3
    elif exclude == "all":
        distinct = np.unique(rows)[:MAX_X]
        ex = np.full((U, len(distinct)), -1, np.int32)
        ex[0] = distinct
    return users, news, cand_rows, ex


def scores64(users, news, cand_rows=None):
    """float64 scores [U, M] by candidate position; a cand_rows entry outside the table scores 0 (the reference skips it anyway)"""
    news = np.asarray(news, dtype=np.float64)
    if cand_rows is not None:
        rows = np.asarray(cand_rows, dtype=np.int64)
        ok = (rows >= 0) & (rows < len(news))
        news = np.where(ok[:, None], news[np.where(ok, rows, 0)], 0.0)
    return np.asarray(users, dtype=np.float64) @ news.T


def summation_bound(users, news, cand_rows=None):
    """b = gamma_F max sum_j |u_j n_j|, gamma_F = F 2^-24 / (1 - F 2^-24): the standard bound of an fp32 dot product of length F
    in any order (fma or not), over all (user, candidate) pairs of the case."""
    F = np.shape(users)[1]
    g = F * 2.0 ** -24 / (1 - F * 2.0 ** -24)
    return g * float(scores64(np.abs(users), np.abs(news), cand_rows).max())


def tie_straddles_boundary(scores, k):
    """per user: does a tie group contain both the k-th and the (k+1)-th best score (so that the tie rule decides the list)?"""
    s = -np.sort(-np.asarray(scores, dtype=np.float64), axis=1)
    return s[:, k - 1] == s[:, k]
