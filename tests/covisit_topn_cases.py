"""Cases and the plain-Python brute force of the co-visitation top-N kernels and twins (plain helpers: nothing is collected from here).

BRUTE FORCE (``brute_topk`` / ``brute_rank``): the matrix as a dict of dicts ``S[c][h]``, one user's chain as a Python loop over the
history in order with ``np.float32`` scalars -- first product stored, later ones added (or maximised), each product and each add
rounded once -- the admissible rows picked by plain comparisons, ``sorted`` by ``(-score, position)``.  None of the twins'
vectorisation.

KERNEL CASES (``kernel_case``): the TRANSPOSED matrix T directly, for a given number of catalogue rows.  Nine rows of T are not
empty: lengths 0 (kept empty on purpose), 1, 255, 256, 257 and 1000 (clipped to n_rows), one row whose columns sit on both sides of
every range boundary, one row that touches EVERY catalogue row, one row of a few columns that holds a stored exact 0.0, a -0.0 and
negative values.  Below 1024 rows every row of T holds every column.  Values: "random" uniform(-1, 1) float32, "count" the small
integers 1 .. 4 (ties everywhere: the position decides most slots), "nan" / "inf" random with one NaN / +inf at
(``special_row``, ``special_col``).  Histories: empty, all entries absent (-1, n_rows, n_rows + 7), length 1 (the every-row row;
the one-column row), 65 and 300 with repeats and absent entries in between, a short one over the zero row; users point at each,
at -1 and at n_hists, and two users share a history."""
import functools

import numpy as np

MAX_K, MAX_X = 64, 256


# ---- brute force ---------------------------------------------------------------------------------------------------------------
def matrix_dict(t_indptr, t_cols, t_vals):
    """T as CSR -> S[c][h]"""
    S = {}
    for h in range(len(t_indptr) - 1):
        for i in range(int(t_indptr[h]), int(t_indptr[h + 1])):
            S.setdefault(int(t_cols[i]), {})[h] = np.float32(t_vals[i])
    return S


def brute_chain(S, n_rows, rows, weights, mode):
    """-> {touched row: np.float32 score} of one history"""
    out = {}
    with np.errstate(all="ignore"):
        for c, stored in S.items():
            first = True
            for j, h in enumerate(rows):
                h = int(h)
                if not 0 <= h < n_rows or h not in stored:
                    continue
                p = np.float32((np.float32(1.0) if weights is None else np.float32(weights[j])) * stored[h])
                if first:
                    acc, first = p, False
                elif mode == 1:
                    acc = p if (p > acc or p != p) else acc
                else:
                    acc = np.float32(acc + p)
            if not first:
                out[c] = acc
    return out


def _brute_user(S, n_rows, case, u, cand_pos, M, window, exclude, mode, flags):
    h = u if case["user_hist"] is None else int(case["user_hist"][u])
    off = case["hist_offsets"]
    chain = {}
    if 0 <= h < len(off) - 1:
        a, b = int(off[h]), int(off[h + 1])
        w = None if case["hist_weights"] is None else case["hist_weights"][a:b]
        chain = brute_chain(S, n_rows, case["hist_rows"][a:b], w, mode)
    lo, hi = 0, M
    if window is not None:
        lo, hi = max(int(window[u][0]), 0), min(int(window[u][1]), M)
        if lo >= hi:
            lo = hi = 0
    adm = []
    for c, s in chain.items():
        p = c if cand_pos is None else int(cand_pos[c])
        if p >= M:
            flags[0] = 1
        if p < 0 or p >= M or not lo <= p < hi or (exclude is not None and c in [int(x) for x in exclude[u]]):
            continue
        if s != s:
            flags[1] = 1
            continue
        adm.append((p, s))
    return adm


def brute_topk(case, cand_pos, M, window, exclude, k, mode):
    """-> (pos [U, k] int32, score [U, k] float32, flags [2])"""
    S, n_rows, U = matrix_dict(case["t_indptr"], case["t_cols"], case["t_vals"]), len(case["t_indptr"]) - 1, case["n_users"]
    pos, score, flags = np.full((U, k), -1, np.int32), np.full((U, k), -np.inf, np.float32), np.zeros(2, np.int32)
    for u in range(U):
        best = sorted(_brute_user(S, n_rows, case, u, cand_pos, M, window, exclude, mode, flags), key=lambda e: (-e[1], e[0]))[:k]
        for i, (p, s) in enumerate(best):
            pos[u, i], score[u, i] = p, s
    return pos, score, flags


def brute_rank(case, cand_pos, M, target_pos, window, exclude, mode):
    """-> (rank [U], count [U], score [U] float32, flags [2])"""
    S, n_rows, U = matrix_dict(case["t_indptr"], case["t_cols"], case["t_vals"]), len(case["t_indptr"]) - 1, case["n_users"]
    rank, count, score, flags = np.zeros(U, np.int32), np.zeros(U, np.int32), np.full(U, -np.inf, np.float32), np.zeros(2, np.int32)
    for u in range(U):
        adm = _brute_user(S, n_rows, case, u, cand_pos, M, window, exclude, mode, flags)
        count[u] = len(adm)
        tp = int(target_pos[u])
        if tp >= M:
            flags[0] = 1
        mine = [s for p, s in adm if p == tp]
        if mine:
            t = mine[0]
            rank[u] = 1 + sum(1 for p, s in adm if s > t or (s == t and p < tp))
            score[u] = t
    return rank, count, score, flags


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def small_case(seed, n_rows=37, weights="positive", values="random", n_users=9):
    """a random matrix and random histories small enough for the brute force: rows of T with 0 to 12 columns, histories of 0 to 9
    entries with repeats and absent ones, user_hist with -1 and n_hists"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 13, n_rows)
    lengths[rng.integers(0, n_rows, 4)] = 0
    t_indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    t_cols = np.concatenate([np.sort(rng.choice(n_rows, int(l), replace=False)) for l in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    t_vals = _values(rng, t_cols.size, values)
    n_hists = 7
    h_len = rng.integers(0, 10, n_hists)
    h_len[0] = 0
    hist_offsets = np.concatenate([[0], np.cumsum(h_len)]).astype(np.int64)
    hist_rows = rng.integers(-1, n_rows + 2, int(hist_offsets[-1])).astype(np.int32)
    user_hist = np.concatenate([np.arange(n_hists), [-1, n_hists], rng.integers(0, n_hists, max(n_users - n_hists - 2, 0))])[:n_users]
    return dict(t_indptr=t_indptr, t_cols=t_cols, t_vals=t_vals, hist_rows=hist_rows, hist_offsets=hist_offsets,
                hist_weights=_weights(rng, hist_rows.size, weights), user_hist=user_hist.astype(np.int32), n_users=int(user_hist.size),
                n_rows=n_rows)


def _values(rng, n, kind):
    if kind == "count":
        return rng.integers(1, 5, n).astype(np.float32)
    v = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    if n > 4:
        v[rng.integers(0, n, 2)] = 0.0  # stored zeros
    return v


def _weights(rng, n, kind):
    if kind is None:
        return None
    return (rng.uniform(0.1, 1.0, n) if kind == "positive" else rng.uniform(-1.0, 1.0, n)).astype(np.float32)


ROW_LENGTHS = [0, 1, 255, 256, 257, 1000]


@functools.lru_cache(maxsize=None)
def kernel_case(n_rows, R, values="random", weights=None, seed=0):
    """see the module docstring; R: the rows of one LDS tile"""
    rng = np.random.default_rng(seed + n_rows)
    rows = {}
    if n_rows < 1024:
        for h in range(n_rows):
            rows[h] = np.arange(n_rows)
        named = dict(one=0, full=0, zero=min(1, n_rows - 1), straddle=0, long=0, empty=-1)
    else:
        ids = [int(v) for v in np.linspace(3, n_rows - 4, 9).astype(np.int64)]  # the rows of T that are not empty
        for h, length in zip(ids[:6], ROW_LENGTHS):
            rows[h] = np.sort(rng.choice(n_rows, min(length, n_rows), replace=False))
        rows[ids[1]] = np.array([n_rows - 1])
        edges = [c for b in range(R, n_rows + R, R) for c in range(b - 5, b + 5) if 0 <= c < n_rows]
        rows[ids[6]] = np.array(sorted(set(edges + [0, n_rows - 1])))
        rows[ids[7]] = np.arange(n_rows)
        rows[ids[8]] = np.sort(rng.choice(n_rows, 6, replace=False))
        named = dict(empty=ids[0], one=ids[1], long=ids[5], straddle=ids[6], full=ids[7], zero=ids[8])
    lengths = np.array([len(rows.get(h, ())) for h in range(n_rows)], np.int64)
    t_indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    t_cols = np.concatenate([rows[h] for h in sorted(rows)]).astype(np.int32)
    t_vals = _values(rng, t_cols.size, "count" if values == "count" else "random")
    z = int(t_indptr[named["zero"]])
    if values != "count" and t_indptr[named["zero"] + 1] - z >= 3:
        t_vals[z:z + 3] = [0.0, -0.0, -0.75]
    special_col = n_rows // 2
    at = int(t_indptr[named["full"]]) + special_col  # the full row holds every column: column c sits at offset c
    if values == "nan":
        t_vals[at] = np.nan
    if values == "inf":
        t_vals[at] = np.inf
    pool = [named[k] for k in ("one", "long", "straddle", "full", "zero")] + [h for h in rows if h not in named.values()]
    draw = lambda n: np.where(rng.random(n) < 0.1, rng.choice([-1, n_rows, n_rows + 7], n), rng.choice(pool, n))
    hists = [np.zeros(0, np.int64), np.array([-1, n_rows, n_rows + 7]), np.array([named["full"]]), np.array([named["one"]]), draw(65), draw(300),
             np.array([named["zero"], named["empty"] if named["empty"] >= 0 else -1, named["zero"]])]
    hist_offsets = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    hist_rows = np.concatenate(hists).astype(np.int32)
    n_hists = len(hists)
    user_hist = np.array(list(range(n_hists)) + [-1, n_hists, 4, 5, 2, 5], np.int32)
    return dict(t_indptr=t_indptr, t_cols=t_cols, t_vals=t_vals, hist_rows=hist_rows, hist_offsets=hist_offsets,
                hist_weights=_weights(rng, hist_rows.size, weights), user_hist=user_hist, n_users=int(user_hist.size), n_rows=n_rows,
                special_row=named["full"], special_col=special_col, named=named)


def positions(n_rows, kind, seed=0):
    """cand_pos variants -> (cand_pos | None, M): None (the identity), "perm" (a permutation), "holes" (a permutation of two thirds
    of the rows, the others negative: no candidates), "oob" (holes, and every 7th position moved to M and above)"""
    if kind is None:
        return None, n_rows
    rng = np.random.default_rng(seed + 17)
    perm = rng.permutation(n_rows).astype(np.int32)
    if kind == "perm":
        return perm, n_rows
    M = max(1, 2 * n_rows // 3)
    pos = np.where(perm < M, perm, -1).astype(np.int32)
    if kind == "oob":
        pos = np.where((pos >= 0) & (pos % 7 == 3), M + pos, pos).astype(np.int32)
    return pos, M


def exclusions(case, X, seed=0):
    """[U, X] int32: rows the user's history touches (the first columns of its rows of T), -1 and rows outside the table"""
    if X == 0:
        return None
    rng = np.random.default_rng(seed + X)
    n_rows, U = case["n_rows"], case["n_users"]
    out = rng.integers(-1, n_rows + 3, (U, X)).astype(np.int32)
    out[:, 0] = case["special_col"] if "special_col" in case else 0
    out[:, X // 2] = -1
    return out


def windows(n_users, M, avoid=None, seed=0):
    """[U, 2] int32 cycling through: full, empty, clamped on both sides, lo >= hi, a proper inner range; ``avoid``: a position every
    window is cut to leave out (at or above it, or below it)"""
    kinds = [(0, M), (5, 5), (-7, M + 9), (M // 2 + 3, M // 2), (M // 4, max(M // 4 + 1, 3 * M // 4))]
    w = np.array([kinds[u % len(kinds)] for u in range(n_users)], np.int64)
    if avoid is not None:
        for u in range(n_users):
            lo, hi = w[u]
            if lo <= avoid < hi:
                w[u] = (avoid + 1, hi) if u % 2 else (lo, avoid)
    return w.astype(np.int32)
