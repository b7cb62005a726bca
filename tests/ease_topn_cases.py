"""Cases and the plain-Python brute force of the EASE top-N kernels and twins (plain helpers: nothing is collected from here).

BRUTE FORCE (``brute_chains`` / ``brute_topk`` / ``brute_rank``): one history's chain per column as a Python loop over the history in
order with ``np.float32`` scalars -- the first present entry's product stored, the later ones added, each product and each add rounded
once -- the admissible columns picked by plain comparisons, ``sorted`` by ``(-score, position)``.  None of the twins' vectorisation.

CASES (``kernel_case``): B [n_rows, n_rows] float32 and a fixed set of histories.  Values: "dyadic" draws from {-1, -0.5, 0, -0.0, 0.5,
1} (every sum is exact, score ties are the rule and the position decides most slots), "normal" standard normal, "nan" / "+inf" /
"-inf" normal with that one value at B[special_row, special_col].  Histories: empty; all entries absent (-1, n_rows, n_rows + 7); one
entry (the special row); 63 / 64 / 65 and 255 / 256 / 257 / 300 entries with repeats and about a tenth of them absent (they straddle
the wave and the 256-entry staging boundaries; 65 and 300 hold the special row); a short one of repeats; 256 absent entries followed
by three present ones (the chain starts in the second staging chunk).  Users point at each history, at -1 and at n_hists, and two users
share a history."""
import functools

import numpy as np

R = 1024  # ebn_ease_topk_range(): tests/test_ease_topn_gpu.py asserts that the library says the same
MAX_K, MAX_X = 64, 256
VALUES = ("dyadic", "normal", "nan", "+inf", "-inf")
WEIGHTS = {"dyadic": (None, "positive", "negative"), "normal": (None, "positive", "negative"), "nan": (None,), "+inf": (None,), "-inf": (None,)}
ROWS = {"1": 1, "3": 3, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+3": 2 * R + 3}


# ---- brute force ---------------------------------------------------------------------------------------------------------------
def brute_chain(B, rows, weights):
    """-> None (no present entry) or the list of np.float32 scores of every column"""
    n_rows = B.shape[0]
    present = [(j, int(h)) for j, h in enumerate(rows) if 0 <= int(h) < n_rows]
    if not present:
        return None
    at = [h for _, h in present]
    w32 = None if weights is None else [np.float32(weights[j]) for j, _ in present]
    out = []
    with np.errstate(all="ignore"):
        for c in range(n_rows):
            stored = list(B[at, c])  # np.float32 scalars, in history order
            acc = None
            for i, b in enumerate(stored):
                p = b if w32 is None else w32[i] * b  # np.float32 * np.float32: one rounding
                acc = p if acc is None else acc + p   # np.float32 + np.float32: one rounding
            out.append(acc)
    return out


def brute_chains(case):
    """the chain of every history of a case, once (``chains=`` of brute_topk / brute_rank)"""
    off, out = case["hist_offsets"], []
    for h in range(len(off) - 1):
        a, b = int(off[h]), int(off[h + 1])
        out.append(brute_chain(case["B"], case["hist_rows"][a:b], None if case["hist_weights"] is None else case["hist_weights"][a:b]))
    return out


def _brute_user(case, chains, u, cand_pos, M, window, exclude, flags):
    h = u if case["user_hist"] is None else int(case["user_hist"][u])
    chain = chains[h] if 0 <= h < len(chains) else None
    if chain is None:
        return []
    lo, hi = 0, M
    if window is not None:
        lo, hi = max(int(window[u][0]), 0), min(int(window[u][1]), M)
        if lo >= hi:
            lo = hi = 0
    ex = set() if exclude is None else {int(x) for x in exclude[u]}
    adm = []
    for c, s in enumerate(chain):
        p = c if cand_pos is None else int(cand_pos[c])
        if p >= M:
            flags[0] = 1
        if p < 0 or p >= M or not lo <= p < hi or c in ex:
            continue
        if s != s:
            flags[1] = 1
            continue
        adm.append((p, s))
    return adm


def brute_topk(case, chains, cand_pos, M, window, exclude, k):
    """-> (pos [U, k] int32, score [U, k] float32, flags [2])"""
    U = case["n_users"]
    pos, score, flags = np.full((U, k), -1, np.int32), np.full((U, k), -np.inf, np.float32), np.zeros(2, np.int32)
    for u in range(U):
        best = sorted(_brute_user(case, chains, u, cand_pos, M, window, exclude, flags), key=lambda e: (-e[1], e[0]))[:k]
        for i, (p, s) in enumerate(best):
            pos[u, i], score[u, i] = p, s
    return pos, score, flags


def brute_rank(case, chains, cand_pos, M, target_pos, window, exclude):
    """-> (rank [U], count [U], score [U] float32, flags [2])"""
    U = case["n_users"]
    rank, count, score, flags = np.zeros(U, np.int32), np.zeros(U, np.int32), np.full(U, -np.inf, np.float32), np.zeros(2, np.int32)
    for u in range(U):
        adm = _brute_user(case, chains, u, cand_pos, M, window, exclude, flags)
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
def _weights(rng, n, kind):
    if kind is None:
        return None
    return (rng.uniform(0.1, 1.0, n) if kind == "positive" else rng.uniform(-1.0, 1.0, n)).astype(np.float32)


HIST_LENGTHS = (63, 64, 65, 255, 256, 257, 300)


@functools.lru_cache(maxsize=4)
def kernel_case(n_rows, values="normal", weights=None, seed=0):
    """see the module docstring"""
    assert values in VALUES
    rng = np.random.default_rng(seed + 31 * n_rows + VALUES.index(values))
    if values == "dyadic":
        B = rng.choice(np.array([-1.0, -0.5, 0.0, -0.0, 0.5, 1.0], np.float32), (n_rows, n_rows))
    else:
        B = rng.standard_normal((n_rows, n_rows), dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    special_row, special_col = n_rows // 3, n_rows // 2
    if values in ("nan", "+inf", "-inf"):
        B[special_row, special_col] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[values]
    B.setflags(write=False)
    draw = lambda n: np.where(rng.random(n) < 0.1, rng.choice([-1, n_rows, n_rows + 7], n), rng.integers(0, n_rows, n))
    other = int(rng.integers(0, n_rows))
    hists = [np.zeros(0, np.int64), np.array([-1, n_rows, n_rows + 7]), np.array([special_row])]
    for length in HIST_LENGTHS:
        h = draw(length)
        h[0] = -1 if length == 64 else h[0]  # the first entry absent: the chain starts at the second
        if length in (65, 300):
            h[length // 2] = special_row
        hists.append(h)
    hists.append(np.array([other, other, n_rows - 1, other, -1, 0]))
    hists.append(np.concatenate([np.full(256, n_rows + 1), [n_rows - 1, other, 0]]))
    hist_offsets = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    hist_rows = np.concatenate(hists).astype(np.int32)
    n_hists = len(hists)
    user_hist = np.array(list(range(n_hists)) + [-1, n_hists, 5], np.int32)
    return dict(B=B, n_rows=n_rows, hist_rows=hist_rows, hist_offsets=hist_offsets, hist_weights=_weights(rng, hist_rows.size, weights),
                user_hist=user_hist, n_users=int(user_hist.size), special_row=special_row, special_col=special_col)


def positions(n_rows, kind, seed=0):
    """cand_pos variants -> (cand_pos | None, M): None (the identity), "perm" (a permutation), "oob" (a permutation of two thirds of the
    rows, the others negative: no candidates; every 7th position moved to M and above)"""
    if kind is None:
        return None, n_rows
    rng = np.random.default_rng(seed + 17)
    perm = rng.permutation(n_rows).astype(np.int32)
    if kind == "perm":
        return perm, n_rows
    M = max(1, 2 * n_rows // 3)
    pos = np.where(perm < M, perm, -1).astype(np.int32)
    pos = np.where((pos >= 0) & (pos % 7 == 3), M + pos, pos).astype(np.int32)
    return pos, M


def exclusions(case, X, seed=0):
    """[U, X] int32: random rows, -1 and rows outside the table; the first of every user is the special column"""
    if X == 0:
        return None
    rng = np.random.default_rng(seed + X)
    out = rng.integers(-1, case["n_rows"] + 3, (case["n_users"], X)).astype(np.int32)
    out[:, 0] = case["special_col"]
    out[:, X // 2] = -1
    return out


def windows(n_users, M, avoid=None):
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


def targets(list64, M, U):
    """per user: one of its own slots (0, 1, 4, 63 -- often empty: -1), a position next to one, none, one past M"""
    t = np.array([list64[u, (0, 1, 4, 63)[u % 4]] for u in range(U)], np.int64)
    t[3::5] = np.minimum(t[3::5] + 1, M - 1)
    t[4::6] = M + 2
    return t.astype(np.int32)
