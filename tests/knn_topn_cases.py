"""Cases and the plain-Python brute force of the history-kNN top-N kernels and twins (plain helpers: nothing is collected from here).

BRUTE FORCE (``brute_chains`` / ``brute_topk`` / ``brute_rank``): the sets as Python sets, one neighbour row's chain as a dict
row -> ``np.float32`` filled by a loop over the slots in LIST order -- the first touching neighbour assigns its sim, every later one
adds it with one ``np.float32`` rounding -- one ``np.float32`` multiply by the item's scale, the admissible rows picked by plain
comparisons, ``sorted`` by ``(-score, position)``.  None of the twins' vectorisation.

KERNEL CASES (``kernel_case(n_rows, R, k_nbr, sims, scaled)``; R = ebn_knn_topk_range(), the kernels cut a range into four tiles of
R / 4 rows).  Sets, all clipped to the catalogue: 0 empty; 1 of length 1 (the last row); 2 the five rows on each side of every
multiple of R / 4 plus row 0 and the last row (straddling every boundary, holding the first and the last row of every tile);
3 a run of 100 rows and 4 a run of 300 rows inside one tile (more than 64 and more than 256 entries: the stride loops); 5 EVERY
row; 6 the special row alone (the NaN neighbour's set); 7 .. 46 the special row and up to 6 random rows (the ORDER-SENSITIVE
row: many neighbours hold it); the others 0 to 30 random rows.  Neighbour rows: 0 nobody; 1 the forty special sets first, then
random ones; 2 with -1 in the middle and at the end; 3 with an id >= n_seqs and a repeated id; 4 the empty set alone (a present
neighbour that touches nothing); 5 the every-row set first; 6 sets 1 .. 4; 7 (sims "nan") the special row's set with a NaN sim.
Sims: "random" non-integers of mixed magnitude and sign, "integer" small integers (ties everywhere: the position decides), "nan".
``item_scale`` holds a zero, negative entries and non-integers.  Users point at every neighbour row, at -1 and at n_hists, and two
users share one.

``order_case`` asserts that the special row's chain, folded in REVERSED list order, has other bits: a kernel that adds in another
order cannot pass."""
import functools

import numpy as np

from tests.covisit_topn_cases import positions, windows  # noqa: F401  (the same position maps and windows)

MAX_K, MAX_X = 64, 256
N_SPECIAL = 40


# ---- brute force ---------------------------------------------------------------------------------------------------------------
def brute_chains(c):
    """per neighbour row: {touched row: np.float32 score}"""
    n_seqs, n_rows = len(c["s_indptr"]) - 1, c["n_rows"]
    sets = [[int(x) for x in c["s_items"][int(c["s_indptr"][s]):int(c["s_indptr"][s + 1])]] for s in range(n_seqs)]
    out = []
    with np.errstate(all="ignore"):
        for seqs, sims in zip(c["nbr_seq"].tolist(), c["nbr_sim"]):
            acc = {}
            for j, s in enumerate(seqs):
                if not 0 <= s < n_seqs:
                    continue
                for row in sets[s]:
                    if 0 <= row < n_rows:
                        acc[row] = np.float32(sims[j]) if row not in acc else np.float32(acc[row] + np.float32(sims[j]))
            if c["item_scale"] is not None:
                acc = {row: np.float32(v * np.float32(c["item_scale"][row])) for row, v in acc.items()}
            out.append(acc)
    return out


def _brute_user(c, chains, u, cand_pos, M, window, exclude, flags):
    h = u if c["user_hist"] is None else int(c["user_hist"][u])
    chain = chains[h] if 0 <= h < len(chains) else {}
    lo, hi = 0, M
    if window is not None:
        lo, hi = max(int(window[u][0]), 0), min(int(window[u][1]), M)
        if lo >= hi:
            lo = hi = 0
    banned = set() if exclude is None else set(int(x) for x in exclude[u])
    adm = []
    for row, s in chain.items():
        p = row if cand_pos is None else int(cand_pos[row])
        if p >= M:
            flags[0] = 1
        if p < 0 or p >= M or not lo <= p < hi or row in banned:
            continue
        if s != s:
            flags[1] = 1
            continue
        adm.append((p, s))
    return adm


def brute_topk(c, chains, cand_pos, M, window, exclude, k):
    """-> (pos [U, k] int32, score [U, k] float32, flags [2])"""
    U = c["n_users"]
    pos, score, flags = np.full((U, k), -1, np.int32), np.full((U, k), -np.inf, np.float32), np.zeros(2, np.int32)
    for u in range(U):
        best = sorted(_brute_user(c, chains, u, cand_pos, M, window, exclude, flags), key=lambda e: (-e[1], e[0]))[:k]
        for i, (p, s) in enumerate(best):
            pos[u, i], score[u, i] = p, s
    return pos, score, flags


def brute_rank(c, chains, cand_pos, M, target_pos, window, exclude):
    """-> (rank [U], count [U], score [U] float32, flags [2])"""
    U = c["n_users"]
    rank, count, score, flags = np.zeros(U, np.int32), np.zeros(U, np.int32), np.full(U, -np.inf, np.float32), np.zeros(2, np.int32)
    for u in range(U):
        adm = _brute_user(c, chains, u, cand_pos, M, window, exclude, flags)
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
def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def kernel_case(n_rows, R, k_nbr=65, sims="random", scaled=True, identity=False, seed=0):
    """see the module docstring; ``identity``: as many users as neighbour rows, user_hist None"""
    rng = np.random.default_rng(seed + 31 * n_rows + k_nbr)
    q = R // 4
    clip = lambda rows: np.unique(np.asarray(rows, np.int64)[np.asarray(rows, np.int64) < n_rows])
    special = n_rows // 2
    edges = [r for b in range(q, n_rows + q, q) for r in range(b - 5, b + 5) if r >= 0] + [0, n_rows - 1]
    run0 = (n_rows // 3 // q) * q + 7  # the runs start inside a tile and stay in it
    sets = [np.zeros(0, np.int64), np.array([n_rows - 1]), clip(edges), clip(np.arange(run0, run0 + 100)), clip(np.arange(run0 + 50, run0 + 350)),
            np.arange(n_rows), np.array([special])]
    sets += [clip(np.concatenate([[special], rng.integers(0, n_rows, int(rng.integers(0, 7)))])) for _ in range(N_SPECIAL)]
    sets += [clip(rng.integers(0, n_rows, int(rng.integers(0, 31)))) for _ in range(560)]
    n_seqs = len(sets)
    s_indptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    s_items = np.concatenate(sets).astype(np.int32)
    first_special, first_random = 7, 7 + N_SPECIAL
    some = lambda n: rng.integers(first_random, n_seqs, n)
    rows = [
        np.full(k_nbr, -1),
        np.concatenate([np.arange(first_special, first_random), some(k_nbr)]),
        np.concatenate([some(2), [-1], some(k_nbr)]),
        np.concatenate([[first_special, n_seqs, first_special, n_seqs + 9], some(k_nbr)]),
        np.concatenate([[0], np.full(k_nbr, -1)]),
        np.concatenate([[5], np.arange(first_special, first_random), some(k_nbr)]),
        np.concatenate([[1, 2, 3, 4], some(k_nbr)]),
        np.concatenate([[6], np.arange(first_special, first_random), some(k_nbr)]),
    ]
    nbr_seq = np.stack([r[:k_nbr] for r in rows]).astype(np.int32)
    if k_nbr > 3:
        nbr_seq[2, -1] = -1  # absent at the end as well
    n_hists = nbr_seq.shape[0]
    if sims == "integer":
        nbr_sim = rng.integers(1, 4, nbr_seq.shape).astype(np.float32)
    else:
        nbr_sim = (np.exp2(rng.uniform(-8.0, 8.0, nbr_seq.shape)) * rng.choice([1.0, 1.0, -1.0], nbr_seq.shape)).astype(np.float32)
    nbr_sim[nbr_seq < 0] = -np.inf  # as ebn_knn_neighbours_f32 leaves an empty slot
    if sims == "nan":
        nbr_sim[7, 0] = np.nan
    item_scale = None
    if scaled:
        item_scale = np.exp2(rng.uniform(-3.0, 3.0, n_rows)).astype(np.float32) * rng.choice([1.0, 1.0, -1.0], n_rows).astype(np.float32)
        item_scale[n_rows // 3] = 0.0
        if sims == "integer":
            item_scale = rng.integers(-1, 3, n_rows).astype(np.float32)
    user_hist = None if identity else np.array(list(range(n_hists)) + [-1, n_hists, 1, 5, 5], np.int32)
    return _freeze(dict(s_indptr=s_indptr, s_items=s_items, n_rows=n_rows, n_seqs=n_seqs, item_scale=item_scale, nbr_seq=nbr_seq, nbr_sim=nbr_sim,
                        user_hist=user_hist, n_users=n_hists if identity else int(user_hist.size), special_col=special, special_row=special,
                        full_seq=5, first_special=first_special))


def fold(sims, reverse=False):
    """the chain of one row: np.float32 adds in (reversed) list order"""
    acc = None
    for s in (sims[::-1] if reverse else sims):
        acc = np.float32(s) if acc is None else np.float32(acc + np.float32(s))
    return acc


@functools.lru_cache(maxsize=None)
def order_case(n_rows, R):
    """the ORDER-SENSITIVE case: neighbour row 1 holds forty neighbours whose sets hold the special row, with non-integer sims of
    mixed magnitude; folded in reversed order the sum has other bits (asserted here)"""
    c = kernel_case(n_rows, R, 65, "random", False)
    holders = [j for j, s in enumerate(c["nbr_seq"][1].tolist())
               if 0 <= s < c["n_seqs"] and c["special_col"] in c["s_items"][int(c["s_indptr"][s]):int(c["s_indptr"][s + 1])].tolist()]
    sims = [c["nbr_sim"][1, j] for j in holders]
    assert len(holders) >= N_SPECIAL and any(float(s) != round(float(s)) for s in sims)
    assert max(abs(float(s)) for s in sims) / min(abs(float(s)) for s in sims) > 2.0 ** 8
    forward, backward = fold(sims), fold(sims, reverse=True)
    assert forward.view(np.int32) != backward.view(np.int32), (forward, backward)
    return c, forward


def exclusions(c, X, seed=0):
    """[U, X] int32: the special row first, -1, rows outside the table and random rows"""
    if X == 0:
        return None
    rng = np.random.default_rng(seed + X)
    out = rng.integers(-1, c["n_rows"] + 3, (c["n_users"], X)).astype(np.int32)
    out[:, 0] = c["special_col"]
    out[:, X // 2] = -1
    return out


def targets(list64, M, U):
    """per user: one of its own slots (0, 1, 4, 63 -- often empty: -1), a position next to one, none, one past M"""
    t = np.array([list64[u, (0, 1, 4, 63)[u % 4]] for u in range(U)], np.int64)
    t[3::5] = np.minimum(t[3::5] + 1, M - 1)
    t[4::6] = M + 2
    return t.astype(np.int32)


def twin_args(c):
    return c["s_indptr"], c["s_items"], c["n_rows"], c["item_scale"], c["nbr_seq"], c["nbr_sim"], c["user_hist"], c["n_users"]
