"""Cases and the plain-Python brute force of the history-kNN kernels and twins (plain helpers: nothing is collected from here).

BRUTE FORCE: dicts, sets and loops.  A query's items are a dict row -> (position, weight) that later entries overwrite, ordered by
position; ``dot`` walks the items in that order and the WHOLE posting list of each (no tails), ``np.float32`` adds, the first
contribution assigning; the union loses ``hist_self``, is sorted, and its last ``sample_size`` ids are the candidates; ``sim`` is one
``np.float32`` multiply; the neighbours are ``sorted`` by (-sim, -id).  Scores: ``math.fsum`` over the exact float64 values of the sims
of the neighbours whose set holds the candidate, one float64 multiply by the item's scale.

NEIGHBOUR CASE (``neighbour_case``; R = ebn_knn_range()): n_seqs = 2 R + 37, so the walk from the most recent id downwards crosses
two range boundaries.  Posting rows: 0 empty; 1 a single sequence; 2 has 700 sequences inside the top range (more than 256 in one
range, more than a tail of 301); 3 every 11th sequence (all ranges, longer than the tails of sample_size 1000); 4 has 600
sequences in the second range only; 5 the 37 oldest ids (the third range) and nothing else; 6 two ids at the two range boundaries
and their neighbours; 7 .. 47 between 0 and 20 random sequences.  Histories: empty; all absent; a single item (row 2) whose
``hist_self`` is the row's most recent sequence -- with equal sims the id-descending order would put it first, and with sample_size
300 the last candidate is entry 301 from the end of the row: inside a tail of sample_size + 1, outside one of sample_size; rows
2 + 4 (sample_size 1000 is reached in the middle of the second range); row 1 alone (one candidate: k above the candidates);
repeated items with different weights; row 0 alone (no candidate); rows 5 and 6 (the walk skips to the boundaries); 65 and 300
entries with repeats and absent rows (the 300 span two chunks of 256).  No union exceeds ``BIG_SAMPLE`` = 4000 (asserted)."""
import functools
import math

import numpy as np

U = 2.0 ** -24
N_ROWS = 48
BIG_SAMPLE = 4000
SAMPLES = (1, 300, 1000, BIG_SAMPLE, 4096)  # 300: the +1 of the tail; 1000: cut inside the second range; 4000: above every union
KS = (1, 300, 512)
VARIANTS = {  # weights, seq_scale, hist_self
    "integer": ("integer", False, True),   # many equal sims: the id-descending order decides
    "scaled": ("float", True, False),
    "unweighted": (None, True, True),
}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- brute force ---------------------------------------------------------------------------------------------------------------
def query_items(rows, weights, n_rows):
    """[(row, weight)] of one history: distinct present rows, the LAST occurrence's weight, ordered by that occurrence"""
    last = {}
    for j, r in enumerate(rows):
        if 0 <= int(r) < n_rows:
            last[int(r)] = (j, 1.0 if weights is None else float(weights[j]))
    return [(r, w) for r, (j, w) in sorted(last.items(), key=lambda kv: kv[1][0])]


def brute_dots(c):
    """per history {sequence: float32 dot} over the WHOLE union (hist_self removed)"""
    n_rows = c["p_indptr"].size - 1
    posting = [[int(s) for s in c["p_seqs"][c["p_indptr"][r]:c["p_indptr"][r + 1]]] for r in range(n_rows)]
    out = []
    for u in range(c["hist_offsets"].size - 1):
        a, b = int(c["hist_offsets"][u]), int(c["hist_offsets"][u + 1])
        w = None if c["hist_weights"] is None else c["hist_weights"][a:b]
        dot = {}
        for r, wv in query_items(c["hist_rows"][a:b], w, n_rows):
            for s in posting[r]:
                dot[s] = np.float32(wv) if s not in dot else np.float32(dot[s] + np.float32(wv))
        if c["hist_self"] is not None:
            dot.pop(int(c["hist_self"][u]), None)
        out.append(dot)
    return out


def brute_neighbours(c, dots, sample_size, k):
    n_hists = len(dots)
    seq, sim = np.full((n_hists, k), -1, np.int32), np.full((n_hists, k), -np.inf, np.float32)
    for u, dot in enumerate(dots):
        cands = sorted(dot)[-sample_size:]
        pairs = [(np.float32(dot[s]) if c["seq_scale"] is None else np.float32(dot[s] * c["seq_scale"][s]), s) for s in cands]
        pairs.sort(key=lambda p: (-float(p[0]), -p[1]))
        for j, (v, s) in enumerate(pairs[:k]):
            seq[u, j], sim[u, j] = s, v
    return seq, sim


def brute_scores(c):
    """-> (want float64 [n], sum |sim| over the hits [n], the plain sum [n])"""
    n_seqs, n_rows = c["s_indptr"].size - 1, c["n_rows"]
    sets = [set(int(x) for x in c["s_items"][c["s_indptr"][s]:c["s_indptr"][s + 1]]) for s in range(n_seqs)]
    n_hists, k = c["nbr_seq"].shape
    n = c["cand_rows"].size
    want, absum, total = np.zeros(n), np.zeros(n), np.zeros(n)
    for l in range(c["cand_offsets"].size - 1):
        u = l if c["list_hist"] is None else int(c["list_hist"][l])
        if not 0 <= u < n_hists:
            continue
        for i in range(int(c["cand_offsets"][l]), int(c["cand_offsets"][l + 1])):
            r = int(c["cand_rows"][i])
            if not 0 <= r < n_rows:
                continue
            hits = [float(c["nbr_sim"][u, j]) for j in range(k) if 0 <= c["nbr_seq"][u, j] < n_seqs and r in sets[int(c["nbr_seq"][u, j])]]
            total[i], absum[i] = math.fsum(hits), math.fsum(abs(h) for h in hits)
            want[i] = total[i] * (1.0 if c["item_scale"] is None else float(c["item_scale"][r]))
    return want, absum, total


def score_bound(c, want, absum, total):
    """|got - want| <= (gamma_k sum |sim| + u |sum|) |item_scale| + u |want|, gamma_k = k u / (1 - k u).
    The kernel adds at most k fp32 sims in an order of its own: whatever the order, k - 1 roundings leave an error of at most
    gamma_(k-1) sum |sim| <= gamma_k sum |sim| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); u |sum| covers
    the reference's own rounding of the sum to fp32 precision; the closing multiply by the fp32 item scale rounds once: u |want|."""
    k = c["nbr_seq"].shape[1]
    gamma = k * U / (1.0 - k * U)
    scale = np.ones(want.size) if c["item_scale"] is None else np.abs(c["item_scale"].astype(np.float64))[np.clip(c["cand_rows"], 0, c["n_rows"] - 1)]
    return (gamma * absum + U * np.abs(total)) * scale + U * np.abs(want)


# ---- neighbour cases -------------------------------------------------------------------------------------------------------------
def _csr(lists):
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    flat = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    return indptr, flat


@functools.lru_cache(maxsize=None)
def neighbour_case(R, variant):
    weights, scaled, with_self = VARIANTS[variant]
    rng = np.random.default_rng(7)  # the same index and histories for every variant
    n_seqs = 2 * R + 37
    top0, second0 = n_seqs - R, n_seqs - 2 * R  # the first two ranges: [top0, n_seqs), [second0, top0)
    post = [np.zeros(0, np.int64) for _ in range(N_ROWS)]
    post[1] = np.array([second0 + 500])
    post[2] = np.sort(rng.choice(np.arange(top0 + 10, n_seqs), 700, replace=False))
    post[3] = np.arange(5, n_seqs, 11)
    post[4] = np.sort(rng.choice(np.arange(second0 + 3, top0 - 3), 600, replace=False))
    post[5] = np.arange(0, 37)
    post[6] = np.array([second0 - 1, second0, top0 - 1, top0, n_seqs - 1])
    for r in range(7, N_ROWS):
        post[r] = np.sort(rng.choice(n_seqs, int(rng.integers(0, 21)), replace=False))
    p_indptr, p_seqs = _csr(post)
    mix = lambda n: np.concatenate([rng.integers(0, N_ROWS, n - 6), [-1, N_ROWS, N_ROWS + 5, 2, 3, 4]])[rng.permutation(n)]
    hists = [[], [-1, N_ROWS, N_ROWS + 5], [2], [2, 4], [1], [3, 2, 3, 7, 2, 9, 3], [0], [5, 6], mix(65), mix(300), [6, 1, 5]]
    selfs = [-1, 5, int(post[2][-1]), int(post[4][300]), second0 + 500, int(post[3][-1]), 3, 36, int(post[3][-2]), int(post[2][-3]), -1]
    n_items = sum(len(h) for h in hists)
    w = {None: None, "integer": rng.integers(1, 4, n_items).astype(np.float32),
         "float": np.exp2(rng.uniform(-4.0, 4.0, n_items)).astype(np.float32)}[weights]
    sizes = rng.integers(1, 50, n_seqs)
    c = dict(p_indptr=p_indptr, p_seqs=p_seqs, n_seqs=n_seqs, n_rows=N_ROWS,
             seq_scale=(1.0 / np.sqrt(sizes)).astype(np.float32) if scaled else None,
             hist_rows=np.concatenate([np.asarray(h, np.int64) for h in hists]).astype(np.int32), hist_weights=w,
             hist_offsets=np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64),
             hist_self=np.array(selfs, np.int32) if with_self else None)
    _freeze(c)
    dots = brute_dots(c)
    assert max(len(d) for d in dots) <= BIG_SAMPLE - 1 and max(len(d) for d in dots) > 1500, [len(d) for d in dots]
    assert 700 < len(dots[3]) and len([s for s in dots[3] if s >= top0]) < 1000 < len(dots[3]) - 100  # 1000 is reached mid second range
    return c, dots


@functools.lru_cache(maxsize=None)
def neighbour_reference(R, variant, sample_size, k):
    c, dots = neighbour_case(R, variant)
    seq, sim = brute_neighbours(c, dots, sample_size, k)
    seq.setflags(write=False)
    sim.setflags(write=False)
    return seq, sim


# ---- score cases -----------------------------------------------------------------------------------------------------------------
SCORE_ROWS = 900
SET_SIZES = [0, 1, 2, 63, 64, 65, 400]
SCORE_CASES = {"k1": (1, False, True), "k65": (65, False, False), "k512": (512, False, True), "integer": (65, True, False),
               "identity": (65, False, True)}  # k, integer sims, item_scale given


@functools.lru_cache(maxsize=None)
def score_case(name):
    """(case, want, bound): sets of 0, 1, 2, 63, 64, 65 and 400 rows and 593 of 0 to 30; neighbour rows that are full, end in -1 / -inf,
    hold an id outside [0, n_seqs), or are all -1; lists of 0, 1 and 300 items that hold the first and the last row of the sets of their
    history's neighbours, absent rows (-1, n_rows) and random ones; list_hist with -1 and n_hists ("identity": NULL)"""
    k, integer, scaled = SCORE_CASES[name]
    rng = np.random.default_rng(40 + k + integer)
    n_seqs, n_rows = 600, SCORE_ROWS
    sets = [np.sort(rng.choice(n_rows, SET_SIZES[s] if s < len(SET_SIZES) else int(rng.integers(0, 31)), replace=False)) for s in range(n_seqs)]
    s_indptr, s_items = _csr(sets)
    n_hists = 9
    nbr_seq, nbr_sim = np.full((n_hists, k), -1, np.int32), np.full((n_hists, k), -np.inf, np.float32)
    for u in range(n_hists):
        n = [k, k, max(k - 3, 1), k, 0, min(k, 7), k, 1, k][u]  # history 4: no neighbour at all
        seqs = rng.choice(n_seqs, n, replace=False) if n <= n_seqs else rng.integers(0, n_seqs, n)
        seqs[:min(n, len(SET_SIZES))] = rng.permutation(len(SET_SIZES))[:min(n, len(SET_SIZES))]  # the special sets come first
        nbr_seq[u, :n] = seqs
        nbr_sim[u, :n] = rng.integers(1, 40, n) if integer else np.exp2(rng.uniform(-8.0, 8.0, n)) * rng.choice([1.0, 1.0, -1.0], n)
    nbr_seq[0, 0] = 6  # the set of 400 rows: also with k = 1 the long list has hits
    if k >= 65:
        nbr_seq[3, 5], nbr_seq[3, 64] = n_seqs, n_seqs + 9  # ids outside the index: skipped

    def items(u, n):
        must = [-1, n_rows]
        for s in nbr_seq[u][nbr_seq[u] >= 0][:8].tolist():
            if s < n_seqs and sets[s].size:
                must += [int(sets[s][0]), int(sets[s][-1])]
        pool = np.concatenate([must, rng.integers(0, n_rows, max(n, 1))])
        return pool[rng.permutation(pool.size)][:n] if n < pool.size else pool[rng.integers(0, pool.size, n)]

    if name == "identity":
        lists = [(items(u, 12), u) for u in range(n_hists)]
    else:
        lists = [(items(0, 300), 0), (np.zeros(0, np.int64), 1), (items(1, 1), 1), (items(2, 40), 2), (items(3, 40), 3), (items(4, 9), 4),
                 (items(5, 20), 5), (items(6, 20), -1), (items(6, 20), n_hists), (items(6, 30), 6), (np.zeros(0, np.int64), 2),
                 (items(7, 15), 7), (items(8, 25), 8), (items(0, 20), 0)]
    c = dict(s_indptr=s_indptr, s_items=s_items, n_rows=n_rows, nbr_seq=nbr_seq, nbr_sim=nbr_sim,
             item_scale=(rng.integers(1, 5, n_rows).astype(np.float32) if integer else np.exp2(rng.uniform(-3.0, 3.0, n_rows)).astype(np.float32))
             if scaled or integer else None,
             cand_rows=np.concatenate([r for r, _ in lists]).astype(np.int32),
             cand_offsets=np.concatenate([[0], np.cumsum([len(r) for r, _ in lists])]).astype(np.int64),
             list_hist=None if name == "identity" else np.array([u for _, u in lists], np.int32), exact=integer)
    _freeze(c)
    want, absum, total = brute_scores(c)
    b = np.zeros_like(want) if integer else score_bound(c, want, absum, total)  # integer sums below 2^24: bit for bit
    assert np.count_nonzero(want) > want.size // 20
    want.setflags(write=False)
    b.setflags(write=False)
    return c, want, b


def random_sequences(seed, n_seqs=60, n_ids=40, longest=12):
    """lists of article ids (with repeats inside a sequence and empty sequences) for the index tests"""
    rng = np.random.default_rng(seed)
    return [rng.integers(100, 100 + n_ids, int(rng.integers(0, longest + 1))).tolist() for _ in range(n_seqs)]
