"""Cases and the plain-Python brute force of the co-visitation kernels and twins (plain helpers: nothing is collected from here).

BRUTE FORCE: loops over sequences, positions and gaps into a dict of dicts ``counts[later][earlier]``; keys, CSR, the three
similarities (Python floats: IEEE doubles, rounded once to float32) and the scores (math.fsum over exact float64 products of
float32 operands) come from it -- none of the twins' vectorisation, sorting, blocking or segment reductions.

PAIR-KEY CASES (``pair_case``): sequence lengths 0, 1, 2, G, G + 1, sequences that straddle the 256-entry workgroup tiles, a run of
300 empty sequences inside one tile (more boundaries than a tile stages), trailing entries past the last sequence, rows -1, n_rows
and n_rows + 5, equal neighbours (a, a), and n_rows = 70 001 with rows next to n_rows: keys beyond 2^32.

SCORE CASES (``score_case``): matrix rows 0 .. 6 hold 0, 1, 2, 63, 64, 65 and 1000 columns out of [5, n_rows - 5) (so a history row
below the first and above the last column of every row exists), the others 0 to 20; histories of 0, 1, 63, 64, 65 and 130
entries that hold, for every one of those rows, its first and last column, a miss between two of its columns, rows 2 and
n_rows - 2 (below / above every column), duplicates and the unknown rows -1 and n_rows; every history is read by a list over the
seven rows, random rows and unknown candidates; further lists share one history, point at -1 and n_hists, or are empty; more than
256 items.  Values and weights are 2^uniform(-10, 10) in float32: no product is subnormal.
BOUNDS (u = 2^-24, n present entries): sum  n u / (1 - n u) sum_j |w_j S_j| (each product and each add rounds once, any order,
with or without fma); max  u |want| (rounding is monotonic).  ``exact``: integer counts as values, no weights, sums below 2^24:
bound 0."""
import functools
import math

import numpy as np

U = 2.0 ** -24
NO_PAIR = 2 ** 63 - 1
MAX_GAP = 64
TILE = 256   # CV_T of csrc/ebn_covisit.hip: entries / items of a workgroup
GROUP = 64   # CV_GW: lanes of one item (a wave)
N_ROWS_KEYS = 70_001
N_ROWS_SCORES = 1200
ROW_COLUMNS = [0, 1, 2, 63, 64, 65, 1000]
HIST_LENGTHS = [0, 1, 63, 64, 65, 130]


# ---- brute force ---------------------------------------------------------------------------------------------------------------
def brute_keys(seq_rows, seq_offsets, n_rows, G, symmetric):
    rows, off = [int(r) for r in seq_rows], [int(o) for o in seq_offsets]
    K = 2 * G if symmetric else G
    keys = [NO_PAIR] * (len(rows) * K)
    for s in range(len(off) - 1):
        for i in range(off[s], off[s + 1]):
            for g in range(1, G + 1):
                j = i + g
                if j < off[s + 1] and 0 <= rows[i] < n_rows and 0 <= rows[j] < n_rows and rows[i] != rows[j]:
                    keys[i * K + g - 1] = rows[j] * n_rows + rows[i]
                    if symmetric:
                        keys[i * K + G + g - 1] = rows[i] * n_rows + rows[j]
    return np.array(keys, np.int64)


def brute_counts(seq_rows, seq_offsets, n_rows, G, symmetric):
    """-> {later row: {earlier row: count}}"""
    rows, off = [int(r) for r in seq_rows], [int(o) for o in seq_offsets]
    counts = {}
    for s in range(len(off) - 1):
        for i in range(off[s], off[s + 1]):
            for j in range(i + 1, min(i + G, off[s + 1] - 1) + 1):
                a, b = rows[i], rows[j]
                if 0 <= a < n_rows and 0 <= b < n_rows and a != b:
                    counts.setdefault(b, {}).setdefault(a, 0)
                    counts[b][a] += 1
                    if symmetric:
                        counts.setdefault(a, {}).setdefault(b, 0)
                        counts[a][b] += 1
    return counts


def brute_csr(counts, n_rows):
    indptr, cols, vals = [0], [], []
    for r in range(n_rows):
        for c in sorted(counts.get(r, {})):
            cols.append(c)
            vals.append(counts[r][c])
        indptr.append(len(cols))
    return np.array(indptr, np.int64), np.array(cols, np.int32), np.array(vals, np.int32)


def brute_values(counts, n_rows, similarity):
    d_row = {r: sum(row.values()) for r, row in counts.items()}
    d_col = {}
    for row in counts.values():
        for c, v in row.items():
            d_col[c] = d_col.get(c, 0) + v
    out = []
    for r in range(n_rows):
        for c in sorted(counts.get(r, {})):
            v = float(counts[r][c])
            out.append(v if similarity == "count" else v / float(d_col[c]) if similarity == "conditional"
                       else v / math.sqrt(float(d_row[r]) * float(d_col[c])))
    return np.array(out, np.float64).astype(np.float32)


def brute_scores(c, mode):
    """-> (want float64 [n], sum_j |w_j S_j| [n], present entries [n]); mode 0: sum, 1: max"""
    indptr, cols, vals = c["indptr"], c["cols"], c["vals"]
    n_rows = indptr.size - 1
    S = [{int(cols[p]): float(vals[p]) for p in range(int(indptr[r]), int(indptr[r + 1]))} for r in range(n_rows)]
    h_off, c_off = c["hist_offsets"], c["cand_offsets"]
    n_hists, n = h_off.size - 1, c["cand_rows"].size
    want, absum, present = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    for l in range(c_off.size - 1):
        u = l if c["list_hist"] is None else int(c["list_hist"][l])
        if not 0 <= u < n_hists:
            continue
        hist = [(int(c["hist_rows"][j]), 1.0 if c["hist_weights"] is None else float(c["hist_weights"][j]))
                for j in range(int(h_off[u]), int(h_off[u + 1])) if 0 <= c["hist_rows"][j] < n_rows]
        for i in range(int(c_off[l]), int(c_off[l + 1])):
            r = int(c["cand_rows"][i])
            if not 0 <= r < n_rows or not hist:
                continue
            prod = [w * S[r].get(h, 0.0) for h, w in hist]  # exact: two float32 factors
            want[i] = max(prod) if mode == 1 else math.fsum(prod)
            absum[i] = math.fsum(abs(p) for p in prod)
            present[i] = len(hist)
    return want, absum, present


def bound(want, absum, present, mode):
    n = present.astype(np.float64)
    return U * np.abs(want) if mode == 1 else n * U / (1.0 - n * U) * absum


# ---- pair-key cases --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_case(G):
    """(seq_rows int32, seq_offsets int64, n_rows): shared by both values of ``symmetric``; read-only"""
    rng = np.random.default_rng(100 + G)
    n_rows = N_ROWS_KEYS
    lengths = [0, 1, 2, G, G + 1, 5, 300, 0] + [0] * 300 + [7, 250, 3, 2 * TILE + 90, 2, 0, G + 1, 1]
    pool = np.concatenate([rng.integers(0, n_rows, 12), [n_rows - 1, n_rows - 2, 0]])
    n_in, tail = sum(lengths), 9
    rows = pool[rng.integers(0, pool.size, n_in + tail)].astype(np.int64)
    rows[rng.permutation(n_in)[:40]] = rng.choice([-1, n_rows, n_rows + 5], 40)
    at = rng.permutation(n_in - 1)[:30]
    rows[at + 1] = rows[at]  # equal neighbours
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows, n_rows_arr = rows.astype(np.int32), n_rows
    rows.setflags(write=False)
    off.setflags(write=False)
    return rows, off, n_rows_arr


@functools.lru_cache(maxsize=None)
def pair_reference(G, symmetric):
    rows, off, n_rows = pair_case(G)
    want = brute_keys(rows, off, n_rows, G, symmetric)
    want.setflags(write=False)
    return want


# ---- score cases -----------------------------------------------------------------------------------------------------------------
def _pow2(rng, n):
    return np.exp2(rng.uniform(-10.0, 10.0, n)).astype(np.float32)


def _matrix(rng, n_rows, integer):
    indptr, cols = [0], []
    for r in range(n_rows):
        k = ROW_COLUMNS[r] if r < len(ROW_COLUMNS) else int(rng.integers(0, 21))
        cols.append(np.sort(rng.choice(np.arange(5, n_rows - 5), k, replace=False)))
        indptr.append(indptr[-1] + k)
    cols = np.concatenate(cols).astype(np.int32)
    vals = rng.integers(1, 51, cols.size).astype(np.float32) if integer else _pow2(rng, cols.size)
    return np.array(indptr, np.int64), cols, vals


def _between(cols_of_row, n_rows):
    """a row between two columns of the matrix row that is not one of them (None: no gap)"""
    gaps = np.flatnonzero(np.diff(cols_of_row) > 1)
    return None if gaps.size == 0 else int(cols_of_row[gaps[0]]) + 1


def _score_case(seed, weighted=True, integer=False, identity=False):
    rng = np.random.default_rng(seed)
    n_rows = N_ROWS_SCORES
    indptr, cols, vals = _matrix(rng, n_rows, integer)
    must = [2, n_rows - 2, -1, n_rows]  # below / above every column, unknown
    for r in range(1, len(ROW_COLUMNS)):
        cr = cols[indptr[r]:indptr[r + 1]]
        must += [int(cr[0]), int(cr[-1])] + ([] if _between(cr, n_rows) is None else [_between(cr, n_rows)])
    big = cols[indptr[6]:indptr[7]]
    hists = []
    for n in HIST_LENGTHS + [40, 3]:
        if n == 0:
            h = np.zeros(0, np.int64)
        elif n == 1:
            h = np.array([big[0]])
        elif n == 3:
            h = np.array([-1, n_rows, -1])  # no present entry
        else:
            fill = np.concatenate([big[rng.integers(0, big.size, n)], rng.integers(0, n_rows, n)])[rng.permutation(2 * n)[:n]]
            h = np.concatenate([must, must[:6], fill])[:n] if n >= 63 else np.concatenate([must[:20], fill])[:n]
            h = h[rng.permutation(n)]
        hists.append(h.astype(np.int32))
    n_hists = len(hists)
    base = lambda: np.concatenate([np.arange(len(ROW_COLUMNS)), rng.integers(0, n_rows, 5), [-1, n_rows]])[rng.permutation(len(ROW_COLUMNS) + 7)]
    if identity:
        lists = [(base(), u) for u in range(n_hists)]
    else:
        lists = [(base(), u) for u in range(n_hists)] + [(np.zeros(0, np.int64), 0)] * 3 + [(base(), 4)] * 6 + [(base(), -1), (base(), n_hists)]
        lists += [(np.zeros(0, np.int64), 2), (rng.integers(0, 7, 70), 5), (base(), 3), (np.zeros(0, np.int64), 1)]
    case = dict(indptr=indptr, cols=cols, vals=vals, hist_rows=np.concatenate(hists).astype(np.int32),
                hist_weights=_pow2(rng, sum(h.size for h in hists)) if weighted else None,
                hist_offsets=np.concatenate([[0], np.cumsum([h.size for h in hists])]).astype(np.int64),
                cand_rows=np.concatenate([r for r, _ in lists]).astype(np.int32),
                cand_offsets=np.concatenate([[0], np.cumsum([r.size for r, _ in lists])]).astype(np.int64),
                list_hist=None if identity else np.array([u for _, u in lists], np.int32), exact=integer and not weighted)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


SCORE_BUILDERS = {
    "weighted": lambda: _score_case(1),
    "unweighted": lambda: _score_case(2, weighted=False),
    "identity": lambda: _score_case(3, identity=True),
    "exact": lambda: _score_case(4, weighted=False, integer=True),
}
SCORE_NAMES = list(SCORE_BUILDERS)


@functools.lru_cache(maxsize=None)
def score_case(name):
    """(case, {mode: (want, bound)}): built once, shared, read-only"""
    c = SCORE_BUILDERS[name]()
    ref = {}
    for mode in (0, 1):
        want, absum, present = brute_scores(c, mode)
        b = np.zeros_like(want) if c["exact"] else bound(want, absum, present, mode)
        want.setflags(write=False)
        b.setflags(write=False)
        ref[mode] = (want, b)
    return c, ref


def random_sequences(seed, n_seqs=40, n_rows=30, longest=25):
    """(rows int32 with unknowns and equal neighbours, offsets) for the matrix tests: small n_rows, so pairs repeat"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, longest + 1, n_seqs)
    lengths[rng.integers(0, n_seqs)] = longest
    rows = rng.integers(-1, n_rows + 1, int(lengths.sum()) + 3).astype(np.int32)  # -1 and n_rows: unknown; 3 trailing entries
    return rows, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def frames_case(cv, behaviors, history, weights_of=None):
    """the operands of ``cv.predict(behaviors, history=history)`` assembled by hand, as a case for ``brute_scores``: one history per
    row of the history frame (cut to cv.history_size), ``weights_of(n)`` (a list function of utils/_decay.py, or None) called once
    per user"""
    hists = [np.asarray(h)[-cv.history_size:] if cv.history_size else np.asarray(h) for h in history["article_id_fixed"]]
    at = {u: k for k, u in enumerate(history["user_id"].tolist())}
    inview = list(behaviors["article_ids_inview"])
    off = lambda lists: np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    w = None if weights_of is None else np.concatenate([np.asarray(weights_of(len(h)), np.float64) for h in hists]).astype(np.float32)
    indptr, cols, _, vals = cv.matrix.host()
    return dict(indptr=indptr, cols=cols, vals=vals, hist_rows=cv.rows_of(np.concatenate(hists)), hist_weights=w, hist_offsets=off(hists),
                cand_rows=cv.rows_of(np.concatenate(inview)), cand_offsets=off(inview),
                list_hist=np.array([at.get(u, -1) for u in behaviors["user_id"]], np.int32))
