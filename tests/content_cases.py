"""Cases and the float64 brute-force reference of the content-similarity kernels (plain helpers: nothing is collected from here).

A case holds the operands of ebn_cs_profiles_f32 / ebn_cs_centroid_scores_f32 / ebn_cs_nearest_scores_f32 as numpy arrays:
``table`` [n_rows, D] float32 unit rows, ``hist_rows`` int32 / ``hist_weights`` float32 or None / ``hist_offsets`` int64 (one
history per user), ``cand_rows`` int32 / ``cand_offsets`` int64 (one list per impression) and ``list_hist`` int32 or None (the
history of every list; None: list l reads history l).  ``reference`` is the yardstick: per history the weighted sum of its
present rows in float64 over the table's float32 values, per list one float64 product of its candidates with its history's rows --
plain numpy, none of the twins' chunking, compaction or segment reductions.

TABLE: rows are unit(c_k + 0.6 g / sqrt(D)), c_k one of four random unit directions, g standard normal, rounded to float32.  The
four directions are drawn again while two of them have a cosine below -0.1: at D = 3 or 4 random directions often nearly oppose
each other and whole histories would cancel (at D >= 63 the first draw almost always stands).
WEIGHTS: drawn from {0.25, 0.5, 1, 2}; the FIRST and LAST present entry of a history with at least 2 present entries weigh
W = max(1, sum of the entries between them) -- W is then half the sum of all the others, the other end included (with exactly two
present entries W = 1).
PLANTING: the first and last present entry of a history are rows that occur nowhere else in it, and every list's first two
candidates are those two rows: dropping either end of the history moves a score of the list (tests/test_content_cpu.py asserts by
how much).  A list of ONE candidate therefore reads a history with one present entry, or one that gives exact zeros.

BOUNDS (derived, u = 2^-24, H present entries of the history, a_k = sum_j |w_j T[h_j, k]|):
    profiles   2 (H + D + 8) u (a_k / ||p|| + |p_k| / ||p||)            H fused multiply-adds, a D-term norm, sqrt, one division
    centroid   2 (H + D + 8) u (sum_k a_k |T[c, k]| / ||p|| + |score|)  the profile's error through a D-term dot
    nearest    2 (D + 8) u max_j w_j                                    a D-term dot of unit rows times w; the max of rounded
                                                                        values is within the largest single error
    zeros (absent candidates, no history, no present entry, all weights 0): exact
The exact case ``d1_exact`` (D = 1, rows +1, power-of-two weights with maximum 1) has bound 0: every score is exactly 1 or 0."""
import functools

import numpy as np

U = 2.0 ** -24
# tile sizes of csrc/ebn_content.hip
CS_THREADS = 256  # history entries one workgroup takes per round (CS_WAVES waves x 64 lanes), threads that own profile columns
CS_WAVES = 4      # a history's entries go round-robin over the waves
CS_WAVE = 64      # candidates of one batch of the centroid kernel
CS_NT = 16        # candidate rows of one LDS tile of the nearest kernel
MAX_D = 1024

DIMS = [3, 4, 63, 64, 65, 96, 255, 256, 257, 768, 1024]
LENGTHS = sorted({0, 1, 2, 3, 4, 5, 63, 64, 65} | {t + d for t in (CS_WAVES, CS_NT, CS_WAVE, CS_THREADS) for d in (-1, 0, 1)})
LONG_HISTORY = 4 * CS_THREADS + 1  # several rounds of every wave
N_ROWS = 160


def make_table(rng, n_rows, D):
    while True:  # at D = 3 or 4 four random directions can nearly oppose each other and histories would cancel: draw again
        centres = rng.standard_normal((4, D))
        centres /= np.linalg.norm(centres, axis=1, keepdims=True)
        if D < 2 or (centres @ centres.T).min() >= -0.1:
            break
    rows = centres[rng.integers(0, 4, n_rows)] + 0.6 * rng.standard_normal((n_rows, D)) / np.sqrt(D)
    return (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)


def _history(rng, n_rows, length, kind):
    """one history -> (rows, weights): kind "normal", "single" (one present entry), "absent" (none), "zero" (weights all 0)"""
    if length == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float32)
    if kind == "absent":
        return rng.choice([-1, n_rows], length).astype(np.int32), rng.choice([0.25, 0.5, 1.0, 2.0], length).astype(np.float32)
    ends = rng.permutation(n_rows)[:2]
    rest = np.setdiff1d(np.arange(n_rows), ends)
    rows = rest[rng.integers(0, rest.size, length)].astype(np.int32)
    w = rng.choice([0.25, 0.5, 1.0, 2.0], length).astype(np.float32)
    if kind == "single":
        rows[:] = rng.choice([-1, n_rows], length)
        rows[rng.integers(0, length)] = ends[0]
        return rows, w
    if length > 4:  # absent entries in the middle and, for some, in front of the first present one
        rows[rng.permutation(length)[:max(1, length // 10)]] = rng.choice([-1, n_rows], max(1, length // 10))
    present = np.flatnonzero((rows >= 0) & (rows < n_rows))
    if present.size == 0:
        rows[0] = rest[0]
        present = np.array([0])
    first, last = int(present[0]), int(present[-1])
    rows[first] = ends[0]
    if last != first:
        rows[last] = ends[1]
    if present.size >= 2:  # with two present entries: W = 1, again half the sum of the others (the other end)
        w[first] = w[last] = max(1.0, float(w[present[1:-1]].astype(np.float64).sum()))
    if kind == "zero":
        w[:] = 0.0
    return rows, w


def _ends(rows, n_rows):
    present = np.flatnonzero((rows >= 0) & (rows < n_rows))
    return (int(rows[present[0]]), int(rows[present[-1]])) if present.size else None


def build(seed, D, hists, lists, weighted=True, identity=False, n_rows=N_ROWS):
    """hists: [(length, kind)]; lists: [(length, u)] with u a history number, -1 or len(hists).  Unweighted cases pass
    hist_weights = None; identity cases pass list_hist = None (lists[l][1] == l)."""
    rng = np.random.default_rng(seed)
    table = make_table(rng, n_rows, D)
    h_rows, h_w, h_off = [], [], [0]
    for length, kind in hists:
        r, w = _history(rng, n_rows, length, kind)
        h_rows.append(r)
        h_w.append(w)
        h_off.append(h_off[-1] + length)
    c_rows, c_off = [], [0]
    for l, (length, u) in enumerate(lists):
        assert not identity or u == l
        r = rng.integers(0, n_rows, length).astype(np.int32)
        if length >= 4:
            r[2 + rng.permutation(length - 2)[:2]] = [-1, n_rows]
        ends = _ends(h_rows[u], n_rows) if 0 <= u < len(hists) else None
        if ends is not None and hists[u][1] != "zero":
            n_present = int(((h_rows[u] >= 0) & (h_rows[u] < n_rows)).sum())
            assert length != 1 or n_present == 1, "a list of one candidate reads a history with one present entry"
            r[:2] = ends[:length]
        c_rows.append(r)
        c_off.append(c_off[-1] + length)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    case = dict(table=table, hist_rows=cat(h_rows, np.int32), hist_weights=cat(h_w, np.float32) if weighted else None,
                hist_offsets=np.array(h_off, np.int64), cand_rows=cat(c_rows, np.int32), cand_offsets=np.array(c_off, np.int64),
                list_hist=None if identity else np.array([u for _, u in lists], np.int32), exact=False)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def reference(case, drop=None):
    """float64 brute force -> dict(profiles [n_hists, D], centroid [n], nearest [n] and their bounds).  ``drop`` = "first" /
    "last": every history without its first / last present entry."""
    T = case["table"].astype(np.float64)
    n_rows, D = T.shape
    h_off, c_off = case["hist_offsets"], case["cand_offsets"]
    n_hists, n_lists, n = h_off.size - 1, c_off.size - 1, case["cand_rows"].size
    hist = []
    profiles, p_bound = np.zeros((n_hists, D)), np.zeros((n_hists, D))
    for u in range(n_hists):
        rows = case["hist_rows"][h_off[u]:h_off[u + 1]].astype(np.int64)
        w = np.ones(rows.size) if case["hist_weights"] is None else case["hist_weights"][h_off[u]:h_off[u + 1]].astype(np.float64)
        ok = (rows >= 0) & (rows < n_rows)
        rows, w = rows[ok], w[ok]
        if drop == "first":
            rows, w = rows[1:], w[1:]
        elif drop == "last":
            rows, w = rows[:-1], w[:-1]
        Th = T[rows]
        p = (w[:, None] * Th).sum(0)
        a = np.abs(w[:, None] * Th).sum(0)
        norm = float(np.sqrt((p * p).sum()))
        if norm > 0:
            profiles[u] = p / norm
            p_bound[u] = 2 * (rows.size + D + 8) * U * (a / norm + np.abs(p) / norm)
        hist.append((Th, w, a, norm))
    centroid, c_bound, nearest, n_bound = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for l in range(n_lists):
        u = l if case["list_hist"] is None else int(case["list_hist"][l])
        if not 0 <= u < n_hists:
            continue
        Th, w, a, norm = hist[u]
        for i in range(int(c_off[l]), int(c_off[l + 1])):
            r = int(case["cand_rows"][i])
            if not 0 <= r < n_rows or w.size == 0:
                continue
            if norm > 0:
                centroid[i] = float(profiles[u] @ T[r])
                c_bound[i] = 2 * (w.size + D + 8) * U * (float(a @ np.abs(T[r])) / norm + abs(centroid[i]))
            nearest[i] = float(np.max(w * (Th @ T[r])))
            n_bound[i] = 2 * (D + 8) * U * float(w.max())
    if case["exact"]:
        p_bound[:], c_bound[:], n_bound[:] = 0.0, 0.0, 0.0
    return dict(profiles=profiles, profiles_bound=p_bound, centroid=centroid, centroid_bound=c_bound, nearest=nearest, nearest_bound=n_bound)


def _lists_for(hists, lengths, rng):
    """one list per length; a list of one candidate reads a "single" history, the others cycle over the normal ones"""
    normal = [u for u, (_, k) in enumerate(hists) if k == "normal"]
    single = [u for u, (_, k) in enumerate(hists) if k == "single"]
    out, k = [], 0
    for length in lengths:
        if length == 1:
            out.append((1, single[k % len(single)]))
        else:
            out.append((length, normal[k % len(normal)]))
        k += 1
    return out


def _dims_case(D):
    def make(seed):
        hists = [(5, "normal"), (1, "single"), (17, "normal"), (3, "absent"), (4, "zero"), (2, "normal"), (70, "normal"), (6, "single")]
        lists = [(5, 0), (1, 1), (18, 2), (3, 3), (4, 4), (2, 5), (17, 6), (1, 7), (3, -1), (2, len(hists)), (12, 6), (0, 0)]
        return build(seed, D, hists, lists)
    return make


def _lengths_case(seed):
    """every history length with a list of a few candidates, every list length against a mid-sized history, at D = 96"""
    hists = [(n, "single" if n == 1 else "normal") for n in LENGTHS if n > 0] + [(0, "normal"), (LONG_HISTORY, "normal"), (9, "single"), (33, "normal")]
    lists = [(3 if hists[u][0] != 1 else 1, u) for u in range(len(hists))]
    mid, one = len(hists) - 1, len(hists) - 2
    lists += [(n, one if n == 1 else mid) for n in LENGTHS]
    return build(seed, 96, hists, lists)


def _shared_case(seed):
    """many lists on one history, runs of empty lists, list_hist of -1 and n_hists"""
    hists = [(20, "normal"), (1, "single"), (40, "normal"), (7, "absent"), (5, "zero")]
    lists = [(0, 0)] * 5 + [(12, 0)] * 30 + [(0, 2)] * 70 + [(7, 2), (1, 1), (4, -1), (4, 5), (0, -1), (6, 3), (6, 4)] + [(0, 1)] * 3
    return build(seed, 64, hists, lists)


def _unweighted_case(seed):
    """hist_weights NULL: every present entry weighs 1 (short histories: one of many equal entries moves no score)"""
    hists = [(1, "single"), (2, "normal"), (3, "normal"), (4, "normal"), (3, "absent"), (5, "single")]
    lists = [(1, 0), (5, 1), (16, 2), (17, 3), (3, 4), (1, 5), (33, 2)]
    return build(seed, 65, hists, lists, weighted=False)


def _identity_case(seed):
    """list_hist NULL: list l reads history l"""
    hists = [(5, "normal"), (1, "single"), (0, "normal"), (18, "normal"), (2, "absent"), (64, "normal")]
    lists = [(4, 0), (1, 1), (3, 2), (0, 3), (5, 4), (20, 5)]
    return build(seed, 256, hists, lists, identity=True)


def _one_list_case(seed):
    return build(seed, 63, [(9, "normal")], [(40, 0)])


def _d1_exact(seed=None):
    """D = 1, rows all +1, power-of-two weights with maximum 1: profiles 1 (0 without a present entry), scores exactly 1 or 0"""
    table = np.ones((8, 1), np.float32)
    h_rows = np.array([0, 3, 7, -1, 2, 8, -1, 5, 1, 1, 4], np.int32)   # histories of 3, 2 (one absent), 2 (all absent), 4
    h_w = np.array([0.25, 0.5, 1.0, 0.5, 1.0, 1.0, 2.0, 0.125, 0.25, 0.5, 1.0], np.float32)
    h_off = np.array([0, 3, 5, 7, 11], np.int64)
    c_rows = np.array([0, 8, 7, 1, -1, 2, 3, 4, 5, 6], np.int32)
    c_off = np.array([0, 3, 5, 7, 9, 10], np.int64)
    list_hist = np.array([0, 1, 2, 3, -1], np.int32)
    return dict(table=table, hist_rows=h_rows, hist_weights=h_w, hist_offsets=h_off, cand_rows=c_rows, cand_offsets=c_off,
                list_hist=list_hist, exact=True)


D1_WANT = np.array([1, 0, 1, 1, 0, 0, 0, 1, 1, 0], np.float64)  # both modes


def _builders():
    b = {f"dims_{D}": _dims_case(D) for D in DIMS}
    b["lengths"] = _lengths_case
    b["shared_and_empty"] = _shared_case
    b["unweighted"] = _unweighted_case
    b["identity"] = _identity_case
    b["one_list"] = _one_list_case
    b["d1_exact"] = _d1_exact
    return b


def synthetic_lookup(behaviors, history, D=24, key="document_vector"):
    """a lookup_dict over the article ids of the two fixture frames, every tenth id left out (unknown ids occur); the vectors are
    3 x unit rows: the class has to normalise them"""
    ids = np.unique(np.concatenate([np.concatenate(list(behaviors["article_ids_inview"])), np.concatenate(list(history["article_id_fixed"]))]))
    kept = ids[np.arange(ids.size) % 10 != 3]
    table = make_table(np.random.default_rng(5), kept.size, D) * 3.0
    return {int(i): {key: table[r]} for r, i in enumerate(kept)}


def frames_case(cs, behaviors, history, weights_of):
    """the operands of ``cs.predict(behaviors, history=history)`` assembled by hand: one history per row of the history frame (cut to
    cs.history_size), ``weights_of(n)`` (a list function of utils/_decay.py, or None) called once per user"""
    hists = [np.asarray(h)[-cs.history_size:] if cs.history_size else np.asarray(h) for h in history["article_id_fixed"]]
    at = {u: k for k, u in enumerate(history["user_id"].tolist())}
    inview = list(behaviors["article_ids_inview"])
    off = lambda lists: np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    w = None if weights_of is None else np.concatenate([np.asarray(weights_of(len(h)), np.float64) for h in hists]).astype(np.float32)
    return dict(table=cs.host_unit_table(), hist_rows=cs.lookup.rows_of(np.concatenate(hists)), hist_weights=w, hist_offsets=off(hists),
                cand_rows=cs.lookup.rows_of(np.concatenate(inview)), cand_offsets=off(inview),
                list_hist=np.array([at.get(u, -1) for u in behaviors["user_id"]], np.int32), exact=False)


BUILDERS = _builders()
NAMES = list(BUILDERS)
BOUNDED = [n for n in NAMES if n != "d1_exact"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(case, reference): built once, shared, read-only"""
    c = BUILDERS[name](NAMES.index(name) + 1)
    ref = reference(c)
    for v in ref.values():
        v.setflags(write=False)
    return c, ref
