"""The shared case of the score-blending tests and a plain-Python brute force of its contract (include/ebnerd_hip.h, "score
blending"): per-list transforms, the weighted sum, and loss / gradient / centred Hessian of the listwise softmax cross-entropy.
Independent of the numpy twins of ebrec/models/ensemble.py: Python floats, list by list, item by item, sums with math.fsum.

THE CASE.  List lengths 0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500 -- both sides of every boundary
between the kernels' forms (16-lane group, wave, workgroup; 256- and 1024-item tiles) -- then 200 lists of 2 to 30: about 10 k
items.  Sixteen sources: source 0 is scaled by 1e6, source 1 is rounded to integers (many ties), source 2 is constant on every
seventh list, the others are plain normals.  One positive per list drawn from a softmax of a latent score, a second one in about
10 % of the lists, lists 40 / 41 all negative, 42 / 43 all positive.  Source 0 holds a NaN in list 25, source 1 a NaN in list 20 and
an inf in list 30.  ``offsets_bad`` appends one malformed list (it ends past n_items) for the calls that take raw offsets.

Computed once per process and never written to (the arrays are read-only)."""
import functools
import math

import numpy as np

RAW, ZSCORE, MINMAX, RANK, RRF = range(5)
KIND_NAMES = ["raw", "zscore", "minmax", "rank", "rrf"]
RRF_K = 60.0
FIXED_LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500]
N_SOURCES = 16
FIT_SOURCES = [3, 1, 2, 4, 5, 6]  # the M = 6 blend: kinds raw, zscore, minmax, rank, rrf, zscore
FIT_KINDS = [RAW, ZSCORE, MINMAX, RANK, RRF, ZSCORE]
FIT_L2 = 1e-3
ALL_NEGATIVE, ALL_POSITIVE = (40, 41), (42, 43)
NONFINITE = {0: [(25, 1, float("nan"))], 1: [(20, 1, float("nan")), (30, 0, float("inf"))]}  # source: (list, position, value)
U32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def case():
    rng = np.random.default_rng(20251021)
    lengths = np.array(FIXED_LENGTHS + rng.integers(2, 31, 200).tolist(), np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n, n_lists = int(offsets[-1]), len(lengths)
    lid = np.repeat(np.arange(n_lists), lengths)
    S = rng.normal(size=(N_SOURCES, n))
    latent = 1.2 * S[3] + 0.8 * S[1] + 0.6 * S[4] + 0.5 * S[5] + 0.4 * S[2] + 0.3 * S[6]
    S[0] *= 1e6
    S[1] = np.round(2.0 * S[1])
    const = (lid % 7 == 3)
    S[2] = np.where(const, np.round(S[2][offsets[lid]], 1), S[2])
    for m, spots in NONFINITE.items():
        for l, pos, v in spots:
            S[m, offsets[l] + pos] = v
    labels = np.zeros(n, np.uint8)
    for l in range(n_lists):
        a, b = int(offsets[l]), int(offsets[l + 1])
        if b == a:
            continue
        p = np.exp(latent[a:b] - latent[a:b].max())
        labels[a + rng.choice(b - a, p=p / p.sum())] = 1
        if b - a >= 3 and rng.random() < 0.1:
            labels[a + rng.integers(0, b - a)] = 1
    for l in ALL_NEGATIVE:
        labels[offsets[l]:offsets[l + 1]] = 0
    for l in ALL_POSITIVE:
        labels[offsets[l]:offsets[l + 1]] = 1
    out = dict(offsets=offsets, offsets_bad=np.append(offsets, n + 7).astype(np.int64), lengths=lengths, labels=labels, n=n, n_lists=n_lists,
               scores64=S, scores32=S.astype(np.float32))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def scores(kind_of_scores: int):
    """the [16, n] sources as float32 (0) or float64 (1)"""
    return case()["scores32" if kind_of_scores == 0 else "scores64"]


def well_formed(offsets, n_items):
    """[(begin, end)] per list; a list whose offsets leave [0, n_items] or run backwards is empty"""
    off = [int(o) for o in offsets]
    return [(a, b) if 0 <= a <= b <= n_items else (0, 0) for a, b in zip(off[:-1], off[1:])]


def midranks(v):
    """r_i = 1 + #{v_j > v_i} + #{j != i: v_j == v_i} / 2 of a list of Python floats (none of them NaN)"""
    order = sorted(range(len(v)), key=lambda i: -v[i])
    r, k = [0.0] * len(v), 0
    while k < len(order):
        e = k
        while e + 1 < len(order) and v[order[e + 1]] == v[order[k]]:
            e += 1
        for i in order[k:e + 1]:
            r[i] = 1.0 + k + 0.5 * (e - k)
        k = e + 1
    return r


@functools.lru_cache(maxsize=None)
def source_reference(m: int, kind_of_scores: int, bad_offsets: bool = True):
    """Source m of the case under EVERY transform -> (want [5, n] float64: the features before their rounding to float32, bound
    [5, n]: the error a correct implementation may show after it, nonfinite [n_lists] bool).

    Bounds: RAW 0 (the float32 rounding of the score itself is applied to `want`); RANK and RRF one float32 ulp (exact integer
    counts, one float64 division, one rounding); ZSCORE and MINMAX 2^-23 |f| + n 2^-50 max|s| / scale with scale = sd or max - min:
    one float32 rounding plus the float64 summation error of mean and sd amplified by the normalisation."""
    c = case()
    s = [float(x) for x in scores(kind_of_scores)[m]]
    n = c["n"]
    want, bound = np.zeros((5, n)), np.zeros((5, n))
    lists = well_formed(c["offsets_bad"] if bad_offsets else c["offsets"], n)
    nonfinite = np.zeros(len(lists), bool)
    for l, (a, b) in enumerate(lists):
        v, k = s[a:b], b - a
        if k == 0:
            continue
        for i in range(k):
            want[RAW, a + i] = float(np.float32(v[i]))
        if not all(math.isfinite(x) for x in v):
            nonfinite[l] = True
            want[1:, a:b] = np.nan
            continue
        mean = math.fsum(v) / k
        sd = math.sqrt(math.fsum((x - mean) ** 2 for x in v) / k)
        mn, mx = min(v), max(v)
        top = max(abs(x) for x in v)
        r = midranks(v)
        for i in range(k):
            z = 0.0 if (sd == 0.0 or mx == mn) else (v[i] - mean) / sd
            mm = 0.0 if mx == mn else (v[i] - mn) / (mx - mn)
            rk = 0.0 if k == 1 else (k - r[i]) / (k - 1)
            rrf = 1.0 / (RRF_K + r[i])
            want[1:, a + i] = (z, mm, rk, rrf)
            bound[ZSCORE, a + i] = 2.0 ** -23 * abs(z) + (0.0 if mx == mn else k * 2.0 ** -50 * top / sd)
            bound[MINMAX, a + i] = 2.0 ** -23 * abs(mm) + (0.0 if mx == mn else k * 2.0 ** -50 * top / (mx - mn))
            bound[RANK, a + i] = float(np.spacing(np.float32(abs(rk))))
            bound[RRF, a + i] = float(np.spacing(np.float32(rrf)))
    for x in (want, bound, nonfinite):
        x.setflags(write=False)
    return want, bound, nonfinite


def features_reference(sources, kinds, kind_of_scores: int, bad_offsets: bool = True):
    """-> (want [M, n], bound [M, n], flags [n_lists] uint8) of the given sources under the given kinds"""
    refs = [source_reference(m, kind_of_scores, bad_offsets) for m in sources]
    want = np.stack([r[0][k] for r, k in zip(refs, kinds)])
    bound = np.stack([r[1][k] for r, k in zip(refs, kinds)])
    flags = np.where(np.any([r[2] for r in refs], axis=0), 2, 0).astype(np.uint8)
    return want, bound, flags


def brute_sums(features, labels, offsets, weights):
    """loss, gradient and centred Hessian of the listwise softmax cross-entropy over features [M][n] (any floats), list by list in
    Python floats -> (sums [1 + M + M (M + 1) / 2], counters [used, one-class, not finite], abs_sums: the sums of the absolute
    terms of every entry)."""
    F = [[float(x) for x in row] for row in features]
    M, n = len(F), len(F[0])
    y = [int(v != 0) for v in labels]
    w = [float(x) for x in weights]
    n_e = 1 + M + M * (M + 1) // 2
    terms, aterms = [[] for _ in range(n_e)], [[] for _ in range(n_e)]
    counters = [0, 0, 0]
    for a, b in well_formed(offsets, n):
        n_pos = sum(y[a:b])
        if not 0 < n_pos < b - a:
            counters[1] += 1
            continue
        if not all(math.isfinite(F[m][i]) for m in range(M) for i in range(a, b)):
            counters[2] += 1
            continue
        counters[0] += 1
        z = [math.fsum(w[m] * F[m][i] for m in range(M)) for i in range(a, b)]
        top = max(z)
        e = [math.exp(x - top) for x in z]
        S = math.fsum(e)
        p = [x / S for x in e]
        t = [y[i] / n_pos for i in range(a, b)]
        loss = -math.fsum(t[i] * ((z[i] - top) - math.log(S)) for i in range(b - a) if t[i])
        terms[0].append(loss), aterms[0].append(abs(loss))
        u = [math.fsum(p[i] * F[m][a + i] for i in range(b - a)) for m in range(M)]
        k = 1 + M
        for m in range(M):
            g = [(p[i] - t[i]) * F[m][a + i] for i in range(b - a)]
            terms[1 + m].append(math.fsum(g)), aterms[1 + m].append(math.fsum(abs(x) for x in g))
            cm = [F[m][a + i] - u[m] for i in range(b - a)]
            for m2 in range(m, M):
                h = [p[i] * (cm[i] * (F[m2][a + i] - u[m2])) for i in range(b - a)]
                terms[k].append(math.fsum(h)), aterms[k].append(math.fsum(abs(x) for x in h))
                k += 1
    return (np.array([math.fsum(x) for x in terms]), np.array(counters, np.int64), np.array([math.fsum(x) for x in aterms]))


def fit_features(kind_of_scores: int = 1):
    """the brute-force features of the M = 6 blend, rounded to float32 as the contract says: [6, n] float32"""
    want, _, flags = features_reference(FIT_SOURCES, FIT_KINDS, kind_of_scores, bad_offsets=False)
    return want.astype(np.float32), flags


def objective(sums, counters, w, l2=FIT_L2):
    """J(w) and its gradient from a sums vector"""
    M, n = len(w), int(counters[0])
    return sums[0] / n + 0.5 * l2 * float(np.dot(w, w)), sums[1:1 + M] / n + l2 * np.asarray(w)
