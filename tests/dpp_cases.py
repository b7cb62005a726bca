"""Restatement of the greedy DPP selection of ebn_dpp_rerank_f32 / dpp_rerank() / recommend(rerank=DPP(...)) in float64 (and in
float32, to calibrate the rounding error), the greedy-property checker and the case generators shared by tests/test_dpp_cpu.py and
tests/test_dpp_gpu.py.  Independent of the product's host path.

The rule.  Pools, absent entries and flags as in tests/rerank_cases.py.  d(i, j) = min(max(1 - u_i . u_j, 0), 2), a NaN dot
product between two present entries (an entry with itself included) gives 0 and sets flag 1.  S = 1 - d / 2, diagonal as computed.
State: d2_i (initially S(i, i)) and a Cholesky row c_i; EPS = 1e-4f.  Round t picks the present unpicked entry with the largest
obj_i = lam rel_i + (1 - lam) log(max(d2_i, EPS)), larger obj first, equal obj to the smaller pool index.  After picking j: if
d2_j <= EPS nothing changes but c_i[t] = 0; else e_i = (S(j, i) - sum_{s<t} c_j[s] c_i[s]) / sqrt(d2_j), c_i[t] = e_i,
d2_i -= e_i^2, the sum over s ascending.  k rounds or until nothing is left, short lists padded with (-1, -inf)."""
import numpy as np

from tests.rerank_cases import present_mask

EPS = float(np.float32(1e-4))

# (U, P, D, k): smallest D with two users per workgroup and odd U; D off the 32-deep slab, two users per workgroup; the first
# one-user-per-workgroup size with k = P; full pool and k at the document-vector width; pool rank 9 far below k; k > P
SHAPES = [(5, 5, 4, 5), (7, 32, 36, 10), (3, 33, 64, 33), (4, 64, 768, 64), (3, 64, 8, 64), (2, 20, 128, 40)]
LAMS = [0.0, 0.3, 0.7, 1.0]


def shape_id(shape):
    return "x".join(map(str, shape))


def similarity(unit, rows, present, dtype=np.float64):
    """[P, P] similarities of one pool in `dtype` (absent entries: zero vectors, never looked at) and whether a dot product of
    two present entries is NaN"""
    unit = np.asarray(unit, dtype=dtype)
    vec = np.where(present[:, None], unit[np.where(present, rows, 0)], dtype(0))
    with np.errstate(invalid="ignore", over="ignore"):
        dots = vec @ vec.T
    nan = np.isnan(dots)
    dist = np.where(nan, dtype(0), np.minimum(np.maximum(dtype(1) - np.where(nan, dtype(0), dots), dtype(0)), dtype(2)))
    S = (dtype(1) - dist / dtype(2)).astype(dtype)
    return S, bool((nan & present[:, None] & present[None, :]).any())


class Walk:
    """The state of one pool in `dtype`: objective() of every entry, pick(j) the update after entry j"""

    def __init__(self, S, rel, lam, k, dtype=np.float64, oml=None):
        self.dt = dtype
        self.S = S.astype(dtype)
        self.lam, self.oml = dtype(lam), dtype(1) - dtype(lam) if oml is None else dtype(oml)
        self.rel = np.where(np.isfinite(rel), rel, 0.0).astype(dtype)  # an absent entry's relevance is never looked at
        self.d2 = np.diag(self.S).copy()
        self.chol = np.zeros((len(rel), k), dtype)
        self.t = 0

    def objective(self):
        return (self.lam * self.rel + self.oml * np.log(np.maximum(self.d2, self.dt(EPS)))).astype(self.dt)

    def pick(self, j):
        t = self.t
        if self.d2[j] > self.dt(EPS):
            prod = self.chol[:, :t] * self.chol[j, :t][None, :]
            acc = np.add.accumulate(prod, axis=1, dtype=self.dt)[:, -1] if t else np.zeros(len(self.d2), self.dt)  # ascending s
            e = ((self.S[j] - acc) / np.sqrt(self.d2[j])).astype(self.dt)
            self.chol[:, t] = e
            self.d2 = (self.d2 - e * e).astype(self.dt)
        self.t = t + 1


def dpp_reference(unit, rows, rel, k, lam, dtype=np.float64):
    """unit [n_rows, D], rows [U, P] int, rel [U, P] -> sel [U, k] int32, obj [U, k] float64, flags (bad row, non-finite)"""
    rows, rel = np.asarray(rows, dtype=np.int64), np.asarray(rel, dtype=np.float64)
    n_rows = len(unit)
    U, P = rows.shape
    sel = np.full((U, k), -1, np.int32)
    out = np.full((U, k), -np.inf)
    in_range = (rows >= 0) & (rows < n_rows)
    flag0 = bool((~in_range & (rows != -1)).any())
    flag1 = bool((~np.isfinite(rel) & ~np.isneginf(rel)).any())
    for u in range(U):
        present = present_mask(rows[u], rel[u], n_rows)
        S, nan_seen = similarity(unit, rows[u], present, dtype)
        flag1 |= nan_seen
        walk = Walk(S, rel[u], lam, k, dtype)
        left = present.copy()
        for t in range(k):
            if not left.any():
                break
            obj = np.where(left, walk.objective(), -np.inf)
            best = int(np.argmax(obj))  # the first maximum: the smaller pool index
            sel[u, t], out[u, t] = best, obj[best]
            left[best] = False
            walk.pick(best)
    return sel, out, (int(flag0), int(flag1))


def _walk_lists(unit, rows, rel, sel, lam):
    """Both restatements along the prefixes `sel`: per user the list of (left mask, d2_64, obj64) before each round, and
    E32 = max |d2_32 - d2_64| over the present unpicked entries and the rounds of all users"""
    rows, rel = np.asarray(rows, dtype=np.int64), np.asarray(rel, dtype=np.float64)
    k = np.asarray(sel).shape[1]
    lam32 = np.float32(lam)
    lam64, oml64 = float(lam32), float(np.float32(1) - lam32)  # the kernel's fp32 lam and 1 - lam
    e32, rounds = 0.0, []
    for u in range(rows.shape[0]):
        present = present_mask(rows[u], rel[u], len(unit))
        w64 = Walk(similarity(unit, rows[u], present, np.float64)[0], rel[u], lam64, k, np.float64, oml64)
        w32 = Walk(similarity(unit, rows[u], present, np.float32)[0], rel[u], lam32, k, np.float32)
        left = present.copy()
        per_user = []
        for s in np.asarray(sel[u]).tolist():
            if left.any():
                e32 = max(e32, float(np.abs(w32.d2.astype(np.float64) - w64.d2)[left].max()))
            per_user.append((left.copy(), w64.d2.copy(), w64.objective()))
            if s < 0 or not left[s]:
                break
            left[s] = False
            w64.pick(s)
            w32.pick(s)
        rounds.append(per_user)
    return rounds, e32


def tolerances(d2, obj, lam, e32):
    """tol(i) = (1 - lam) delta / max(d2_i - delta, EPS) + 4 * 2^-23 (1 + |obj_i|), delta = max(4 E32, 2^-20): four times the
    float32 restatement's own error in d2 (the margin of the Fastformer tests), carried through the derivative of log at the
    clamped argument; four ulp for lam, 1 - lam, the two products and their sum."""
    delta = max(4.0 * e32, 2.0 ** -20)
    oml = float(np.float32(1) - np.float32(lam))
    return oml * delta / np.maximum(d2 - delta, EPS) + 4 * 2.0 ** -23 * (1.0 + np.abs(obj))


def check_greedy_dpp(unit, rows, rel, sel, obj, lam):
    """The greedy property of lists `sel` [U, k] (with objectives `obj`, or None): no repeats, no absent entry, the padding only
    once nothing is left; every pick s, GIVEN the earlier picks of the list, has obj64(s) >= obj64(best) - tol(s) - tol(best),
    and |obj - obj64(s)| <= tol(s).  -> (largest shortfall against the best, largest |obj - float64|, E32)."""
    rounds, e32 = _walk_lists(unit, rows, rel, sel, lam)
    worst_gap, worst_obj = 0.0, 0.0
    for u, per_user in enumerate(rounds):
        picks = np.asarray(sel[u]).tolist()
        for t, (left, d2, o64) in enumerate(per_user):
            s = picks[t]
            if s < 0:
                assert not left.any(), (u, t, "padding while entries are left")
                assert (np.asarray(sel[u][t:]) == -1).all() and (obj is None or np.isneginf(obj[u][t:]).all()), (u, t)
                break
            assert left[s], (u, t, s, "absent or repeated")
            tol = tolerances(d2, o64, lam, e32)
            best = int(np.argmax(np.where(left, o64, -np.inf)))
            gap = float(o64[best] - o64[s])
            worst_gap = max(worst_gap, gap)
            assert gap <= tol[s] + tol[best], (u, t, s, best, gap, tol[s], tol[best])
            if obj is not None:
                err = abs(float(obj[u][t]) - float(o64[s]))
                worst_obj = max(worst_obj, err)
                assert err <= tol[s], (u, t, s, err, tol[s])
        assert len(per_user) == len(picks) or picks[len(per_user) - 1] < 0, (u, "the walk stopped early")
    return worst_gap, worst_obj, e32


def margin_ok(unit, rows, rel, k, lam, factor=100.0):
    """(ok, sel): whether the float64 reference's best entry leads the runner-up by at least factor * (tol(best) + tol(runner-up))
    in every round of every user, the tolerances taken along the reference's own picks"""
    sel = dpp_reference(unit, rows, rel, k, lam)[0]
    rounds, e32 = _walk_lists(unit, rows, rel, sel, lam)
    for per_user in rounds:
        for left, d2, o64 in per_user:
            if left.sum() < 2:
                continue
            tol = tolerances(d2, o64, lam, e32)
            order = np.argsort(-np.where(left, o64, -np.inf), kind="stable")
            a, b = int(order[0]), int(order[1])
            if o64[a] - o64[b] < factor * (tol[a] + tol[b]):
                return False, sel
    return True, sel


def dpp_case(U, P, D, seed):
    """Standard-normal rows normalised in float32 (a table of 4 P rows), uniform relevances; every pool holds P - 1 distinct rows
    and, when P >= 2, one duplicate of its first row at another place (with its own relevance); about 10 % padding when P >= 20."""
    rng = np.random.default_rng(seed)
    n_rows = 4 * P
    x = rng.standard_normal((n_rows, D)).astype(np.float32)
    unit = (x / np.sqrt((x * x).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    rows = np.stack([rng.choice(n_rows, P, replace=False) for _ in range(U)]).astype(np.int32)
    if P >= 2:
        rows[np.arange(U), rng.integers(1, P, U)] = rows[:, 0]
    rel = rng.random((U, P)).astype(np.float32)
    if P >= 20:
        gone = rng.random((U, P)) < 0.1
        gone[:, 0] = False
        rows[gone], rel[gone] = -1, -np.inf
    return unit, rows, rel
