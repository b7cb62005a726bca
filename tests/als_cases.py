"""Cases, the float64 brute force and the DERIVED bound of the implicit-ALS kernels and twins (plain helpers: nothing is collected
from here).

BRUTE FORCE: per row, A = gram + reg I + sum_k a_k y_k y_k^T and b = sum_k (1 + a_k) y_k are formed entry by entry in float64 from the
float32 operands (gram as the float32 matrix the kernel is handed, reg as a float32), together with ``Aabs`` / ``babs``, the same
sums over the absolute values of the terms; x* = numpy.linalg.solve in float64.

CASES (``solve_case(F)``), F in {1, 3, 4, 33, 64, 128} (33: no multiple of 4, above half a wave; 128: the LDS limit): 300 fixed rows,
values (random sign) and confidences 2^uniform(-6, 6) in float32; rows of 0, 1, 2, T - 1, T, T + 1 and 2 T + 1 entries for the kernel's
staging tile T; a row whose entries are all absent (-1, n_fixed, n_fixed + 5); a row of present and absent entries; a row with a
repeated column; one LONG row of 3 * SPLIT_SMALL + 7 entries with its part tables for split_len = SPLIT_SMALL = 64 (solved once
directly and once through the partials).  reg is 1.0 or 0.01 depending on F.
BREAKDOWN (``breakdown_case``): F = 2, gram zeros, reg = 1e-30, one entry y = (1, 1) with a = 1: A = [[1, 1], [1, 1]] in float32 (and in
float64), the second pivot is exactly 0: the row must be NaN.

BOUND (derived, not measured).  u = 2^-24, gamma_k = k u / (1 - k u), n = the row's present entries (on the partials route: the
number of parts plus the longest part).  The float64 residual of a computed row x^ against the brute-force system satisfies

    ||b - A x^||_2 <= (gamma_{n+4} ||Aabs||_F + F gamma_{3F+1} ||A||_2) ||x^||_2 + gamma_{n+2} ||babs||_2

First and last term: forming A and b in float32 -- two roundings per product a_k y_i y_j, at most n + 2 adds with gram and reg (a
part's sum is rounded when stored and the parts are added: n as defined above), any order, with or without fma; for b one rounding
of 1 + a_k, one of the product, n adds.  Middle term: Higham's backward error of a Cholesky solve, |dA| <= gamma_{3F+1} |R^T||R| with
|| |R^T||R| ||_2 <= F ||A||_2 (Accuracy and Stability of Numerical Algorithms, 2nd ed., theorem 10.4 and (10.7)).  Correctly rounded
sqrt and division are assumed.  Forward form (lambda_min(A) >= reg): ||x^ - x*||_2 <= residual bound / reg.
``check_reference`` asserts that the brute force's own residual stays below a hundredth of this bound."""
import functools

import numpy as np

U = 2.0 ** -24
TILE = 16          # ALS_T of csrc/ebn_als.hip: entries of a staged tile
SPLIT_LEN = 4096   # the default split_len of ImplicitALS
SPLIT_SMALL = 64
MAX_F = 128
FS = [1, 3, 4, 33, 64, 128]
REG = {1: 1.0, 3: 0.01, 4: 1.0, 33: 0.01, 64: 0.01, 128: 1.0}
N_FIXED = 300
ROW_LENGTHS = [0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- brute force ---------------------------------------------------------------------------------------------------------------
def brute_row(fixed, gram, reg, cols, conf):
    """one row's system from its entries -> dict(A, b, x, n, normAabs, normA2, normbabs)"""
    n_fixed, F = fixed.shape
    reg = float(np.float32(reg))
    A = np.zeros((F, F))
    Aabs = np.zeros((F, F))
    b, babs = np.zeros(F), np.zeros(F)
    n = 0
    for c, a in zip([int(c) for c in cols], [float(a) for a in conf]):
        if not 0 <= c < n_fixed:
            continue
        n += 1
        y = [float(v) for v in fixed[c]]
        for i in range(F):
            b[i] += (1.0 + a) * y[i]
            babs[i] += abs((1.0 + a) * y[i])
        yy = np.outer(np.array(y), np.array(y))  # exact products of float32 values in float64
        A += a * yy
        Aabs += abs(a) * np.abs(yy)
    for i in range(F):
        for j in range(F):
            g = float(gram[i, j]) if i >= j else float(gram[j, i])  # the kernel reads the lower triangle
            A[i, j] += g
            Aabs[i, j] += abs(g)
        A[i, i] += reg
        Aabs[i, i] += reg
    return dict(A=A, b=b, n=n, x=np.linalg.solve(A, b) if n else np.zeros(F), normAabs=float(np.linalg.norm(Aabs)),
                normA2=float(np.linalg.norm(A, 2)), normbabs=float(np.linalg.norm(babs)))


def residual_bound(ref, xhat, n=None):
    """the bound above for one row; ``n``: present entries (default), or parts + longest part on the partials route"""
    F = ref["b"].size
    n = ref["n"] if n is None else n
    return (gamma(n + 4) * ref["normAabs"] + F * gamma(3 * F + 1) * ref["normA2"]) * float(np.linalg.norm(xhat)) + gamma(n + 2) * ref["normbabs"]


def residual(ref, xhat):
    return float(np.linalg.norm(ref["b"] - ref["A"] @ np.asarray(xhat, np.float64)))


def check_rows(out, refs, what, n_of=None):
    """every row of ``out`` [n, F] float32 against its reference: exact +0 where the row has no present entry, the residual bound
    elsewhere (a NaN fails); prints the largest observed / bound.  ``n_of``: {row: n} overrides (the partials route)"""
    assert out.dtype == np.float32 and out.shape == (len(refs), refs[0]["b"].size), (what, out.dtype, out.shape)
    worst = 0.0
    for r, ref in enumerate(refs):
        n = (n_of or {}).get(r, ref["n"])
        if n == 0:
            assert not out[r].view(np.int32).any(), f"{what}: row {r} without a present entry is not exact +0: {out[r]}"
            continue
        res, bound = residual(ref, out[r]), residual_bound(ref, out[r], n)
        assert res <= bound, f"{what}: row {r} (n = {n}): residual {res:.3e} above its bound {bound:.3e} ({int(np.isnan(out[r]).sum())} NaN)"
        worst = max(worst, res / bound)
    print(f"{what}: largest residual / bound = {worst:.3e}")
    return worst


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def _pow2(rng, shape, signed=False):
    v = np.exp2(rng.uniform(-6.0, 6.0, shape))
    return (v * rng.choice([-1.0, 1.0], shape) if signed else v).astype(np.float32)


@functools.lru_cache(maxsize=None)
def solve_case(F):
    """dict(fixed [300, F], gram [F, F] float32, reg, indptr, cols, conf, long_row, all_absent, row_parts / part_begin / part_end for
    SPLIT_SMALL); shared and read-only"""
    rng = np.random.default_rng(500 + F)
    fixed = _pow2(rng, (N_FIXED, F), signed=True)
    gram = (fixed.astype(np.float64).T @ fixed.astype(np.float64)).astype(np.float32)
    rows = [rng.integers(0, N_FIXED, n) for n in ROW_LENGTHS]
    all_absent = len(rows)
    rows.append(np.array([-1, N_FIXED, N_FIXED + 5]))
    mixed = rng.integers(0, N_FIXED, TILE + 3)
    mixed[[0, 5, TILE]] = [-1, N_FIXED, N_FIXED + 5]
    rows.append(mixed)
    rep = rng.integers(0, N_FIXED, 6)
    rep[4] = rep[1]  # a repeated column: counts twice
    rows.append(rep)
    long_row = len(rows)
    long = rng.integers(0, N_FIXED, 3 * SPLIT_SMALL + 7)
    long[[3, 70, 198]] = [-1, N_FIXED, N_FIXED + 5]
    rows.append(long)
    rows.append(rng.integers(0, N_FIXED, 5))  # a short row behind the long one
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    cols = np.concatenate(rows).astype(np.int32)
    conf = _pow2(rng, cols.size)
    length = np.diff(indptr)
    n_of = np.where(length > SPLIT_SMALL, -(-length // SPLIT_SMALL), 0)
    row_parts = np.concatenate([[0], np.cumsum(n_of)]).astype(np.int64)
    begin = indptr[long_row] + SPLIT_SMALL * np.arange(int(n_of[long_row]), dtype=np.int64)
    case = dict(F=F, fixed=fixed, gram=gram, reg=REG[F], indptr=indptr, cols=cols, conf=conf, long_row=long_row, all_absent=all_absent,
                row_parts=row_parts, part_begin=begin, part_end=np.minimum(begin + SPLIT_SMALL, indptr[long_row + 1]))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def reference(F):
    """the brute-force rows of ``solve_case(F)``, computed once"""
    c = solve_case(F)
    return [brute_row(c["fixed"], c["gram"], c["reg"], c["cols"][a:b], c["conf"][a:b]) for a, b in zip(c["indptr"][:-1], c["indptr"][1:])]


def parts_n(c):
    """{long row: parts + longest part}: the n of the bound on the partials route"""
    n_parts = c["part_begin"].size
    return {c["long_row"]: n_parts + int((c["part_end"] - c["part_begin"]).max())}


def check_reference(F):
    """the float64 brute force's own residual is below a hundredth of the bound of its own solution"""
    for r, ref in enumerate(reference(F)):
        if ref["n"]:
            assert residual(ref, ref["x"]) <= 0.01 * residual_bound(ref, ref["x"]), (F, r)


def breakdown_case():
    return dict(F=2, fixed=np.ones((1, 2), np.float32), gram=np.zeros((2, 2), np.float32), reg=1e-30, indptr=np.array([0, 1], np.int64),
                cols=np.zeros(1, np.int32), conf=np.ones(1, np.float32))


def random_problem(seed, n_users=7, n_items=9, F=3):
    """a small dense-able problem for the loss test: (X, Y float32, indptr, cols ascending per row without repeats, conf)"""
    rng = np.random.default_rng(seed)
    X, Y = rng.standard_normal((n_users, F)).astype(np.float32), rng.standard_normal((n_items, F)).astype(np.float32)
    rows = [np.sort(rng.choice(n_items, int(rng.integers(0, n_items + 1)), replace=False)) for _ in range(n_users)]
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    cols = np.concatenate(rows).astype(np.int32)
    return X, Y, indptr, cols, _pow2(rng, cols.size)


# ---- whole half-sweeps (the class tests) ---------------------------------------------------------------------------------------------
def half_sweep_rows(fixed, indptr, cols, conf, reg, gram=None):
    """per row of a half-sweep (CSR with duplicates combined, every column known) the float64 system and the norms of the bound:
    yields (r, dict(A, b, n, normAabs, normA2, normbabs)); rows without an entry are skipped.  ``gram``: the float32 matrix the
    kernel was handed (default: the float64 Gram of ``fixed``)"""
    Y = np.asarray(fixed).astype(np.float64)
    F = Y.shape[1]
    G = Y.T @ Y if gram is None else np.asarray(gram).astype(np.float64)
    G = np.tril(G) + np.tril(G, -1).T
    base, base_abs = G + float(np.float32(reg)) * np.eye(F), np.abs(G) + float(np.float32(reg)) * np.eye(F)
    for r in range(indptr.size - 1):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        if hi <= lo:
            continue
        y, a = Y[cols[lo:hi]], np.asarray(conf[lo:hi]).astype(np.float64)
        A, Aabs = base + (y.T * a) @ y, base_abs + (np.abs(y).T * a) @ np.abs(y)
        yield r, dict(A=A, b=((1.0 + a)[:, None] * y).sum(axis=0), n=hi - lo, normAabs=float(np.linalg.norm(Aabs)),
                      normA2=float(np.linalg.norm(A, 2)), normbabs=float(np.linalg.norm(((1.0 + a)[:, None] * np.abs(y)).sum(axis=0))))


def half_sweep_residuals(fixed, indptr, cols, conf, reg, solved):
    """sum over the rows of ||b_r - A_r x_r||^2 in float64 (exact Gram of ``fixed``): what a computed half-sweep may exceed the
    exact minimiser by, times 1 / reg"""
    solved = np.asarray(solved).astype(np.float64)
    return float(sum(np.sum((ref["b"] - ref["A"] @ solved[r]) ** 2) for r, ref in half_sweep_rows(fixed, indptr, cols, conf, reg)))


FIT_KW = dict(factors=32, regularization=0.01, alpha=400.0, history_size=30)
"""Why these: the first half-sweep can only halve L when the users can reach p = 1 on their items against item factors of scale 0.01.
With at most history_size = 30 <= F distinct items a user can interpolate them (x~ = pinv(Y_s) 1), at the price of the all-pairs term
x~^T Y^T Y x~ ~ n_u n_items / F (Y^T Y ~ n_items sigma^2 I, |y|^2 ~ F sigma^2); before, the user's share of L is (1 + alpha) n_u.  The exact
minimiser is no worse than x~: L_after / L_before <~ (n_items / F) / (1 + alpha) = (2194 / 32) / 401 = 0.17."""


def check_monotone(models, host=lambda t: t):
    """after every half-sweep L_after <= L_before + sum_r ||r_r||^2 / reg (exact ALS never increases L; a computed row exceeds its
    minimum by r^T A^-1 r <= ||r||^2 / reg), and the first half-sweep more than halves L.  ``models``: fits of 1, 2, 3 sweeps."""
    from ebrec.models.baselines.als import als_loss_host

    last = models[-1]
    users, items = (side.host() for side in last._sides)
    reg, F = last.regularization, last.factors
    Y = (np.random.default_rng(last.seed).standard_normal((len(last.article_ids), F)).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    X = np.zeros((users[0].size - 1, F), np.float32)
    before = als_loss_host(X, Y, *users, reg)
    losses = last.losses
    assert losses.dtype == np.float64 and losses.size == 6 and losses[0] < 0.5 * before, (before, losses)
    for k, m in enumerate(models):
        assert np.array_equal(m.losses, losses[:2 * k + 2])  # the shorter fits are prefixes of the longest
        X = host(m.user_factors)
        slack = half_sweep_residuals(Y, *users, reg, X) / reg
        print(f"sweep {k + 1} users: L {before:.9e} -> {losses[2 * k]:.9e}, slack {slack:.3e}")
        assert losses[2 * k] <= before + slack
        Y = host(m.item_factors)
        slack = half_sweep_residuals(X, *items, reg, Y) / reg
        print(f"sweep {k + 1} items: L {losses[2 * k]:.9e} -> {losses[2 * k + 1]:.9e}, slack {slack:.3e}")
        assert losses[2 * k + 1] <= losses[2 * k] + slack
        before = losses[2 * k + 1]
