"""The entries of csrc/ebn_ease.hip through the C ABI on guard-banded operands with padded leading dimensions, against the numpy
twins and the float64 brute force of tests/ease_cases.py -- the Gram matrix bit for bit, the inverse within
C * kappa * eps32 * max |P_ref| (tests/ease_cases.py has the reasoning and the measured ratios behind C), the scores within their
derived bound -- and ``EASE`` on the device against the host path.

Every input sits inside poison (tests/guarded.py), with the choices of tests/test_knn_gpu.py: int64 arrays as pairs of int32 words
inside zero words, rows and history indices inside VALID indices (an over-read entry is used and shows), weights and matrices
inside NaN / 3e18.  Outputs are written into canary buffers: guards and padding columns intact."""
import ctypes
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from ebrec.models import ease_gram_host, ease_invert_host, ease_system_host, ease_weights_host
from tests import ease_cases as ec
from tests import guarded

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
POISON = 3.0e18
GUARD = 16384
GOLDEN = Path(__file__).resolve().parent / "golden" / "ebnerd"
P = lambda t: ctypes.c_void_p(t.data_ptr())
F = ctypes.c_float


@pytest.fixture(scope="module")
def NB(hip):
    return int(hip.lib().ebn_ease_block())


def _guard_i64(x):
    """an int64 operand as int32 words inside guards of zero words -> (pointer, handle)"""
    view, h = guarded.guard_in(np.ascontiguousarray(np.asarray(x, np.int64)).view(np.int32), fill=0, guard=GUARD)
    return P(view), h


def _inout(values, ld, dtype=torch.float32):
    """an in/out matrix at row stride ld inside canaries: guards and padding columns must survive, the payload may change"""
    values = np.asarray(values)
    view, h = guarded.guard_out(values.shape, ld=ld, dtype=dtype)
    h.fill_payload(values)
    return view, h


def _scratch(shape, ld=None, dtype=torch.float32, guard=None):
    """an output that need not be written everywhere (the lower triangle of G, a workspace): pre-filled, only the canaries checked"""
    view, h = guarded.guard_out(shape, ld=ld, dtype=dtype, guard=guard)
    h.prefilled = False
    return view, h


# ---- gram ----------------------------------------------------------------------------------------------------------------------
def _run_gram(hip, n):
    indptr, cols, _ = ec.gram_case(n)
    p_ind, h_ind = _guard_i64(indptr)
    t_cols, h_cols = guarded.guard_in(cols, fill=0, guard=GUARD)  # a valid column in the guards: an over-read entry is counted
    G, h = _scratch((n, n), ld=n + 3, dtype=torch.int32)
    assert hip.lib().ebn_ease_gram_i32(p_ind, P(t_cols), indptr.size - 1, cols.size, n, P(G), n + 3, hip.stream_handle()) == OK
    torch.cuda.synchronize()
    h_ind.check("indptr")
    h_cols.check("cols")
    h.check("G")
    return h.payload().cpu().numpy()


@pytest.mark.parametrize("n", [1, 5, 300])
def test_gram_equals_the_twin_bit_for_bit(hip, n):
    indptr, cols, rows = ec.gram_case(n)
    assert {0, 1, 60} <= {len(r) for r in rows} and cols.min() == -1 and cols.max() > n
    want = ease_gram_host(indptr, cols, n)
    got = _run_gram(hip, n)
    low = np.tril(np.ones((n, n), bool))
    assert np.array_equal(got[low], want[low]) and want.any()
    pre = np.int32(guarded.PREFILL_I32)
    assert (got[~low] == pre).all()  # the upper triangle is not touched
    assert np.array_equal(_run_gram(hip, n), got)  # integer atomics: two runs, the same bits


# ---- system --------------------------------------------------------------------------------------------------------------------
def _run_system(hip, G, reg, lda):
    n = G.shape[0]
    t_G, h_G = guarded.guard_in(G, ld=n + 2, fill=(1 << 24) + 5)  # an over-read count would raise the flag
    A, h_A = guarded.guard_out((n, n), ld=lda)
    flag, h_flag = _inout(np.zeros(1, np.int32), 1, torch.int32)
    assert hip.lib().ebn_ease_system_f32(P(t_G), n + 2, n, F(reg), P(A), lda, P(flag), hip.stream_handle()) == OK
    torch.cuda.synchronize()
    h_G.check("G")
    h_A.check("A")
    h_flag.check("flag")
    return h_A.payload().cpu().numpy(), int(h_flag.payload().item())


@pytest.mark.parametrize("n", [1, 5, 300])
def test_system_mirrors_the_lower_triangle_and_adds_reg(hip, n):
    indptr, cols, _ = ec.gram_case(n)
    G = ease_gram_host(indptr, cols, n)
    G[np.triu_indices(n, 1)] = 77777  # never read
    for lda in (n, n + 5):
        A, flag = _run_system(hip, G, 2.5, lda)
        assert flag == 0 and np.array_equal(A.view(np.int32), ease_system_host(G, 2.5).view(np.int32))
        assert np.array_equal(A, A.T)


def test_system_flags_a_count_above_two_to_the_24(hip):
    G = np.array([[5, 0, 0], [1, 1 << 24, 0], [2, 3, 7]], np.int32)
    assert _run_system(hip, G, 1.0, 3)[1] == 0  # 2^24 itself is exact
    G[2, 1] = (1 << 24) + 1
    A, flag = _run_system(hip, G, 1.0, 8)
    assert flag == 1 and A[2, 1] == A[1, 2] == np.float32((1 << 24) + 1)
    G[2, 1], G[0, 2] = 3, (1 << 24) + 1  # above the diagonal: not read, not flagged
    assert _run_system(hip, G, 1.0, 3)[1] == 0


# ---- invert --------------------------------------------------------------------------------------------------------------------
def _run_invert(hip, A32, lda, nb=None):
    n = A32.shape[0]
    low = np.array(A32)
    low[np.triu_indices(n, 1)] = np.nan  # only the lower triangle is read
    A, h_A = _inout(low, lda)
    floats = int(hip.lib().ebn_ease_workspace_floats(n))
    work, h_work = _scratch((floats,), guard=GUARD)  # NaN inside: written before it is read
    info, h_info = guarded.guard_out((1,), dtype=torch.int32)
    L, st = hip.lib(), hip.stream_handle()
    rc = L.ebn_ease_invert_f32(P(A), lda, n, P(work), floats, P(info), st) if nb is None else \
        L.ebn_ease_invert_nb_f32(P(A), lda, n, P(work), floats, P(info), nb, st)
    assert rc == OK
    torch.cuda.synchronize()
    h_A.check("A")
    h_work.check("work")
    h_info.check("info")
    return h_A.payload().cpu().numpy(), int(h_info.payload().item())


def _check_inverse(got, n, what):
    """symmetry bit for bit; the error and the residual within C kappa eps32 (max |P_ref| and 1); returns the two ratios to
    kappa eps32 that C is set from"""
    _, A64, P_ref = ec.spd_case(n)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), got.T.view(np.int32)), what
    k = ec.kappa(A64)
    err = float(np.abs(got.astype(np.float64) - P_ref).max())
    res = float(np.abs(A64 @ got.astype(np.float64) - np.eye(n)).max())
    r_err, r_res = err / (k * ec.EPS32 * np.abs(P_ref).max()), res / (k * ec.EPS32)
    print(f"{what}: kappa {k:.4g}  error {err:.3e} = {r_err:.4f} kappa eps32 max|P|  residual {res:.3e} = {r_res:.4f} kappa eps32  (C = {ec.INVERT_C})")
    assert err <= ec.invert_bound(A64, P_ref), what  # NaN fails
    assert res <= ec.residual_bound(A64), what
    return r_err, r_res


def test_inverse_against_the_float64_reference(hip, NB):
    """n in {1, 2, NB - 1, NB, NB + 1, 2 NB + 3, 300} at lda = n and n + 5; the ratios printed here are the ones C is set from"""
    worst = (0.0, 0.0)
    for n in ec.invert_sizes(NB):
        A32 = ec.spd_case(n)[0]
        for lda in (n, n + 5):
            got, info = _run_invert(hip, A32, lda)
            assert info == 0
            r = _check_inverse(got, n, f"n={n} lda={lda} NB={NB}")
            worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"worst ratios over the cases: error {worst[0]:.4f}, residual {worst[1]:.4f}")


@pytest.mark.parametrize("nb", [32, 64, 128])
def test_inverse_at_every_block_size_and_two_runs_give_the_same_bits(hip, nb):
    for n in (nb + 1, 300):
        A32 = ec.spd_case(n)[0]
        got, info = _run_invert(hip, A32, n + 5, nb)
        assert info == 0
        _check_inverse(got, n, f"n={n} nb={nb}")
        again, _ = _run_invert(hip, A32, n + 5, nb)
        assert np.array_equal(again.view(np.int32), got.view(np.int32))


def test_info_names_the_first_pivot_that_is_not_positive(hip):
    """each case is one call that returns normally; the twin names the same pivot"""
    got, info = _run_invert(hip, np.array([[1, 2], [2, 1]], np.float32), 2)
    assert info == 2 == ease_invert_host(np.array([[1, 2], [2, 1]], np.float32))[1]
    A = np.array(ec.spd_case(300)[0])
    A[250, 250] = -5.0  # the trailing block becomes indefinite; the pivots before it do not depend on this row
    got, info = _run_invert(hip, A, 305)
    assert info == 251 == ease_invert_host(A)[1] and not np.isfinite(got).all()
    A = np.array(ec.spd_case(300)[0])
    A[7, 7] = np.nan
    got, info = _run_invert(hip, A, 300)
    assert info == 8 == ease_invert_host(A)[1] and np.isnan(got).any()
    got, info = _run_invert(hip, np.zeros((1, 1), np.float32), 1)
    assert info == 1


# ---- weights -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 300])
def test_weights_in_place_and_out_of_place_are_bit_equal(hip, n):
    Pm = np.linalg.inv(ec.spd_case(n)[1]).astype(np.float32)
    L, st = hip.lib(), hip.stream_handle()
    t_P, h_P = guarded.guard_in(Pm, ld=n + 1)
    B, h_B = guarded.guard_out((n, n), ld=n + 5)
    assert L.ebn_ease_weights_f32(P(t_P), n + 1, n, P(B), n + 5, st) == OK
    io, h_io = _inout(Pm, n + 2)
    assert L.ebn_ease_weights_f32(P(io), n + 2, n, P(io), n + 2, st) == OK
    torch.cuda.synchronize()
    h_P.check("P")
    h_B.check("B")
    h_io.check("P = B")
    out, inplace = h_B.payload().cpu().numpy(), h_io.payload().cpu().numpy()
    assert np.array_equal(out.view(np.int32), inplace.view(np.int32))
    assert not out[np.diag_indices(n)].view(np.int32).any()  # exact +0.0
    assert np.array_equal(out.view(np.int32), ease_weights_host(Pm).view(np.int32))  # one correctly rounded division: the twin's bits


# ---- scores --------------------------------------------------------------------------------------------------------------------
SCORE_NAMES = ("B", "n_items", "ldb", "hist_rows", "hist_weights", "hist_offsets", "n_hists", "n_hist_items", "list_hist", "cand_rows",
               "cand_offsets", "n_lists", "n")


class _ScoreOperands:
    def __init__(self, c, ldb):
        self.h = {}
        t, self.h["B"] = guarded.guard_in(c["B"], ld=ldb, fill=POISON)
        self.B, self.n_items, self.ldb = P(t), c["B"].shape[0], ldb
        for name, fill in (("hist_rows", 2), ("list_hist", 0), ("cand_rows", 1)):  # valid values in the guards: an over-read is used
            if c[name] is None:
                setattr(self, name, None)
            else:
                t, self.h[name] = guarded.guard_in(np.asarray(c[name], np.int32), fill=fill, guard=GUARD)
                setattr(self, name, P(t))
        self.hist_weights = None
        if c["hist_weights"] is not None:
            t, self.h["hist_weights"] = guarded.guard_in(c["hist_weights"], fill=POISON, guard=GUARD)
            self.hist_weights = P(t)
        self.hist_offsets, self.h["hist_offsets"] = _guard_i64(c["hist_offsets"])
        self.cand_offsets, self.h["cand_offsets"] = _guard_i64(c["cand_offsets"])
        self.n_hists, self.n_hist_items = c["hist_offsets"].size - 1, c["hist_rows"].size
        self.n_lists, self.n = c["cand_offsets"].size - 1, c["cand_rows"].size

    def args(self, **k):
        return [k.get(n, getattr(self, n)) for n in SCORE_NAMES]

    def check_inputs(self):
        for what, h in self.h.items():
            h.check(what)


def _run_scores(hip, c, ldb):
    o = _ScoreOperands(c, ldb)
    out, h_out = guarded.guard_out((o.n,))
    assert hip.lib().ebn_ease_scores_f32(*o.args(), P(out), hip.stream_handle()) == OK
    torch.cuda.synchronize()
    o.check_inputs()
    h_out.check("scores")
    return h_out.payload().cpu().numpy()


@pytest.mark.parametrize("name", ec.SCORE_CASES)
def test_scores_against_the_brute_force(hip, name):
    c, want, bound, length = ec.score_case(name)
    assert sorted(set(length.tolist())) == [0, 1, 63, 64, 200]  # histories of 0, 1, 64, 65 (two entries unknown) and 200 entries
    got = _run_scores(hip, c, c["B"].shape[0] + 3)
    err = np.abs(got.astype(np.float64) - want)
    print(f"{name}: largest error {err.max():.3e}, closest to its bound: {np.max(err[bound > 0] / bound[bound > 0]):.4f} of it")
    assert got.dtype == np.float32 and not (~(err <= bound)).any()
    assert (length == 0).sum() > 10 and not got[length == 0].view(np.int32).any()  # exact +0: absent, no history, nothing present
    again = _run_scores(hip, c, c["B"].shape[0])
    assert np.array_equal(again.view(np.int32), got.view(np.int32))  # another leading dimension, a second run: the same bits


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_argument_checks_return_codes_and_launch_nothing(hip):
    L, st = hip.lib(), hip.stream_handle()
    big, n = 2 ** 31, 5
    indptr, cols, _ = ec.gram_case(n)
    p_ind, _h1 = _guard_i64(indptr)
    t_cols, _h2 = guarded.guard_in(cols, fill=0, guard=GUARD)
    G, h_G = guarded.guard_out((n, n), ld=n + 3, dtype=torch.int32)
    A, h_A = guarded.guard_out((n, n), ld=n + 5)
    B, h_B = guarded.guard_out((n, n), ld=n + 5)
    flag, h_flag = guarded.guard_out((1,), dtype=torch.int32)
    info, h_info = guarded.guard_out((1,), dtype=torch.int32)
    floats = int(L.ebn_ease_workspace_floats(n))
    work, h_work = guarded.guard_out((floats,), guard=GUARD)
    before = L.ebn_launch_count()

    def gram(IND=p_ind, COLS=P(t_cols), users=indptr.size - 1, nnz=cols.size, items=n, OUT=P(G), ldg=n + 3):
        return L.ebn_ease_gram_i32(IND, COLS, users, nnz, items, OUT, ldg, st)

    for kw in (dict(users=-1), dict(users=big), dict(nnz=-1), dict(nnz=big), dict(items=-1), dict(items=big), dict(ldg=-1), dict(ldg=big),
               dict(ldg=n - 1), dict(OUT=None), dict(IND=None), dict(COLS=None)):
        assert gram(**kw) == BAD_ARG, kw
    assert gram(items=32769, ldg=32769) == UNSUPPORTED and gram(items=32769, ldg=32769, OUT=None) == BAD_ARG  # BAD_ARG comes first
    assert gram(items=0) == OK and gram(items=0, OUT=None, IND=None, COLS=None, users=0, nnz=0, ldg=0) == OK

    def system(SRC=P(G), ldg=n + 3, size=n, reg=1.0, OUT=P(A), lda=n + 5, FLAG=P(flag)):
        return L.ebn_ease_system_f32(SRC, ldg, size, F(reg), OUT, lda, FLAG, st)

    for kw in (dict(size=-1), dict(size=big), dict(ldg=n - 1), dict(lda=n - 1), dict(ldg=big), dict(lda=-1), dict(reg=float("nan")),
               dict(reg=float("inf")), dict(SRC=None), dict(OUT=None), dict(FLAG=None)):
        assert system(**kw) == BAD_ARG, kw
    assert system(size=32769, ldg=32769, lda=32769) == UNSUPPORTED and system(size=32769, ldg=32769, lda=32768) == BAD_ARG
    assert system(size=0) == OK and system(size=0, SRC=None, OUT=None, FLAG=None) == OK

    def invert(MAT=P(A), lda=n + 5, size=n, WORK=P(work), wf=floats, INFO=P(info), nb=None):
        if nb is None:
            return L.ebn_ease_invert_f32(MAT, lda, size, WORK, wf, INFO, st)
        return L.ebn_ease_invert_nb_f32(MAT, lda, size, WORK, wf, INFO, nb, st)

    for nb in (None, 64):
        for kw in (dict(size=-1), dict(size=big), dict(lda=n - 1), dict(lda=big), dict(MAT=None), dict(WORK=None), dict(INFO=None),
                   dict(size=0, MAT=None)):
            assert invert(nb=nb, **kw) == BAD_ARG, (nb, kw)
        assert invert(nb=nb, size=32769, lda=32769) == UNSUPPORTED and invert(nb=nb, wf=n * 8 - 1) == UNSUPPORTED
        assert invert(nb=nb, wf=-1) == UNSUPPORTED and invert(nb=nb, size=32769, lda=32768) == BAD_ARG  # BAD_ARG comes first
        assert invert(nb=nb, size=0) == OK and invert(nb=nb, size=0, wf=0) == OK
    for nb in (0, 16, 48, 256, -64):
        assert invert(nb=nb) == BAD_ARG, nb

    def weights(SRC=P(A), ldp=n + 5, size=n, OUT=P(B), ldb=n + 5):
        return L.ebn_ease_weights_f32(SRC, ldp, size, OUT, ldb, st)

    for kw in (dict(size=-1), dict(size=big), dict(ldp=n - 1), dict(ldb=n - 1), dict(ldp=big), dict(ldb=-1), dict(SRC=None), dict(OUT=None)):
        assert weights(**kw) == BAD_ARG, kw
    assert weights(size=32769, ldp=32769, ldb=32769) == UNSUPPORTED and weights(size=32769, ldp=32769, ldb=5) == BAD_ARG
    assert weights(size=0) == OK and weights(size=0, SRC=None, OUT=None) == OK

    c, _, _, _ = ec.score_case("weighted")
    o = _ScoreOperands(c, 53)
    out, h_out = guarded.guard_out((o.n,))
    scores = lambda OUT=P(out), **kw: L.ebn_ease_scores_f32(*o.args(**kw), OUT, st)
    for kw in (dict(n_items=-1), dict(n_items=big), dict(ldb=49), dict(ldb=big), dict(n_hists=-1), dict(n_hists=big), dict(n_hist_items=-1),
               dict(n_hist_items=big), dict(n_lists=-1), dict(n_lists=big), dict(n=-1), dict(n=big), dict(n_lists=0), dict(n_hists=0),
               dict(B=None), dict(hist_rows=None), dict(hist_offsets=None), dict(cand_rows=None), dict(cand_offsets=None), dict(OUT=None)):
        assert scores(**kw) == BAD_ARG, kw
    assert scores(n=0) == OK and scores(n=0, n_lists=0, cand_rows=None, cand_offsets=None, OUT=None, B=None, n_items=0, ldb=0) == OK
    assert L.ebn_launch_count() == before
    torch.cuda.synchronize()
    for h, what in ((h_G, "G"), (h_A, "A"), (h_B, "B"), (h_flag, "flag"), (h_info, "info"), (h_work, "work"), (h_out, "scores")):
        h.check_untouched(what)
    # ---- the legal empty forms: zeros
    for kw in (dict(n_hists=0, n_hist_items=0, hist_rows=None, hist_offsets=None, hist_weights=None), dict(n_items=0, ldb=0, B=None),
               dict(n_hist_items=0, hist_rows=None)):
        z, h = guarded.guard_out((o.n,))
        assert scores(OUT=P(z), **kw) == OK, kw
        torch.cuda.synchronize()
        h.check("scores")
        assert not h.payload().view(torch.int32).any(), kw  # +0.0 everywhere
    G2, h_G2 = _scratch((n, n), ld=n + 3, dtype=torch.int32)
    assert gram(OUT=P(G2), users=0, IND=None) == OK and gram(OUT=P(G2), nnz=0, COLS=None) == OK
    torch.cuda.synchronize()
    h_G2.check("G")
    assert not np.tril(h_G2.payload().cpu().numpy()).any()
    o.check_inputs()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


def test_class_on_the_device_against_the_host_path(hip, frames):
    """device against device=None on the fixture frames: the weights within the inverse's bound carried through the division, the
    scores within that times the history's weight plus the score kernel's own bound (scores, not orderings); two runs, equal bits"""
    from ebrec.models import EASE

    behaviors, history = frames
    kw = dict(regularization=50.0, history_weights="exponential", lambda_factor=0.9, history_size=30)
    dev_m, host_m = EASE(**kw).fit(history), EASE(device=None, **kw).fit(history)
    assert dev_m.weights.is_cuda and dev_m.weights.dtype == torch.float32 and isinstance(host_m.weights, np.ndarray)
    assert np.array_equal(dev_m.article_ids, host_m.article_ids) and np.array_equal(dev_m.item_counts, host_m.item_counts)
    n = host_m.article_ids.size
    assert dev_m.weights.shape == (n, n) and n > 500  # the padded system's identity tail never shows
    Bd, Bh = dev_m.weights.cpu().numpy(), host_m.weights
    assert not Bd[np.diag_indices(n)].view(np.int32).any()
    # the float64 system of the host path: G from the weights' own inputs
    flat = [list(h)[-30:] for h in history["article_id_fixed"]]
    rows = {a: i for i, a in enumerate(host_m.article_ids.tolist())}
    G = ec.brute_gram([[rows[a] for a in s] for s in flat], n)
    A64 = ec.system(G, 50.0, small=False)  # kappa asserted there
    P_ref = np.linalg.inv(A64)
    eps_P = ec.INVERT_C * ec.kappa(A64) * ec.EPS32 * np.abs(P_ref).max()
    B_ref = ec.weights_of(P_ref)
    # |dB_ij| <= (|dP_ij| + |B_ij| |dP_jj|) / (P_jj - |dP_jj|), plus the rounding of the division and of the store
    w_bound = eps_P * (1.0 + np.abs(B_ref).max()) / (np.diag(P_ref).min() - eps_P) + 4 * ec.EPS32 * np.abs(B_ref).max()
    err_d, err_h = np.abs(Bd - B_ref).max(), np.abs(Bh - B_ref).max()
    print(f"n = {n}: weights: device error {err_d:.3e}, host twin error {err_h:.3e}, bound {w_bound:.3e}")
    assert err_d <= w_bound and err_h <= w_bound
    dev, host = dev_m.predict(behaviors, history=history), host_m.predict(behaviors, history=history)
    assert isinstance(dev.flat, torch.Tensor) and dev.flat.is_cuda and dev.flat.dtype == torch.float64
    assert isinstance(host.flat, np.ndarray) and np.array_equal(dev.offsets, host.offsets) and np.count_nonzero(host.flat) > 100
    got = dev.host_flat()
    # per item: sum_j w_j (|B_dev - B_host| <= 2 w_bound) + the score kernel's (m + 7) eps32 sum_j |w_j B[h_j, c]|, with the
    # sums over the item's history taken as bounds: m <= 30, w_j <= 1, |B| <= max |B|
    s_bound = 30 * 2 * w_bound + (30 + 7) * ec.EPS32 * 30 * np.abs(Bh).max()
    print(f"scores: largest difference {np.abs(got - host.flat).max():.3e}, bound {s_bound:.3e}")
    assert np.abs(got - host.flat).max() <= s_bound
    again = EASE(**kw).fit(history)
    assert torch.equal(again.weights, dev_m.weights) and torch.equal(again.predict(behaviors, history=history).flat, dev.flat)
    filled = EASE(fill=-3.0, **kw).fit(history.iloc[:30]).predict(behaviors, history=history.iloc[5:])
    want_f = EASE(device=None, fill=-3.0, **kw).fit(history.iloc[:30]).predict(behaviors, history=history.iloc[5:])
    assert filled.flat.is_cuda and np.array_equal(filled.host_flat() == -3.0, want_f.flat == -3.0) and (want_f.flat == -3.0).sum() > 500


def test_predict_feeds_the_device_evaluator(hip, frames):
    from ebrec.evaluation import AucScore, DeviceMetricEvaluator, MetricEvaluator, MrrScore, NdcgScore, RaggedLists
    from ebrec.models import EASE

    behaviors, history = frames
    scores = EASE(regularization=50.0).fit(history).predict(behaviors, history=history)
    assert scores.flat.is_cuda and scores.flat.dtype == torch.float64
    labels = RaggedLists.from_lists([np.isin(v, c).astype(np.int64) for v, c in zip(behaviors["article_ids_inview"], behaviors["article_ids_clicked"])])
    keep = [l for l in range(len(labels)) if 0 < sum(labels.row(l)) < len(labels.row(l))]  # auc needs both classes
    assert len(keep) > 900
    host_scores = scores.host_flat()
    y = RaggedLists.from_lists([np.asarray(labels.row(l)) for l in keep])
    p = RaggedLists.from_lists([host_scores[scores.offsets[l]:scores.offsets[l + 1]] for l in keep])
    metrics = [AucScore(), MrrScore(), NdcgScore(k=5), NdcgScore(k=10)]
    dev = DeviceMetricEvaluator(y, RaggedLists(torch.from_numpy(p.flat).cuda(), p.offsets), metrics).evaluate()
    host = MetricEvaluator(y.to_lists(), p.to_lists(), metrics).evaluate()
    assert dev.on_device
    for name, v in host.evaluations.items():
        assert dev.evaluations[name] == pytest.approx(v, rel=1e-12, abs=1e-12), name
