"""ebn_calibrated_rerank_f32 / ebn_label_target_f32 (csrc/ebn_calibrate.hip), calibrated_rerank() over a DeviceLookup and
recommend(rerank=Calibrated(...)) on the GPU, against the float64 restatement of tests/calibrate_cases.py.

Nobody had measured the kernel's error when the tolerance of calibrate_cases.tolerance() was written: the tests print the worst
shortfall and the worst |obj - float64| next to it."""
import functools

import numpy as np
import pytest
import torch

from tests import calibrate_cases as cc
from tests.hip_testutil import P as PTR, S, dev

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
A32 = float(np.float32(cc.ALPHA))  # what the kernel is handed


def run_target(hip, W, hist, weights=None):
    """-> (target [U, C] float32, flags [2]) as numpy arrays"""
    U, H = hist.shape
    W_d, hist_d = dev(W), dev(hist, torch.int32)
    w_d = None if weights is None else dev(weights)
    out_d = torch.full((U, W.shape[1]), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    code = hip.lib().ebn_label_target_f32(PTR(W_d), W.shape[0], W.shape[1], PTR(hist_d), H, PTR(w_d), PTR(out_d), PTR(flags_d), U, S())
    assert code == OK, code
    torch.cuda.synchronize()
    return out_d.cpu().numpy(), flags_d.cpu().numpy()


def run_cal(hip, W, rows, rel, target, k, lam, alpha=cc.ALPHA, want_obj=True):
    """target [U, C] (a row per user) or [C] (one row for all) -> (sel [U, k] int32, obj [U, k] float32, flags [2])"""
    U, P = rows.shape
    C = W.shape[1]
    W_d, rows_d, rel_d, t_d = dev(W), dev(rows, torch.int32), dev(rel), dev(target)
    sel_d = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
    obj_d = torch.full((U, k), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    code = hip.lib().ebn_calibrated_rerank_f32(PTR(W_d), W.shape[0], C, PTR(rows_d), PTR(rel_d), P, PTR(t_d), C if np.ndim(target) == 2 else 0,
                                               k, lam, alpha, PTR(sel_d), PTR(obj_d) if want_obj else None, PTR(flags_d), U, S())
    assert code == OK, code
    torch.cuda.synchronize()
    return sel_d.cpu().numpy(), obj_d.cpu().numpy(), flags_d.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def gathered(rel, sel):
    return np.where(sel >= 0, np.take_along_axis(rel, np.maximum(sel, 0).astype(np.int64), 1), -np.inf).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the hand case
def test_the_hand_computed_case(hip):
    """Labels [0, 0, 0, 0, 1, 1], rel .9 .. .4, p = (.5, .5), alpha = .01, k = 4 (computed in float64 in tests/test_calibrate_cpu.py:
    the smallest winning margin at lam = .5 is 0.08; the ties at lam = 0 are two-term sums, exact in any order)."""
    W = np.eye(2, dtype=np.float32)[[0, 0, 0, 0, 1, 1]]
    rows, rel = np.arange(6, dtype=np.int32)[None], np.array([[.9, .8, .7, .6, .5, .4]], np.float32)
    for lam, picks in ((1.0, [0, 1, 2, 3]), (0.5, [0, 4, 1, 2]), (0.0, [0, 4, 1, 5])):
        for target in (np.array([.5, .5], np.float32), np.array([[.5, .5]], np.float32)):
            sel, obj, flags = run_cal(hip, W, rows, rel, target, 4, lam, 0.01)
            assert sel.tolist() == [picks] and tuple(flags) == (0, 0), (lam, sel)
    assert obj[0, 1] == 0.0 and obj[0, 3] == 0.0  # lam = 0: the balanced lists have KL 0 exactly
    assert abs(obj[0, 0] + 1.9585177736) < cc.tolerance(0.0, 2, 4) and abs(obj[0, 2] + 0.0576493122) < cc.tolerance(0.0, 2, 4)


# ------------------------------------------------------------------------------------------------ exact invariants
@functools.lru_cache(maxsize=None)
def _exact(shape):
    U, P, C, k, H = shape
    return cc.exact_case(U, P, C, H, seed=U + P + C)


def _label_order_holds(W, rows, rel, sel):
    """one-hot W: the picks of any one label appear in descending relevance, equal relevance to the smaller pool index"""
    label = np.asarray(W).argmax(1)
    for u in range(rows.shape[0]):
        last = {}
        for s in sel[u].tolist():
            if s < 0:
                break
            c = label[rows[u, s]]
            if c in last:
                r0, i0 = last[c]
                assert rel[u, s] < r0 or (rel[u, s] == r0 and s > i0), (u, s, c)
            last[c] = (rel[u, s], s)


@pytest.mark.parametrize("shape", cc.EXACT_SHAPES, ids=cc.shape_id)
def test_exact_invariants(hip, shape):
    """lam = 1: the stable relevance order with out_obj bit-equal to rel.  An all-zero target: the objective is lam * rel (exact:
    relevances in multiples of 1/64, dyadic lam), so the relevance order at every lam > 0 -- and at lam = 0, where every
    objective is 0, the rule's own tie-break: the pool order.  One-hot W, dyadic lam: the picks of one label in descending
    relevance (identical label rows have identical KL bits).  No absent entry is picked, padding only once nothing is left,
    user 1 is all padding; every list also satisfies the greedy property.  The target comes from ebn_label_target_f32 over the
    case's histories (user 2: an empty history, a zero row)."""
    U, P, C, k, H = shape
    W, rows, rel, hist = _exact(shape)
    p, tflags = run_target(hip, W, hist)
    p64, _ = cc.target_reference(W, hist)
    assert tuple(tflags) == (0, 0) and (np.abs(p - p64) <= (H + 2) * 2.0 ** -23 * p64).all()
    if U > 2:
        assert (p[2] == 0).all()
    by_rel = cc.relevance_order(W, rows, rel, k)

    sel, obj, flags = run_cal(hip, W, rows, rel, p, k, 1.0)
    assert np.array_equal(sel, by_rel) and np.array_equal(bits(obj), bits(gathered(rel, sel))) and tuple(flags) == (0, 0)
    sel_only, untouched, _ = run_cal(hip, W, rows, rel, p, k, 1.0, want_obj=False)
    assert np.array_equal(sel_only, by_rel) and (untouched == 123.0).all()

    zero = np.zeros((U, C), np.float32)
    for lam in (0.25, 0.5, 1.0):
        sel, obj, flags = run_cal(hip, W, rows, rel, zero, k, lam)
        assert np.array_equal(sel, by_rel) and np.array_equal(bits(obj), bits(np.float32(lam) * gathered(rel, sel))), lam
    sel, obj, _ = run_cal(hip, W, rows, rel, zero[0], k, 0.0)  # one shared row
    present = cc.present_mask(rows, rel, len(W))
    for u in range(U):
        want = np.flatnonzero(present[u])[:k]
        assert sel[u, :len(want)].tolist() == want.tolist() and (sel[u, len(want):] == -1).all() and (obj[u, :len(want)] == 0).all()

    for lam in cc.EXACT_LAMS:
        tol = cc.tolerance(lam, C, k)
        for target in ((p, p[0]) if U <= 9 else (p,)):  # the shared row: one user's target for everybody
            sel, obj, flags = run_cal(hip, W, rows, rel, target, k, lam)
            assert tuple(flags) == (0, 0)
            gap, err = cc.check_greedy(W, rows, rel, target, sel, obj, lam, tol, A32)
            _label_order_holds(W, rows, rel, sel)
            print(f"shape {shape} lam {lam} {'shared' if target.ndim == 1 else 'own'} target: tol = {tol:.3e}, worst shortfall {gap:.3e}, "
                  f"worst |obj - float64| {err:.3e}")
            if U > 1:
                assert (sel[1] == -1).all() and np.isneginf(obj[1]).all()  # the user whose every entry is padding


@pytest.mark.parametrize("shape", [(7, 33, 33, 10, 7), (5, 32, 3, 5, 20)], ids=cc.shape_id)
def test_rows_outside_the_table_and_nan_relevances_are_absent_and_flagged(hip, shape):
    U, P, C, k, H = shape
    for bad_row, nan_rel in ((True, False), (False, True), (True, True)):
        W, rows, rel, hist = cc.exact_case(U, P, C, H, seed=3, bad_row=bad_row, nan_rel=nan_rel)
        p = cc.target_reference(W, hist)[0].astype(np.float32)
        sel, obj, flags = run_cal(hip, W, rows, rel, p, k, 0.5)
        assert tuple(flags) == (int(bad_row), int(nan_rel))
        gone = ~cc.present_mask(rows[U - 1], rel[U - 1], len(W))
        assert gone[P // 2] or gone[(P // 2 + 1) % P]
        assert not np.isin(sel[U - 1], np.flatnonzero(gone)).any()
        cc.check_greedy(W, rows, rel, p, sel, obj, 0.5, cc.tolerance(0.5, C, k), A32)
        # the same bits as with the entries written as padding
        rows2, rel2 = np.where((rows >= 0) & (rows < len(W)), rows, -1).astype(np.int32), np.where(np.isfinite(rel), rel, -np.inf).astype(np.float32)
        sel2, obj2, flags2 = run_cal(hip, W, rows2, rel2, p, k, 0.5)
        assert tuple(flags2) == (0, 0) and np.array_equal(sel, sel2) and np.array_equal(bits(obj), bits(obj2))


def test_a_negative_or_nan_target_entry_counts_as_zero_and_is_flagged(hip):
    U, P, C, k, H = 7, 33, 33, 10, 7
    W, rows, rel, hist = _exact((U, P, C, k, H))
    p = cc.target_reference(W, hist)[0].astype(np.float32)
    clean = p.copy()
    clean[0, :5], clean[3, 7], clean[6, C - 1] = 0.0, 0.0, 0.0
    for marks in ((-0.5, np.nan, np.inf), (-np.inf, -1e-30, np.nan)):
        dirty = clean.copy()
        dirty[0, :5], dirty[3, 7], dirty[6, C - 1] = marks
        sel, obj, flags = run_cal(hip, W, rows, rel, dirty, k, 0.5)
        want_sel, want_obj, want_flags = run_cal(hip, W, rows, rel, clean, k, 0.5)
        assert tuple(flags) == (0, 1) and tuple(want_flags) == (0, 0)
        assert np.array_equal(sel, want_sel) and np.array_equal(bits(obj), bits(want_obj))
        assert cc.calibrated_reference(W, rows, rel, dirty, k, 0.5)[2] == (0, 1)
        shared = run_cal(hip, W, rows, rel, dirty[0], k, 0.5)
        assert tuple(shared[2]) == (0, 1) and np.array_equal(shared[0], run_cal(hip, W, rows, rel, clean[0], k, 0.5)[0])


# ------------------------------------------------------------------------------------------------ rounded cases
@functools.lru_cache(maxsize=None)
def _rounded(shape, multi):
    U, P, C, k, H = shape
    W, rows, rel, hist = cc.rounded_case(U, P, C, H, seed=11 + C, multi=multi)
    return W, rows, rel, cc.target_reference(W, hist)[0].astype(np.float32)


@pytest.mark.parametrize("multi", [False, True], ids=["one-hot", "lists"])
@pytest.mark.parametrize("lam", cc.ROUNDED_LAMS)
@pytest.mark.parametrize("shape", cc.ROUNDED_SHAPES, ids=cc.shape_id)
def test_rounded_cases_by_the_greedy_property(hip, shape, lam, multi):
    """Every pick's objective, recomputed in float64 GIVEN the kernel's earlier picks, is within 2 tol of the best one left, and
    out_obj within tol of it; no pick repeats, no absent entry is picked (calibrate_cases.check_greedy, tolerance).  The case
    exercises the calibration term: the lists differ from the relevance order."""
    U, P, C, k, H = shape
    W, rows, rel, p = _rounded(shape, multi)
    lam32 = float(np.float32(lam))
    tol = cc.tolerance(lam, C, k)
    by_rel = cc.relevance_order(W, rows, rel, k)
    want = cc.calibrated_reference(W, rows, rel, p, k, lam32, A32)[0]
    assert (want != by_rel).any(1).mean() > 0.9, "the case must exercise the calibration term"
    sel, obj, flags = run_cal(hip, W, rows, rel, p, k, lam)
    assert tuple(flags) == (0, 0)
    gap, err = cc.check_greedy(W, rows, rel, p, sel, obj, lam32, tol, A32)
    differ = (sel != by_rel).any(1).mean()
    print(f"shape {shape} lam {lam} {'lists' if multi else 'one-hot'}: tol = {tol:.3e}, worst shortfall {gap:.3e}, worst |obj - float64| "
          f"{err:.3e}; {differ:.3f} of the lists differ from the relevance order, {(sel == want).all(1).mean():.3f} equal the restatement's")
    assert (sel[:, 0] >= 0).all() and differ > 0.9


# ------------------------------------------------------------------------------------------------ the target kernel
@pytest.mark.parametrize("shape", [(3, 1, 1), (5, 33, 4), (9, 128, 32), (6, 65, 256)], ids=cc.shape_id)
def test_history_target_is_exact_on_dyadic_inputs(hip, shape):
    """One-hot rows, H a power of two, every slot valid, weights all ones or multiples of 1/4 summing to a power of two: every
    product and sum is exact in fp32 and the division is by a power of two, so the result equals the float64 one."""
    U, C, H = shape
    rng = np.random.default_rng(U + C + H)
    W = cc.label_table(40, C, rng)
    hist = rng.integers(0, 40, (U, H)).astype(np.int32)
    for weights in (None, cc.dyadic_weights(H, rng)):
        got, flags = run_target(hip, W, hist, weights)
        want, flag0 = cc.target_reference(W, hist, weights)
        assert np.array_equal(got.astype(np.float64), want) and tuple(flags) == (0, 0) and flag0 == 0
        assert np.array_equal(want.sum(1), np.ones(U))


@pytest.mark.parametrize("shape", [(7, 33, 7), (9, 128, 256), (64, 24, 50)], ids=cc.shape_id)
def test_history_target_rounded_flags_and_empty_histories(hip, shape):
    """Otherwise within (H + 2) * 2^-23 relative: H products and additions in slot order and the division.  A row of -1 is silent,
    any other row outside the table is skipped and flagged, no valid slot (or a weight sum of 0) gives a zero row."""
    from ebrec.utils._decay import exponential_decay_weights

    U, C, H = shape
    rng = np.random.default_rng(U + C + H)
    W = cc.label_table(100, C, rng, multi=True)
    hist = rng.integers(0, 100, (U, H)).astype(np.int32)
    hist[rng.random((U, H)) < 0.2] = -1
    hist[1] = -1
    weights = np.asarray(exponential_decay_weights(H, 0.97), np.float32)
    for w in (None, weights):
        got, flags = run_target(hip, W, hist, w)
        want, _ = cc.target_reference(W, hist, w)
        err = np.abs(got - want)
        assert (err <= (H + 2) * 2.0 ** -23 * want).all() and tuple(flags) == (0, 0) and (got[1] == 0).all()
        print(f"target {shape} weights {w is not None}: worst relative error {np.max(err[want > 0] / want[want > 0]) * 2 ** 23:.2f} ulp of {H + 2}")
        bad = hist.copy()
        bad[0, 0], bad[U - 1, H - 1] = 100, -5
        silent = np.where((bad >= 0) & (bad < 100), bad, -1).astype(np.int32)
        got_bad, flags_bad = run_target(hip, W, bad, w)
        assert tuple(flags_bad) == (1, 0) and cc.target_reference(W, bad, w)[1] == 1
        assert np.array_equal(bits(got_bad), bits(run_target(hip, W, silent, w)[0]))
    zero_w, _ = run_target(hip, W, hist, np.zeros(H, np.float32))
    assert (zero_w == 0).all()


# ------------------------------------------------------------------------------------------------ determinism
def test_two_runs_and_any_set_of_co_launched_users_give_the_same_bits(hip):
    """A user's output depends neither on U nor on who shares its launch: users [0, 7) alone and users [1, 8) alone against the
    same users inside 130."""
    for (P, C, k, H), multi in (((64, 64, 64, 50), False), ((33, 33, 10, 7), True)):
        W, rows, rel, hist = cc.rounded_case(130, P, C, H, seed=17, multi=multi)
        p_full = run_target(hip, W, hist)[0]
        assert np.array_equal(bits(p_full), bits(run_target(hip, W, hist)[0]))
        assert np.array_equal(bits(run_target(hip, W, hist[:7])[0]), bits(p_full[:7]))
        assert np.array_equal(bits(run_target(hip, W, hist[1:8])[0]), bits(p_full[1:8]))
        full = run_cal(hip, W, rows, rel, p_full, k, 0.7)
        again = run_cal(hip, W, rows, rel, p_full, k, 0.7)
        head = run_cal(hip, W, rows[:7], rel[:7], p_full[:7], k, 0.7)
        odd = run_cal(hip, W, rows[1:8], rel[1:8], p_full[1:8], k, 0.7)
        assert np.array_equal(full[0], again[0]) and np.array_equal(bits(full[1]), bits(again[1]))
        assert np.array_equal(head[0], full[0][:7]) and np.array_equal(bits(head[1]), bits(full[1][:7]))
        assert np.array_equal(odd[0], full[0][1:8]) and np.array_equal(bits(odd[1]), bits(full[1][1:8]))


# ------------------------------------------------------------------------------------------------ error codes
def test_unsupported_and_bad_calls_return_their_code_and_write_nothing(hip):
    U, P, C, k, H = 5, 33, 8, 4, 6
    W, rows, rel, hist = cc.exact_case(U, P, C, H, seed=4)
    W_d = dev(np.zeros((len(W), 129), np.float32))
    rows_d, rel_d, hist_d = dev(np.zeros((U, 65)), torch.int32), dev(np.zeros((U, 65))), dev(np.zeros((U, 257)), torch.int32)
    t_d = torch.full((U, 129), 0.5, device="cuda")
    sel_d = torch.full((U, 65), -7, dtype=torch.int32, device="cuda")
    obj_d = torch.full((U, 65), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")

    def call(**kw):
        a = {**dict(W=PTR(W_d), n_rows=len(W), C=C, rows=PTR(rows_d), rel=PTR(rel_d), P=P, target=PTR(t_d), stride=C, k=k, lam=0.5,
                    alpha=0.01, sel=PTR(sel_d), obj=PTR(obj_d), flags=PTR(flags_d), U=U, stream=S()), **kw}
        return hip.lib().ebn_calibrated_rerank_f32(*a.values())

    def target(**kw):
        a = {**dict(W=PTR(W_d), n_rows=len(W), C=C, hist=PTR(hist_d), H=H, w=None, target=PTR(t_d), flags=PTR(flags_d), U=U, stream=S()), **kw}
        return hip.lib().ebn_label_target_f32(*a.values())

    assert call(P=65) == UNSUPPORTED and call(P=0) == UNSUPPORTED and call(k=65) == UNSUPPORTED and call(k=0) == UNSUPPORTED
    assert call(C=129, stride=129) == UNSUPPORTED and call(C=0, stride=0) == UNSUPPORTED
    assert call(lam=1.5) == BAD_ARG and call(lam=-0.1) == BAD_ARG and call(lam=float("nan")) == BAD_ARG
    assert call(alpha=0.0) == BAD_ARG and call(alpha=1.0) == BAD_ARG and call(alpha=float("nan")) == BAD_ARG
    assert call(stride=C + 1) == BAD_ARG and call(stride=1) == BAD_ARG and call(stride=-C) == BAD_ARG
    assert target(C=129) == UNSUPPORTED and target(C=0) == UNSUPPORTED and target(H=257) == UNSUPPORTED and target(H=0) == UNSUPPORTED
    assert target(U=-1) == BAD_ARG and call(U=-1) == BAD_ARG
    torch.cuda.synchronize()
    assert (sel_d == -7).all() and (obj_d == 123.0).all() and (flags_d == 0).all() and (t_d == 0.5).all()
    assert call(U=0) == OK and target(U=0) == OK
    torch.cuda.synchronize()
    assert (sel_d == -7).all() and (flags_d == 0).all() and (t_d == 0.5).all()
    assert call() == OK and call(stride=0) == OK  # the same calls within the limits run
    torch.cuda.synchronize()
    assert (sel_d.view(-1)[:U * k] != -7).all() and (flags_d == 0).all()
    assert target() == OK
    torch.cuda.synchronize()
    assert (t_d.view(-1)[:U * C] != 0.5).all() and (t_d.view(-1)[U * C:] == 0.5).all() and (flags_d == 0).all()


# ------------------------------------------------------------------------------------------------ calibrated_rerank() over a DeviceLookup
def _lookup_case(shape, multi, seed):
    """A rounded case whose pools hold every article at most once (so an id names one pool entry), as a lookup: article 100 + r
    with the labels of row r of the table under 'lab' (a string, or with `multi` a list; None for a zero row).  Labels no row
    uses are dropped from the table, as the lookup's vocabulary drops them."""
    U, P, C, k, H = shape
    W, _, rel, hist = cc.rounded_case(U, P, C, H, seed=seed, multi=multi)
    rng = np.random.default_rng(seed + 1)
    rows = np.stack([rng.permutation(len(W))[:P] for _ in range(U)]).astype(np.int32)
    rows[~np.isfinite(rel)] = -1
    W = W[:, W.any(0)]
    names = [[f"t{c:03d}" for c in np.flatnonzero(w)] for w in W]
    articles = {100 + r: {"lab": (v if multi else v[0]) if v else None} for r, v in enumerate(names)}
    W64 = np.where(W > 0, 1.0 / np.maximum((W > 0).sum(1, keepdims=True), 1), 0.0)
    return articles, W, W64, rows, rel, hist


@pytest.mark.parametrize("lam", cc.ROUNDED_LAMS)
@pytest.mark.parametrize("shape,multi", [(cc.ROUNDED_SHAPES[0], False), (cc.ROUNDED_SHAPES[1], True), (cc.ROUNDED_SHAPES[2], False),
                                         (cc.ROUNDED_SHAPES[2], True)], ids=lambda v: cc.shape_id(v) if isinstance(v, tuple) else str(v))
def test_calibrated_rerank_on_the_device_against_the_host_path(hip, shape, multi, lam):
    """calibrated_rerank over a DeviceLookup equals the dict path on every user the float64 restatement decides by more than
    2 tol in every round (the winner against the best entry with ANOTHER label row: entries with the same label row have the
    same KL bits on the device); at least 0.8 of the users are decided so; every user's list has the greedy property."""
    from ebrec.evaluation import calibrated_rerank, history_distribution
    from ebrec.evaluation.beyond_accuracy import DeviceLookup

    U, P, C, k, H = shape
    articles, W, W64, rows, rel, hist = _lookup_case(shape, multi, seed=23)
    ids, hist_ids = np.where(rows >= 0, rows + 100, -1), hist + 100
    tol = cc.tolerance(lam, W.shape[1], k)
    p64, _ = cc.target_reference(W64, hist)
    want_sel, _, _, lead = cc.calibrated_reference(W64, rows, rel, p64, k, lam, cc.ALPHA, margins=True)
    decided = lead > 2 * tol
    print(f"shape {shape} lam {lam} {'lists' if multi else 'one-hot'}: {decided.mean():.3f} of the users decided by more than 2 tol = {2 * tol:.3e}")
    assert decided.mean() >= 0.8

    lookup = DeviceLookup(articles, label_keys=["lab"])
    assert np.array_equal(lookup.device_table("lab").cpu().numpy(), W)
    got, got_sc = calibrated_rerank(ids, rel, lookup, "lab", k, histories=hist_ids, lam=lam, return_scores=True)
    host = calibrated_rerank(ids, rel, articles, "lab", k, histories=hist_ids, lam=lam)
    want_ids = np.where(want_sel >= 0, np.take_along_axis(ids, np.maximum(want_sel, 0).astype(np.int64), 1), -1)
    assert np.array_equal(host[decided], want_ids[decided]) and np.array_equal(got[decided], host[decided])
    print(f"    lists equal to the host path: {(got == host).all(1).mean():.3f}")
    sel = np.full((U, k), -1, np.int64)
    for u in range(U):
        pos = {a: i for i, a in enumerate(ids[u].tolist()) if a != -1}
        sel[u] = [pos.get(a, -1) for a in got[u].tolist()]
    assert np.array_equal(got_sc, gathered(rel, sel))
    p_dev, vocab = history_distribution(hist_ids, lookup, "lab")
    assert vocab == lookup.label_vocabulary("lab") and np.abs(p_dev - p64).max() <= (H + 2) * 2.0 ** -23
    gap, _ = cc.check_greedy(W, rows, rel, p_dev, sel, None, float(np.float32(lam)), tol, A32)
    print(f"    worst shortfall {gap:.3e} of 2 tol = {2 * tol:.3e}")
    # one editorial mix for everybody (normalised on the host: zero label rows leave a history target short of 1)
    mix = p64[0] / p64[0].sum()
    mix_sel, _, _, mix_lead = cc.calibrated_reference(W64, rows, rel, mix, k, lam, cc.ALPHA, margins=True)
    sure = mix_lead > 2 * tol
    mix_ids = np.where(mix_sel >= 0, np.take_along_axis(ids, np.maximum(mix_sel, 0).astype(np.int64), 1), -1)
    for target in (p64[0] * 7.0, dict(zip(lookup.label_vocabulary("lab"), p64[0].tolist()))):
        shared = calibrated_rerank(ids, rel, lookup, "lab", k, target=target, lam=lam)
        assert sure.mean() >= 0.8 and np.array_equal(shared[sure], mix_ids[sure])


# ------------------------------------------------------------------------------------------------ whole model
from tests.test_data_pipeline import frames  # noqa: E402,F401  (the fixture parquets under tests/golden/ebnerd)
from tests.test_recommend_gpu import N_CANDIDATES, N_IMPRESSIONS, TOP_N, _nrms_case  # noqa: E402

POOL = 20


def test_nrms_recommend_with_calibration(hip, frames):  # noqa: F811
    """lam = 1 is plain recommend(); lam = 1/2 gives subsets of the plain top-20 that hold no history article, carry the model's
    scores in selection order, differ from the plain lists, satisfy the greedy property recomputed in float64 from the plain
    top-20 and the history target, and equal calibrated_rerank() over the plain top-20 with the same histories.  A shared dict
    target obeys the same property."""
    from ebrec.evaluation import Calibrated, calibrated_rerank, history_distribution
    from ebrec.evaluation.beyond_accuracy import DeviceLookup
    from ebrec.evaluation.rerank import given_target
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL

    model, mk = _nrms_case(frames)
    beh = frames[0].iloc[:N_IMPRESSIONS].reset_index(drop=True)
    loader = mk(beh)
    rng = np.random.default_rng(7)
    index = model._recommend_index(loader)
    read = sorted({a for h in beh[DEFAULT_HISTORY_ARTICLE_ID_COL] for a in h} & set(index))
    cand = rng.choice(read, 10, replace=False)
    cand = rng.permutation(np.concatenate([cand, rng.choice(sorted(set(index) - set(cand.tolist())), N_CANDIDATES - 10, replace=False)]))
    articles = {int(a): {"cat": "abcd"[int(rng.integers(0, 4))]} for a in index}
    lookup = DeviceLookup(articles, label_keys=["cat"])
    W = lookup.host_table("cat")
    histories = [list(h) for h in beh[DEFAULT_HISTORY_ARTICLE_ID_COL]]

    plain_ids, plain_sc = model.recommend(loader, cand, top_n=TOP_N, return_scores=True)
    same_ids, same_sc = model.recommend(loader, cand, top_n=TOP_N, return_scores=True, rerank=Calibrated(lookup, "cat", lam=1.0, pool=POOL))
    assert np.array_equal(same_ids, plain_ids) and np.array_equal(same_sc.view(np.int32), plain_sc.view(np.int32))

    ids20, sc20 = model.recommend(loader, cand, top_n=POOL, return_scores=True)
    rows20 = lookup.rows_of(ids20).reshape(ids20.shape)
    hist_rows = np.full((N_IMPRESSIONS, max(len(h) for h in histories)), -1, np.int64)
    for u, h in enumerate(histories):
        hist_rows[u, :len(h)] = lookup.rows_of(np.asarray(h))
    p_hist = history_distribution(histories, lookup, "cat")[0]  # what the kernel computed, checked against float64 here
    p64, _ = cc.target_reference(W, hist_rows)
    assert (np.abs(p_hist - p64) <= (hist_rows.shape[1] + 2) * 2.0 ** -23 * p64).all()
    assert (p_hist.sum(1) > 0).mean() > 0.5, "the case must have histories the lookup knows"
    mix = given_target({"a": 3, "d": 1}, lookup.label_vocabulary("cat")).astype(np.float32)
    tol = cc.tolerance(0.5, W.shape[1], TOP_N)
    history = [set(h) for h in histories]

    for rerank, target, kw in ((Calibrated(lookup, "cat", lam=0.5, pool=POOL), p_hist, dict(histories=histories)),
                               (Calibrated(lookup, "cat", lam=0.5, pool=POOL, target={"a": 3, "d": 1}),
                                mix, dict(target={"a": 3, "d": 1}))):
        ids, sc = model.recommend(loader, cand, top_n=TOP_N, return_scores=True, rerank=rerank)
        assert ids.shape == sc.shape == (N_IMPRESSIONS, TOP_N) and sc.dtype == np.float32
        assert np.array_equal(model.recommend(loader, cand, top_n=TOP_N, rerank=rerank), ids)
        assert not np.array_equal(ids, plain_ids), "the case must exercise the calibration term"
        sel = np.empty((N_IMPRESSIONS, TOP_N), np.int64)
        for u in range(N_IMPRESSIONS):
            pos = {a: i for i, a in enumerate(ids20[u].tolist()) if a != -1}
            assert set(ids[u].tolist()) <= set(pos) and len(set(ids[u].tolist())) == TOP_N and not set(ids[u].tolist()) & history[u]
            sel[u] = [pos[a] for a in ids[u].tolist()]
        assert np.array_equal(sc, np.take_along_axis(sc20, sel, 1))  # the model's scores of the kept items, in selection order
        gap, _ = cc.check_greedy(W, rows20, sc20, target, sel, None, 0.5, tol, A32)
        print(f"whole model, {'history' if 'histories' in kw else 'shared'} target: tol = {tol:.3e}, worst shortfall {gap:.3e}, "
              f"{(ids != plain_ids).any(1).mean():.2f} of the lists differ from the plain ones")
        assert np.array_equal(calibrated_rerank(ids20, sc20, lookup, "cat", TOP_N, lam=0.5, **kw), ids)
    # exclude_history=False still needs the history for the target
    ids_all = model.recommend(loader, cand, top_n=TOP_N, exclude_history=False, rerank=Calibrated(lookup, "cat", lam=0.5, pool=POOL))
    ids20_all, sc20_all = model.recommend(loader, cand, top_n=POOL, exclude_history=False, return_scores=True)
    assert np.array_equal(calibrated_rerank(ids20_all, sc20_all, lookup, "cat", TOP_N, lam=0.5, histories=histories), ids_all)
