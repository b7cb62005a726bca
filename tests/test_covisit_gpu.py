"""ebn_cv_pair_keys_i64 / ebn_cv_scores_f32 (csrc/ebn_covisit.hip) through the C ABI on guard-banded operands, against the
plain-Python brute force of tests/covisit_cases.py -- the keys exactly, the scores within its derived bounds -- and CoVisitation on
the device.

Every input sits inside poison (tests/guarded.py): int64 arrays as pairs of int32 words inside zero words, rows, columns and
history indices inside VALID indices (an over-read entry is used and shows), values and weights inside 3e18 (large and finite: an
over-read value swamps a score instead of vanishing in a select).  The keys and the scores are written into canary buffers: guards
intact, every payload element written."""
import ctypes
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from tests import covisit_cases as cc
from tests import guarded

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
POISON = 3.0e18
GUARD = 16384  # elements on each side of the flat operands (nothing here strides by a leading dimension)
GOLDEN = Path(__file__).resolve().parent / "golden" / "ebnerd"
P = lambda t: ctypes.c_void_p(t.data_ptr())


def _guard_i64(x, front=0):
    """an int64 operand as int32 words inside guards of zero words, ``front`` extra zero words ahead of it -> (pointer, handle)"""
    words = np.concatenate([np.zeros(front, np.int32), np.ascontiguousarray(np.asarray(x, np.int64)).view(np.int32)])
    view, h = guarded.guard_in(words, fill=0, guard=GUARD)
    return ctypes.c_void_p(view.data_ptr() + 4 * front), h


def _keys_out(n_slots):
    """a canary buffer of n_slots int64 keys as 2 n_slots int32 words"""
    view, h = guarded.guard_out((2 * n_slots,), dtype=torch.int32, guard=GUARD)
    return view, h


def _run_keys(hip, G, symmetric, front=0):
    rows, off, n_rows = cc.pair_case(G)
    K = 2 * G if symmetric else G
    r, h_r = guarded.guard_in(np.concatenate([np.ones(front, np.int32), rows]), fill=1, guard=GUARD)
    o, h_o = _guard_i64(off, front=2 * front)
    out, h_out = _keys_out(rows.size * K)
    rc = hip.lib().ebn_cv_pair_keys_i64(ctypes.c_void_p(r.data_ptr() + 4 * front), o, off.size - 1, rows.size, n_rows, G, int(symmetric), P(out),
                                        hip.stream_handle())
    assert rc == OK
    torch.cuda.synchronize()
    h_r.check("seq_rows")
    h_o.check("seq_offsets")
    h_out.check("keys")
    return h_out.payload().cpu().numpy().view(np.int64)


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("G", [1, 3, cc.MAX_GAP])
def test_pair_keys_equal_the_brute_force(hip, G, symmetric):
    want = cc.pair_reference(G, symmetric)
    got = _run_keys(hip, G, symmetric)
    assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} keys differ"
    assert np.array_equal(_run_keys(hip, G, symmetric, front=3), want)  # another placement of the operands (rows at 4 mod 16 bytes)


class _ScoreOperands:
    """the guarded inputs of one score case; ``front``: extra guard elements ahead of every operand (another placement)"""

    def __init__(self, c, front=0):
        self.c, self.n_rows, self.nnz = c, c["indptr"].size - 1, c["cols"].size
        self.n_hists, self.n_hist_items = c["hist_offsets"].size - 1, c["hist_rows"].size
        self.n_lists, self.n = c["cand_offsets"].size - 1, c["cand_rows"].size
        self.h = {}

        def place(name, fill, dtype):
            x = np.concatenate([np.full(front, fill, dtype), c[name]])
            t, self.h[name] = guarded.guard_in(x, fill=fill, guard=GUARD)
            return ctypes.c_void_p(t.data_ptr() + 4 * front)

        self.indptr, self.h["indptr"] = _guard_i64(c["indptr"], front=2 * front)
        self.cols = place("cols", 7, np.int32)  # a valid column
        self.vals = place("vals", POISON, np.float32)
        self.hist_rows = place("hist_rows", 1, np.int32)
        self.hist_weights = None if c["hist_weights"] is None else place("hist_weights", POISON, np.float32)
        self.hist_offsets, self.h["hist_offsets"] = _guard_i64(c["hist_offsets"], front=2 * front)
        self.cand_rows = place("cand_rows", 1, np.int32)
        self.cand_offsets, self.h["cand_offsets"] = _guard_i64(c["cand_offsets"], front=2 * front)
        self.list_hist = None if c["list_hist"] is None else place("list_hist", 0, np.int32)

    def args(self, **k):
        names = ("indptr", "cols", "vals", "n_rows", "nnz", "hist_rows", "hist_weights", "hist_offsets", "n_hists", "n_hist_items", "list_hist",
                 "cand_rows", "cand_offsets", "n_lists", "n")
        return [k.get(n, getattr(self, n)) for n in names]

    def check_inputs(self):
        for what, h in self.h.items():
            h.check(what)


def _run_scores(hip, c, mode, front=0):
    o = _ScoreOperands(c, front)
    out, h_out = guarded.guard_out((o.n,))
    assert hip.lib().ebn_cv_scores_f32(*o.args(), mode, P(out), hip.stream_handle()) == OK
    torch.cuda.synchronize()
    o.check_inputs()
    h_out.check("scores")
    return h_out.payload().cpu().numpy()


def _within(got, want, bound, what):
    """|got - want| <= bound element-wise, written so that a NaN fails; prints the largest error next to its bound"""
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= bound)
    if err.size:
        worst = int(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), err)))
        print(f"{what}: largest error {err.max():.3e} (bounds up to {bound.max():.3e}); closest to its bound: "
              f"error {err.ravel()[worst]:.3e} of {bound.ravel()[worst]:.3e}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {err.size} outside the bound, {int(np.isnan(got).sum())} NaN"


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", cc.SCORE_NAMES)
def test_scores_against_the_brute_force(hip, name, mode):
    c, ref = cc.score_case(name)
    want, bound = ref[mode]
    got = _run_scores(hip, c, mode)
    _within(got, want, bound, f"{name} mode {mode}")
    assert np.array_equal(got == 0.0, want == 0.0) and not np.signbit(got[got == 0.0]).any()  # the zeros are exact +0
    if c["exact"]:
        assert np.array_equal(got.astype(np.float64), want)  # integer sums below 2^24: bit for bit


@pytest.mark.parametrize("mode", [0, 1])
def test_two_runs_and_other_placements_give_the_same_bits(hip, mode):
    c, _ = cc.score_case("weighted")
    first = _run_scores(hip, c, mode)
    for front in (0, 1, 3):
        assert np.array_equal(first.view(np.int32), _run_scores(hip, c, mode, front=front).view(np.int32)), front


def test_argument_checks_return_codes_and_launch_nothing(hip):
    L, st = hip.lib(), hip.stream_handle()
    big = 2 ** 31
    # ---- pair keys
    rows, off, n_rows = cc.pair_case(3)
    r, h_r = guarded.guard_in(rows, fill=1, guard=GUARD)
    o, h_o = _guard_i64(off)
    out, h_out = _keys_out(rows.size * 6)
    base = dict(R=P(r), O=o, NS=off.size - 1, NE=rows.size, NR=n_rows, G=3, SYM=1, K=P(out))
    keys = lambda **k: L.ebn_cv_pair_keys_i64(*[k.get(n, v) for n, v in base.items()], st)
    before = L.ebn_launch_count()
    for kw in (dict(NS=-1), dict(NS=big), dict(NE=-1), dict(NE=big), dict(NR=-1), dict(NR=big), dict(G=0), dict(G=-1), dict(R=None), dict(O=None),
               dict(K=None), dict(NS=0)):
        assert keys(**kw) == BAD_ARG, kw
    assert keys(G=cc.MAX_GAP + 1) == UNSUPPORTED
    for kw in (dict(NE=-1), dict(R=None), dict(NS=0)):
        assert keys(G=cc.MAX_GAP + 1, **kw) == BAD_ARG, kw  # BAD_ARG comes first
    assert keys(NE=0) == OK and keys(NE=0, NS=0, R=None, O=None, K=None, NR=0) == OK  # no entries: nothing to do
    assert keys(NE=0, G=cc.MAX_GAP + 1) == UNSUPPORTED
    # ---- scores
    c, _ = cc.score_case("weighted")
    so = _ScoreOperands(c)
    sc, h_sc = guarded.guard_out((so.n,))
    scores = lambda mode=0, S=P(sc), **k: L.ebn_cv_scores_f32(*so.args(**k), mode, S, st)
    for kw in (dict(n_rows=-1), dict(n_rows=big), dict(nnz=-1), dict(nnz=big), dict(n_hists=-1), dict(n_hists=big), dict(n_hist_items=-1),
               dict(n_hist_items=big), dict(n_lists=-1), dict(n_lists=big), dict(n=-1), dict(n=big), dict(mode=-1), dict(mode=2),
               dict(n_lists=0), dict(n_hists=0), dict(indptr=None), dict(cols=None), dict(vals=None), dict(hist_rows=None),
               dict(hist_offsets=None), dict(cand_rows=None), dict(cand_offsets=None), dict(S=None)):
        assert scores(**kw) == BAD_ARG, kw
    assert scores(n=0) == OK and scores(n=0, n_lists=0, cand_rows=None, cand_offsets=None, S=None, indptr=None, n_rows=0) == OK
    assert scores(n=0, mode=5) == BAD_ARG
    assert L.ebn_launch_count() == before
    torch.cuda.synchronize()
    h_out.check_untouched("keys")
    h_sc.check_untouched("scores")
    # ---- the legal empty forms: zeros in one launch each
    legal = (dict(n_rows=0, indptr=None), dict(n_rows=0, nnz=0, indptr=None, cols=None, vals=None), dict(nnz=0, cols=None, vals=None),
             dict(n_hists=0, n_hist_items=0, hist_rows=None, hist_offsets=None, hist_weights=None))
    for k, kw in enumerate(legal):
        for mode in (0, 1):
            z, h = guarded.guard_out((so.n,))
            assert scores(mode=mode, S=P(z), **kw) == OK, kw
            torch.cuda.synchronize()
            h.check("scores")
            assert not h.payload().view(torch.int32).any(), kw  # +0.0 everywhere
    assert L.ebn_launch_count() == before + 2 * len(legal)
    so.check_inputs()
    h_r.check("seq_rows")
    h_o.check("seq_offsets")


@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


@pytest.mark.parametrize("similarity,mode", [("cosine", "sum"), ("conditional", "max"), ("count", "sum")])
def test_class_on_the_device_against_the_host_path(hip, frames, similarity, mode):
    """device against device=None on the fixture frames.  article_ids, indptr, cols and counts are equal exactly; vals are compared
    within 2 u relative and TURN OUT BIT-EQUAL (float64 division and square root are correctly rounded on both paths, the sums are
    sums of integers).  The scores agree within the kernel's bound plus 2 u sum_j |w_j S_j| for the values.  max_keys = 20 000 cuts
    the device build into several blocks."""
    from ebrec.models import CoVisitation
    from ebrec.models.baselines import covisit as cv_mod
    from ebrec.utils._decay import exponential_decay_weights

    behaviors, history = frames
    kw = dict(max_gap=3, symmetric=True, similarity=similarity, mode=mode, history_weights="exponential", lambda_factor=0.9, history_size=30)
    dev_cv = CoVisitation(max_keys=20_000, **kw).fit(history.iloc[:30])
    host_cv = CoVisitation(device=None, **kw).fit(history.iloc[:30])
    d, h = dev_cv.matrix, host_cv.matrix
    assert d.on_device and not h.on_device and all(t.is_cuda for t in (d.indptr, d.cols, d.counts, d.vals))
    assert (d.indptr.dtype, d.cols.dtype, d.counts.dtype, d.vals.dtype) == (torch.int64, torch.int32, torch.int32, torch.float32)
    assert len(cv_mod.sequence_blocks(np.concatenate([[0], np.cumsum([len(x) for x in history.iloc[:30]["article_id_fixed"]])]), 6, 20_000)) > 3
    assert np.array_equal(d.article_ids, h.article_ids)
    for a, b, what in zip(d.host()[:3], h.host()[:3], ("indptr", "cols", "counts")):
        assert a.dtype == b.dtype and np.array_equal(a, b), what
    dv, hv = d.host()[3].astype(np.float64), h.host()[3].astype(np.float64)
    assert np.all(np.abs(dv - hv) <= 2 * cc.U * np.abs(hv))
    print(f"vals: {int((d.host()[3] != h.host()[3]).sum())} of {hv.size} differ in their bits")
    dev, host = dev_cv.predict(behaviors, history=history), host_cv.predict(behaviors, history=history)
    assert isinstance(dev.flat, torch.Tensor) and dev.flat.is_cuda and dev.flat.dtype == torch.float64
    assert isinstance(host.flat, np.ndarray) and np.array_equal(dev.offsets, host.offsets) and np.count_nonzero(host.flat) > 100
    m = cv_mod.MODES.index(mode)
    case = cc.frames_case(host_cv, behaviors, history, lambda n: exponential_decay_weights(n, 0.9, ascending=True))
    want, absum, present = cc.brute_scores(case, m)
    got = dev.host_flat().astype(np.float32)
    assert np.array_equal(got.astype(np.float64), dev.host_flat())  # float32 values in a float64 tensor
    _within(got, host.flat, cc.bound(want, absum, present, m) + 2 * cc.U * absum, f"{similarity} {mode} device against host")
    filled = CoVisitation(fill=-3.0, **kw).fit(history.iloc[:30]).predict(behaviors, history=history.iloc[5:])
    want_f = CoVisitation(device=None, fill=-3.0, **kw).fit(history.iloc[:30]).predict(behaviors, history=history.iloc[5:])
    assert filled.flat.is_cuda and np.array_equal(filled.host_flat() == -3.0, want_f.flat == -3.0) and (want_f.flat == -3.0).sum() > 500


def test_predict_feeds_the_device_evaluator(hip, frames):
    from ebrec.evaluation import AucScore, DeviceMetricEvaluator, MetricEvaluator, MrrScore, NdcgScore, RaggedLists
    from ebrec.models import CoVisitation

    behaviors, history = frames
    scores = CoVisitation(max_gap=3, history_weights="linear").fit(history).predict(behaviors, history=history)
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
