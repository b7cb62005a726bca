"""ebn_knn_neighbours_f32 / ebn_knn_scores_f32 (csrc/ebn_knn.hip) through the C ABI on guard-banded operands, against the
plain-Python brute force of tests/knn_cases.py -- the neighbours bit for bit, the scores within its derived bound -- and HistoryKNN
on the device.

Every input sits inside poison (tests/guarded.py), with the choices of tests/test_covisit_gpu.py: int64 arrays as pairs of int32
words inside zero words, rows / sequence ids / history indices inside VALID indices (an over-read entry is used and shows), weights,
scales and sims inside 3e18 (large and finite: an over-read value swamps a result instead of vanishing in a select).  The outputs
are written into canary buffers: guards intact, every payload element written.  Every case runs at a second placement of its
operands (``front``: extra guard elements ahead of each, rows at 4 mod 16 bytes)."""
import ctypes
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from tests import guarded
from tests import knn_cases as kc

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
POISON = 3.0e18
GUARD = 16384
GOLDEN = Path(__file__).resolve().parent / "golden" / "ebnerd"
P = lambda t: ctypes.c_void_p(t.data_ptr())
PAIRS = [(S, k) for S in kc.SAMPLES for k in kc.KS if k <= S]


@pytest.fixture(scope="module")
def R(hip):
    return int(hip.lib().ebn_knn_range())


def _guard_i64(x, front=0):
    """an int64 operand as int32 words inside guards of zero words, ``front`` extra zero words ahead of it -> (pointer, handle)"""
    words = np.concatenate([np.zeros(front, np.int32), np.ascontiguousarray(np.asarray(x, np.int64)).view(np.int32)])
    view, h = guarded.guard_in(words, fill=0, guard=GUARD)
    return ctypes.c_void_p(view.data_ptr() + 4 * front), h


class _Operands:
    """guarded inputs: ``spec`` = [(name, kind, fill)], kind "i64" / np.int32 / np.float32; a None array stays a NULL pointer"""

    def __init__(self, c, spec, front=0):
        self.h = {}
        for name, kind, fill in spec:
            if c[name] is None:
                setattr(self, name, None)
            elif kind == "i64":
                ptr, self.h[name] = _guard_i64(c[name], front=2 * front)
                setattr(self, name, ptr)
            else:
                x = np.concatenate([np.full(front, fill, kind), np.asarray(c[name], kind).ravel()])
                t, self.h[name] = guarded.guard_in(x, fill=fill, guard=GUARD)
                setattr(self, name, ctypes.c_void_p(t.data_ptr() + 4 * front))

    def check_inputs(self):
        for what, h in self.h.items():
            h.check(what)


class _NeighbourOperands(_Operands):
    NAMES = ("p_indptr", "p_seqs", "n_rows", "nnz_p", "n_seqs", "seq_scale", "hist_rows", "hist_weights", "hist_offsets", "n_hists", "n_hist_items",
             "hist_self")

    def __init__(self, c, front=0):
        # a valid sequence id, a valid row and a valid self in the guards: what is read past an operand is USED
        super().__init__(c, [("p_indptr", "i64", 0), ("p_seqs", np.int32, c["n_seqs"] - 1), ("seq_scale", np.float32, POISON),
                             ("hist_rows", np.int32, 2), ("hist_weights", np.float32, POISON), ("hist_offsets", "i64", 0),
                             ("hist_self", np.int32, c["n_seqs"] - 2)], front)
        self.n_rows, self.nnz_p, self.n_seqs = c["p_indptr"].size - 1, c["p_seqs"].size, c["n_seqs"]
        self.n_hists, self.n_hist_items = c["hist_offsets"].size - 1, c["hist_rows"].size

    def args(self, **k):
        return [k.get(n, getattr(self, n)) for n in self.NAMES]


def _run_neighbours(hip, c, S, k, front=0):
    o = _NeighbourOperands(c, front)
    seq, h_seq = guarded.guard_out((o.n_hists, k), dtype=torch.int32)
    sim, h_sim = guarded.guard_out((o.n_hists, k))
    assert hip.lib().ebn_knn_neighbours_f32(*o.args(), S, k, P(seq), P(sim), hip.stream_handle()) == OK
    torch.cuda.synchronize()
    o.check_inputs()
    h_seq.check("out_seq")
    h_sim.check("out_sim")
    return h_seq.payload().cpu().numpy(), h_sim.payload().cpu().numpy()


@pytest.mark.parametrize("variant", list(kc.VARIANTS))
def test_neighbours_equal_the_brute_force_bit_for_bit(hip, R, variant):
    """n_seqs = 2 R + 37; sample_size 1 / 300 / 1000 / 4000 / 4096 x k 1 / 300 / 512 (k <= sample_size); NULL and given weights, scales
    and hist_self over the variants; the cases of tests/knn_cases.py"""
    c, _ = kc.neighbour_case(R, variant)
    assert c["n_seqs"] == 2 * R + 37
    for S, k in PAIRS:
        want_seq, want_sim = kc.neighbour_reference(R, variant, S, k)
        for front in (0, 3):
            seq, sim = _run_neighbours(hip, c, S, k, front)
            bad = (seq != want_seq) | (sim.view(np.int32) != want_sim.view(np.int32))
            assert not bad.any(), f"{variant} S={S} k={k} front={front}: {int(bad.sum())} of {bad.size} slots differ, first in history {np.argwhere(bad)[0]}"
    seq, sim = kc.neighbour_reference(R, variant, 4096, 512)
    assert (seq[0] == -1).all() and (seq[1] == -1).all() and (seq[6] == -1).all() and np.isneginf(sim[0]).all()  # empty, absent, empty posting
    assert (seq[4, 1:] == -1).all() and (seq[4, 0] >= 0) == (c["hist_self"] is None)  # one candidate (it is hist_self where that is given)


class _ScoreOperands(_Operands):
    NAMES = ("s_indptr", "s_items", "n_seqs", "nnz_s", "n_rows", "item_scale", "nbr_seq", "nbr_sim", "n_hists", "k", "list_hist", "cand_rows",
             "cand_offsets", "n_lists", "n")

    def __init__(self, c, front=0):
        super().__init__(c, [("s_indptr", "i64", 0), ("s_items", np.int32, 7), ("item_scale", np.float32, POISON), ("nbr_seq", np.int32, 6),
                             ("nbr_sim", np.float32, POISON), ("list_hist", np.int32, 0), ("cand_rows", np.int32, 1), ("cand_offsets", "i64", 0)],
                         front)
        self.n_seqs, self.nnz_s, self.n_rows = c["s_indptr"].size - 1, c["s_items"].size, c["n_rows"]
        self.n_hists, self.k = c["nbr_seq"].shape
        self.n_lists, self.n = c["cand_offsets"].size - 1, c["cand_rows"].size

    def args(self, **k):
        return [k.get(n, getattr(self, n)) for n in self.NAMES]


def _run_scores(hip, c, front=0):
    o = _ScoreOperands(c, front)
    out, h_out = guarded.guard_out((o.n,))
    assert hip.lib().ebn_knn_scores_f32(*o.args(), P(out), hip.stream_handle()) == OK
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


@pytest.mark.parametrize("name", list(kc.SCORE_CASES))
def test_scores_against_the_brute_force(hip, name):
    c, want, bound = kc.score_case(name)
    got = _run_scores(hip, c)
    _within(got, want, bound, name)
    unscored = np.repeat(~np.isin(np.arange(c["cand_offsets"].size - 1) if c["list_hist"] is None else c["list_hist"],
                                  [u for u in range(c["nbr_seq"].shape[0]) if (c["nbr_seq"][u] >= 0).any()]), np.diff(c["cand_offsets"]))
    unscored |= (c["cand_rows"] < 0) | (c["cand_rows"] >= c["n_rows"])
    assert unscored.any() and not got[unscored].view(np.int32).any()  # exact +0: absent, no history, no neighbour
    if c["exact"]:
        assert np.array_equal(got.astype(np.float64), want)  # integer sums below 2^24: bit for bit
    again = _run_scores(hip, c, front=3)
    assert np.array_equal(again.view(np.int32), got.view(np.int32))  # another placement, a second run: the same bits


def test_two_runs_give_the_same_bits(hip, R):
    c, _ = kc.neighbour_case(R, "scaled")
    first = _run_neighbours(hip, c, 1000, 512)
    for front in (0, 1):
        again = _run_neighbours(hip, c, 1000, 512, front=front)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1].view(np.int32), again[1].view(np.int32)), front


def test_argument_checks_return_codes_and_launch_nothing(hip, R):
    L, st = hip.lib(), hip.stream_handle()
    big = 2 ** 31
    # ---- neighbours
    c, _ = kc.neighbour_case(R, "unweighted")
    o = _NeighbourOperands(c)
    seq, h_seq = guarded.guard_out((o.n_hists, 8), dtype=torch.int32)
    sim, h_sim = guarded.guard_out((o.n_hists, 8))
    nb = lambda S=16, k=8, SEQ=P(seq), SIM=P(sim), **kw: L.ebn_knn_neighbours_f32(*o.args(**kw), S, k, SEQ, SIM, st)
    before = L.ebn_launch_count()
    for kw in (dict(n_rows=-1), dict(n_rows=big), dict(nnz_p=-1), dict(nnz_p=big), dict(n_seqs=-1), dict(n_seqs=big), dict(n_hists=-1),
               dict(n_hists=big), dict(n_hist_items=-1), dict(n_hist_items=big), dict(S=0), dict(S=-1), dict(k=0), dict(k=-1), dict(k=17),
               dict(n_hists=0), dict(p_indptr=None), dict(p_seqs=None), dict(hist_rows=None), dict(hist_offsets=None), dict(SEQ=None), dict(SIM=None)):
        assert nb(**kw) == BAD_ARG, kw
    assert nb(S=4097, k=8) == UNSUPPORTED and nb(S=4096, k=513) == UNSUPPORTED
    for kw in (dict(n_rows=-1), dict(SEQ=None), dict(hist_offsets=None)):
        assert nb(S=4097, k=8, **kw) == BAD_ARG, kw  # BAD_ARG comes first
    assert nb(S=4097, k=4098) == BAD_ARG  # k > sample_size
    empty = dict(n_hists=0, n_hist_items=0)
    assert nb(**empty) == OK and nb(hist_rows=None, hist_offsets=None, hist_weights=None, hist_self=None, SEQ=None, SIM=None, p_indptr=None,
                                    p_seqs=None, n_rows=0, nnz_p=0, **empty) == OK  # no histories: nothing to do
    assert nb(S=4097, **empty) == UNSUPPORTED
    # ---- scores
    sc, _, _ = kc.score_case("k65")
    so = _ScoreOperands(sc)
    out, h_out = guarded.guard_out((so.n,))
    scores = lambda OUT=P(out), **kw: L.ebn_knn_scores_f32(*so.args(**kw), OUT, st)
    for kw in (dict(n_seqs=-1), dict(n_seqs=big), dict(nnz_s=-1), dict(nnz_s=big), dict(n_rows=-1), dict(n_rows=big), dict(n_hists=-1),
               dict(n_hists=big), dict(n_lists=-1), dict(n_lists=big), dict(n=-1), dict(n=big), dict(k=0), dict(k=-1), dict(n_lists=0),
               dict(s_indptr=None), dict(s_items=None), dict(nbr_seq=None), dict(nbr_sim=None), dict(cand_rows=None), dict(cand_offsets=None),
               dict(OUT=None)):
        assert scores(**kw) == BAD_ARG, kw
    assert scores(k=513) == UNSUPPORTED and scores(k=513, n_rows=-1) == BAD_ARG and scores(k=513, n=0) == UNSUPPORTED
    assert scores(n=0) == OK and scores(n=0, n_lists=0, cand_rows=None, cand_offsets=None, OUT=None, s_indptr=None, n_seqs=0) == OK
    assert L.ebn_launch_count() == before
    torch.cuda.synchronize()
    for h, what in ((h_seq, "out_seq"), (h_sim, "out_sim"), (h_out, "scores")):
        h.check_untouched(what)
    # ---- the legal empty forms: one launch each
    for kw in (dict(nnz_p=0, p_seqs=None), dict(n_rows=0, nnz_p=0, p_indptr=None, p_seqs=None), dict(n_seqs=0)):
        s2, h2 = guarded.guard_out((o.n_hists, 8), dtype=torch.int32)
        v2, g2 = guarded.guard_out((o.n_hists, 8))
        assert nb(SEQ=P(s2), SIM=P(v2), **kw) == OK, kw
        torch.cuda.synchronize()
        h2.check("out_seq")
        g2.check("out_sim")
        assert (h2.payload() == -1).all() and torch.isneginf(g2.payload()).all(), kw
    legal = (dict(nnz_s=0, s_items=None), dict(n_seqs=0, nnz_s=0, s_indptr=None, s_items=None), dict(n_hists=0, nbr_seq=None, nbr_sim=None),
             dict(n_rows=0))
    for kw in legal:
        z, h = guarded.guard_out((so.n,))
        assert scores(OUT=P(z), **kw) == OK, kw
        torch.cuda.synchronize()
        h.check("scores")
        assert not h.payload().view(torch.int32).any(), kw  # +0.0 everywhere
    assert L.ebn_launch_count() == before + 3 + len(legal)
    o.check_inputs()
    so.check_inputs()


@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


@pytest.mark.parametrize("similarity,idf", [("cosine", False), ("dot", True)])
def test_class_on_the_device_against_the_host_path(hip, frames, similarity, idf):
    """device against device=None on the fixture frames: the index arrays and scales are equal exactly (max_keys = 2 000 cuts the
    device build into several blocks), the neighbours are equal bit for bit, the scores agree within the kernel's bound; two runs
    give equal bits"""
    from ebrec.models import HistoryKNN

    behaviors, history = frames
    kw = dict(k=20, sample_size=30, similarity=similarity, idf=idf, history_weights="exponential", lambda_factor=0.9, history_size=30)
    dev_knn = HistoryKNN(max_keys=2_000, **kw).fit(history)
    host_knn = HistoryKNN(device=None, **kw).fit(history)
    d, h = dev_knn.index, host_knn.index
    assert d.on_device and not h.on_device and all(t.is_cuda for t in (d.p_indptr, d.p_seqs, d.s_indptr, d.s_items))
    assert (d.p_indptr.dtype, d.p_seqs.dtype, d.s_indptr.dtype, d.s_items.dtype) == (torch.int64, torch.int32, torch.int64, torch.int32)
    assert sum(len(x) for x in history["article_id_fixed"]) > 3 * 1_000  # more than three blocks
    assert np.array_equal(d.article_ids, h.article_ids) and np.array_equal(d.sequence_of, h.sequence_of) and np.array_equal(d.keys, h.keys)
    for a, b, what in zip(d.host(), h.host(), ("p_indptr", "p_seqs", "s_indptr", "s_items", "seq_scale", "item_scale")):
        assert (a is None and b is None) or (a.dtype == b.dtype and np.array_equal(a, b)), what
    hists, users = list(history["article_id_fixed"]), history["user_id"].to_numpy()
    (d_rows, d_sims), (h_rows, h_sims) = dev_knn.neighbours(hists, history_keys=users), host_knn.neighbours(hists, history_keys=users)
    assert d_rows.is_cuda and d_sims.is_cuda and d_rows.dtype == torch.int64 and d_sims.dtype == torch.float32
    assert np.array_equal(d_rows.cpu().numpy(), h_rows) and np.array_equal(d_sims.cpu().numpy().view(np.int32), h_sims.view(np.int32))
    assert (h_rows[:, 0] >= 0).all() and not (h_rows == np.arange(len(hists))[:, None]).any()
    dev, host = dev_knn.predict(behaviors, history=history), host_knn.predict(behaviors, history=history)
    assert isinstance(dev.flat, torch.Tensor) and dev.flat.is_cuda and dev.flat.dtype == torch.float64
    assert isinstance(host.flat, np.ndarray) and np.array_equal(dev.offsets, host.offsets) and np.count_nonzero(host.flat) > 100
    got = dev.host_flat().astype(np.float32)
    assert np.array_equal(got.astype(np.float64), dev.host_flat())  # float32 values in a float64 tensor
    # the bound of tests/knn_cases.py over the host path's own neighbours (equal to the device's, above)
    uniq = np.unique(users)
    first = {u: i for i, u in reversed(list(enumerate(users.tolist())))}
    seq, sim = host_knn._neighbours(*host_knn._histories([hists[first[u]] for u in uniq.tolist()]), host_knn._self_of(uniq, uniq.size))
    at = {u: i for i, u in enumerate(uniq.tolist())}
    case = dict(s_indptr=h.s_indptr, s_items=h.s_items, n_rows=h.n_rows, nbr_seq=seq, nbr_sim=sim, item_scale=h.item_scale,
                cand_rows=host_knn.rows_of(np.concatenate(list(behaviors["article_ids_inview"]))), cand_offsets=host.offsets,
                list_hist=np.array([at.get(u, -1) for u in behaviors["user_id"]], np.int32))
    want, absum, total = kc.brute_scores(case)
    assert np.all(np.abs(host.flat - want) <= 1e-12 * np.maximum(np.abs(want), 1.0))
    _within(got, want, kc.score_bound(case, want, absum, total), f"{similarity} idf={idf} device against the brute force")
    again = dev_knn.predict(behaviors, history=history)
    assert torch.equal(again.flat, dev.flat)
    filled = HistoryKNN(fill=-3.0, **kw).fit(history.iloc[:30]).predict(behaviors, history=history.iloc[5:])
    want_f = HistoryKNN(device=None, fill=-3.0, **kw).fit(history.iloc[:30]).predict(behaviors, history=history.iloc[5:])
    assert filled.flat.is_cuda and np.array_equal(filled.host_flat() == -3.0, want_f.flat == -3.0) and (want_f.flat == -3.0).sum() > 500


def test_predict_feeds_the_device_evaluator(hip, frames):
    from ebrec.evaluation import AucScore, DeviceMetricEvaluator, MetricEvaluator, MrrScore, NdcgScore, RaggedLists
    from ebrec.models import HistoryKNN

    behaviors, history = frames
    scores = HistoryKNN().fit(history).predict(behaviors, history=history)
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
