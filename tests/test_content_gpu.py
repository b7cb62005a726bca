"""ebn_cs_profiles_f32 / ebn_cs_centroid_scores_f32 / ebn_cs_nearest_scores_f32 (csrc/ebn_content.hip) through the C ABI on
guard-banded operands, against the float64 brute force of tests/content_cases.py within its derived bounds, and ContentSimilarity on
the device.

Every input sits inside poison (tests/guarded.py): the table at ld = D + 3 with 3e18 in the guards and the padding columns (large
and finite: an over-read row or column swamps a score instead of vanishing in a select), weights of 3e18, rows of 1 and history
indices of 0 (valid, so an over-read entry is used and shows), offsets as pairs of int32 words inside zeros.  The profiles are
written into a canary buffer at ldp = D + 3 and read from there by the centroid kernel (the canaries, 1.5e16, are its padding);
the scores sit in canary buffers: guards intact, every payload element written."""
import ctypes
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from tests import content_cases as cc
from tests import guarded

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
PAD = 3
POISON = 3.0e18
GOLDEN = Path(__file__).resolve().parent / "golden" / "ebnerd"
KEY = "document_vector"


def _guard_i64(x):
    """an int64 operand as int32 words inside guards of zero words -> (device pointer, handle)"""
    words = np.ascontiguousarray(np.asarray(x, np.int64)).view(np.int32)
    view, h = guarded.guard_in(words, fill=0)
    assert view.data_ptr() % 16 == 0
    return ctypes.c_void_p(view.data_ptr()), h


class _Operands:
    """the guarded inputs of one case"""

    def __init__(self, c, pad=PAD):
        self.c, self.n_rows, self.D = c, c["table"].shape[0], c["table"].shape[1]
        self.ld = self.D + pad
        self.n_hists, self.n_hist_items = c["hist_offsets"].size - 1, c["hist_rows"].size
        self.n_lists, self.n = c["cand_offsets"].size - 1, c["cand_rows"].size
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        self.h = {}
        t, self.h["table"] = guarded.guard_in(c["table"], ld=self.ld, fill=POISON)
        self.table = P(t)
        t, self.h["hist_rows"] = guarded.guard_in(c["hist_rows"], fill=1)
        self.hist_rows = P(t)
        self.hist_weights = None
        if c["hist_weights"] is not None:
            t, self.h["hist_weights"] = guarded.guard_in(c["hist_weights"], fill=POISON)
            self.hist_weights = P(t)
        self.hist_offsets, self.h["hist_offsets"] = _guard_i64(c["hist_offsets"])
        t, self.h["cand_rows"] = guarded.guard_in(c["cand_rows"], fill=1)
        self.cand_rows = P(t)
        self.cand_offsets, self.h["cand_offsets"] = _guard_i64(c["cand_offsets"])
        self.list_hist = None
        if c["list_hist"] is not None:
            t, self.h["list_hist"] = guarded.guard_in(c["list_hist"], fill=0)
            self.list_hist = P(t)

    def check_inputs(self):
        for what, h in self.h.items():
            h.check(what)


def _run(hip, c, pad=PAD):
    """the three entry points on guarded operands -> (profiles [n_hists, D], centroid [n], nearest [n]) as numpy arrays"""
    o, L, st = _Operands(c, pad), hip.lib(), hip.stream_handle()
    prof, h_prof = guarded.guard_out((o.n_hists, o.D), ld=o.ld)
    s_c, h_c = guarded.guard_out((o.n,))
    s_n, h_n = guarded.guard_out((o.n,))
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.ebn_cs_profiles_f32(o.table, o.n_rows, o.D, o.ld, o.hist_rows, o.hist_weights, o.hist_offsets, o.n_hists, o.n_hist_items,
                                 P(prof), o.ld, st) == OK
    assert L.ebn_cs_centroid_scores_f32(o.table, o.n_rows, o.D, o.ld, P(prof), o.n_hists, o.ld, o.list_hist, o.cand_rows, o.cand_offsets,
                                        o.n_lists, o.n, P(s_c), st) == OK
    assert L.ebn_cs_nearest_scores_f32(o.table, o.n_rows, o.D, o.ld, o.hist_rows, o.hist_weights, o.hist_offsets, o.n_hists, o.n_hist_items,
                                       o.list_hist, o.cand_rows, o.cand_offsets, o.n_lists, o.n, P(s_n), st) == OK
    torch.cuda.synchronize()
    o.check_inputs()
    h_prof.check("profiles")
    h_c.check("centroid scores")
    h_n.check("nearest scores")
    return h_prof.payload().cpu().numpy(), h_c.payload().cpu().numpy(), h_n.payload().cpu().numpy()


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


@pytest.mark.parametrize("name", cc.NAMES)
def test_kernels_against_the_brute_force(hip, name):
    c, ref = cc.case(name)
    prof, s_c, s_n = _run(hip, c)
    _within(prof, ref["profiles"], ref["profiles_bound"], f"{name} profiles")
    _within(s_c, ref["centroid"], ref["centroid_bound"], f"{name} centroid")
    _within(s_n, ref["nearest"], ref["nearest_bound"], f"{name} nearest")
    if name == "d1_exact":
        assert np.array_equal(s_c, cc.D1_WANT) and np.array_equal(s_n, cc.D1_WANT)


@pytest.mark.parametrize("name", ["dims_257", "dims_64", "lengths"])
def test_two_runs_and_other_leading_dimensions_give_the_same_bits(hip, name):
    """ld = D + 3, the same again, D + 4 and D + 64: with D = 257 the second is the only one with 16-byte loads, with D = 64 the first
    is the only one without"""
    c, _ = cc.case(name)
    first = _run(hip, c)
    for pad in (PAD, PAD + 1, PAD + 61):
        again = _run(hip, c, pad=pad)
        for a, b, what in zip(first, again, ("profiles", "centroid", "nearest")):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (what, pad)


def test_argument_checks_return_codes_and_launch_nothing(hip):
    L, st = hip.lib(), hip.stream_handle()
    c, _ = cc.case("dims_64")
    o = _Operands(c)
    prof, h_prof = guarded.guard_out((o.n_hists, o.D), ld=o.ld)
    sc, h_sc = guarded.guard_out((o.n,))
    Pf, S = ctypes.c_void_p(prof.data_ptr()), ctypes.c_void_p(sc.data_ptr())
    T, R, D, ld = o.table, o.n_rows, o.D, o.ld
    HR, HW, HO, NH, NHI = o.hist_rows, o.hist_weights, o.hist_offsets, o.n_hists, o.n_hist_items
    LH, CR, CO, NL, N = o.list_hist, o.cand_rows, o.cand_offsets, o.n_lists, o.n
    big = 2 ** 31
    profiles = lambda **k: L.ebn_cs_profiles_f32(*[k.get(n, v) for n, v in (
        ("T", T), ("R", R), ("D", D), ("ld", ld), ("HR", HR), ("HW", HW), ("HO", HO), ("NH", NH), ("NHI", NHI), ("P", Pf), ("ldp", ld))], st)
    centroid = lambda **k: L.ebn_cs_centroid_scores_f32(*[k.get(n, v) for n, v in (
        ("T", T), ("R", R), ("D", D), ("ld", ld), ("P", Pf), ("NH", NH), ("ldp", ld), ("LH", LH), ("CR", CR), ("CO", CO), ("NL", NL), ("N", N),
        ("S", S))], st)
    nearest = lambda **k: L.ebn_cs_nearest_scores_f32(*[k.get(n, v) for n, v in (
        ("T", T), ("R", R), ("D", D), ("ld", ld), ("HR", HR), ("HW", HW), ("HO", HO), ("NH", NH), ("NHI", NHI), ("LH", LH), ("CR", CR),
        ("CO", CO), ("NL", NL), ("N", N), ("S", S))], st)
    before = L.ebn_launch_count()
    for call in (profiles, centroid, nearest):
        assert call(D=0) == BAD_ARG and call(D=-1) == BAD_ARG                                  # D < 1
        assert call(ld=D - 1) == BAD_ARG                                                       # ld < D
        assert call(R=-1) == BAD_ARG and call(R=big) == BAD_ARG and call(NH=-1) == BAD_ARG and call(NH=big) == BAD_ARG
        assert call(D=cc.MAX_D + 1, ld=cc.MAX_D + 1, ldp=cc.MAX_D + 1) == UNSUPPORTED          # D > EBN_CS_MAX_D
        assert call(D=cc.MAX_D + 1, ld=cc.MAX_D, ldp=cc.MAX_D + 1) == BAD_ARG                  # BAD_ARG comes first
        assert call(T=None) == BAD_ARG
    for call in (profiles, centroid):
        assert call(ldp=D - 1) == BAD_ARG                                                      # ldp < D
        assert call(P=None) == BAD_ARG
    for call in (profiles, nearest):
        assert call(NHI=-1) == BAD_ARG and call(NHI=big) == BAD_ARG
        assert call(NH=0) == BAD_ARG                                                           # history items but no history
        assert call(HR=None) == BAD_ARG and call(HO=None) == BAD_ARG
    for call in (centroid, nearest):
        assert call(NL=-1) == BAD_ARG and call(NL=big) == BAD_ARG and call(N=-1) == BAD_ARG and call(N=big) == BAD_ARG
        assert call(NL=0) == BAD_ARG                                                           # items but no list
        assert call(CR=None) == BAD_ARG and call(CO=None) == BAD_ARG and call(S=None) == BAD_ARG
        assert call(N=0) == OK and call(N=0, NL=0, CR=None, CO=None, S=None, T=None, R=0) == OK  # no items: nothing to do
    assert profiles(NH=0, NHI=0) == OK and profiles(NH=0, NHI=0, HR=None, HO=None, P=None, T=None, R=0) == OK
    assert L.ebn_launch_count() == before
    torch.cuda.synchronize()
    h_prof.check_untouched("profiles")
    h_sc.check_untouched("scores")
    # legal calls without a table, without histories, without weights or list_hist: exact zeros, one launch each
    assert profiles(T=None, R=0) == OK and L.ebn_launch_count() == before + 1
    torch.cuda.synchronize()
    h_prof.check("profiles")
    assert not h_prof.payload().any()
    assert centroid(T=None, R=0) == OK and L.ebn_launch_count() == before + 2
    torch.cuda.synchronize()
    h_sc.check("scores")
    assert not h_sc.payload().any()
    for call, kw in ((nearest, dict(T=None, R=0)), (nearest, dict(NH=0, NHI=0, HR=None, HO=None, HW=None)), (centroid, dict(NH=0, P=None))):
        out, h = guarded.guard_out((o.n,))
        assert call(S=ctypes.c_void_p(out.data_ptr()), **kw) == OK
        torch.cuda.synchronize()
        h.check("scores")
        assert not h.payload().any()
    assert L.ebn_launch_count() == before + 5
    o.check_inputs()


@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


@pytest.mark.parametrize("mode", ["centroid", "nearest"])
def test_class_on_the_device_against_the_brute_force_and_the_host_path(hip, frames, mode):
    """the device path against the brute force over the DEVICE's unit table within the bounds, and against device=None: the host
    path normalises the table in float64, ebn_ba_unit_rows_f32 with an fp32 norm over D terms ((D / 2 + 4) u per row), so two
    rows of a dot may differ by (D + 8) u of it between the paths -- that much, times the weight, is added for this comparison"""
    from ebrec.evaluation.beyond_accuracy import DeviceLookup
    from ebrec.models import ContentSimilarity
    from ebrec.utils._decay import exponential_decay_weights

    behaviors, history = frames
    D = 96
    table = cc.synthetic_lookup(behaviors, history, D=D, key=KEY)
    kw = dict(mode=mode, history_weights="exponential", lambda_factor=0.9, history_size=40)
    dev_cs = ContentSimilarity(DeviceLookup(table, vector_keys=(KEY,)), KEY, **kw)
    host_cs = ContentSimilarity(table, KEY, device=None, **kw)
    dev, host = dev_cs.predict(behaviors, history=history), host_cs.predict(behaviors, history=history)
    assert isinstance(dev.flat, torch.Tensor) and dev.flat.is_cuda and dev.flat.dtype == torch.float64
    assert isinstance(host.flat, np.ndarray) and np.array_equal(dev.offsets, host.offsets) and np.abs(host.flat).max() > 0.5
    c = cc.frames_case(host_cs, behaviors, history, lambda n: exponential_decay_weights(n, 0.9, ascending=True))
    c = dict(c, table=dev_cs.lookup.device_table(KEY).cpu().numpy())
    ref = cc.reference(c)
    got = dev.host_flat().astype(np.float32)
    assert np.array_equal(got.astype(np.float64), dev.host_flat())  # float32 values in a float64 tensor
    _within(got, ref[mode], ref[mode + "_bound"], f"{mode} device against the brute force")
    between = (D + 8) * cc.U * (float(c["hist_weights"].max()) if mode == "nearest" else 1.0)
    _within(got, host.flat, ref[mode + "_bound"] + between, f"{mode} device against host")
    filled = ContentSimilarity(DeviceLookup(table, vector_keys=(KEY,)), KEY, fill=-3.0, **kw).predict(behaviors, history=history.iloc[5:])
    want = ContentSimilarity(table, KEY, device=None, fill=-3.0, **kw).predict(behaviors, history=history.iloc[5:])
    assert filled.flat.is_cuda and np.array_equal(filled.host_flat() == -3.0, want.flat == -3.0) and (want.flat == -3.0).sum() > 500
    if mode == "centroid":
        hists = list(history["article_id_fixed"])
        p_dev, p_host = dev_cs.profiles(hists), host_cs.profiles(hists)
        assert p_dev.is_cuda and p_dev.dtype == torch.float32 and tuple(p_dev.shape) == p_host.shape == (len(history), D)
        _within(p_dev.cpu().numpy(), ref["profiles"], ref["profiles_bound"], "profiles device against the brute force")
        _within(p_dev.cpu().numpy(), p_host.astype(np.float64), ref["profiles_bound"] + (D + 8) * cc.U, "profiles device against host")


def test_predict_feeds_the_device_evaluator(hip, frames):
    from ebrec.evaluation import AucScore, DeviceMetricEvaluator, MetricEvaluator, MrrScore, NdcgScore, RaggedLists
    from ebrec.evaluation.beyond_accuracy import DeviceLookup
    from ebrec.models import ContentSimilarity

    behaviors, history = frames
    lookup = DeviceLookup(cc.synthetic_lookup(behaviors, history, D=64, key=KEY), vector_keys=(KEY,))
    scores = ContentSimilarity(lookup, KEY, mode="centroid", history_weights="linear").predict(behaviors, history=history)
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
    assert dev.on_device and dev.n_host_fallback < len(keep)
    for name, v in host.evaluations.items():
        assert dev.evaluations[name] == pytest.approx(v, rel=1e-12, abs=1e-12), name
