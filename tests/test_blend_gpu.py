"""ebn_blend_features_f32 / ebn_blend_combine_f64 / ebn_blend_sums_f64 (csrc/ebn_blend.hip) through the C ABI on guard-banded
operands, against the plain-Python brute force of tests/blend_cases.py within its derived bounds, and ScoreBlend on the device
against its host path.

Every operand sits inside poison (tests/guarded.py): int64 offsets as pairs of int32 words inside zero words, float32 scores and
features inside 3e18, float64 scores, params and weights as int32 words inside a word that makes every guard double 3e18, labels as
bytes inside 1 (a valid label), kinds inside 99 (an unknown kind: NaN features).  Outputs are written into canary buffers: guards
intact, every payload element written; the flag bytes behind the last list keep their pre-fill.  Every case runs at a second
placement of its operands too."""
import ctypes

import numpy as np
import pytest
import torch

from tests import blend_cases as bc
from tests import guarded

pytestmark = pytest.mark.gpu

OK, BAD_ARG = 0, -1
POISON = 3.0e18
POISON_WORD = 0x43C4D1C4  # hi and lo word of a double of about 3.0e18
GUARD = 16384
PREFILL_BYTE = 0xC5       # every byte of guarded.PREFILL_I32


def _ptr(view, front_bytes=0):
    return ctypes.c_void_p(view.data_ptr() + front_bytes)


def _guard_words(words, fill, front):
    """int32 words behind `front` extra fill words, inside guards of `fill` -> (pointer to the payload, handle)"""
    x = np.concatenate([np.full(front, fill, np.int32), np.ascontiguousarray(words).view(np.int32).ravel()])
    view, h = guarded.guard_in(x, fill=fill, guard=GUARD)
    return _ptr(view, 4 * front), h


def _guard_f32(x, front):
    y = np.concatenate([np.full(front, POISON, np.float32), np.ascontiguousarray(x, np.float32).ravel()])
    view, h = guarded.guard_in(y, fill=POISON, guard=GUARD)
    return _ptr(view, 4 * front), h


def _guard_f64(x, front):
    return _guard_words(np.ascontiguousarray(x, np.float64), POISON_WORD, 2 * front)


def _guard_labels(y, front):
    """uint8 labels padded with ones to whole words, inside words of four ones; `front` bytes ahead (any alignment)"""
    b = np.concatenate([np.ones(front, np.uint8), np.asarray(y, np.uint8), np.ones((-(len(y) + front)) % 4, np.uint8)])
    view, h = guarded.guard_in(b.view(np.int32), fill=0x01010101, guard=GUARD)
    return _ptr(view, front), h


def _out_words(n_words):
    return guarded.guard_out((max(n_words, 1),), dtype=torch.int32, guard=GUARD)


def _flags_out(n_lists):
    view, h = _out_words((n_lists + 3) // 4)
    return view, h


def _read_flags(h, n_lists, what="flags"):
    h.check(what)
    b = h.payload().cpu().numpy().view(np.uint8)
    assert (b[n_lists:] == PREFILL_BYTE).all(), f"{what}: bytes behind the last list were written"
    return b[:n_lists].copy()


class _Inputs:
    """scores [M, n] of the case's first M sources (or `sources`), the malformed offsets, kinds and params, all guarded"""

    def __init__(self, sources, kinds, kind_of_scores, front=0, weights=None):
        c = bc.case()
        self.M, self.n, self.n_lists, self.kind_of_scores = len(sources), c["n"], len(c["offsets_bad"]) - 1, kind_of_scores
        s = bc.scores(kind_of_scores)[list(sources)]
        self.h = {}
        self.scores, self.h["scores"] = _guard_f32(s, front) if kind_of_scores == 0 else _guard_f64(s, front)
        self.offsets, self.h["offsets"] = _guard_words(c["offsets_bad"], 0, 2 * front)
        self.kinds, self.h["kinds"] = _guard_words(np.asarray(kinds, np.int32), 99, front)
        self.params, self.h["params"] = _guard_f64([bc.RRF_K] * self.M, front)
        if weights is not None:
            self.weights, self.h["weights"] = _guard_f64(weights, front)

    def check(self):
        for what, h in self.h.items():
            h.check(what)


def _run_features(hip, sources, kinds, kind_of_scores, form, front=0):
    i = _Inputs(sources, kinds, kind_of_scores, front)
    f, h_f = guarded.guard_out((i.M * i.n,), guard=GUARD)
    fl, h_fl = _flags_out(i.n_lists)
    rc = hip.lib().ebn_blend_features_f32(i.scores, kind_of_scores, i.M, i.n, i.offsets, i.n_lists, i.kinds, i.params, form, _ptr(f), _ptr(fl),
                                          hip.stream_handle())
    assert rc == OK
    torch.cuda.synchronize()
    i.check()
    h_f.check("features")
    return h_f.payload().cpu().numpy().reshape(i.M, i.n), _read_flags(h_fl, i.n_lists)


def _within(got, want, bound, what):
    """|got - want| <= bound element-wise; NaN passes only where both are NaN; prints the largest error next to its bound"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.where(np.isnan(got) & np.isnan(want), 0.0, np.abs(got - want))
    bad = ~(err <= bound)
    if err.size:
        k = int(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), err)))
        print(f"{what}: largest error {np.nanmax(err):.3e} (bounds up to {np.max(bound):.3e}); closest to its bound: "
              f"error {err.ravel()[k]:.3e} of {np.asarray(bound).ravel()[k]:.3e}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {err.size} outside the bound, {int(np.isnan(got).sum())} NaN"


# ---- features --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(5), ids=bc.KIND_NAMES)
@pytest.mark.parametrize("kind_of_scores", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("M", [1, 3, 8, 16])
def test_features_against_the_brute_force(hip, M, kind_of_scores, kind):
    src = list(range(M))
    want, bound, flags = bc.features_reference(src, [kind] * M, kind_of_scores)
    got, got_flags = _run_features(hip, src, [kind] * M, kind_of_scores, form=0)
    assert got.dtype == np.float32 and np.array_equal(got_flags, flags) and flags.sum() == 2 * (1 if M == 1 else 3)
    if kind == bc.RAW:
        assert np.array_equal(got, want.astype(np.float32), equal_nan=True)  # bit-equal: one rounding of the score itself
    else:
        _within(got, want, bound, f"{bc.KIND_NAMES[kind]}, M = {M}, {('float32', 'float64')[kind_of_scores]} scores")
    general, general_flags = _run_features(hip, src, [kind] * M, kind_of_scores, form=1)
    assert np.array_equal(got.view(np.int32), general.view(np.int32)) and np.array_equal(got_flags, general_flags)  # both forms: the same bits
    moved, moved_flags = _run_features(hip, src, [kind] * M, kind_of_scores, form=0, front=3)
    assert np.array_equal(got.view(np.int32), moved.view(np.int32)) and np.array_equal(got_flags, moved_flags)


def test_unknown_kind_gives_nan_features(hip):
    got, flags = _run_features(hip, [3, 4], [7, bc.RANK], 0, form=0)
    assert np.isnan(got[0]).all() and not np.isnan(got[1]).any() and not flags.any()


# ---- combine ---------------------------------------------------------------------------------------------------------------------
def _run_combine(hip, sources, kinds, kind_of_scores, weights, form, front=0):
    i = _Inputs(sources, kinds, kind_of_scores, front, weights=weights)
    out, h_out = _out_words(2 * i.n)
    fl, h_fl = _flags_out(i.n_lists)
    rc = hip.lib().ebn_blend_combine_f64(i.scores, kind_of_scores, i.M, i.n, i.offsets, i.n_lists, i.kinds, i.params, i.weights, form, _ptr(out),
                                         _ptr(fl), hip.stream_handle())
    assert rc == OK
    torch.cuda.synchronize()
    i.check()
    h_out.check("out")
    return h_out.payload().cpu().numpy().view(np.float64), _read_flags(h_fl, i.n_lists)


@pytest.mark.parametrize("kind_of_scores", [0, 1], ids=["f32", "f64"])
def test_combine_against_the_brute_force(hip, kind_of_scores):
    c = bc.case()
    w = np.array([0.7, -1.3, 0.2, 2.0, 31.0, 0.5])
    want, fbound, flags = bc.features_reference(bc.FIT_SOURCES, bc.FIT_KINDS, kind_of_scores)
    flagged = np.repeat(flags[:-1] != 0, c["lengths"])
    ref = np.where(flagged, np.nan, w @ np.nan_to_num(want))
    bound = np.abs(w) @ fbound + 2.0 ** -50 * (np.abs(w) @ np.abs(np.nan_to_num(want)))
    got, got_flags = _run_combine(hip, bc.FIT_SOURCES, bc.FIT_KINDS, kind_of_scores, w, form=0)
    _within(got, ref, bound, f"combine of {('float32', 'float64')[kind_of_scores]} scores")
    assert np.array_equal(got_flags, flags) and np.array_equal(np.isnan(got), flagged) and flagged.sum() > 2
    for form, front in ((1, 0), (0, 3)):
        again, again_flags = _run_combine(hip, bc.FIT_SOURCES, bc.FIT_KINDS, kind_of_scores, w, form=form, front=front)
        assert np.array_equal(got.view(np.int64), again.view(np.int64)) and np.array_equal(got_flags, again_flags), (form, front)


# ---- sums ------------------------------------------------------------------------------------------------------------------------
def _run_sums(hip, features, weights, form, front=0):
    """features [M, n] float32 as the kernel wrote them -> (sums, counters)"""
    c = bc.case()
    M, n, n_lists = features.shape[0], c["n"], len(c["offsets_bad"]) - 1
    h = {}
    f, h["features"] = _guard_f32(features, front)
    y, h["labels"] = _guard_labels(c["labels"], front)
    off, h["offsets"] = _guard_words(c["offsets_bad"], 0, 2 * front)
    w, h["weights"] = _guard_f64(weights, front)
    n_e = 1 + M + M * (M + 1) // 2
    sums, h_sums = _out_words(2 * n_e)
    counters, h_cnt = _out_words(6)
    ws_bytes = int(hip.lib().ebn_blend_sums_workspace_bytes(n_lists, M))
    assert ws_bytes > 0
    ws = guarded.poison(torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"))
    rc = hip.lib().ebn_blend_sums_f64(f, y, M, n, off, n_lists, w, form, _ptr(sums), _ptr(counters), _ptr(ws), ws_bytes, hip.stream_handle())
    assert rc == OK
    torch.cuda.synchronize()
    for what, hh in h.items():
        hh.check(what)
    h_sums.check("sums")
    h_cnt.check("counters")
    return h_sums.payload().cpu().numpy().view(np.float64), h_cnt.payload().cpu().numpy().view(np.int64)


@pytest.fixture(scope="module")
def fit6(hip):
    """the M = 6 blend of the case: the kernel's own features and the optimum of the host fit"""
    from ebrec.evaluation import RaggedLists
    from ebrec.models import ScoreBlend

    c = bc.case()
    features, _ = _run_features(hip, bc.FIT_SOURCES, bc.FIT_KINDS, 1, form=0)
    blend = ScoreBlend(transforms=[bc.KIND_NAMES[k] for k in bc.FIT_KINDS], l2=bc.FIT_L2, rrf_k=bc.RRF_K, device=None)
    blend.fit(RaggedLists(c["labels"].astype(np.int64), c["offsets"]), [RaggedLists(bc.scores(1)[m], c["offsets"]) for m in bc.FIT_SOURCES])
    assert blend.converged
    return features, blend


@pytest.mark.parametrize("which", ["zero", "optimum", "saturated"])
def test_sums_stage_by_stage_against_the_twin(hip, fit6, which):
    """the twin on the kernel's own features, so that feature ulps do not enter.  1e-10 A_e: float64 rounding of about 1e4 terms plus
    exp's few ulps is about 1e-12 of the sum A_e of an entry's absolute terms; two orders of margin; a float32 accumulation anywhere
    would miss it by four."""
    from ebrec.models import blend_sums_host

    c = bc.case()
    features, blend = fit6
    w = {"zero": np.zeros(6), "optimum": blend.weights, "saturated": np.array([30.0, -30.0, 30.0, 30.0, -30.0, 30.0])}[which]
    want, counters, absum = blend_sums_host(features, c["labels"], c["offsets_bad"], w, return_abs=True)
    got, got_counters = _run_sums(hip, features, w, form=0)
    assert np.array_equal(got_counters, counters) and counters[2] == 2 and counters.sum() == c["n_lists"] + 1
    _within(got, want, 1e-10 * absum, f"sums at the {which} weights")
    assert np.isfinite(got).all()
    for form, front in ((0, 0), (1, 0), (0, 3), (1, 1)):  # a second run, the general form, other placements: the same bits
        again, again_counters = _run_sums(hip, features, w, form=form, front=front)
        assert np.array_equal(got.view(np.int64), again.view(np.int64)) and np.array_equal(got_counters, again_counters), (form, front)


@pytest.mark.parametrize("M", [1, 16])
def test_sums_at_the_narrowest_and_the_widest_blend(hip, M):
    from ebrec.models import blend_sums_host

    c = bc.case()
    kinds = [(bc.ZSCORE, bc.RAW, bc.MINMAX, bc.RANK, bc.RRF)[m % 5] for m in range(M)]
    src = [3] if M == 1 else list(range(M))  # M = 16: source 1 is raw here, source 0 (1e6) a z-score
    features, _ = _run_features(hip, src, kinds, 0, form=0)
    w = np.random.default_rng(M).normal(size=M)
    want, counters, absum = blend_sums_host(features, c["labels"], c["offsets_bad"], w, return_abs=True)
    got, got_counters = _run_sums(hip, features, w, form=0)
    assert np.array_equal(got_counters, counters) and counters[0] > 190
    _within(got, want, 1e-10 * absum, f"sums of {M} sources")
    general, general_counters = _run_sums(hip, features, w, form=1, front=2)
    assert np.array_equal(got.view(np.int64), general.view(np.int64)) and np.array_equal(got_counters, general_counters)


def test_hessian_stays_positive_semidefinite_with_the_1e6_raw_source(hip):
    from ebrec.models import ensemble as en

    features, _ = _run_features(hip, [0, 1, 4], [bc.RAW, bc.ZSCORE, bc.RANK], 1, form=0)
    got, counters = _run_sums(hip, features, np.array([1e-6, 0.5, -0.3]), form=0)
    _, _, H = en.unpack_sums(got, 3)
    lam = np.linalg.eigvalsh(H)
    print(f"eigenvalues {lam}, trace {np.trace(H):.3e}")
    assert counters[0] > 190 and H[0, 0] > 1e12 and lam.min() >= -1e-12 * np.trace(H)


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_codes_and_launch_nothing(hip):
    L, st = hip.lib(), hip.stream_handle()
    big, c = 2 ** 31, bc.case()
    i = _Inputs(bc.FIT_SOURCES, bc.FIT_KINDS, 0, weights=np.ones(6))
    f, h_f = guarded.guard_out((i.M * i.n,), guard=GUARD)
    out, h_out = _out_words(2 * i.n)
    fl, h_fl = _flags_out(i.n_lists)
    base = dict(S=i.scores, SK=0, M=i.M, N=i.n, O=i.offsets, NL=i.n_lists, K=i.kinds, P=i.params)
    feats = lambda FORM=0, F=_ptr(f), FL=_ptr(fl), **k: L.ebn_blend_features_f32(*[k.get(n, v) for n, v in base.items()], FORM, F, FL, st)
    comb = lambda W=i.weights, FORM=0, OUT=_ptr(out), FL=_ptr(fl), **k: L.ebn_blend_combine_f64(*[k.get(n, v) for n, v in base.items()], W, FORM, OUT,
                                                                                            FL, st)
    before = L.ebn_launch_count()
    bad = (dict(M=0), dict(M=17), dict(M=-1), dict(N=-1), dict(N=big - 256), dict(N=big), dict(NL=-1), dict(NL=big), dict(SK=2), dict(SK=-1),
           dict(S=None), dict(O=None), dict(K=None), dict(P=None), dict(FL=None), dict(FORM=2), dict(FORM=-1))
    for kw in bad:
        assert feats(**kw) == BAD_ARG, kw
        assert comb(**kw) == BAD_ARG, kw
    assert feats(F=None) == BAD_ARG and comb(OUT=None) == BAD_ARG and comb(W=None) == BAD_ARG
    # sums
    features = np.zeros((6, i.n), np.float32)
    fe, h_fe = _guard_f32(features, 0)
    y, h_y = _guard_labels(c["labels"], 0)
    sums, h_sums = _out_words(2 * 28)
    counters, h_cnt = _out_words(6)
    ws_bytes = int(L.ebn_blend_sums_workspace_bytes(i.n_lists, 6))
    assert ws_bytes >= 8 * (28 + 3) and L.ebn_blend_sums_workspace_bytes(0, 6) == 0
    for n_lists, M in ((-1, 6), (big, 6), (10, 0), (10, 17), (10, -1)):
        assert L.ebn_blend_sums_workspace_bytes(n_lists, M) == 0, (n_lists, M)
    ws = guarded.poison(torch.empty(ws_bytes + 16, dtype=torch.uint8, device="cuda"))
    sbase = dict(F=fe, Y=y, M=6, N=i.n, O=i.offsets, NL=i.n_lists, W=i.weights, FORM=0, SUMS=_ptr(sums), CNT=_ptr(counters), WS=_ptr(ws), WSB=ws_bytes)
    run = lambda **k: L.ebn_blend_sums_f64(*[k.get(n, v) for n, v in sbase.items()], st)
    for kw in (dict(M=0), dict(M=17), dict(N=-1), dict(N=big - 256), dict(NL=-1), dict(NL=big), dict(F=None), dict(Y=None), dict(O=None),
               dict(W=None), dict(SUMS=None), dict(CNT=None), dict(WS=None), dict(WSB=ws_bytes - 1), dict(WSB=0), dict(FORM=2),
               dict(WS=_ptr(ws, 8))):
        assert run(**kw) == BAD_ARG, kw
    assert L.ebn_launch_count() == before
    torch.cuda.synchronize()
    for h, what in ((h_f, "features"), (h_out, "out"), (h_fl, "flags"), (h_sums, "sums"), (h_cnt, "counters")):
        h.check_untouched(what)
    # the legal empty forms
    assert feats(NL=0) == OK and comb(NL=0) == OK and L.ebn_launch_count() == before
    assert run(NL=0, N=0, F=None, Y=None, O=None, WS=None, WSB=0) == OK  # zeros in one launch
    torch.cuda.synchronize()
    h_sums.check("sums")
    h_cnt.check("counters")
    assert not h_sums.payload().any() and not h_cnt.payload().any() and L.ebn_launch_count() == before + 1
    i.check()
    h_fe.check("features")
    h_y.check("labels")


# ---- the class on the device -----------------------------------------------------------------------------------------------------
def test_class_on_the_device_against_the_host_path(hip, fit6):
    from ebrec.evaluation import RaggedLists
    from ebrec.models import ScoreBlend, blend_features_host, blend_sums_host
    from ebrec.models import ensemble as en

    c = bc.case()
    _, host = fit6
    names = [bc.KIND_NAMES[k] for k in bc.FIT_KINDS]
    labels = RaggedLists(c["labels"].astype(np.int64), c["offsets"])
    src = [RaggedLists(bc.scores(1)[m].copy(), c["offsets"]) for m in bc.FIT_SOURCES]
    src[2] = RaggedLists(torch.from_numpy(bc.scores(1)[bc.FIT_SOURCES[2]].copy()).cuda(), c["offsets"])  # one source already on the device
    dev = ScoreBlend(transforms=names, l2=bc.FIT_L2, rrf_k=bc.RRF_K, device="cuda").fit(labels, src)
    assert dev.converged and host.converged and len(dev.losses) - 1 <= 20
    assert (dev.n_lists_used, dev.n_one_class, dev.n_nonfinite) == (host.n_lists_used, host.n_one_class, host.n_nonfinite)
    # |w_dev - w_host| <= 10 ||(H / n + l2 I)^-1|| (2 tol + 1e-10 max_e A_e / n): both gradients are below tol, the device sums carry
    # their rounding; first order, with a factor 10 of margin
    features, flags = blend_features_host(bc.scores(1)[bc.FIT_SOURCES], c["offsets"], bc.FIT_KINDS, [bc.RRF_K] * 6)
    sums, counters, absum = blend_sums_host(features, c["labels"], c["offsets"], host.weights, return_abs=True)
    n = int(counters[0])
    Hn = en.unpack_sums(sums, 6)[2] / n + bc.FIT_L2 * np.eye(6)
    w_bound = 10.0 * np.linalg.norm(np.linalg.inv(Hn), 2) * (2 * host.tol + 1e-10 * absum.max() / n)
    print(f"weights: largest difference {np.abs(dev.weights - host.weights).max():.3e} of {w_bound:.3e}; device {dev.weights}")
    assert np.abs(dev.weights - host.weights).max() <= w_bound
    # predict: the combine bound plus the weight bound times sum_m |f_m|
    want, fbound, _ = bc.features_reference(bc.FIT_SOURCES, bc.FIT_KINDS, 1, bad_offsets=False)
    fabs = np.abs(np.nan_to_num(want))
    p_bound = np.abs(host.weights) @ fbound + 2.0 ** -50 * (np.abs(host.weights) @ fabs) + w_bound * fabs.sum(axis=0)
    p_dev, p_host = dev.predict(src), host.predict([RaggedLists(bc.scores(1)[m], c["offsets"]) for m in bc.FIT_SOURCES])
    assert p_dev.flat.is_cuda and p_dev.flat.dtype == torch.float64 and isinstance(p_host.flat, np.ndarray)
    flagged = np.repeat(flags != 0, c["lengths"])
    assert np.array_equal(np.isnan(p_dev.host_flat()), flagged)
    _within(p_dev.host_flat(), p_host.flat, p_bound, "predict, device against host")
    # cross_fit_predict: the same bounds with each item's largest fold weight
    o_dev, fw_dev = ScoreBlend(transforms=names, l2=bc.FIT_L2, device="cuda").cross_fit_predict(labels, src, folds=3)
    o_host, fw_host = ScoreBlend(transforms=names, l2=bc.FIT_L2, device=None).cross_fit_predict(labels, src, folds=3)
    assert o_dev.flat.is_cuda and np.abs(fw_dev - fw_host).max() <= w_bound
    x_bound = np.abs(fw_host).max(axis=0) @ fbound + 2.0 ** -50 * (np.abs(fw_host).max(axis=0) @ fabs) + w_bound * fabs.sum(axis=0)
    _within(o_dev.host_flat(), o_host.flat, x_bound, "cross_fit_predict, device against host")


def test_a_device_tensor_is_used_in_place(hip):
    from ebrec.evaluation import RaggedLists
    from ebrec.models import RankFusion, ScoreBlend

    c = bc.case()
    for dtype in (torch.float32, torch.float64):
        t = torch.from_numpy(bc.scores(1)[4].copy()).to("cuda", dtype)
        stack, _ = ScoreBlend(device="cuda")._stack([RaggedLists(t, c["offsets"])])
        assert stack.data_ptr() == t.data_ptr() and stack.dtype == dtype and stack.shape == (1, c["n"])
    t32 = torch.from_numpy(bc.scores(0)[4].copy()).cuda()
    mixed, _ = ScoreBlend(device="cuda")._stack([RaggedLists(t32, c["offsets"]), RaggedLists(bc.scores(1)[5], c["offsets"])])
    assert mixed.is_cuda and mixed.dtype == torch.float64 and mixed.shape == (2, c["n"])
    fused = RankFusion(device="cuda").predict([RaggedLists(t32, c["offsets"]), RaggedLists(bc.scores(0)[5], c["offsets"])])
    host = RankFusion(device=None).predict([RaggedLists(bc.scores(0)[4], c["offsets"]), RaggedLists(bc.scores(0)[5], c["offsets"])])
    assert fused.flat.is_cuda and np.array_equal(fused.host_flat(), host.flat)  # ranks are exact, the sum of two float32 values too
