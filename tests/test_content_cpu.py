"""The content-similarity baselines on the host (ebrec/models/baselines/content.py): the conditions the cases of
tests/content_cases.py must meet for their bounds to mean something, the numpy twins of the ebn_cs_* kernels against the float64
brute force, and ContentSimilarity(device=None) on the fixture frames -- the three call forms, history_size, the weight kinds
against utils/_decay.py, fill and the errors."""
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from ebrec import _hip
from ebrec.evaluation import RaggedLists
from ebrec.evaluation.beyond_accuracy import DeviceLookup
from ebrec.models import ContentSimilarity, content_centroid_scores_host, content_nearest_scores_host, content_profiles_host
from ebrec.models.baselines import content as cs_mod
from ebrec.utils import _constants as C
from ebrec.utils._decay import exponential_decay_weights, linear_decay_weights
from tests import content_cases as cc

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "ebnerd"
KEY = "document_vector"


def test_header_kernel_and_case_constants_agree():
    text = _hip.header_path().read_text()
    assert int(re.search(r"#define\s+EBN_CS_MAX_D\s+(\d+)", text).group(1)) == cs_mod.MAX_D == cc.MAX_D == max(cc.DIMS)
    src = (ROOT / "ebnerd-benchmark_amd" / "csrc" / "ebn_content.hip").read_text()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1))
    assert (define("CS_THREADS"), define("CS_WAVES"), define("CS_NT")) == (cc.CS_THREADS, cc.CS_WAVES, cc.CS_NT)
    assert cc.CS_WAVES * cc.CS_WAVE == cc.CS_THREADS
    for T in (cc.CS_WAVES, cc.CS_NT, cc.CS_WAVE, cc.CS_THREADS):
        assert {T - 1, T, T + 1} <= set(cc.LENGTHS)
    decl = _hip.declared_functions()
    assert [len(decl[n][1]) for n in ("ebn_cs_profiles_f32", "ebn_cs_centroid_scores_f32", "ebn_cs_nearest_scores_f32")] == [12, 14, 16]


def test_the_exact_case_by_hand():
    c, ref = cc.case("d1_exact")
    assert np.array_equal(ref["centroid"], cc.D1_WANT) and np.array_equal(ref["nearest"], cc.D1_WANT)
    assert ref["profiles"].ravel().tolist() == [1.0, 1.0, 0.0, 1.0]
    assert not ref["centroid_bound"].any() and not ref["nearest_bound"].any() and not ref["profiles_bound"].any()


def test_the_cases_cover_the_listed_edges():
    c, _ = cc.case("lengths")
    h_len, c_len = np.diff(c["hist_offsets"]), np.diff(c["cand_offsets"])
    assert set(cc.LENGTHS) <= set(h_len.tolist()) and set(cc.LENGTHS) <= set(c_len.tolist()) and cc.LONG_HISTORY in h_len
    assert [cc.case(f"dims_{D}")[0]["table"].shape[1] for D in cc.DIMS] == cc.DIMS
    c, _ = cc.case("shared_and_empty")
    lh, n_hists = c["list_hist"], c["hist_offsets"].size - 1
    assert -1 in lh and n_hists in lh and np.bincount(lh[lh >= 0]).max() >= 30 and (np.diff(c["cand_offsets"]) == 0).sum() >= 70
    assert cc.case("unweighted")[0]["hist_weights"] is None and cc.case("identity")[0]["list_hist"] is None
    assert cc.case("one_list")[0]["cand_offsets"].size == 2
    for name in cc.BOUNDED:
        c, ref = cc.case(name)
        w_max = 1.0 if c["hist_weights"] is None else float(c["hist_weights"].max())
        assert np.allclose(np.linalg.norm(c["table"].astype(np.float64), axis=1), 1.0, atol=1e-6)
        assert ref["centroid_bound"].max() < 6e-4 and ref["profiles_bound"].max() < 6e-4
        assert ref["nearest_bound"].max() <= 2 * (c["table"].shape[1] + 8) * cc.U * w_max  # scales with the weight, as the scores do
        assert np.abs(ref["centroid"]).max() > 0.5 and ref["nearest"].max() > 0.5, "a vacuous case"
    c, _ = cc.case("dims_768")
    assert -1 in c["hist_rows"] and c["table"].shape[0] in c["hist_rows"] and -1 in c["cand_rows"] and c["table"].shape[0] in c["cand_rows"]


def _present(c, u):
    a, b = int(c["hist_offsets"][u]), int(c["hist_offsets"][u + 1])
    rows = c["hist_rows"][a:b].astype(np.int64)
    w = np.ones(b - a) if c["hist_weights"] is None else c["hist_weights"][a:b].astype(np.float64)
    ok = (rows >= 0) & (rows < c["table"].shape[0])
    return rows[ok], w[ok]


@pytest.mark.parametrize("name", cc.BOUNDED)
def test_profiles_do_not_cancel(name):
    """||p|| >= 0.4 sum w for every history: the centroid bounds divide by ||p||"""
    c, _ = cc.case(name)
    T = c["table"].astype(np.float64)
    worst = np.inf
    for u in range(c["hist_offsets"].size - 1):
        rows, w = _present(c, u)
        if w.sum() > 0:
            ratio = float(np.linalg.norm((w[:, None] * T[rows]).sum(0)) / w.sum())
            worst = min(worst, ratio)
            assert ratio >= 0.4, (u, ratio)
    print(f"{name}: smallest ||p|| / sum w = {worst:.3f}")


@pytest.mark.parametrize("name", cc.BOUNDED)
def test_dropping_an_end_of_a_history_moves_every_list_that_reads_it(name):
    """in both modes, without a history's first or last present entry at least one score of every list that reads the history
    moves by more than 50 x that item's bound: an implementation that loses an entry cannot hide inside the tolerance"""
    c, ref = cc.case(name)
    n_hists, n_rows = c["hist_offsets"].size - 1, c["table"].shape[0]
    checked, least = 0, np.inf
    for drop in ("first", "last"):
        other = cc.reference(c, drop=drop)
        for l in range(c["cand_offsets"].size - 1):
            u = l if c["list_hist"] is None else int(c["list_hist"][l])
            a, b = int(c["cand_offsets"][l]), int(c["cand_offsets"][l + 1])
            if not 0 <= u < n_hists or a == b or _present(c, u)[1].sum() == 0:
                continue  # exact zeros with or without the entry
            for mode in ("centroid", "nearest"):
                shift = np.abs(other[mode][a:b] - ref[mode][a:b])
                assert np.any(shift > 50 * ref[mode + "_bound"][a:b]), (drop, mode, l, u, shift.max(), ref[mode + "_bound"][a:b].max())
                least = min(least, float(shift.max()))
                checked += 1
    assert checked > 0
    print(f"{name}: {checked} (list, mode, end) checks, smallest largest shift {least:.3f}")


def _within(got, want, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    assert got.shape == want.shape and np.all(err <= bound), f"{what}: {int((err > bound).sum())} of {err.size} outside the bound"
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("name", cc.NAMES)
def test_twins_against_the_brute_force(name):
    c, ref = cc.case(name)
    p = content_profiles_host(c["table"], c["hist_rows"], c["hist_weights"], c["hist_offsets"])
    s_c = content_centroid_scores_host(c["table"], p, c["list_hist"], c["cand_rows"], c["cand_offsets"])
    s_n = content_nearest_scores_host(c["table"], c["hist_rows"], c["hist_weights"], c["hist_offsets"], c["list_hist"], c["cand_rows"],
                                      c["cand_offsets"])
    assert p.dtype == s_c.dtype == s_n.dtype == np.float64
    tiny = 1e-12  # float64 twins: far inside the fp32 bounds; the exact case must still be exact
    for got, key in ((p, "profiles"), (s_c, "centroid"), (s_n, "nearest")):
        bound = ref[key + "_bound"] if c["exact"] else np.minimum(ref[key + "_bound"], tiny)
        err = _within(got, ref[key], bound, f"{name} {key}")
        print(f"{name} {key}: largest error {err:.3e}, fp32 bound up to {ref[key + '_bound'].max():.3e}")


def test_twins_in_small_chunks_give_the_same_scores(monkeypatch):
    c, ref = cc.case("lengths")
    monkeypatch.setattr(cs_mod, "_CHUNK_FLOATS", 96 * 7)
    p = content_profiles_host(c["table"], c["hist_rows"], c["hist_weights"], c["hist_offsets"])
    _within(p, ref["profiles"], np.minimum(ref["profiles_bound"], 1e-12), "profiles")
    s_c = content_centroid_scores_host(c["table"], p, c["list_hist"], c["cand_rows"], c["cand_offsets"])
    _within(s_c, ref["centroid"], np.minimum(ref["centroid_bound"], 1e-12), "centroid")
    s_n = content_nearest_scores_host(c["table"], c["hist_rows"], c["hist_weights"], c["hist_offsets"], c["list_hist"], c["cand_rows"],
                                      c["cand_offsets"])
    _within(s_n, ref["nearest"], np.minimum(ref["nearest_bound"], 1e-12), "nearest")


# ---- the class on the fixture frames -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


@pytest.fixture(scope="module")
def lookup(frames):
    return cc.synthetic_lookup(*frames, key=KEY)


@pytest.mark.parametrize("mode", ["centroid", "nearest"])
def test_class_on_the_fixture_frames(frames, lookup, mode):
    behaviors, history = frames
    cs = ContentSimilarity(lookup, KEY, mode=mode, history_weights="exponential", lambda_factor=0.8, device=None)
    assert isinstance(cs.lookup, DeviceLookup) and np.allclose(np.linalg.norm(cs.host_unit_table().astype(np.float64), axis=1), 1, atol=1e-6)
    scores = cs.predict(behaviors, history=history)
    c = cc.frames_case(cs, behaviors, history, lambda n: exponential_decay_weights(n, 0.8, ascending=True))
    ref = cc.reference(c)
    assert isinstance(scores, RaggedLists) and isinstance(scores.flat, np.ndarray) and scores.flat.dtype == np.float64
    assert np.array_equal(scores.offsets, c["cand_offsets"]) and (c["cand_rows"] < 0).mean() > 0.02 and (c["hist_rows"] < 0).mean() > 0.02
    err = _within(scores.flat, ref[mode], ref[mode + "_bound"], mode)  # fp32 weights and profiles: inside the fp32 bounds
    print(f"{mode}: {scores.flat.size} scores, largest error {err:.3e}, bound up to {ref[mode + '_bound'].max():.3e}")
    assert np.abs(scores.flat).max() > 0.5 and np.all(scores.flat[c["cand_rows"] < 0] == 0)
    # the joined frame carries the history per impression; the raw-lists forms
    joined = behaviors.merge(history[[C.DEFAULT_USER_COL, C.DEFAULT_HISTORY_ARTICLE_ID_COL]], on=C.DEFAULT_USER_COL, how="inner")
    assert len(joined) == len(behaviors)
    per_impression = cs.predict(joined)
    assert np.array_equal(per_impression.flat, scores.flat) and np.array_equal(per_impression.offsets, scores.offsets)
    raw = cs.predict(list(joined[C.DEFAULT_INVIEW_ARTICLES_COL]), list(joined[C.DEFAULT_HISTORY_ARTICLE_ID_COL]))
    assert np.array_equal(raw.flat, scores.flat)
    shared = cs.predict(RaggedLists.from_lists([np.asarray(v) for v in behaviors[C.DEFAULT_INVIEW_ARTICLES_COL]]),
                        list(history[C.DEFAULT_HISTORY_ARTICLE_ID_COL]), list_hist=c["list_hist"])
    assert np.array_equal(shared.flat, scores.flat)
    # a user the history frame does not hold: -1, every score of theirs is the fill
    gone = history[C.DEFAULT_USER_COL].iloc[0]
    fewer = ContentSimilarity(lookup, KEY, mode=mode, history_weights="exponential", lambda_factor=0.8, fill=-7.0, device=None) \
        .predict(behaviors, history=history.iloc[1:])
    theirs = np.repeat((behaviors[C.DEFAULT_USER_COL] == gone).to_numpy(), np.diff(scores.offsets))
    assert theirs.any() and np.all(fewer.flat[theirs] == -7.0)
    keep = ~theirs & (c["cand_rows"] >= 0)
    assert np.all(fewer.flat[~theirs & (c["cand_rows"] < 0)] == -7.0) and np.array_equal(fewer.flat[keep], scores.flat[keep])


def test_history_size_and_profiles(frames, lookup):
    behaviors, history = frames
    cs = ContentSimilarity(lookup, KEY, history_weights="linear", history_size=5, device=None)
    c = cc.frames_case(cs, behaviors, history, lambda n: linear_decay_weights(n, ascending=True))
    assert np.diff(c["hist_offsets"]).max() == 5 and np.diff(c["hist_offsets"]).min() >= 1
    ref = cc.reference(c)
    _within(cs.predict(behaviors, history=history).flat, ref["centroid"], ref["centroid_bound"], "centroid")
    p = cs.profiles(list(history[C.DEFAULT_HISTORY_ARTICLE_ID_COL]))
    assert p.dtype == np.float32 and p.shape == (len(history), 24)
    _within(p, ref["profiles"], ref["profiles_bound"] + 2.0 ** -24, "profiles")  # + the rounding to float32
    full = ContentSimilarity(lookup, KEY, history_weights="linear", device=None).predict(behaviors, history=history)
    assert not np.array_equal(full.flat, cs.predict(behaviors, history=history).flat)


def test_weight_kinds_against_the_list_functions():
    offsets = np.array([0, 5, 5, 6, 16, 19], np.int64)
    lin = cs_mod.history_weight_values("linear", offsets)
    exp = cs_mod.history_weight_values("exponential", offsets, 0.5)
    assert lin[:5].tolist() == [0.2, 0.4, 0.6, 0.8, 1.0] and exp[:5].tolist() == [0.0625, 0.125, 0.25, 0.5, 1.0]  # the doctests
    assert lin[6:16].tolist() == [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0] and lin[5] == 1.0
    for kind, fn in (("linear", lambda n: linear_decay_weights(n, True)), ("exponential", lambda n: exponential_decay_weights(n, 0.9, True))):
        got = cs_mod.history_weight_values(kind, offsets, 0.9)
        want = np.concatenate([fn(int(n)) for n in np.diff(offsets)])
        assert got.dtype == np.float64 and np.array_equal(got, want), kind
    calls = []

    def ramp(n):
        calls.append(n)
        return np.arange(1, n + 1) * 0.5

    got = cs_mod.history_weight_values(ramp, offsets)
    assert sorted(calls) == [1, 3, 5, 10] and got[:5].tolist() == [0.5, 1.0, 1.5, 2.0, 2.5] and got[16:].tolist() == [0.5, 1.0, 1.5]
    assert cs_mod.history_weight_values(None, offsets) is None
    for bad in (lambda n: [-1.0] * n, lambda n: [float("nan")] * n, lambda n: [float("inf")] * n):
        with pytest.raises(ValueError, match="finite and not negative"):
            cs_mod.history_weight_values(bad, offsets)
    with pytest.raises(ValueError, match="finite and not negative"):
        cs_mod.history_weight_values("exponential", offsets, -0.5)
    with pytest.raises(ValueError, match="returned 2 weights"):
        cs_mod.history_weight_values(lambda n: [1.0, 1.0], offsets)


def test_fill_and_errors():
    table = {i: {KEY: v} for i, v in zip((10, 20, 30), np.eye(3, dtype=np.float32) * 2)}
    table[40] = {KEY: np.zeros(3, np.float32)}  # a zero row stays zero
    cs = ContentSimilarity(table, KEY, mode="nearest", fill=-1.0, device=None)
    got = cs.predict([[10, 20, 99], [10], [30, 40]], [[10, 99], [77, 88], [40, 30]])
    assert got.to_lists() == [[1.0, 0.0, -1.0], [-1.0], [1.0, 0.0]]  # unknown candidate; no known history article
    got = ContentSimilarity(table, KEY, mode="centroid", fill=0.5, device=None).predict([[10, 20], [10]], [[10], []], list_hist=[0, -1])
    assert got.to_lists() == [[1.0, 0.0], [0.5]]
    assert ContentSimilarity(table, KEY, device=None).predict([[], []], [[10], [20]]).to_lists() == [[], []]
    with pytest.raises(ValueError, match="mode"):
        ContentSimilarity(table, KEY, mode="knn", device=None)
    with pytest.raises(ValueError, match="history_weights"):
        ContentSimilarity(table, KEY, history_weights="quadratic", device=None)
    with pytest.raises(ValueError, match="history_size"):
        ContentSimilarity(table, KEY, history_size=0, device=None)
    with pytest.raises(ValueError, match="vector keys"):
        ContentSimilarity(DeviceLookup(table, vector_keys=(), device=None), KEY, device=None)
    with pytest.raises(ValueError, match="pass list_hist"):
        cs.predict([[10], [20]], [[10]])
    with pytest.raises(ValueError, match="history indices"):
        cs.predict([[10], [20]], [[10]], list_hist=[0])
    with pytest.raises(ValueError, match="needs the histories"):
        cs.predict([[10], [20]])
    with pytest.raises(ValueError, match="article_id_fixed"):
        cs.predict(pd.DataFrame({C.DEFAULT_INVIEW_ARTICLES_COL: [[10]]}))
    with pytest.raises(ValueError, match="finite and not negative"):
        ContentSimilarity(table, KEY, history_weights=lambda n: [-1.0] * n, device=None).predict([[10]], [[10, 20]])
    wide = {1: {KEY: np.ones(cs_mod.MAX_D + 1, np.float32)}}
    with pytest.raises(ValueError, match="at most 1024"):
        ContentSimilarity(wide, KEY, device=None)
