"""Host side of calibrated re-ranking: the float64 restatement on the hand-computed case, the product's host path against it,
history_distribution(), Calibration, the decay weights, DeviceLookup's label keys, argument validation of calibrated_rerank(),
recommend(rerank=Calibrated(...)) and the two entry points.  No GPU: nothing here launches a kernel."""
import ctypes
import doctest
import re

import numpy as np
import pytest

from ebrec.evaluation import Calibrated, Calibration, calibrated_rerank, history_distribution
from ebrec.evaluation.beyond_accuracy import DeviceLookup
from ebrec.models.newsrec._recommend import recommend
from ebrec.utils._decay import exponential_decay_weights, linear_decay_weights
from tests import calibrate_cases as cc
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)
from tests.test_recommend_cpu import _HostOnlyModel, _loader

HAND_W = np.eye(2)[[0, 0, 0, 0, 1, 1]]
HAND_ROWS, HAND_REL = np.arange(6)[None], np.array([[.9, .8, .7, .6, .5, .4]])
HAND_PICKS = {1.0: [0, 1, 2, 3], 0.5: [0, 4, 1, 2], 0.0: [0, 4, 1, 5]}


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_the_hand_computed_case():
    """Labels [0, 0, 0, 0, 1, 1], p = (.5, .5), alpha = .01, k = 4.  lam = 0: a list of one label has KL
    .5 ln(.5 / .995) + .5 ln(.5 / .005) = 1.95852 whichever label (a tie: the smaller index), the balanced lists of two and four have
    KL 0 exactly, a 2 : 1 list .05765.  lam = .5: the smallest winning margin is .08 (round 3, entry 2 over entry 5)."""
    for lam, picks in HAND_PICKS.items():
        sel, obj, flags, lead = cc.calibrated_reference(HAND_W, HAND_ROWS, HAND_REL, np.array([.5, .5]), 4, lam, 0.01, margins=True)
        assert sel.tolist() == [picks] and flags == (0, 0), lam
    assert obj.tolist()[0][1] == 0.0 and obj.tolist()[0][3] == 0.0 and lead[0] == 0.0  # lam = 0: exact zeros, and a tie
    assert abs(obj[0, 0] + (.5 * np.log(.5 / .995) + .5 * np.log(.5 / .005))) < 1e-15
    assert abs(obj[0, 2] + (.5 * np.log(.5 / (.99 * 2 / 3 + .005)) + .5 * np.log(.5 / (.99 / 3 + .005)))) < 1e-15
    lead = cc.calibrated_reference(HAND_W, HAND_ROWS, HAND_REL, np.array([.5, .5]), 4, 0.5, 0.01, margins=True)[3]
    assert abs(lead[0] - 0.0797) < 1e-4
    sel, obj, _ = cc.calibrated_reference(HAND_W, HAND_ROWS, HAND_REL, np.array([.5, .5]), 4, 1.0)
    assert obj.tolist() == [[.9, .8, .7, .6]]


def test_restatement_absence_flags_targets_and_short_lists():
    W = np.eye(2)
    rows = np.array([[-1, 1, 0, 2, 0], [-1, -1, -1, -1, -1]])
    rel = np.array([[-np.inf, 0.25, 0.5, 9.0, np.nan], [-np.inf] * 5])
    sel, obj, flags = cc.calibrated_reference(W, rows, rel, np.array([0.5, 0.5]), 3, 0.5)
    assert sel.tolist() == [[2, 1, -1], [-1, -1, -1]] and flags == (1, 1) and np.isneginf(obj[1]).all() and np.isneginf(obj[0, 2])
    assert cc.calibrated_reference(W, rows[:, :3], rel[:, :3], np.array([0.5, 0.5]), 3, 0.5)[2] == (0, 0)
    # a negative or NaN target entry counts as 0 and is flagged; the target is not renormalised
    a = cc.calibrated_reference(W, rows[:, :3], rel[:, :3], np.array([[-1.0, 0.5], [np.nan, 0.5]]), 3, 0.5)
    b = cc.calibrated_reference(W, rows[:, :3], rel[:, :3], np.array([0.0, 0.5]), 3, 0.5)
    assert a[2] == (0, 1) and b[2] == (0, 0) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # an all-zero target: lam * rel alone; a zero label row is a legal pick that only dilutes the list
    sel, obj, _ = cc.calibrated_reference(W, np.array([[0, 1, 0]]), np.array([[0.25, 0.75, 0.5]]), np.zeros(2), 3, 0.5)
    assert sel.tolist() == [[1, 2, 0]] and obj.tolist() == [[0.375, 0.25, 0.125]]
    Wz = np.array([[1.0, 0.0], [0.0, 0.0]])
    sel, obj, _ = cc.calibrated_reference(Wz, np.array([[1, 0]]), np.array([[0.5, 0.5]]), np.array([1.0, 0.0]), 2, 0.0)
    assert sel.tolist() == [[1, 0]] and obj[0, 0] == 0.0 and abs(obj[0, 1] + np.log(1 / 0.505)) < 1e-12  # alone it would cost ln 100
    # the history target: weights per slot, -1 silent, another row outside flagged, nothing valid gives zeros
    p, flag = cc.target_reference(W, np.array([[0, 1, 1, -1], [-1, -1, -1, -1], [0, 2, -1, -1]]))
    assert p.tolist() == [[1 / 3, 2 / 3], [0.0, 0.0], [1.0, 0.0]] and flag == 1
    p, flag = cc.target_reference(W, np.array([[0, 1, 1, -1]]), [0.5, 0.25, 0.25, 8.0])
    assert p.tolist() == [[0.5, 0.5]] and flag == 0
    assert cc.target_reference(W, np.array([[0, 1]]), [0.0, 0.0])[0].tolist() == [[0.0, 0.0]]


def test_tolerance_is_the_stated_bound():
    for lam, C, k in ((0.3, 64, 10), (0.7, 24, 5), (0.5, 1, 1)):
        B = 2.0 ** -23 * ((8 + k) + (4 + 1 + C) * (np.log(100.0) + np.log(max(C, 2))))
        assert cc.tolerance(lam, C, k) == (1 - lam) * B + 4 * 2.0 ** -23
    assert cc.tolerance(1.0, 128, 64) == 4 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the product's host path
def _articles(n_rows, C, seed, multi):
    """articles 100 + r with a label attribute 'lab' (a string; with `multi` a list of one to three, sometimes with a repeat, an
    empty list or None) -> (lookup dict, vocabulary, W float64 [n_rows, len(vocabulary)]) -- the table built here, by the rule"""
    rng = np.random.default_rng(seed)
    per_row = []
    for r in range(n_rows):
        if multi:
            labels = [f"t{c:03d}" for c in rng.choice(C, min(C, int(rng.integers(1, 4))), replace=False)]
            roll = rng.random()
            per_row.append(None if roll < 0.05 else [] if roll < 0.1 else labels + labels[:1] if roll < 0.2 else labels)
        else:
            per_row.append(None if rng.random() < 0.05 else f"t{int(rng.integers(0, C)):03d}")
    as_list = [[] if v is None else sorted(set(v)) if isinstance(v, list) else [v] for v in per_row]
    vocab = sorted({l for v in as_list for l in v})
    W = np.zeros((n_rows, len(vocab)))
    for r, v in enumerate(as_list):
        for l in v:
            W[r, vocab.index(l)] = 1.0 / len(v)
    return {100 + r: {"lab": per_row[r], "pop": 0.5} for r in range(n_rows)}, vocab, W


def _as_ids(rows, unknown):
    """rows -> ids: article 100 + row; -1 for a row of -1, or (every other one) an id the lookup does not know"""
    ids = np.where(rows >= 0, rows + 100, -1)
    flat = ids.ravel()
    gone = np.flatnonzero(flat == -1)
    flat[gone[::2]] = unknown
    return ids


@pytest.mark.parametrize("multi", [False, True], ids=["one-hot", "lists"])
@pytest.mark.parametrize("shape", [(3, 3, 2, 10, 4), (7, 33, 33, 10, 7), (6, 50, 65, 10, 20)], ids=cc.shape_id)
def test_host_path_equals_the_restatement(shape, multi):
    U, P, C, k, H = shape
    _, rows, rel, hist = cc.rounded_case(U, P, C, H, seed=sum(shape))
    rel[0, 0] = np.nan  # absent
    lookup, vocab, W = _articles(4 * P, C, seed=P, multi=multi)
    ids, hist_ids = _as_ids(rows, 7), _as_ids(hist, 9)
    ragged = [h[:1 + (u * 3) % H].tolist() for u, h in enumerate(hist_ids)]  # ragged histories, unknown ids among them
    ragged_rows = np.full((U, H), -1)
    for u, h in enumerate(ragged):
        ragged_rows[u, :len(h)] = hist[u, :len(h)]
    weights = np.asarray(exponential_decay_weights(H, 0.8))
    p_hist = cc.target_reference(W, ragged_rows, weights)[0]
    total = p_hist.sum(1, keepdims=True)
    p_rows = p_hist * 3.0 / np.where(total == 0, 1.0, total * 3.0)
    shared = np.random.default_rng(1).random(len(vocab))
    shared[::3] = 0.0
    for lam in (0.3, 0.7, 1.0):
        for target, kw in ((p_hist, dict(histories=ragged, history_weights=weights)), (shared / shared.sum(), dict(target=shared)),
                           (shared / shared.sum(), dict(target={l: float(x) for l, x in zip(vocab, shared) if x > 0})),
                           (p_rows, dict(target=p_hist * 3.0))):  # an [n, C] target is normalised row by row
            want_sel, _, _, lead = cc.calibrated_reference(W, rows, rel, target, k, lam, 0.02, margins=True)
            assert (lead > 1e-9).all() or lam == 1.0  # nothing for float64 rounding in another order to decide
            kept = np.maximum(want_sel, 0).astype(np.int64)
            want_ids = np.where(want_sel >= 0, np.take_along_axis(ids, kept, 1), -1)
            want_scores = np.where(want_sel >= 0, np.take_along_axis(rel, kept, 1), -np.inf)
            got_ids, got_scores = calibrated_rerank(ids, rel, lookup, "lab", k, lam=lam, alpha=0.02, return_scores=True, **kw)
            assert np.array_equal(got_ids, want_ids) and np.array_equal(got_scores, want_scores) and got_scores.dtype == rel.dtype
            dl = DeviceLookup(lookup, label_keys=["lab"], device=None)
            assert np.array_equal(calibrated_rerank(ids, rel, dl, "lab", k, lam=lam, alpha=0.02, **kw), want_ids)
    assert (want_sel[:, 0] >= 0).all() and not np.isin(0, want_sel[0])


def test_host_path_on_the_hand_case_strings_fill_and_empty_inputs():
    lookup = {f"a{i}": {"g": "x" if i < 4 else "y"} for i in range(6)}
    ids = np.array([[f"a{i}" for i in range(6)] + ["zz"]])
    scores = np.append(HAND_REL, 5.0)[None]
    for lam, picks in HAND_PICKS.items():
        got, kept = calibrated_rerank(ids, scores, lookup, "g", 4, target={"x": 2, "y": 2}, lam=lam, return_scores=True, fill_id="none")
        assert got.tolist() == [[f"a{i}" for i in picks]] and kept.tolist() == [HAND_REL[0, picks].tolist()]
        assert calibrated_rerank(ids, scores, lookup, "g", 4, histories=[["a0", "a5", "unknown"]], lam=lam).tolist() == got.tolist()
        assert calibrated_rerank(ids, scores, lookup, "g", 4, histories=np.array([["a0", "a5"]]), lam=lam).tolist() == got.tolist()
    assert calibrated_rerank(ids, scores, lookup, "g", 8, lam=1.0, target=[1, 1], fill_id="none").tolist() == [[f"a{i}" for i in range(6)] + ["none"] * 2]
    assert calibrated_rerank(np.empty((0, 4), "<U2"), np.empty((0, 4)), lookup, "g", 3, target=[1, 0]).shape == (0, 3)
    # an empty history: the relevance order
    assert calibrated_rerank(ids, scores, lookup, "g", 3, histories=[[]], lam=0.5).tolist() == [["a0", "a1", "a2"]]


def test_history_distribution_with_decay_weights():
    lookup = {1: {"t": ["a", "b"]}, 2: {"t": ["b"]}, 3: {"t": None}, 4: {"t": "c"}}
    p, vocab = history_distribution([[1, 2, 4], [4, 99], [], [3]], lookup, "t")
    assert vocab == ["a", "b", "c"]
    assert np.allclose(p, [[1 / 6, 1 / 2, 1 / 3], [0, 0, 1], [0, 0, 0], [0, 0, 0]], atol=1e-15) and p.dtype == np.float64
    w = linear_decay_weights(4)  # .25, .5, .75, 1: one weight per SLOT, an unknown id's slot drops out of both sums
    p, _ = history_distribution(np.array([[1, 99, 2, 4]]), lookup, "t", weights=w)
    assert np.allclose(p, [[0.125 / 2, (0.125 + 0.75) / 2, 1.0 / 2]], atol=1e-15)
    p, _ = history_distribution([[1, 2], [4]], DeviceLookup(lookup, label_keys=["t"], device=None), "t", weights=exponential_decay_weights(2, 0.5))
    assert np.allclose(p, [[0.25 / 1.5, 1.25 / 1.5, 0], [0, 0, 1]], atol=1e-15)
    assert np.array_equal(p, cc.target_reference(np.array([[.5, .5, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1]]), np.array([[0, 1], [3, -1]]), [0.5, 1.0])[0])
    with pytest.raises(ValueError, match="history_weights has 2 entries, the longest history 3"):
        history_distribution([[1, 2, 4]], lookup, "t", weights=[1, 1])
    with pytest.raises(ValueError, match="finite weights >= 0"):
        history_distribution([[1, 2, 4]], lookup, "t", weights=[1, -1, 1])


def test_calibration_metric_against_a_hand_value_and_its_doctest():
    lookup = {f"a{i}": {"g": "x" if i < 4 else "y"} for i in range(6)}
    H = [["a0", "a4"], ["a0", "a4"], ["a0", "a1", "a5", "gone"], [], ["a0"]]
    R = [["a0", "a5"], ["a0", "a1"], ["a0", "a1", "a4"], ["a0"], ["nothing"]]
    got = Calibration()(R, H, lookup, "g")
    one_sided = .5 * np.log(.5 / .995) + .5 * np.log(.5 / .005)
    assert np.allclose(got[:4], [0.0, one_sided, 0.0, 0.0], atol=1e-15) and np.isnan(got[4]) and abs(one_sided - 1.9585177736) < 1e-9
    assert np.allclose(Calibration()(R, H, lookup, "g", alpha=0.5)[1], .5 * np.log(.5 / .75) + .5 * np.log(.5 / .25), atol=1e-15)
    dl = DeviceLookup(lookup, label_keys=["g"], device=None)
    assert np.array_equal(Calibration()(R, H, dl, "g"), got, equal_nan=True)
    assert np.array_equal(Calibration()(np.array(R[:2]), np.array(H[:2]), lookup, "g"), got[:2])
    # it reports what the re-ranker optimises: the lam = 0 list of the hand case is calibrated, the relevance order is not
    ids = np.array([[f"a{i}" for i in range(6)]])
    cal = calibrated_rerank(ids, HAND_REL, lookup, "g", 4, histories=[["a0", "a4"]], lam=0.0)
    assert abs(Calibration()(cal, [["a0", "a4"]], lookup, "g")[0]) < 1e-15 and Calibration()(ids[:, :4], [["a0", "a4"]], lookup, "g")[0] > 1.9
    with pytest.raises(ValueError, match="do not match"):
        Calibration()(R, H[:2], lookup, "g")
    with pytest.raises(ValueError, match="alpha must lie in"):
        Calibration()(R, H, lookup, "g", alpha=1.0)
    import ebrec.evaluation.beyond_accuracy as ba
    finder, runner = doctest.DocTestFinder(), doctest.DocTestRunner(optionflags=doctest.NORMALIZE_WHITESPACE)
    tests = [t for t in finder.find(ba.Calibration, "Calibration", globs=vars(ba).copy()) if t.examples]
    assert tests and all(runner.run(t).failed == 0 for t in tests)


def test_decay_weights_give_the_four_documented_examples():
    assert linear_decay_weights(5, True) == [0.2, 0.4, 0.6, 0.8, 1.0]
    assert linear_decay_weights(10, False) == [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1]
    assert exponential_decay_weights(5, 0.5, True) == [0.0625, 0.125, 0.25, 0.5, 1.0]
    assert exponential_decay_weights(10, 0.5, False) == [1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125, 0.00390625, 0.001953125]
    assert linear_decay_weights(0) == [] and exponential_decay_weights(1, 0.3) == [1.0] and linear_decay_weights(3, lambda_factor=9) == [1 / 3, 2 / 3, 1.0]
    import ebrec.utils._decay as decay
    assert doctest.testmod(decay).failed == 0 and doctest.testmod(decay).attempted == 4


def test_device_lookup_label_tables_and_vocabulary_on_the_host():
    lookup = {30: {"cat": "news", "topics": ["b", "a", "b"], "v": [1.0, 0.0], "s": 0.5},
              10: {"cat": "sport", "topics": [], "v": [0.0, 1.0], "s": 0.25},
              20: {"cat": None, "topics": None, "v": [1.0, 1.0], "s": 0.0},
              40: {"cat": "news", "topics": np.array(["c"]), "v": [2.0, 0.0], "s": 1.0}}
    dl = DeviceLookup(lookup, ["v"], ["s"], label_keys=["cat", "topics"], device=None)
    assert dl.ids.tolist() == [10, 20, 30, 40] and dl.label_keys == ("cat", "topics")
    assert dl.label_vocabulary("cat") == ["news", "sport"] and dl.label_vocabulary("topics") == ["a", "b", "c"]
    assert dl.host_table("cat").tolist() == [[0, 1], [0, 0], [1, 0], [1, 0]] and dl.host_table("cat").dtype == np.float32
    assert dl.host_table("topics").tolist() == [[0, 0, 0], [0, 0, 0], [0.5, 0.5, 0], [0, 0, 1]]
    assert dl.host_table("v").shape == (4, 2) and dl.host_table("s").tolist() == [0.25, 0.0, 0.5, 1.0]  # the old keys as before
    assert not dl.holds("cat") and DeviceLookup(lookup, label_keys=["cat"]).holds("cat") and not DeviceLookup(lookup, ["v"]).holds("cat")
    assert DeviceLookup(lookup, ["v"]).label_keys == () and dict(dl) == lookup
    with pytest.raises(KeyError):
        dl.label_vocabulary("v")
    with pytest.raises(ValueError, match="not present"):
        DeviceLookup(lookup, label_keys=["nothing"], device=None)
    thirds = DeviceLookup({1: {"t": ["x", "y", "z"]}}, label_keys=["t"], device=None).host_table("t")
    assert thirds.tolist() == [[np.float32(1 / 3)] * 3]


# ------------------------------------------------------------------------------------------------ calibrated_rerank(): validation
def test_calibrated_rerank_validates_its_arguments():
    lookup = {i: {"cat": "abcd"[i % 4], "emb": np.eye(4)[i % 4]} for i in range(8)}
    ids, scores, hist = np.arange(8).reshape(2, 4), np.ones((2, 4)), [[0], [1]]
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"lam must lie in \[0, 1\]"):
            calibrated_rerank(ids, scores, lookup, "cat", 2, histories=hist, lam=bad)
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match=r"alpha must lie in \(0, 1\)"):
            calibrated_rerank(ids, scores, lookup, "cat", 2, histories=hist, alpha=bad)
    with pytest.raises(ValueError, match="at most 64 entries"):
        calibrated_rerank(np.zeros((2, 65), int), np.zeros((2, 65)), lookup, "cat", 2, histories=hist)
    for bad in (65, 0):
        with pytest.raises(ValueError, match="top_n must lie in"):
            calibrated_rerank(ids, scores, lookup, "cat", bad, histories=hist)
    for dl in (DeviceLookup(lookup, ["emb"], device=None), DeviceLookup(lookup, ["emb"]), DeviceLookup(lookup, label_keys=["cat"])):
        with pytest.raises(ValueError, match="not a label key"):
            calibrated_rerank(ids, scores, dl, "emb", 2, histories=hist)
    with pytest.raises(ValueError, match="not present"):
        calibrated_rerank(ids, scores, lookup, "nothing", 2, histories=hist)
    with pytest.raises(ValueError, match="needs the click histories"):
        calibrated_rerank(ids, scores, lookup, "cat", 2)
    with pytest.raises(ValueError, match="1 histories for 2 lists"):
        calibrated_rerank(ids, scores, lookup, "cat", 2, histories=hist[:1])
    with pytest.raises(ValueError, match="target must be 'history'"):
        calibrated_rerank(ids, scores, lookup, "cat", 2, target="editorial")
    with pytest.raises(ValueError, match="outside the lookup's vocabulary"):
        calibrated_rerank(ids, scores, lookup, "cat", 2, target={"a": 1, "q": 1})
    with pytest.raises(ValueError, match=r"\[C\] or \[n, C\] with C = 4"):
        calibrated_rerank(ids, scores, lookup, "cat", 2, target=[1, 1, 1])
    with pytest.raises(ValueError, match="3 target rows for 2 lists"):
        calibrated_rerank(ids, scores, lookup, "cat", 2, target=np.ones((3, 4)))
    with pytest.raises(ValueError, match="finite and not negative"):
        calibrated_rerank(ids, scores, lookup, "cat", 2, target=[1, -1, 1, 1])
    with pytest.raises(ValueError, match="one shape"):
        calibrated_rerank(ids, scores[:, :3], lookup, "cat", 2, histories=hist)
    # the limits of the device path are found on the host, before anything is uploaded
    wide = DeviceLookup({i: {"cat": i} for i in range(129)}, label_keys=["cat"])
    with pytest.raises(ValueError, match="1 to 128 labels, 'cat' has 129"):
        calibrated_rerank(ids, scores, wide, "cat", 2, histories=hist)
    with pytest.raises(ValueError, match="1 to 128 labels, 'cat' has 129"):
        history_distribution(hist, wide, "cat")
    assert calibrated_rerank(ids, scores, dict(wide), "cat", 2, histories=hist).shape == (2, 2)  # the host path has no such limit
    dl = DeviceLookup(lookup, label_keys=["cat"])
    with pytest.raises(ValueError, match="histories of at most 256 articles, got 257"):
        calibrated_rerank(ids, scores, dl, "cat", 2, histories=np.zeros((2, 257), int))
    with pytest.raises(ValueError, match="histories of at most 256 articles, got 257"):
        history_distribution(np.zeros((2, 257), int), dl, "cat")
    assert calibrated_rerank(np.zeros((2, 64), int), np.zeros((2, 64)), lookup, "cat", 64, histories=np.zeros((2, 300), int)).shape == (2, 64)


# ------------------------------------------------------------------------------------------------ recommend(rerank=...): validation
def test_recommend_validates_calibrated_before_the_device_works(frames):  # noqa: F811
    loader, mapping = _loader(frames, True)
    model, ids = _HostOnlyModel(), sorted(mapping)[:12]
    articles = {int(a): {"cat": "abc"[j % 3], "topics": ["x", "y"][:j % 3], "emb": np.eye(4)[j % 4], "pop": 0.5} for j, a in enumerate(ids)}
    lookup = DeviceLookup(articles, ["emb"], ["pop"], label_keys=["cat", "topics"])
    ok = [Calibrated(lookup, "cat", lam=0.5, pool=10), Calibrated(lookup, "topics", pool=64),  # clamped to the 12 candidates
          Calibrated(lookup, "cat", pool=5), Calibrated(lookup, "cat", pool=10, target={"a": 2, "c": 1}),
          Calibrated(lookup, "cat", pool=10, target=np.array([0.2, 0.3, 0.5])),
          Calibrated(lookup, "cat", pool=10, history_weights=linear_decay_weights(20))]
    for rerank in ok:
        with pytest.raises(RuntimeError, match="validation passed"):
            recommend(model, loader, ids, top_n=5, rerank=rerank)
    for pool in (4, 65):
        with pytest.raises(ValueError, match=r"Calibrated pool must lie in \[top_n, 64\] = \[5, 64\]"):
            recommend(model, loader, ids, top_n=5, rerank=Calibrated(lookup, "cat", pool=pool))
    for lam in (-0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="lam must lie in"):
            recommend(model, loader, ids, top_n=5, rerank=Calibrated(lookup, "cat", lam=lam, pool=10))
    for alpha in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match="alpha must lie in"):
            recommend(model, loader, ids, top_n=5, rerank=Calibrated(lookup, "cat", alpha=alpha, pool=10))
    few = DeviceLookup({a: articles[a] for a in ids[:9]}, label_keys=["cat"])
    with pytest.raises(ValueError, match=rf"without a 'cat' label row in the Calibrated lookup: \[{ids[9]}, {ids[10]}, {ids[11]}\]"):
        recommend(model, loader, ids, top_n=5, rerank=Calibrated(few, "cat", pool=10))
    for lk, key in ((lookup, "emb"), (lookup, "pop"), (lookup, "nothing"), (articles, "cat"),
                    (DeviceLookup(articles, label_keys=["cat"], device=None), "cat")):
        with pytest.raises(ValueError, match="needs a DeviceLookup that holds"):
            recommend(model, loader, ids, top_n=5, rerank=Calibrated(lk, key, pool=10))
    wide = DeviceLookup({a: {"cat": list(range(200))} for a in ids}, label_keys=["cat"])
    with pytest.raises(ValueError, match="1 to 128 labels, 'cat' has 200"):
        recommend(model, loader, ids, top_n=5, rerank=Calibrated(wide, "cat", pool=10))
    none = DeviceLookup({a: {"cat": None} for a in ids}, label_keys=["cat"])
    with pytest.raises(ValueError, match="1 to 128 labels, 'cat' has 0"):
        recommend(model, loader, ids, top_n=5, rerank=Calibrated(none, "cat", pool=10))
    for target, msg in (("editorial", "target must be 'history'"), ({"a": 1, "zz": 1}, "outside the lookup's vocabulary"),
                        (np.ones(4), r"\[C\] or \[n, C\] with C = 3"), (np.ones((2, 3)), "ONE distribution"), ([1, -1, 0], "not negative")):
        with pytest.raises(ValueError, match=msg):
            recommend(model, loader, ids, top_n=5, rerank=Calibrated(lookup, "cat", pool=10, target=target))
    for weights in ([1.0, float("nan")], [[1.0, 1.0]], [], np.ones(257)):
        with pytest.raises(ValueError, match="history_weights must be"):
            recommend(model, loader, ids, top_n=5, rerank=Calibrated(lookup, "cat", pool=10, history_weights=weights))
    with pytest.raises(ValueError, match="rerank must be None or an MMR"):
        recommend(model, loader, ids, top_n=5, rerank="calibrated")
    with pytest.raises(ValueError, match="top_n must lie in"):  # the plain checks come first
        recommend(model, loader, ids, top_n=65, rerank=Calibrated(lookup, "cat"))


# ------------------------------------------------------------------------------------------------ host side of the entry points
DEV = ctypes.c_void_p(0x7E0000000000)


def test_calibrated_rerank_argument_checks_need_no_device():
    """Every limit is checked before anything is dereferenced or launched (the pointers here are made-up device addresses)."""
    from ebrec import _hip

    lib = _hip.lib()
    call = lambda **kw: lib.ebn_calibrated_rerank_f32(*{**dict(W=DEV, n_rows=1000, C=64, rows=DEV, rel=DEV, P=64, target=DEV, stride=64,
                                                               k=10, lam=0.7, alpha=0.01, sel=DEV, obj=None, flags=DEV, U=100,
                                                               stream=None), **kw}.values())
    assert call(P=65) == -2 and call(P=0) == -2 and call(k=65) == -2 and call(k=0) == -2
    assert call(C=129, stride=129) == -2 and call(C=0, stride=0) == -2 and call(C=-4, stride=0) == -2
    assert call(lam=1.5) == -1 and call(lam=-0.25) == -1 and call(lam=float("nan")) == -1
    assert call(alpha=0.0) == -1 and call(alpha=1.0) == -1 and call(alpha=-0.5) == -1 and call(alpha=float("nan")) == -1
    assert call(stride=63) == -1 and call(stride=128) == -1 and call(stride=-64) == -1 and call(stride=1 << 40) == -1
    assert call(rows=None) == -1 and call(rel=None) == -1 and call(sel=None) == -1 and call(flags=None) == -1
    assert call(W=None) == -1 and call(target=None) == -1
    assert call(U=-1) == -1 and call(U=1 << 31) == -1 and call(U=1 << 62) == -1 and call(n_rows=-1) == -1 and call(n_rows=1 << 40) == -1
    assert call(U=0, W=None, rows=None, sel=None, target=None) == 0  # nothing to do
    assert call(U=0, stride=0) == 0 and call(U=0, C=128, stride=128, P=1, k=64) == 0 and call(U=0, P=65) == -2


def test_label_target_argument_checks_need_no_device():
    from ebrec import _hip

    lib = _hip.lib()
    call = lambda **kw: lib.ebn_label_target_f32(*{**dict(W=DEV, n_rows=1000, C=64, hist=DEV, H=20, w=None, target=DEV, flags=DEV, U=100,
                                                          stream=None), **kw}.values())
    assert call(C=129) == -2 and call(C=0) == -2 and call(H=257) == -2 and call(H=0) == -2 and call(H=-1) == -2
    assert call(hist=None) == -1 and call(target=None) == -1 and call(flags=None) == -1 and call(W=None) == -1
    assert call(U=-1) == -1 and call(U=1 << 31) == -1 and call(U=1 << 62) == -1 and call(n_rows=-1) == -1 and call(n_rows=1 << 40) == -1
    assert call(U=0, W=None, hist=None, target=None) == 0 and call(U=0, C=128, H=256, w=DEV) == 0 and call(U=0, H=257) == -2


def test_the_header_declares_both_entry_points_with_their_limits():
    from ebrec import _hip

    decl = _hip.declared_functions()
    i32, i64, ptr, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    assert decl["ebn_label_target_f32"] == (i32, [ptr, i64, i32, ptr, i32, ptr, ptr, ptr, i64, ptr])
    assert decl["ebn_calibrated_rerank_f32"] == (i32, [ptr, i64, i32, ptr, ptr, i32, ptr, i64, i32, f32, f32, ptr, ptr, ptr, i64, ptr])
    text = re.sub(r"\s+\*?\s*", " ", _hip.header_path().read_text())
    for phrase in ("1 <= C <= 128", "1 <= H <= 256", "32 KiB of the CU's 160 KiB", "target_stride not in {0, C}", "A failing call writes nothing"):
        assert phrase in text, phrase
