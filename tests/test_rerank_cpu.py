"""Host side of MMR re-ranking: the float64 restatement on hand-computed answers, the product's host path against it, argument
validation of mmr_rerank(), recommend(rerank=...) and ebn_mmr_rerank_f32.  No GPU: nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest

from ebrec.evaluation import MMR, mmr_rerank
from ebrec.evaluation.beyond_accuracy import DeviceLookup
from ebrec.models.newsrec._recommend import recommend
from tests import rerank_cases as rr
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)
from tests.test_recommend_cpu import _HostOnlyModel, _loader

E = np.eye(4)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_a_hand_computed_three_item_pool():
    unit = np.stack([E[0], E[1]])                 # row 0 and row 1 are orthogonal: d = 1; an entry and its duplicate: d = 0
    rows, rel = np.array([[0, 0, 1]]), np.array([[1.0, 0.875, 0.5]])
    # lam = 1/2: after entry 0, the duplicate scores 0.4375 + 0, the other 0.25 + 0.5; then the duplicate is all that is left
    sel, obj, flags = rr.mmr_reference(unit, rows, rel, 3, 0.5)
    assert sel.tolist() == [[0, 2, 1]] and obj.tolist() == [[1.0, 0.75, 0.4375]] and flags == (0, 0)
    # lam = 3/4: 0.65625 against 0.375 + 0.25 -- relevance wins
    sel, obj, _ = rr.mmr_reference(unit, rows, rel, 3, 0.75)
    assert sel.tolist() == [[0, 1, 2]] and obj.tolist() == [[1.0, 0.65625, 0.625]]
    # lam = 0: distances alone after the first pick; k > P pads with (-1, -inf)
    sel, obj, _ = rr.mmr_reference(unit, rows, rel, 5, 0.0)
    assert sel.tolist() == [[0, 2, 1, -1, -1]] and obj[0, :3].tolist() == [1.0, 1.0, 0.0] and np.isneginf(obj[0, 3:]).all()


def test_restatement_ties_absence_and_flags():
    unit = np.stack([E[0], E[1]])
    # entries 1 and 2 are the same article with the same relevance: equal objectives go to the smaller pool index
    sel, obj, _ = rr.mmr_reference(unit, np.array([[0, 1, 1]]), np.array([[1.0, 0.5, 0.5]]), 3, 0.5)
    assert sel.tolist() == [[0, 1, 2]] and obj.tolist() == [[1.0, 0.75, 0.25]]
    # an unsorted pool; -1 / -inf padding sets nothing; row 2 of a 2-row table and a NaN relevance are absent and flagged
    rows = np.array([[-1, 1, 0, 2, 0], [-1, -1, -1, -1, -1]])
    rel = np.array([[-np.inf, 0.25, 0.5, 9.0, np.nan], [-np.inf] * 5])
    sel, obj, flags = rr.mmr_reference(unit, rows, rel, 3, 0.5)
    assert sel.tolist() == [[2, 1, -1], [-1, -1, -1]] and flags == (1, 1)
    assert obj[0, :2].tolist() == [0.5, 0.625] and np.isneginf(obj[1]).all()
    assert rr.mmr_reference(unit, rows[:, :3], rel[:, :3], 3, 0.5)[2] == (0, 0)
    sel, _, flags = rr.mmr_reference(unit, np.array([[0, 1]]), np.array([[np.inf, 1.0]]), 2, 0.5)
    assert sel.tolist() == [[1, -1]] and flags == (0, 1)
    # a NaN dot product between present entries is distance 0 and flag 1
    bad = np.stack([E[0], E[1] * np.nan])
    sel, obj, flags = rr.mmr_reference(bad, np.array([[0, 1]]), np.array([[1.0, 0.5]]), 2, 0.5)
    assert sel.tolist() == [[0, 1]] and obj.tolist() == [[1.0, 0.25]] and flags == (0, 1)


@pytest.mark.parametrize("shape", rr.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_cases_are_exact_in_float32_and_lam_one_is_the_relevance_order(shape):
    U, P, D, k = shape
    unit, rows, rel = rr.exact_case(U, P, D, seed=U + P)
    rng = np.random.default_rng(0)
    order = rng.permutation(D)
    dots = unit.astype(np.float64) @ unit.astype(np.float64).T
    acc = np.zeros((len(unit), len(unit)), np.float32)
    for j in order:  # an fp32 sum in another order, one rounding per product and per add
        acc = (acc + np.outer(unit[:, j], unit[:, j]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(acc.astype(np.float64), dots) and np.array_equal(dots, np.round(dots * 16) / 16)
    if D >= 36:
        assert (dots > 1).any() and (dots < -1).any() and ((dots > -1) & (dots < 1)).any()  # clipped on both sides, and not
    sel, obj, flags = rr.mmr_reference(unit, rows, rel, k, 1.0)
    assert flags == (0, 0)
    for u in range(U):
        present = np.flatnonzero(rr.present_mask(rows[u], rel[u], len(unit)))
        want = present[np.argsort(-rel[u, present].astype(np.float64), kind="stable")][:k]
        assert sel[u, :len(want)].tolist() == want.tolist() and (sel[u, len(want):] == -1).all()
    if U > 1:
        assert (sel[1] == -1).all()
    for lam in (0.25, 0.5):
        _, obj, _ = rr.mmr_reference(unit, rows, rel, k, lam)
        fin = np.isfinite(obj)
        assert np.array_equal(obj[fin], obj[fin].astype(np.float32).astype(np.float64)) and np.array_equal(obj[fin] * 256, np.round(obj[fin] * 256))


# ------------------------------------------------------------------------------------------------ the product's host path
def _lookup_case(shape, seed):
    """the pools of an exact case over a table of dyadic unit rows, as ids: article 100 + row, -1 for a row of -1"""
    U, P, D, k = shape
    _, rows, rel = rr.exact_case(U, P, D, seed)
    table = rr.exact_unit_table(max(3, (3 * P) // 4), D, np.random.default_rng(seed))
    lookup = {100 + r: {"emb": table[r], "pop": 0.5} for r in range(len(table))}
    ids = np.where(rows >= 0, rows + 100, -1)
    return table, lookup, rows, ids, rel


@pytest.mark.parametrize("lam", rr.EXACT_LAMS)
@pytest.mark.parametrize("shape", rr.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_path_equals_the_restatement_on_the_exact_cases(shape, lam):
    k = shape[3]
    table, lookup, rows, ids, rel = _lookup_case(shape, seed=sum(shape))
    assert np.array_equal((table.astype(np.float64) ** 2).sum(1), np.ones(len(table)))
    want_sel, _, _ = rr.mmr_reference(table, rows, rel, k, lam)
    want_ids = np.where(want_sel >= 0, np.take_along_axis(ids, np.maximum(want_sel, 0).astype(np.int64), 1), -1)
    want_scores = np.where(want_sel >= 0, np.take_along_axis(rel, np.maximum(want_sel, 0).astype(np.int64), 1), -np.inf)
    got_ids, got_scores = mmr_rerank(ids, rel, lookup, "emb", k, lam, return_scores=True)
    assert np.array_equal(got_ids, want_ids) and np.array_equal(got_scores, want_scores) and got_scores.dtype == rel.dtype
    assert np.array_equal(mmr_rerank(ids, rel, DeviceLookup(lookup, ["emb"], device=None), "emb", k, lam), want_ids)


def test_host_path_normalises_the_vectors_and_takes_string_ids():
    lookup = {"a": {"v": [3.0, 0.0]}, "b": {"v": [0.5, 0.0]}, "c": {"v": [0.0, 7.0]}}
    ids, scores = np.array([["a", "b", "c", "zz"]]), np.array([[1.0, 0.9, 0.5, 5.0]])
    got, kept = mmr_rerank(ids, scores, lookup, "v", 3, 0.5, return_scores=True, fill_id="none")
    assert got.tolist() == [["a", "c", "b"]] and kept.tolist() == [[1.0, 0.5, 0.9]]  # selection order: not monotone
    assert mmr_rerank(ids, scores, lookup, "v", 4, 1.0, fill_id="none").tolist() == [["a", "b", "c", "none"]]
    assert mmr_rerank(np.empty((0, 4), "<U2"), np.empty((0, 4)), lookup, "v", 3).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ mmr_rerank(): validation
def test_mmr_rerank_validates_its_arguments():
    lookup = {i: {"emb": E[i % 4], "pop": 0.1} for i in range(8)}
    ids, scores = np.arange(8).reshape(2, 4), np.ones((2, 4))
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"lam must lie in \[0, 1\]"):
            mmr_rerank(ids, scores, lookup, "emb", 2, bad)
    with pytest.raises(ValueError, match="at most 64 entries"):
        mmr_rerank(np.zeros((2, 65), int), np.zeros((2, 65)), lookup, "emb", 2)
    for bad in (65, 0):
        with pytest.raises(ValueError, match="top_n must lie in"):
            mmr_rerank(ids, scores, lookup, "emb", bad)
    with pytest.raises(ValueError, match="not a vector key"):
        mmr_rerank(ids, scores, lookup, "pop", 2)
    with pytest.raises(ValueError, match="not a vector key"):
        mmr_rerank(ids, scores, DeviceLookup(lookup, ["emb"], ["pop"], device=None), "pop", 2)
    with pytest.raises(ValueError, match="not present"):
        mmr_rerank(ids, scores, lookup, "nothing", 2)
    with pytest.raises(ValueError, match="one shape"):
        mmr_rerank(ids, scores[:, :3], lookup, "emb", 2)
    assert mmr_rerank(np.zeros((2, 64), int), np.zeros((2, 64)), lookup, "emb", 64).shape == (2, 64)


# ------------------------------------------------------------------------------------------------ recommend(rerank=...): validation
def test_recommend_validates_rerank_before_the_device_works(frames):  # noqa: F811
    loader, mapping = _loader(frames, True)
    model, ids = _HostOnlyModel(), sorted(mapping)[:12]
    articles = {int(a): {"emb": E[j % 4], "pop": 0.5} for j, a in enumerate(ids)}
    lookup = DeviceLookup(articles, ["emb"], ["pop"])
    with pytest.raises(RuntimeError, match="validation passed"):
        recommend(model, loader, ids, top_n=5, rerank=MMR(lookup, "emb", lam=0.5, pool=10))
    with pytest.raises(RuntimeError, match="validation passed"):
        recommend(model, loader, ids, top_n=5, rerank=MMR(lookup, "emb", pool=64))  # clamped to the 12 candidates
    with pytest.raises(RuntimeError, match="validation passed"):
        recommend(model, loader, ids, top_n=5, rerank=MMR(lookup, "emb", pool=5))
    for pool in (4, 65):
        with pytest.raises(ValueError, match=r"pool must lie in \[top_n, 64\] = \[5, 64\]"):
            recommend(model, loader, ids, top_n=5, rerank=MMR(lookup, "emb", pool=pool))
    for lam in (-0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="lam must lie in"):
            recommend(model, loader, ids, top_n=5, rerank=MMR(lookup, "emb", lam=lam, pool=10))
    few = DeviceLookup({a: articles[a] for a in ids[:9]}, ["emb"])
    with pytest.raises(ValueError, match=rf"without a 'emb' vector in the MMR lookup: \[{ids[9]}, {ids[10]}, {ids[11]}\]"):
        recommend(model, loader, ids, top_n=5, rerank=MMR(few, "emb", pool=10))
    for lk, key in ((lookup, "pop"), (lookup, "nothing"), (articles, "emb"), (DeviceLookup(articles, ["emb"], device=None), "emb")):
        with pytest.raises(ValueError, match="needs a DeviceLookup that holds"):
            recommend(model, loader, ids, top_n=5, rerank=MMR(lk, key, pool=10))
    odd = DeviceLookup({a: {"emb": np.ones(6)} for a in ids}, ["emb"])
    with pytest.raises(ValueError, match="multiple of 4"):
        recommend(model, loader, ids, top_n=5, rerank=MMR(odd, "emb", pool=10))
    with pytest.raises(ValueError, match="rerank must be None or an MMR"):
        recommend(model, loader, ids, top_n=5, rerank="mmr")
    with pytest.raises(ValueError, match="top_n must lie in"):  # the plain checks come first
        recommend(model, loader, ids, top_n=65, rerank=MMR(lookup, "emb"))


# ------------------------------------------------------------------------------------------------ host side of the entry point
def test_rerank_argument_checks_need_no_device():
    """Every limit is checked before anything is dereferenced or launched (the pointers here are made-up device addresses)."""
    from ebrec import _hip

    lib = _hip.lib()
    dev = ctypes.c_void_p(0x7E0000000000)
    call = lambda **kw: lib.ebn_mmr_rerank_f32(*{**dict(unit=dev, n_rows=1000, D=768, rows=dev, rel=dev, P=64, k=10, lam=0.7, sel=dev,
                                                        obj=None, flags=dev, U=100, stream=None), **kw}.values())
    assert call(P=65) == -2 and call(P=0) == -2 and call(k=65) == -2 and call(k=0) == -2
    assert call(D=6) == -2 and call(D=0) == -2 and call(D=8196) == -2
    assert call(lam=1.5) == -1 and call(lam=-0.25) == -1 and call(lam=float("nan")) == -1
    assert call(unit=ctypes.c_void_p(0x7E0000000004)) == -3
    assert call(rows=None) == -1 and call(rel=None) == -1 and call(sel=None) == -1 and call(flags=None) == -1 and call(unit=None) == -1
    assert call(U=-1) == -1 and call(U=1 << 31) == -1 and call(n_rows=-1) == -1 and call(n_rows=1 << 40) == -1 and call(D=-4) == -1
    assert call(U=0, unit=None, rows=None, sel=None) == 0  # nothing to do
    assert call(U=0, D=1024) == 0 and call(U=0, D=768, P=1, k=64) == 0
