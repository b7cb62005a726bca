"""Host side of DPP re-ranking: the float64 restatement against the definition (log det), its limits (lam = 1, duplicates, a
rank-deficient pool), the product's host path, argument validation of dpp_rerank() and recommend(rerank=DPP(...)), the header.
No GPU: nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest

from ebrec.evaluation import DPP, IntralistDiversity, dpp_rerank
from ebrec.evaluation.beyond_accuracy import DeviceLookup
from ebrec.models.newsrec._recommend import recommend
from tests import dpp_cases as dc
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)
from tests.test_recommend_cpu import _HostOnlyModel, _loader

E = np.eye(8)


def _unit64(n, D, seed):
    x = np.random.default_rng(seed).standard_normal((n, D))
    return x / np.sqrt((x * x).sum(1, keepdims=True))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("D,lam", [(16, 0.0), (16, 0.5), (6, 0.7)])
def test_restatement_d2_is_the_log_det_gain_of_the_definition(D, lam):
    """log d2_i given the picks Y equals log det S[Y + i] - log det S[Y], for every round and entry with all d2 > 1e-3 so far:
    float64 units, so S itself carries no float32 rounding"""
    P, k = 12, 8
    unit = _unit64(P, D, seed=D)
    rows, rel = np.arange(P)[None, :], np.random.default_rng(1).random((1, P))
    sel = dc.dpp_reference(unit, rows, rel, k, lam)[0][0]
    present = np.ones(P, bool)
    S = dc.similarity(unit, rows[0], present)[0]
    walk = dc.Walk(S, rel[0], lam, k)
    Y, checked, worst = [], 0, 0.0
    for s in sel.tolist():
        base = np.linalg.slogdet(S[np.ix_(Y, Y)])[1] if Y else 0.0
        for i in range(P):
            if i in Y or walk.d2[i] <= 1e-3:
                continue
            sign, logdet = np.linalg.slogdet(S[np.ix_(Y + [i], Y + [i])])
            assert sign == 1.0
            worst = max(worst, abs(np.log(walk.d2[i]) - (logdet - base)))
            checked += 1
        if walk.d2[s] <= 1e-3:
            break
        Y.append(int(s))
        walk.pick(int(s))
    assert checked >= 3 * P and worst <= 1e-9, (checked, worst)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=dc.shape_id)
def test_lam_one_is_the_stable_relevance_order(shape):
    U, P, D, k = shape
    unit, rows, rel = dc.dpp_case(U, P, D, seed=3)
    rel[:, P // 2] = rel[:, 0]  # a tie: the smaller pool index first
    sel, obj, flags = dc.dpp_reference(unit, rows, rel, k, 1.0)
    assert flags == (0, 0)
    for u in range(U):
        present = np.flatnonzero(dc.present_mask(rows[u], rel[u], len(unit)))
        want = present[np.argsort(-rel[u, present].astype(np.float64), kind="stable")][:k]
        assert sel[u, :len(want)].tolist() == want.tolist() and (sel[u, len(want):] == -1).all()
        assert np.array_equal(obj[u, :len(want)], rel[u, want].astype(np.float64)) and np.isneginf(obj[u, len(want):]).all()


def test_duplicates_keep_the_list_full_and_sort_after_every_unspanned_entry():
    unit = E[:4]
    rows = np.array([[0, 0, 1, 2, 3, 1]])
    rel = np.array([[1.0, 0.99, 0.9, 0.8, 0.7, 0.95]])
    # lam = 1/2: entry 0 first; its duplicate (entry 1) and, once entry 5 is in, that one's twin (entry 2) are spanned:
    # 0.5 rel + 0.5 log(EPS) is below every unspanned entry's 0.5 rel + 0.5 log(d2) with d2 >= 1/2; among themselves by relevance
    sel, obj, flags = dc.dpp_reference(unit, rows, rel, 6, 0.5)
    assert sel.tolist() == [[0, 5, 3, 4, 1, 2]] and flags == (0, 0)
    assert np.allclose(obj[0, 4:], 0.5 * rel[0, [1, 2]] + 0.5 * np.log(dc.EPS), rtol=0, atol=1e-12)
    # a degenerate pick updates nothing: the order of the spanned tail is the relevance order whatever was picked before
    lookup = {i: {"v": unit[r]} for i, r in enumerate(rows[0])}
    assert dpp_rerank(np.arange(6)[None, :], rel, lookup, "v", 6, 0.5).tolist() == sel.tolist()


def test_a_rank_deficient_pool_still_gives_full_distinct_lists():
    U, P, D, k = 3, 12, 4, 12
    unit, rows, rel = dc.dpp_case(U, P, D, seed=2)
    for lam in (0.0, 0.5):
        for dtype in (np.float64, np.float32):
            sel = dc.dpp_reference(unit, rows, rel, k, lam, dtype)[0]
            assert all(sorted(sel[u].tolist()) == list(range(P)) for u in range(U)), (lam, dtype)
    assert np.linalg.matrix_rank(dc.similarity(unit, rows[0], np.ones(P, bool))[0], tol=1e-5) <= D + 1


def test_dpp_lists_are_at_least_as_diverse_as_plain_top_k_on_a_three_cluster_pool():
    rng = np.random.default_rng(5)
    centres = E[:3]
    vec = np.concatenate([c + 0.05 * rng.standard_normal((6, 8)) for c in centres])  # 18 items, three tight clusters
    rel = np.concatenate([0.9 + 0.05 * rng.random(6), 0.6 + 0.05 * rng.random(6), 0.3 + 0.05 * rng.random(6)])  # cluster 0 leads
    lookup = {i: {"v": vec[i]} for i in range(18)}
    ids = np.arange(18)[None, :]
    plain = ids[:, np.argsort(-rel, kind="stable")[:5]]
    assert np.array_equal(dpp_rerank(ids, rel[None, :], lookup, "v", 5, lam=1.0), plain)
    got = dpp_rerank(ids, rel[None, :], lookup, "v", 5, lam=0.5)
    div = IntralistDiversity()
    d_plain, d_dpp = div(plain, lookup, "v")[0], div(got, lookup, "v")[0]
    assert d_dpp >= d_plain and d_dpp > 0.3 > d_plain, (d_plain, d_dpp)
    assert {int(i) // 6 for i in got[0]} == {0, 1, 2}  # every cluster is represented


# ------------------------------------------------------------------------------------------------ the product's host path
@pytest.mark.parametrize("lam", [0.3, 0.7, 1.0])
@pytest.mark.parametrize("shape", [(5, 5, 4, 5), (7, 32, 36, 10), (2, 20, 128, 40)], ids=dc.shape_id)
def test_host_path_equals_the_restatement(shape, lam):
    """on float64 unit vectors (so normalising again changes nothing beyond an ulp) and pools whose every round has a margin
    (lam = 0 has none: round 0 is a tie of every entry at log 1, decided by the last bit of each diagonal)"""
    U, P, D, k = shape
    _, rows, rel = dc.dpp_case(U, P, D, seed=4)
    table = _unit64(4 * P, D, seed=4)
    if lam < 1.0:
        assert dc.margin_ok(table, rows, rel, k, lam, factor=10.0)[0]
    want_sel = dc.dpp_reference(table, rows, rel, k, lam)[0]
    lookup = {100 + r: {"emb": table[r], "pop": 0.5} for r in range(len(table))}
    ids = np.where(rows >= 0, rows + 100, -1)
    kept = np.maximum(want_sel, 0).astype(np.int64)
    want_ids = np.where(want_sel >= 0, np.take_along_axis(ids, kept, 1), -1)
    want_scores = np.where(want_sel >= 0, np.take_along_axis(rel, kept, 1), -np.inf)
    got_ids, got_scores = dpp_rerank(ids, rel, lookup, "emb", k, lam, return_scores=True)
    assert np.array_equal(got_ids, want_ids) and np.array_equal(got_scores, want_scores) and got_scores.dtype == rel.dtype
    assert np.array_equal(dpp_rerank(ids, rel, DeviceLookup(lookup, ["emb"], device=None), "emb", k, lam), want_ids)


def test_host_path_padding_fill_id_absent_ids_and_non_finite_scores():
    lookup = {"a": {"v": [3.0, 0.0, 0.0]}, "b": {"v": [0.5, 0.0, 0.0]}, "c": {"v": [0.0, 7.0, 0.0]}, "d": {"v": [0.0, 0.0, 2.0]}}
    ids = np.array([["a", "b", "c", "zz", "d"], ["zz", "yy", "xx", "ww", "vv"]])
    scores = np.array([[1.0, 0.9, 0.5, 5.0, np.nan], [1.0, 1.0, 1.0, 1.0, 1.0]])
    # "zz" is no key and "d" has a NaN score: absent; "b" is "a" again (normalised), so it is spanned and comes last
    got, kept = dpp_rerank(ids, scores, lookup, "v", 4, 0.5, return_scores=True, fill_id="none")
    assert got.tolist() == [["a", "c", "b", "none"], ["none"] * 4]
    assert kept[0, :3].tolist() == [1.0, 0.5, 0.9] and np.isneginf(kept[0, 3]) and np.isneginf(kept[1]).all()  # selection order
    scores[0, 4], scores[0, 0] = np.inf, -np.inf
    assert dpp_rerank(ids, scores, lookup, "v", 4, 1.0, fill_id="none").tolist()[0] == ["b", "c", "none", "none"]
    assert dpp_rerank(np.empty((0, 4), "<U2"), np.empty((0, 4)), lookup, "v", 3).shape == (0, 3)
    out, sc = dpp_rerank(np.empty((2, 0), int), np.empty((2, 0)), lookup, "v", 3, return_scores=True)
    assert out.tolist() == [[-1] * 3] * 2 and np.isneginf(sc).all()
    assert dpp_rerank(np.array([[7, 8]]), np.array([[2, 1]]), {7: {"v": [1.0, 0.0]}, 8: {"v": [0.0, 1.0]}}, "v", 3).tolist() == [[7, 8, -1]]


def test_dpp_rerank_validates_its_arguments():
    lookup = {i: {"emb": E[i % 4], "pop": 0.1} for i in range(8)}
    ids, scores = np.arange(8).reshape(2, 4), np.ones((2, 4))
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"lam must lie in \[0, 1\]"):
            dpp_rerank(ids, scores, lookup, "emb", 2, bad)
    with pytest.raises(ValueError, match="at most 64 entries"):
        dpp_rerank(np.zeros((2, 65), int), np.zeros((2, 65)), lookup, "emb", 2)
    for bad in (65, 0):
        with pytest.raises(ValueError, match="top_n must lie in"):
            dpp_rerank(ids, scores, lookup, "emb", bad)
    with pytest.raises(ValueError, match="not a vector key"):
        dpp_rerank(ids, scores, lookup, "pop", 2)
    with pytest.raises(ValueError, match="not a vector key"):
        dpp_rerank(ids, scores, DeviceLookup(lookup, ["emb"], ["pop"], device=None), "pop", 2)
    with pytest.raises(ValueError, match="not present"):
        dpp_rerank(ids, scores, lookup, "nothing", 2)
    with pytest.raises(ValueError, match="one shape"):
        dpp_rerank(ids, scores[:, :3], lookup, "emb", 2)
    assert dpp_rerank(np.zeros((2, 64), int), np.zeros((2, 64)), lookup, "emb", 64).shape == (2, 64)


# ------------------------------------------------------------------------------------------------ recommend(rerank=DPP(...)): validation
def test_recommend_validates_a_dpp_rerank_before_the_device_works(frames):  # noqa: F811
    loader, mapping = _loader(frames, True)
    model, ids = _HostOnlyModel(), sorted(mapping)[:12]
    articles = {int(a): {"emb": E[j % 4][:4], "pop": 0.5} for j, a in enumerate(ids)}
    lookup = DeviceLookup(articles, ["emb"], ["pop"])
    for pool in (10, 64, 5):  # 64: clamped to the 12 candidates
        with pytest.raises(RuntimeError, match="validation passed"):
            recommend(model, loader, ids, top_n=5, rerank=DPP(lookup, "emb", lam=0.5, pool=pool))
    for pool in (4, 65):
        with pytest.raises(ValueError, match=r"the DPP pool must lie in \[top_n, 64\] = \[5, 64\]"):
            recommend(model, loader, ids, top_n=5, rerank=DPP(lookup, "emb", pool=pool))
    for lam in (-0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="lam must lie in"):
            recommend(model, loader, ids, top_n=5, rerank=DPP(lookup, "emb", lam=lam, pool=10))
    few = DeviceLookup({a: articles[a] for a in ids[:9]}, ["emb"])
    with pytest.raises(ValueError, match=rf"without a 'emb' vector in the DPP lookup: \[{ids[9]}, {ids[10]}, {ids[11]}\]"):
        recommend(model, loader, ids, top_n=5, rerank=DPP(few, "emb", pool=10))
    for lk, key in ((lookup, "pop"), (lookup, "nothing"), (articles, "emb"), (DeviceLookup(articles, ["emb"], device=None), "emb")):
        with pytest.raises(ValueError, match="DPP needs a DeviceLookup that holds"):
            recommend(model, loader, ids, top_n=5, rerank=DPP(lk, key, pool=10))
    odd = DeviceLookup({a: {"emb": np.ones(6)} for a in ids}, ["emb"])
    with pytest.raises(ValueError, match="DPP needs a vector width that is a positive multiple of 4"):
        recommend(model, loader, ids, top_n=5, rerank=DPP(odd, "emb", pool=10))
    with pytest.raises(ValueError, match="rerank must be None or an MMR.*a DPP"):
        recommend(model, loader, ids, top_n=5, rerank="dpp")
    with pytest.raises(ValueError, match="top_n must lie in"):  # the plain checks come first
        recommend(model, loader, ids, top_n=65, rerank=DPP(lookup, "emb"))


# ------------------------------------------------------------------------------------------------ host side of the entry point
def test_the_prototype_parses_with_thirteen_arguments():
    from ebrec import _hip

    ptr, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    decl = _hip.declared_functions()
    assert decl["ebn_dpp_rerank_f32"] == (i32, [ptr, i64, i32, ptr, ptr, i32, i32, f32, ptr, ptr, ptr, i64, ptr])
    assert len(decl["ebn_dpp_rerank_f32"][1]) == 13 and decl["ebn_dpp_rerank_f32"] == decl["ebn_mmr_rerank_f32"]


def test_dpp_argument_checks_need_no_device():
    """Every limit is checked before anything is dereferenced or launched (the pointers here are made-up device addresses)."""
    from ebrec import _hip

    lib = _hip.lib()
    dev = ctypes.c_void_p(0x7E0000000000)
    call = lambda **kw: lib.ebn_dpp_rerank_f32(*{**dict(unit=dev, n_rows=1000, D=768, rows=dev, rel=dev, P=64, k=10, lam=0.7, sel=dev,
                                                        obj=None, flags=dev, U=100, stream=None), **kw}.values())
    assert call(P=65) == -2 and call(P=0) == -2 and call(k=65) == -2 and call(k=0) == -2
    assert call(D=6) == -2 and call(D=0) == -2 and call(D=8196) == -2
    assert call(lam=1.5) == -1 and call(lam=-0.1) == -1 and call(lam=float("nan")) == -1
    assert call(unit=ctypes.c_void_p(0x7E0000000004)) == -3
    assert call(rows=None) == -1 and call(rel=None) == -1 and call(sel=None) == -1 and call(flags=None) == -1 and call(unit=None) == -1
    assert call(U=-1) == -1 and call(U=1 << 31) == -1 and call(n_rows=-1) == -1 and call(n_rows=1 << 40) == -1 and call(D=-4) == -1
    assert call(U=0, unit=None, rows=None, sel=None) == 0  # nothing to do
    assert call(U=0, D=1024) == 0 and call(U=0, D=768, P=1, k=64) == 0
