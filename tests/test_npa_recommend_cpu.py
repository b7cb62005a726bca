"""Host side of NPAModel.recommend_pairwise and ebn_npa_topk_score_f32: the float64 restatement against the pool-then-dot order,
the entry points' declarations, every limit and argument check (before anything is dereferenced or launched) and the model's
hooks.  No GPU."""
import ctypes
import re

import numpy as np
import pytest

from tests import npa_recommend_cases as nc


def test_restatement_equals_the_pool_then_dot_form():
    """sum_l w_l (u . Vd_l) = (sum_l w_l Vd_l) . u: the two orders agree to 1e-12 in float64, with cand_rows NULL and as a list with
    duplicates; a row outside the catalogue scores 0."""
    for shape, cand in (((5, 11, 9, 32, 24, 3), "null"), ((4, 13, 33, 8, 4, 3), "subset"), ((1, 1, 1, 4, 4, 1), "null")):
        c = nc.case(shape, seed=3, cand=cand)
        a = nc.pair_scores64(c["users"], c["Q"], c["Ua"], c["Vd"], c["cand_rows"])
        b = nc.pooled_then_dot64(c["users"], c["Q"], c["Ua"], c["Vd"], c["cand_rows"])
        assert a.shape == b.shape == (shape[0], shape[1])
        assert np.abs(a - b).max() <= 1e-12
    assert np.ptp(a) == 0 and abs(a[0, 0]) > 0  # the 1 x 1 case: one token, weight 1, score = u . Vd
    assert np.abs(a[0, 0] - np.float64(c["users"][0]) @ np.float64(c["Vd"][0, 0])) <= 1e-15
    c = nc.case((5, 11, 9, 32, 24, 3), seed=3, cand="subset")
    rows = c["cand_rows"].copy()
    rows[[2, 7]] = [-1, c["n_rows"]]
    s = nc.pair_scores64(c["users"], c["Q"], c["Ua"], c["Vd"], rows)
    keep = np.ones(11, bool)
    keep[[2, 7]] = False
    assert (s[:, ~keep] == 0).all() and np.array_equal(s[:, keep], nc.pair_scores64(c["users"], c["Q"], c["Ua"], c["Vd"], c["cand_rows"])[:, keep])
    assert np.ptp(s) > 1e-2 and (s > 0).any() and (s < 0).any()  # scores of both signs


def test_header_declares_both_entry_points_and_the_library_exports_them():
    from ebrec import _hip

    text = _hip.header_path().read_text()
    decl = _hip.binding.declared_functions()
    assert "ebn_npa_topk_score_f32" in decl and "ebn_npa_topk_auto_splits" in decl
    assert len(decl["ebn_npa_topk_score_f32"][1]) == 22 and len(decl["ebn_npa_topk_auto_splits"][1]) == 3
    assert decl["ebn_npa_topk_score_f32"][1][-5:] == [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    lib = _hip.lib()
    assert hasattr(lib, "ebn_npa_topk_score_f32") and hasattr(lib, "ebn_npa_topk_auto_splits")
    # the contract names what it is not bit-equal to, and whose workspace query it shares
    block = text[text.index("top-N recommendation for NPA"):text.index("int ebn_npa_topk_score_f32")]
    assert re.search(r"NOT bit-equal to ebn_pap_indexed_f32", block) and "ebn_topk_workspace_bytes" in block


def test_npa_topk_host_queries_and_argument_checks_need_no_device():
    """The planner is a pure host query, and every limit is checked before anything is dereferenced or launched (the pointers
    here are made-up device addresses)."""
    from ebrec import _hip

    lib = _hip.lib()
    auto = lib.ebn_npa_topk_auto_splits
    assert auto(200000, 250, 30) == 1  # 1563 user tiles fill the chip on their own
    assert auto(100, 20000, 30) == 64 and auto(100, 3, 30) == 1  # capped at 64; one step of four candidates
    assert auto(100, 8, 32) == 2 and auto(100, 8, 33) == 4  # two candidates a step once L spills into the second tile
    assert auto(0, 0, 30) == 1 and auto(-3, 1 << 40, 30) == 1 and auto(100, 100, 0) == 1 and auto(100, 100, 65) == 1
    dev = ctypes.c_void_p(0x7E0000000000)
    off = ctypes.c_void_p(0x7E0000000004)
    base = dict(users=dev, Q=dev, Ua=dev, Vd=dev, n_rows=500, cand=None, M=500, ex=None, X=0, k=10, mode=1, n_splits=1, pos=dev,
                score=dev, flags=dev, ws=None, ws_bytes=0, U=64, L=30, F=400, A=200, stream=None)
    call = lambda **kw: lib.ebn_npa_topk_score_f32(*{**base, **kw}.values())
    for bad in (dict(k=65), dict(k=0), dict(ex=dev, X=257), dict(L=0), dict(L=65), dict(A=6), dict(A=0), dict(A=1028), dict(F=6),
                dict(F=0), dict(F=4100)):
        assert call(**bad) == -2, bad  # EBN_ERR_UNSUPPORTED
    for bad in (dict(users=off), dict(Q=off), dict(Ua=off), dict(Vd=ctypes.c_void_p(0x7E0000000008))):
        assert call(**bad) == -3, bad  # EBN_ERR_ALIGN
    for bad in (dict(users=None), dict(Q=None), dict(Ua=None), dict(Vd=None), dict(pos=None), dict(score=None), dict(flags=None),
                dict(M=499), dict(mode=2), dict(mode=-1), dict(U=-1), dict(U=1 << 31), dict(M=-1, cand=dev), dict(n_rows=-1, cand=dev),
                dict(n_rows=0, cand=dev), dict(L=-1), dict(F=-4), dict(A=-4), dict(X=-1), dict(n_splits=-1), dict(ws_bytes=-1)):
        assert call(**bad) == -1, bad  # EBN_ERR_BAD_ARG
    need = lib.ebn_topk_workspace_bytes(64, 10, 2)  # the partial-list layout is ebn_topk_score_f32's
    assert need >= 2 * 64 * 10 * 8
    assert call(n_splits=2, ws=dev, ws_bytes=need - 1) == -1 and call(n_splits=2, ws=None, ws_bytes=need) == -1
    assert call(n_splits=2, ws=off, ws_bytes=need) == -3
    assert call(U=0, users=None, Q=None, pos=None) == 0  # nothing to do


def test_npa_model_has_recommend_pairwise_and_the_hooks():
    import inspect

    from ebrec.models.newsrec import NPAModel
    from ebrec.models.newsrec import _recommend

    for name in ("recommend_pairwise", "_recommend_index", "_recommend_cache", "_user_vectors_cached", "_recommend_topk"):
        assert callable(getattr(NPAModel, name)), name
    assert NPAModel._recommend_loader_method == "user_index_eval_batch"
    assert list(inspect.signature(NPAModel.recommend_pairwise).parameters)[:3] == ["self", "loader", "candidate_ids"]
    assert inspect.signature(NPAModel.recommend_pairwise).parameters["candidate_ids"].default is None
    # recommend() itself stays as it was, and points at the new method
    doc = NPAModel.recommend.__doc__
    assert "36 kFLOP" in doc and "recommend_pairwise" in doc
    assert callable(_recommend.npa_topk)
    # the engine's user stage is one function that score_cached calls
    from ebrec.models.newsrec._engine_npa import NPAEngine

    assert callable(NPAEngine.user_state_cached) and "_user_state" in inspect.getsource(NPAEngine.score_cached)


class _Loader:
    eval_mode = True
    lookup_article_index = {10: 1, 20: 2, 30: 3}
    lookup_article_matrix = np.zeros((4, 5), np.int64)

    def user_index_eval_batch(self, i):
        raise AssertionError("validation comes first")

    def __len__(self):
        return 1


def test_recommend_pairwise_validates_like_recommend_and_names_the_budget():
    """The arguments are checked by _recommend.recommend before the device works (the same messages as the other models), and a
    catalogue above catalogue_max_bytes raises a ValueError naming it: ranking has no per-batch fallback."""
    from types import SimpleNamespace

    from ebrec.models.newsrec import NPAModel

    model = object.__new__(NPAModel)
    model._engine = SimpleNamespace(catalogue_bytes=lambda n: 1000 * n, encode_catalogue=lambda tokens: pytest.fail("must not encode"))
    model.catalogue_max_bytes = 1
    with pytest.raises(ValueError, match="top_n must lie in"):
        model.recommend_pairwise(_Loader(), [10, 20], top_n=65)
    with pytest.raises(ValueError, match=r"not in the loader's article index: \[-5\]"):
        model.recommend_pairwise(_Loader(), [10, -5], top_n=1)
    with pytest.raises(ValueError, match="larger than the number of candidates"):
        model.recommend_pairwise(_Loader(), [10, 20], top_n=3)
    with pytest.raises(ValueError, match="'sigmoid' or 'raw'"):
        model.recommend_pairwise(_Loader(), [10, 20], top_n=1, scores="softmax")
    with pytest.raises(ValueError, match="catalogue_max_bytes"):
        model.recommend_pairwise(_Loader(), [10, 20], top_n=1)
