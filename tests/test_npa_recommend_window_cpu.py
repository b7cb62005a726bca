"""Host side of ebn_npa_topk_score_window_f32 / NPAModel.recommend_pairwise_windowed: the declared entry point, every argument
code with made-up device addresses, and what recommend_pairwise_windowed refuses before any catalogue is built.  No GPU."""
import ctypes
import inspect
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest


# ------------------------------------------------------------------------------------------------ the entry point
def test_the_header_declares_the_windowed_entry_and_the_library_exports_it():
    from ebrec import _hip

    decl = _hip.declared_functions()
    res, argt = decl["ebn_npa_topk_score_window_f32"]
    plain = decl["ebn_npa_topk_score_f32"][1]
    assert res is ctypes.c_int and len(argt) == 23
    assert argt[:7] == plain[:7] and argt[7] is ctypes.c_void_p and argt[8:] == plain[7:]  # window inserted after M
    assert hasattr(_hip.lib(), "ebn_npa_topk_score_window_f32")
    text = _hip.header_path().read_text()
    block = text[text.index("int ebn_npa_topk_score_f32"):text.index("int ebn_npa_topk_score_window_f32")]
    # the contract is stated by reference to the two entries it combines, with the either-value clause of the flags
    assert "ebn_topk_score_window_f32" in block and "ebn_npa_topk_score_f32" in block and "EITHER value" in block
    assert "window == NULL is EBN_ERR_BAD_ARG" in block and "ebn_topk_workspace_bytes" in block and "ebn_npa_topk_auto_splits" in block


def test_window_entry_point_argument_checks_need_no_device():
    """every limit and code is checked before anything is dereferenced or launched (the pointers are made-up device addresses)"""
    from ebrec import _hip

    lib = _hip.lib()
    dev = ctypes.c_void_p(0x7E0000000000)
    off = ctypes.c_void_p(0x7E0000000004)
    base = dict(users=dev, Q=dev, Ua=dev, Vd=dev, n_rows=500, cand=None, M=500, window=dev, ex=None, X=0, k=10, mode=1, n_splits=1, pos=dev,
                score=dev, flags=dev, ws=None, ws_bytes=0, U=64, L=30, F=400, A=200, stream=None)
    call = lambda **kw: lib.ebn_npa_topk_score_window_f32(*{**base, **kw}.values())
    assert call(window=None) == -1 and call(window=None, M=0, n_rows=0) == -1
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
    assert call(n_splits=2, ws=dev, ws_bytes=need - 1) == -1 and call(n_splits=2, ws=None, ws_bytes=need) == -1
    assert call(n_splits=2, ws=off, ws_bytes=need) == -3
    # n_splits = 0 stands for ebn_npa_topk_auto_splits(64, 500, 30) ranges, and the workspace is sized by it
    auto = lib.ebn_npa_topk_auto_splits(64, 500, 30)
    assert auto > 2 and call(n_splits=0, ws=dev, ws_bytes=lib.ebn_topk_workspace_bytes(64, 10, auto) - 1) == -1
    assert call(U=0, users=None, Q=None, pos=None, window=None) == 0  # nothing to do


# ------------------------------------------------------------------------------------------------ the model
class _Loader:
    eval_mode = True
    lookup_article_index = {10: 1, 20: 2, 30: 3}
    lookup_article_matrix = np.zeros((4, 5), np.int64)
    batch_size = 4
    X = pd.DataFrame({"impression_time": [5.0, 6.0]})

    def user_index_eval_batch(self, i):
        raise AssertionError("validation comes first")

    def __len__(self):
        return 1


class _TrainLoader(_Loader):
    eval_mode = False


class _UntimedLoader(_Loader):
    X = pd.DataFrame({"article_ids_inview": [[10, 20], [20, 30]]})


def test_npa_model_has_recommend_pairwise_windowed_and_the_hooks():
    from ebrec.models.newsrec import NPAModel, _recommend

    assert callable(NPAModel.recommend_pairwise_windowed) and callable(NPAModel._recommend_topk_window)
    sig = inspect.signature(NPAModel.recommend_pairwise_windowed)
    assert list(sig.parameters)[:4] == ["self", "loader", "candidate_ids", "window"]
    assert sig.parameters["window"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["window"].default is inspect.Parameter.empty
    assert list(inspect.signature(NPAModel._recommend_topk_window).parameters) == ["self", "cache", "users", "cand_rows", "window", "exclude",
                                                                                   "k", "sigmoid", "flags"]
    assert list(inspect.signature(_recommend.npa_topk_window).parameters) == ["users", "Q", "Ua_all", "Vd_all", "cand_rows", "window", "exclude",
                                                                              "k", "sigmoid", "flags", "n_splits"]
    assert "model_window_launch" in inspect.signature(_recommend._recommend).parameters
    assert "recommend_pairwise_windowed" in NPAModel.recommend_pairwise.__doc__
    assert "recommend_pairwise_windowed" in NPAModel.rank_targets_pairwise.__doc__


def test_recommend_pairwise_windowed_checks_its_arguments_before_any_catalogue_is_built():
    from ebrec.evaluation.freshness import Freshness
    from ebrec.models.newsrec import NPAModel

    model = object.__new__(NPAModel)
    model._engine = SimpleNamespace(catalogue_bytes=lambda n: 1000 * n, encode_catalogue=lambda tokens: pytest.fail("must not encode"))
    model.catalogue_max_bytes = 1
    fresh = Freshness({10: 1.0, 20: 2.0, 30: 3.0}, max_age=10.0)
    with pytest.raises(ValueError, match="recommend_pairwise_windowed needs window=.*recommend_pairwise"):
        model.recommend_pairwise_windowed(_Loader(), [10, 20], window=None, top_n=1)
    with pytest.raises(TypeError, match="window"):
        model.recommend_pairwise_windowed(_Loader(), [10, 20], top_n=1)
    with pytest.raises(ValueError, match=r"window must be None or a Freshness\(published, max_age, min_age\), got tuple"):
        model.recommend_pairwise_windowed(_Loader(), [10, 20], window=(0, 5), top_n=1)
    with pytest.raises(ValueError, match="eval-mode loader"):
        model.recommend_pairwise_windowed(_TrainLoader(), [10, 20], window=fresh, top_n=1)
    with pytest.raises(ValueError, match="lacks the column 'impression_time'"):
        model.recommend_pairwise_windowed(_UntimedLoader(), [10, 20], window=fresh, top_n=1)
    with pytest.raises(ValueError, match=r"candidate ids without a publish time: \[20\]"):
        model.recommend_pairwise_windowed(_Loader(), [10, 20], window=Freshness({10: 1.0}, max_age=10.0), top_n=1)
    with pytest.raises(ValueError, match="larger than the number of candidates"):
        model.recommend_pairwise_windowed(_Loader(), [10, 20], window=fresh, top_n=3)
    with pytest.raises(ValueError, match="rerank must be None or"):
        model.recommend_pairwise_windowed(_Loader(), [10, 20], window=fresh, top_n=1, rerank="mmr")
    # everything on the host passed: the catalogue is what stops this one
    with pytest.raises(ValueError, match="catalogue_max_bytes"):
        model.recommend_pairwise_windowed(_Loader(), [10, 20, 30], window=fresh, top_n=2, exclude_history=False, scores="raw")


def test_recommend_pairwise_with_a_window_still_raises_its_pinned_message():
    from ebrec.evaluation.freshness import Freshness
    from ebrec.models.newsrec import NPAModel

    model = object.__new__(NPAModel)
    with pytest.raises(NotImplementedError, match="window= is not supported for NPAModel: its scoring launch has no windowed form"):
        model.recommend_pairwise(_Loader(), [10, 20], top_n=1, window=Freshness({10: 1.0, 20: 2.0}, max_age=10.0))
    with pytest.raises(NotImplementedError, match="NPA's news vector depends on the user"):
        model.recommend(_Loader(), [10, 20], top_n=1)
