"""Host side of ebn_npa_target_rank_f32 / NPAModel.rank_targets_pairwise: the declared entry points, the workspace query, every
argument code of the entry point with made-up device addresses, and what rank_targets_pairwise refuses before the device works.
No GPU."""
import ctypes
import inspect
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from tests import npa_target_rank_cases as nt


# ------------------------------------------------------------------------------------------------ the cases
def test_the_case_module_is_the_existing_generators():
    c = nt.case(nt.SHAPES[2], seed=5, cand="subset", exclude="x3")
    U, M, L, F, A = nt.SHAPES[2]
    assert c["users"].shape == (U, F) and c["Q"].shape == (U, A) and c["Ua"].shape == (M + 5, L, A) and c["Vd"].shape == (M + 5, L, F)
    assert c["cand_rows"].shape == (M,) and c["exclude"].shape == (U, 3) and "k" not in c
    s64 = nt.scores64(c)
    adm = nt.admissible(c)
    window = nt.windows("random", U, M, seed=1)
    target = nt.targets(U, M, 3, window, c["cand_rows"], c["n_rows"], c["exclude"])
    rank, count, flags = nt.rank_reference(s64, target, window, c["cand_rows"], c["n_rows"], c["exclude"])
    adm_w = nt.admissible(c, window)
    assert np.array_equal(count, adm_w.sum(1)) and (adm_w <= adm).all()
    b = nt.band(s64, adm_w, target, 0.0)  # tol 0: the band is the float64 rank, up to float64 ties
    ranked = rank > 0
    assert ranked.any() and (~ranked).any() and ((b[:, 0] == 0) == ~ranked).all()
    assert (b[ranked, 0] <= rank[ranked]).all() and (rank[ranked] <= b[ranked, 1]).all()


# ------------------------------------------------------------------------------------------------ the entry points
def test_both_symbols_are_declared_with_their_arguments():
    from ebrec import _hip

    decl = _hip.declared_functions()
    res, argt = decl["ebn_npa_target_rank_workspace_bytes"]
    assert res is ctypes.c_int64 and argt == [ctypes.c_int64, ctypes.c_int32]
    res, argt = decl["ebn_npa_target_rank_f32"]
    assert res is ctypes.c_int and len(argt) == 24
    i64 = [i for i, t in enumerate(argt) if t is ctypes.c_int64]
    assert i64 == [4, 6, 18, 19]  # n_rows, M, workspace_bytes, U
    assert argt[-4:] == [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    lib = _hip.lib()
    assert hasattr(lib, "ebn_npa_target_rank_f32") and hasattr(lib, "ebn_npa_target_rank_workspace_bytes")
    text = _hip.header_path().read_text()
    block = text[text.index("rank of one target candidate per user for NPA"):text.index("int64_t ebn_npa_target_rank_workspace_bytes")]
    assert "ebn_npa_topk_score_f32" in block and "ebn_target_rank_f32" in block and "bit for bit" in block


def test_the_workspace_query_is_never_negative():
    from ebrec import _hip

    q = _hip.lib().ebn_npa_target_rank_workspace_bytes
    sizes = [-1, 0, 1, 2, 127, 128, 129, 200000, (1 << 31) - 1, 1 << 31, 1 << 40, (1 << 62) + 3]
    for U in sizes:
        for s in (-1, 0, 1, 2, 3, 64, 65, (1 << 31) - 1):
            got = q(U, s)
            assert got >= 0, (U, s)
            if U < 0 or U > (1 << 31) - 1 or s < 1:
                assert got == 0, (U, s)
            elif U > 0:
                assert got >= (2 * min(s, 64) + 1) * U * 4, (U, s)
    # one range needs the target scores and its counts too: [U] floats, [2, s, U] int32
    assert q(1000, 1) == (2 * 1000 + 1000) * 4 + 16 and q(0, 7) == 16
    assert q(1000, 3) == (2 * 3 * 1000 + 1000) * 4 + 16 and q(1000, 200) == q(1000, 64)


def test_entry_point_argument_checks_need_no_device():
    """every limit and code is checked before anything is dereferenced or launched (the pointers are made-up device addresses)"""
    from ebrec import _hip

    lib = _hip.lib()
    dev = ctypes.c_void_p(0x7E0000000000)
    off = ctypes.c_void_p(0x7E0000000004)
    need1 = lib.ebn_npa_target_rank_workspace_bytes(64, 1)
    base = dict(users=dev, Q=dev, Ua=dev, Vd=dev, n_rows=500, cand=None, M=500, target=dev, window=dev, ex=None, X=0, mode=1, n_splits=1,
                rank=dev, count=dev, score=dev, flags=dev, ws=dev, ws_bytes=need1, U=64, L=30, F=400, A=200, stream=None)
    call = lambda **kw: lib.ebn_npa_target_rank_f32(*{**base, **kw}.values())
    for bad in (dict(ex=dev, X=257), dict(L=0), dict(L=65), dict(A=6), dict(A=0), dict(A=1028), dict(F=6), dict(F=0), dict(F=4100)):
        assert call(**bad) == -2, bad  # EBN_ERR_UNSUPPORTED
    for bad in (dict(users=off), dict(Q=off), dict(Ua=off), dict(Vd=ctypes.c_void_p(0x7E0000000008)), dict(ws=off)):
        assert call(**bad) == -3, bad  # EBN_ERR_ALIGN
    for bad in (dict(users=None), dict(Q=None), dict(Ua=None), dict(Vd=None), dict(target=None), dict(target=None, M=0, n_rows=0),
                dict(rank=None), dict(count=None), dict(score=None), dict(flags=None), dict(M=499), dict(mode=2), dict(mode=-1), dict(U=-1),
                dict(U=1 << 31), dict(M=-1, cand=dev), dict(n_rows=-1, cand=dev), dict(n_rows=0, cand=dev), dict(L=-1), dict(F=-4),
                dict(A=-4), dict(X=-1), dict(n_splits=-1), dict(ws_bytes=-1)):
        assert call(**bad) == -1, bad  # EBN_ERR_BAD_ARG
    # the workspace: one range needs it as well
    assert call(ws_bytes=need1 - 1) == -1 and call(ws=None) == -1 and call(ws=None, ws_bytes=0) == -1
    need = lib.ebn_npa_target_rank_workspace_bytes(64, 2)
    assert need > need1
    assert call(n_splits=2, ws_bytes=need - 1) == -1 and call(n_splits=2, ws=None, ws_bytes=need) == -1
    assert call(n_splits=2, ws=off, ws_bytes=need) == -3
    # n_splits = 0 stands for ebn_npa_topk_auto_splits(64, 500, 30) ranges, and is sized by it
    auto = lib.ebn_npa_topk_auto_splits(64, 500, 30)
    assert auto > 2 and call(n_splits=0, ws_bytes=lib.ebn_npa_target_rank_workspace_bytes(64, auto) - 1) == -1
    assert call(U=0, users=None, Q=None, rank=None, target=None, window=None, ws=None, ws_bytes=0) == 0  # nothing to do


# ------------------------------------------------------------------------------------------------ the model
class _Loader:
    eval_mode = True
    lookup_article_index = {10: 1, 20: 2, 30: 3}
    lookup_article_matrix = np.zeros((4, 5), np.int64)
    inview_col = "article_ids_inview"
    batch_size = 4
    X = pd.DataFrame({"article_ids_inview": [[10, 20], [20, 30]], "impression_time": [5.0, 6.0]})
    y = [[1, 0], [0, 1]]

    def user_index_eval_batch(self, i):
        raise AssertionError("validation comes first")

    def __len__(self):
        return 1


class _TrainLoader(_Loader):
    eval_mode = False


def test_npa_model_has_rank_targets_pairwise_and_the_hook():
    from ebrec.models.newsrec import NPAModel, _recommend

    assert callable(NPAModel.rank_targets_pairwise) and callable(NPAModel._rank_launch) and callable(_recommend.npa_target_rank)
    assert list(inspect.signature(NPAModel.rank_targets_pairwise).parameters)[:4] == ["self", "loader", "targets", "candidate_ids"]
    assert list(inspect.signature(NPAModel._rank_launch).parameters) == ["self", "cache", "users", "cand_rows", "target_pos", "window",
                                                                          "exclude", "sigmoid", "flags"]
    assert list(inspect.signature(_recommend.npa_target_rank).parameters) == ["users", "Q", "Ua_all", "Vd_all", "cand_rows", "target_pos",
                                                                              "window", "exclude", "sigmoid", "flags", "n_splits"]
    doc = NPAModel.rank_targets_pairwise.__doc__
    assert "recommend_pairwise(loader, candidate_ids" in doc and "r - 1" in doc and "do not exist yet" in doc


def test_rank_targets_pairwise_checks_its_arguments_before_the_device_works():
    from ebrec.evaluation.freshness import Freshness
    from ebrec.models.newsrec import NPAModel

    model = object.__new__(NPAModel)
    model._engine = SimpleNamespace(catalogue_bytes=lambda n: 1000 * n, encode_catalogue=lambda tokens: pytest.fail("must not encode"))
    model.catalogue_max_bytes = 1
    fresh = Freshness({10: 1.0, 20: 2.0, 30: 3.0}, max_age=10.0)
    with pytest.raises(ValueError, match="eval-mode loader"):
        model.rank_targets_pairwise(_TrainLoader(), None, [10, 20])
    with pytest.raises(ValueError, match="window must be None or a Freshness"):
        model.rank_targets_pairwise(_Loader(), None, [10, 20], window=(0, 5))
    with pytest.raises(ValueError, match="scores must be 'sigmoid' or 'raw'"):
        model.rank_targets_pairwise(_Loader(), None, [10, 20], scores="logit")
    with pytest.raises(ValueError, match=r"not in the loader's article index: \[-5\]"):
        model.rank_targets_pairwise(_Loader(), None, [10, -5])
    with pytest.raises(ValueError, match="one id or one list of ids per impression: the loader has 2 rows, got 3"):
        model.rank_targets_pairwise(_Loader(), [10, 20, 30], [10, 20])
    with pytest.raises(ValueError, match="candidate ids without a publish time"):
        model.rank_targets_pairwise(_Loader(), None, [10, 20], window=Freshness({10: 1.0}, max_age=10.0))
    # everything on the host passed: the catalogue is what stops these, with and without a window
    with pytest.raises(ValueError, match="catalogue_max_bytes"):
        model.rank_targets_pairwise(_Loader(), None, [10, 20])
    with pytest.raises(ValueError, match="catalogue_max_bytes"):
        model.rank_targets_pairwise(_Loader(), [[10, -7], 30], [10, 20, 30], window=fresh, exclude_history=False, scores="raw")


def test_rank_targets_still_refuses_npa():
    from ebrec.evaluation.freshness import Freshness
    from ebrec.models.newsrec import NPAModel

    model = object.__new__(NPAModel)
    with pytest.raises(NotImplementedError, match="rank_targets is not supported for NPAModel: its scoring launch has no counting form"):
        model.rank_targets(_Loader(), None, [10, 20])
    with pytest.raises(NotImplementedError, match="rank_targets is not supported for NPAModel"):
        model.rank_targets(_Loader(), None, [10, 20], window=Freshness({10: 1.0, 20: 2.0}, max_age=10.0))
    with pytest.raises(NotImplementedError, match="window= is not supported for NPAModel"):
        model.recommend_pairwise(_Loader(), [10, 20], top_n=1, window=Freshness({10: 1.0, 20: 2.0}, max_age=10.0))
