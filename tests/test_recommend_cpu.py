"""Host side of model.recommend(): the float64 restatement on hand-written answers, argument validation, the id <-> row
mapping.  No GPU: nothing here reaches a model's device hooks."""
import numpy as np
import pytest

from ebrec.models.newsrec._recommend import candidate_rows, recommend
from ebrec.models.newsrec.dataloader import NRMSDataLoader
from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL
from tests import recommend_cases as rc
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_breaks_ties_by_position_and_pads_short_lists():
    scores = np.array([[1.0, 3.0, 3.0, 2.0, 3.0],
                       [5.0, 5.0, 5.0, 5.0, 5.0]])
    pos, out, flags = rc.topk_reference(scores, 3)
    assert pos.tolist() == [[1, 2, 4], [0, 1, 2]] and out.tolist() == [[3.0, 3.0, 3.0], [5.0, 5.0, 5.0]] and flags == (0, 0)
    pos, out, _ = rc.topk_reference(scores[:1], 7)
    assert pos.tolist() == [[1, 2, 4, 3, 0, -1, -1]]
    assert out[0, :5].tolist() == [3.0, 3.0, 3.0, 2.0, 1.0] and np.isneginf(out[0, 5:]).all()


def test_restatement_duplicates_exclusion_rows_outside_the_table_and_nan():
    # positions 0..5 are rows 4, 2, 4, 9 (outside a 6-row table), 0, -1: duplicates of row 4 are two candidates
    cand_rows = np.array([4, 2, 4, 9, 0, -1])
    scores = np.array([[7.0, 1.0, 7.0, 99.0, np.nan, 99.0]])
    pos, out, flags = rc.topk_reference(scores, 4, cand_rows, n_rows=6)
    assert pos.tolist() == [[0, 2, 1, -1]] and flags == (1, 1)
    # excluding row 4 removes BOTH of its positions; -1 and 6 (past the table) in the exclusion list match nothing
    pos, out, flags = rc.topk_reference(scores, 4, cand_rows, n_rows=6, exclude=np.array([[4, -1, 6]]))
    assert pos.tolist() == [[1, -1, -1, -1]] and out[0, 0] == 1.0
    # a NaN on an excluded or out-of-range candidate is still a NaN only where the row is inside the table
    pos, _, flags = rc.topk_reference(np.array([[np.nan, 1.0, 2.0, np.nan, 3.0, 0.0]]), 2, cand_rows, n_rows=6)
    assert pos.tolist() == [[4, 2]] and flags == (1, 1)
    pos, _, flags = rc.topk_reference(np.array([[-np.inf, np.inf, 0.0]]), 3)
    assert pos.tolist() == [[1, 2, 0]] and flags == (0, 0)


def test_integer_cases_are_exact_in_float32_and_exercise_the_tie_rule():
    users, news, cand_rows, ex = rc.integer_case(70, 300, 36, seed=1)
    s64 = rc.scores64(users, news)
    assert np.array_equal(s64, (users @ news.T).astype(np.float64)) and np.abs(s64).max() < 2 ** 24
    assert rc.tie_straddles_boundary(s64, 10).mean() > 0.1  # about one user in five has a tie across the k boundary
    users, news, cand_rows, ex = rc.integer_case(9, 50, 8, seed=2, cand="subset", exclude="all")
    assert len(cand_rows) == 50 and news.shape[0] == 55 and len(np.unique(cand_rows)) < 50  # duplicates
    pos, _, _ = rc.topk_reference(rc.scores64(users, news, cand_rows), 5, cand_rows, 55, ex)
    assert (pos[0] == -1).all() and (pos[1:] >= 0).all()


# ------------------------------------------------------------------------------------------------ id <-> row mapping
def test_candidate_rows_maps_ids_and_drops_row_zero():
    index = {10: 1, 30: 3, 20: 2}  # create_lookup_objects: rows start at 1, row 0 is the unknown article
    ids, rows = candidate_rows(index, None)
    assert ids.tolist() == [10, 20, 30] and rows.tolist() == [1, 2, 3] and rows.dtype == np.int32 and 0 not in rows
    ids, rows = candidate_rows(index, [30, 10, 30])
    assert ids.tolist() == [30, 10, 30] and rows.tolist() == [3, 1, 3]  # order and duplicates are the caller's
    with pytest.raises(ValueError, match=r"\[7, 8, 9, 11, 12\] and 1 more"):
        candidate_rows(index, [10, 7, 8, 9, 7, 11, 12, 13])


# ------------------------------------------------------------------------------------------------ recommend(): validation
class _HostOnlyModel:
    """the hooks of a model, without a device: reaching the cache means the arguments passed validation"""
    _recommend_loader_method = "index_eval_batch"

    def _recommend_index(self, loader):
        return loader.lookup_article_index

    def _recommend_cache(self, loader):
        raise RuntimeError("validation passed")

    def _user_vectors_cached(self, cache, loader, i):
        raise AssertionError


def _loader(frames, eval_mode):  # noqa: F811
    beh, train, mapping = frames
    return NRMSDataLoader(behaviors=(beh if eval_mode else train).iloc[:8].reset_index(drop=True), article_dict=mapping,
                          unknown_representation="zeros", history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=4,
                          eval_mode=eval_mode), mapping


def test_recommend_validates_its_arguments_before_the_device_works(frames):  # noqa: F811
    loader, mapping = _loader(frames, True)
    model, ids = _HostOnlyModel(), sorted(mapping)[:12]
    with pytest.raises(RuntimeError, match="validation passed"):
        recommend(model, loader, ids, top_n=12)
    with pytest.raises(ValueError, match=r"not in the loader's article index: \[-5, -6\]"):
        recommend(model, loader, ids + [-5, -6], top_n=5)
    with pytest.raises(ValueError, match="larger than the number of candidates"):
        recommend(model, loader, ids, top_n=13)
    with pytest.raises(ValueError, match="larger than the number of candidates"):
        recommend(model, loader, None, top_n=64) if len(mapping) < 64 else recommend(model, loader, ids[:3], top_n=4)
    with pytest.raises(ValueError, match="top_n must lie in"):
        recommend(model, loader, ids, top_n=65)
    with pytest.raises(ValueError, match="top_n must lie in"):
        recommend(model, loader, ids, top_n=0)
    with pytest.raises(ValueError, match="'sigmoid' or 'raw'"):
        recommend(model, loader, ids, top_n=5, scores="softmax")
    train_loader, _ = _loader(frames, False)
    with pytest.raises(ValueError, match="eval-mode loader"):
        recommend(model, train_loader, ids, top_n=5)
    model._recommend_loader_method = "user_index_eval_batch"
    with pytest.raises(ValueError, match=r"NRMSDataLoader lacks user_index_eval_batch\(\)"):
        recommend(model, loader, ids, top_n=5)
    with pytest.raises(NotImplementedError, match="no catalogue"):
        recommend(object(), loader, ids, top_n=5)


def test_npa_has_no_catalogue_to_rank_against(frames):  # noqa: F811
    from ebrec.models.newsrec import NPAModel

    loader, mapping = _loader(frames, True)
    with pytest.raises(NotImplementedError, match="depends on the user"):
        NPAModel.recommend(object.__new__(NPAModel), loader, sorted(mapping)[:5])


# ------------------------------------------------------------------------------------------------ host side of the entry points
def test_topk_host_queries_and_argument_checks_need_no_device():
    """The planners are pure host queries, and every limit is checked before anything is dereferenced or launched (the
    pointers here are made-up device addresses)."""
    import ctypes

    from ebrec import _hip

    lib = _hip.lib()
    assert lib.ebn_topk_auto_splits(200000, 20000) == 1  # 1563 user tiles fill the chip on their own
    assert lib.ebn_topk_auto_splits(100, 20000) > 100 // 128 + 1 and lib.ebn_topk_auto_splits(100, 100) == 1  # one candidate tile
    assert lib.ebn_topk_auto_splits(0, 0) == 1 and lib.ebn_topk_auto_splits(-3, 1 << 40) == 1
    assert lib.ebn_topk_workspace_bytes(1000, 10, 4) >= 4 * 1000 * 10 * 8 and lib.ebn_topk_workspace_bytes(1000, 10, 1) > 0
    assert lib.ebn_topk_workspace_bytes(1000, 65, 2) == 0 and lib.ebn_topk_workspace_bytes(1000, 0, 2) == 0
    assert lib.ebn_topk_workspace_bytes(-1, 10, 2) == 0 and lib.ebn_topk_workspace_bytes(1 << 40, 10, 2) == 0
    dev = ctypes.c_void_p(0x7E0000000000)
    call = lambda **kw: lib.ebn_topk_score_f32(*{**dict(users=dev, news=dev, n_rows=500, cand=None, M=500, ex=None, X=0, k=10, mode=1,
                                                        n_splits=1, pos=dev, score=dev, flags=dev, ws=None, ws_bytes=0, U=64, F=400,
                                                        stream=None), **kw}.values())
    assert call(k=65) == -2 and call(k=0) == -2 and call(ex=dev, X=257) == -2 and call(F=6) == -2 and call(F=8196) == -2
    assert call(users=ctypes.c_void_p(0x7E0000000004)) == -3 and call(news=ctypes.c_void_p(0x7E0000000008)) == -3
    assert call(users=None) == -1 and call(pos=None) == -1 and call(flags=None) == -1 and call(M=499) == -1 and call(mode=2) == -1
    assert call(U=-1) == -1 and call(U=1 << 31) == -1 and call(n_splits=-1) == -1
    assert call(n_splits=2, ws=dev, ws_bytes=lib.ebn_topk_workspace_bytes(64, 10, 2) - 1) == -1
    assert call(U=0, users=None, pos=None) == 0  # nothing to do
