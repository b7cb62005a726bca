"""Host side of ebn_target_rank_f32 / model.rank_targets(): the float64 restatement pinned against the accepted restatements of
the top-N lists, the declared entry points and their argument checks, rank_metrics, and what rank_targets() refuses before the
device works.  No GPU."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_IMPRESSION_TIMESTAMP_COL
from tests import recommend_cases as rc
from tests import recommend_window_cases as wc
from tests import target_rank_cases as tc
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)
from tests.test_recommend_window_cpu import _HostOnlyModel


# ------------------------------------------------------------------------------------------------ the restatement
def _agrees_with_the_lists(rank, count, target, lists):
    """lists: {k: pos [U, k]}.  rank r <= k iff the list has the target at index r - 1; min(count, k) slots are filled"""
    for k, pos in lists.items():
        assert np.array_equal((pos >= 0).sum(1), np.minimum(count, k)), k
        for u in range(len(rank)):
            r, tp = int(rank[u]), int(target[u])
            if 1 <= r <= k:
                assert pos[u, r - 1] == tp, (k, u)
            else:
                assert tp < 0 or tp not in pos[u].tolist(), (k, u)


@pytest.mark.parametrize("cand,exclude", [("null", None), ("subset", "x3"), ("null", "all")])
@pytest.mark.parametrize("pattern", [None] + wc.PATTERNS)
def test_the_restatement_agrees_with_the_restatements_of_the_lists(pattern, cand, exclude):
    U, M, F = 37, 90, 8  # M above 64: the longest list does not hold everybody
    users, news, cand_rows, ex = rc.integer_case(U, M, F, seed=5, cand=cand, exclude=exclude)
    n_rows = news.shape[0]
    if cand_rows is not None:
        cand_rows = tc.with_bad_rows(cand_rows, n_rows)
    s64 = rc.scores64(users, news, cand_rows)
    s64[3, 17] = np.nan
    window = None if pattern is None else wc.windows(pattern, U, M, seed=2)
    target = tc.targets(U, M, 1, window, cand_rows, n_rows, ex)
    target[3] = 17  # the NaN pair
    rank, count, flags = tc.rank_reference(s64, target, window, cand_rows, n_rows, ex)
    lists = {}
    for k in range(1, 65):
        if window is None:
            pos, _s, want_flags = rc.topk_reference(s64, k, cand_rows, n_rows, ex)
        else:
            pos, _s, want_flags = wc.window_reference(s64, k, window, cand_rows, n_rows, ex)
        lists[k] = pos
    _agrees_with_the_lists(rank, count, target, lists)
    assert rank[3] == 0
    assert (rank[(target < 0) | (target >= M)] == 0).all() and (rank <= count).all()
    # the lists' flags, plus flags[0] for the targets past the end (this target mix has some)
    assert (target >= M).any() and flags == (1, want_flags[1])
    in_list = target.clip(0, M - 1)
    assert tc.rank_reference(s64, np.where(target >= M, -1, in_list), window, cand_rows, n_rows, ex)[2] == want_flags


def test_the_restatement_on_a_hand_written_case():
    scores = np.array([[1.0, 3.0, 3.0, 2.0, 3.0, np.nan]] * 6)
    target = [2, 3, 0, 5, -1, 6]
    rank, count, flags = tc.rank_reference(scores, target)
    assert rank.tolist() == [2, 4, 5, 0, 0, 0] and count.tolist() == [5] * 6 and flags == (1, 1)
    rank, count, flags = tc.rank_reference(scores, [2, 3, 0, 4, 1, 4], window=[[0, 6], [2, 5], [3, 3], [4, 2], [-7, 2], [0, 5]])
    assert rank.tolist() == [2, 3, 0, 0, 1, 3] and count.tolist() == [5, 3, 0, 0, 2, 5] and flags == (0, 1)
    # exclusion is by ROW: both positions of row 1 leave, and a target on one of them has no rank
    rank, count, flags = tc.rank_reference(scores[:2], [4, 1], cand_rows=[0, 1, 1, 3, 4, 9], n_rows=6, exclude=[[1, -1], [1, 7]])
    assert rank.tolist() == [1, 0] and count.tolist() == [3, 3] and flags == (1, 0)


def test_target_kinds_are_what_they_say():
    U, M, F = 130, 1000, 8
    users, news, cand_rows, ex = rc.integer_case(U, M, F, seed=1, cand="subset", exclude="x3")
    n_rows = news.shape[0]
    cand_rows = tc.with_bad_rows(cand_rows, n_rows)
    window = wc.windows("random", U, M, seed=3)
    t = tc.targets(U, M, 0, window, cand_rows, n_rows, ex)
    kind = np.array([tc.KINDS[u % 8] for u in range(U)])
    c = wc.clamp(window, M)
    assert (t[kind == "none"] < 0).all() and (t[kind == "past-the-end"] >= M).all()
    assert np.isin(t[kind == "bad-row"], [1, M // 2]).all()
    outside = (t < c[:, 0]) | (t >= c[:, 1])
    assert outside[kind == "outside-window"].all()
    rows = cand_rows[t.clip(0, M - 1)]
    assert any(rows[u] in ex[u] for u in np.flatnonzero(kind == "excluded"))
    assert all((cand_rows == rows[u]).sum() >= 2 for u in np.flatnonzero(kind == "duplicate"))


# ------------------------------------------------------------------------------------------------ the entry points
def test_both_symbols_are_declared_with_their_arguments():
    from ebrec import _hip

    decl = _hip.declared_functions()
    res, argt = decl["ebn_target_rank_workspace_bytes"]
    assert res is ctypes.c_int64 and argt == [ctypes.c_int64, ctypes.c_int32]
    res, argt = decl["ebn_target_rank_f32"]
    assert res is ctypes.c_int and len(argt) == 20
    assert argt[2] is ctypes.c_int64 and argt[4] is ctypes.c_int64 and argt[16] is ctypes.c_int64 and argt[17] is ctypes.c_int64


def test_the_workspace_query_is_never_negative():
    from ebrec import _hip

    q = _hip.lib().ebn_target_rank_workspace_bytes
    sizes = [-1, 0, 1, 2, 127, 128, 129, 200000, (1 << 31) - 1, 1 << 31, 1 << 40, (1 << 62) + 3]
    for U in sizes:
        for s in (-1, 0, 1, 2, 3, 64, 65, (1 << 31) - 1):
            got = q(U, s)
            assert got >= 0, (U, s)
            if U < 0 or U > (1 << 31) - 1 or s < 1:
                assert got == 0, (U, s)
    assert q(1000, 1) == 16 and q(0, 7) == 16
    assert q(1000, 3) == (2 * 3 * 1000 + 1000) * 4 + 16 and q(1000, 200) == q(1000, 64)


def test_entry_point_argument_checks_need_no_device():
    from ebrec import _hip

    lib = _hip.lib()
    dev = ctypes.c_void_p(0x7E0000000000)
    call = lambda **kw: lib.ebn_target_rank_f32(*{**dict(users=dev, news=dev, n_rows=500, cand=None, M=500, target=dev, window=dev, ex=None,
                                                         X=0, mode=1, n_splits=1, rank=dev, count=dev, score=dev, flags=dev, ws=None,
                                                         ws_bytes=0, U=64, F=400, stream=None), **kw}.values())
    assert call(target=None) == -1 and call(target=None, M=0, n_rows=0) == -1
    assert call(ex=dev, X=257) == -2 and call(F=6) == -2 and call(F=0) == -2 and call(F=8196) == -2
    assert call(users=ctypes.c_void_p(0x7E0000000004)) == -3 and call(news=ctypes.c_void_p(0x7E0000000008)) == -3
    assert call(users=None) == -1 and call(rank=None) == -1 and call(count=None) == -1 and call(score=None) == -1
    assert call(flags=None) == -1 and call(M=499) == -1 and call(mode=2) == -1 and call(X=-1) == -1
    assert call(U=-1) == -1 and call(U=1 << 31) == -1 and call(n_splits=-1) == -1 and call(ws_bytes=-1) == -1
    need = lib.ebn_target_rank_workspace_bytes(64, 2)
    assert call(n_splits=2, ws=dev, ws_bytes=need - 1) == -1 and call(n_splits=2, ws=None, ws_bytes=need) == -1
    assert call(n_splits=2, ws=ctypes.c_void_p(0x7E0000000004), ws_bytes=need) == -3
    assert call(U=0, users=None, rank=None, target=None, window=None) == 0  # nothing to do


# ------------------------------------------------------------------------------------------------ rank_metrics
def test_rank_metrics_known_answers():
    from ebrec.evaluation import rank_metrics

    m = rank_metrics([1, 3, 0, 11], ks=(5, 10), counts=[10, 21, 0, 11])
    assert set(m) == {"hit_rate@5", "hit_rate@10", "ndcg@5", "ndcg@10", "mrr", "unranked", "mean_percentile"}
    assert m["hit_rate@5"] == m["hit_rate@10"] == pytest.approx(2 / 3)
    assert m["ndcg@5"] == m["ndcg@10"] == pytest.approx((1 + 0.5) / 3)  # 1 / log2(2), 1 / log2(4), 0
    assert m["mrr"] == pytest.approx((1 + 1 / 3 + 1 / 11) / 3) and m["unranked"] == 0.25
    assert m["mean_percentile"] == pytest.approx((0 + 2 / 20 + 10 / 10) / 3)
    assert rank_metrics([11], ks=(11, 10)) == {"hit_rate@11": 1.0, "ndcg@11": pytest.approx(1 / np.log2(12)), "hit_rate@10": 0.0,
                                               "ndcg@10": 0.0, "mrr": pytest.approx(1 / 11), "unranked": 0.0}
    assert rank_metrics([1], counts=[1])["mean_percentile"] == 0.0  # a single candidate: max(count - 1, 1)
    for ranks, unranked in (([], np.nan), ([0, 0, 0], 1.0)):
        m = rank_metrics(np.array(ranks, np.int32), ks=(5,), counts=np.zeros(len(ranks), np.int32))
        assert all(np.isnan(m[key]) for key in ("hit_rate@5", "ndcg@5", "mrr", "mean_percentile"))
        assert m["unranked"] == unranked or (np.isnan(unranked) and np.isnan(m["unranked"]))
    with pytest.raises(ValueError, match="negative"):
        rank_metrics([1, -1])
    with pytest.raises(ValueError, match="one entry per rank"):
        rank_metrics([1, 2], counts=[3])


# ------------------------------------------------------------------------------------------------ rank_targets(): validation
def test_rank_targets_checks_its_arguments_before_the_device_works(frames):  # noqa: F811
    from ebrec.evaluation.freshness import Freshness
    from ebrec.models.newsrec import NPAModel
    from ebrec.models.newsrec._recommend import rank_targets
    from ebrec.models.newsrec.dataloader import NRMSDataLoader

    beh, _train, mapping = frames
    beh = beh.iloc[:8].reset_index(drop=True)
    t0 = pd.Timestamp("2023-02-24")
    mk = lambda b, **kw: NRMSDataLoader(behaviors=b, article_dict=mapping, unknown_representation="zeros",
                                        history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=4, **{"eval_mode": True, **kw})
    timed = beh.assign(**{DEFAULT_IMPRESSION_TIMESTAMP_COL: [t0 + pd.Timedelta(hours=h) for h in range(8)]})
    model, ids = _HostOnlyModel(), sorted(mapping)[:12]
    fresh = Freshness({a: t0 - pd.Timedelta(days=30) for a in ids}, max_age=pd.Timedelta(days=2))
    with pytest.raises(RuntimeError, match="validation passed"):
        rank_targets(model, mk(timed), None, ids, window=fresh)
    with pytest.raises(RuntimeError, match="validation passed"):  # targets outside the candidates and the index are no error
        rank_targets(model, mk(beh), [[ids[0], -5], ids[1], [], sorted(mapping)[40], [ids[2]], [ids[2]], 7, 7], ids)
    with pytest.raises(ValueError, match="one id or one list of ids per impression: the loader has 8 rows, got 3"):
        rank_targets(model, mk(beh), [ids[0], ids[1], ids[2]], ids)
    with pytest.raises(ValueError, match="candidate ids not in the loader's article index"):
        rank_targets(model, mk(beh), None, ids + [-5])
    with pytest.raises(ValueError, match="scores must be 'sigmoid' or 'raw'"):
        rank_targets(model, mk(beh), None, ids, scores="logit")
    with pytest.raises(ValueError, match="eval-mode loader"):
        rank_targets(model, mk(frames[1].iloc[:8].reset_index(drop=True), eval_mode=False), None, ids)
    with pytest.raises(ValueError, match="lacks the column 'impression_time'"):
        rank_targets(model, mk(beh), None, ids, window=fresh)
    with pytest.raises(ValueError, match="window must be None or a Freshness"):
        rank_targets(model, mk(timed), None, ids, window=(0, 5))
    # a model with a scoring launch of its own has no counting form: refused before anything else is looked at
    with pytest.raises(NotImplementedError, match="rank_targets is not supported for NPAModel"):
        NPAModel.rank_targets(object.__new__(NPAModel), mk(timed), None, ids)
    with pytest.raises(NotImplementedError, match="rank_targets is not supported for NPAModel"):
        NPAModel.rank_targets(object.__new__(NPAModel), mk(timed), None, ids, window=fresh)


def test_target_pairs_follow_the_labels(frames):  # noqa: F811
    from ebrec.models.newsrec._recommend import _target_pairs
    from ebrec.models.newsrec.dataloader import NRMSDataLoader
    from ebrec.utils._constants import DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_LABELS_COL

    beh, _train, mapping = frames
    beh = beh.iloc[:6].reset_index(drop=True).copy()
    labels = [list(l) for l in beh[DEFAULT_LABELS_COL]]
    labels[2] = [1, 1] + [0] * (len(labels[2]) - 2)  # two clicks
    labels[4] = [0] * len(labels[4])                 # none
    beh[DEFAULT_LABELS_COL] = labels
    loader = NRMSDataLoader(behaviors=beh, article_dict=mapping, unknown_representation="zeros",
                            history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=4, eval_mode=True)
    imp, ids = _target_pairs(loader, None)
    inview = [list(l) for l in beh[DEFAULT_INVIEW_ARTICLES_COL]]
    want = [(r, a) for r in range(6) for a, l in zip(inview[r], labels[r]) if l == 1]
    assert list(zip(imp.tolist(), ids.tolist())) == want and imp.tolist().count(2) == 2 and 4 not in imp.tolist()
    imp, ids = _target_pairs(loader, [5, [6, 7], [], np.array([8]), 9, [10, 10]])
    assert imp.tolist() == [0, 1, 1, 3, 4, 5, 5] and ids.tolist() == [5, 6, 7, 8, 9, 10, 10]
