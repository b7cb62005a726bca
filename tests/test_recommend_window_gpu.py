"""ebn_topk_score_window_f32 (csrc/ebn_topk.hip, the windowed instantiation) and model.recommend(window=Freshness(...)) on the
GPU, against the float64 restatement of tests/recommend_window_cases.py, against ebn_topk_score_f32 and against the unwindowed
recommend() filtered on the host."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from tests import recommend_window_cases as wc
from tests.hip_testutil import P, S, dev
from tests.test_recommend_gpu import _docvec_case, _nrms_case, run_topk

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3


def _raw_call(hip, users_d, news_d, n_rows, cand_d, M, window_d, ex_d, X, k, mode, n_splits, pos_d, score_d, flags_d, ws_d, ws_bytes, U, F,
              users_ptr=None):
    return hip.lib().ebn_topk_score_window_f32(users_ptr if users_ptr is not None else P(users_d), P(news_d), n_rows, P(cand_d), M,
                                               P(window_d), P(ex_d), X, k, mode, n_splits, P(pos_d), P(score_d), P(flags_d), P(ws_d),
                                               ws_bytes, U, F, S())


def launch_window(hip, users_d, news_d, cand_d, window_d, ex_d, k, mode=0, n_splits=0):
    """one call on device tensors -> (pos [U, k] int32, score [U, k] float32, flags [2]) as numpy arrays"""
    U, F = users_d.shape
    n_rows = news_d.shape[0]
    M = n_rows if cand_d is None else len(cand_d)
    X = 0 if ex_d is None else ex_d.shape[1]
    pos_d = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
    score_d = torch.full((U, k), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    splits = n_splits if n_splits > 0 else int(hip.lib().ebn_topk_auto_splits(U, M))
    ws_bytes = int(hip.lib().ebn_topk_workspace_bytes(U, k, splits))
    assert ws_bytes > 0
    ws_d = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    code = _raw_call(hip, users_d, news_d, n_rows, cand_d, M, window_d, ex_d, X, k, mode, n_splits, pos_d, score_d, flags_d, ws_d, ws_bytes, U, F)
    assert code == OK, code
    torch.cuda.synchronize()
    return pos_d.cpu().numpy(), score_d.cpu().numpy(), flags_d.cpu().numpy()


def run_window(hip, users, news, cand_rows, window, exclude, k, mode=0, n_splits=0):
    return launch_window(hip, dev(users), dev(news), None if cand_rows is None else dev(cand_rows, torch.int32), dev(window, torch.int32),
                         None if exclude is None else dev(exclude, torch.int32), k, mode, n_splits)


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("exclude", [None, "x3"])
@pytest.mark.parametrize("cand", ["null", "subset"])
@pytest.mark.parametrize("pattern", wc.PATTERNS)
@pytest.mark.parametrize("shape", wc.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_cases_equal_the_restatement(hip, shape, pattern, cand, exclude):
    """Integer-valued inputs: fp32 is exact in any order, so positions AND raw scores must equal the float64 restatement; with
    every window open the positions and the score bits are also ebn_topk_score_f32's."""
    U, M, F, k = shape
    users, news, cand_rows, ex = wc.integer_case(U, M, F, seed=U + M, cand=cand, exclude=exclude)
    window = wc.windows(pattern, U, M, seed=U)
    s64 = wc.scores64(users, news, cand_rows)
    want_pos, want_score, want_flags = wc.window_reference(s64, k, window, cand_rows, news.shape[0], ex)
    pos, score, flags = run_window(hip, users, news, cand_rows, window, ex, k)
    assert np.array_equal(pos, want_pos)
    assert np.array_equal(score.astype(np.float64), want_score)
    assert tuple(flags) == want_flags == (0, 0)
    if pattern == "empty":
        assert (pos == -1).all() and np.isneginf(score).all()
    if pattern == "all":
        plain_pos, plain_score, _ = run_topk(hip, users, news, cand_rows, ex, k)
        assert np.array_equal(pos, plain_pos) and np.array_equal(bits(score), bits(plain_score))
        pos1, score1, _ = run_window(hip, users, news, cand_rows, window, ex, k, mode=1)
        plain_pos1, plain_score1, _ = run_topk(hip, users, news, cand_rows, ex, k, mode=1)
        assert np.array_equal(pos1, plain_pos1) and np.array_equal(bits(score1), bits(plain_score1))


# ------------------------------------------------------------------------------------------------ split invariance
def _inside_300_420(U, M):
    rng = np.random.default_rng(8)
    a, b = rng.integers(300, 421, U), rng.integers(300, 421, U)
    return np.stack([np.minimum(a, b), np.maximum(a, b)], 1).astype(np.int32)


SPLIT_CASES = [(shape, "random") for shape in wc.SPLIT_SHAPES] + [((130, 1000, 400, 64), "inside-300-420")]


@pytest.mark.parametrize("shape,which", SPLIT_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_every_split_and_every_run_gives_the_same_bits(hip, shape, which):
    """standard-normal operands: n_splits 1, 2, 7, auto and a second run; "inside-300-420": the union of the windows covers two
    candidate tiles, fewer than there are splits, so some ranges have nothing to visit"""
    U, M, F, k = shape
    rng = np.random.default_rng(5)
    users, news = rng.standard_normal((U, F)).astype(np.float32), rng.standard_normal((M, F)).astype(np.float32)
    ex = rng.integers(-1, M, (U, 4)).astype(np.int32)
    window = wc.windows("random", U, M, seed=6) if which == "random" else _inside_300_420(U, M)
    runs = {s: run_window(hip, users, news, None, window, ex, k, mode=1, n_splits=s) for s in (1, 2, 7, 0)}
    again = run_window(hip, users, news, None, window, ex, k, mode=1, n_splits=7)
    for s, (pos, score, flags) in list(runs.items()) + [("again", again)]:
        assert np.array_equal(pos, runs[1][0]), s
        assert np.array_equal(bits(score), bits(runs[1][1])), s
        assert tuple(flags) == (0, 0)
    pos = runs[1][0]
    c = wc.clamp(window, M)
    for u in range(U):  # every admissible position of a short window, k of a long one, nothing from outside or excluded
        admissible = np.setdiff1d(np.arange(c[u, 0], c[u, 1]), ex[u])
        kept = pos[u][pos[u] >= 0]
        assert len(kept) == min(k, len(admissible)) and np.isin(kept, admissible).all() and len(set(kept.tolist())) == len(kept), u
    # and the kept scores are the bits the plain entry gives the same pairs
    plain_pos, plain_score, _ = run_topk(hip, users, news, None, ex, min(M, 64), mode=1)
    for u in range(U):
        at = {p: s for p, s in zip(plain_pos[u].tolist(), bits(plain_score[u]).tolist())}
        assert all(at[p] == s for p, s in zip(pos[u].tolist(), bits(runs[1][1][u]).tolist()) if p in at), u


# ------------------------------------------------------------------------------------------------ launch company
def test_a_list_does_not_depend_on_the_other_users_of_the_launch(hip):
    """sliding windows over (130, 1000, 400, 64): the users in order (neighbours share tiles), shuffled (a workgroup's union is
    most of the list) and every user alone: the same positions and score bits"""
    U, M, F, k = 130, 1000, 400, 64
    rng = np.random.default_rng(12)
    users, news = rng.standard_normal((U, F)).astype(np.float32), rng.standard_normal((M, F)).astype(np.float32)
    ex = rng.integers(-1, M, (U, 4)).astype(np.int32)
    window = wc.windows("sliding", U, M)
    users_d, news_d, window_d, ex_d = dev(users), dev(news), dev(window, torch.int32), dev(ex, torch.int32)
    pos, score, flags = launch_window(hip, users_d, news_d, None, window_d, ex_d, k)
    assert tuple(flags) == (0, 0) and (pos >= 0).all()  # 250 wide, 4 excluded at most
    assert ((pos >= window[:, :1]) & (pos < window[:, 1:])).all()
    perm = rng.permutation(U)
    pos_s, score_s, _ = run_window(hip, users[perm], news, None, window[perm], ex[perm], k)
    assert np.array_equal(pos_s, pos[perm]) and np.array_equal(bits(score_s), bits(score[perm]))
    for u in range(U):
        pos_1, score_1, _ = launch_window(hip, users_d[u:u + 1], news_d, None, window_d[u:u + 1], ex_d[u:u + 1], k)
        assert np.array_equal(pos_1[0], pos[u]) and np.array_equal(bits(score_1[0]), bits(score[u])), u


# ------------------------------------------------------------------------------------------------ flags
def test_a_nan_counts_only_inside_a_window(hip):
    U, M, F, k = 9, 300, 8, 6
    users, news, _c, _e = wc.integer_case(U, M, F, seed=3)
    news[200] = np.nan
    with np.errstate(invalid="ignore"):
        s64 = wc.scores64(users, news)
    for window, want_flags in ((np.tile([[150, 250]], (U, 1)), (0, 1)),
                               (np.tile([[0, 150]], (U, 1)), (0, 0)),      # the NaN column is in a visited tile, outside every window
                               (np.array([[0, 150]] * (U - 1) + [[200, 201]]), (0, 1))):
        window = window.astype(np.int32)
        want_pos, want_score, flags64 = wc.window_reference(s64, k, window)
        pos, score, flags = run_window(hip, users, news, None, window, None, k)
        assert flags64 == want_flags and tuple(flags) == want_flags
        assert np.array_equal(pos, want_pos) and np.array_equal(score.astype(np.float64), want_score)
        assert not (pos == 200).any()
    assert (pos[-1] == -1).all()  # the user whose window holds the NaN row alone


def test_a_row_outside_the_table_counts_only_inside_a_window(hip):
    U, M, F, k = 9, 300, 8, 6
    users, news, _c, _e = wc.integer_case(U, M, F, seed=2)
    cand_rows = np.arange(M, dtype=np.int32)[::-1].copy()
    cand_rows[[200, 210]] = [M, -1]  # n_rows and -1
    s64 = wc.scores64(users, news, cand_rows)
    for window, want_flags in ((np.tile([[150, 250]], (U, 1)), (1, 0)),
                               (np.array([[0, 10]] * (U - 1) + [[205, 211]]), (1, 0)),
                               (np.tile([[0, 150]], (U, 1)), (0, 0)),      # in a visited tile, outside [min lo, max hi)
                               # in nobody's window but inside [min lo, max hi): the header allows either value
                               (np.array([[0, 150]] * (U - 1) + [[211, 300]]), None)):
        window = window.astype(np.int32)
        want_pos, want_score, flags64 = wc.window_reference(s64, k, window, cand_rows, M)
        pos, score, flags = run_window(hip, users, news, cand_rows, window, None, k)
        if want_flags is not None:
            assert flags64 == want_flags and tuple(flags) == want_flags
        else:
            assert flags64 == (0, 0) and flags[0] in (0, 1) and flags[1] == 0
        assert np.array_equal(pos, want_pos) and np.array_equal(score.astype(np.float64), want_score)
        assert not np.isin(pos, [200, 210]).any()


# ------------------------------------------------------------------------------------------------ errors
def test_failing_calls_return_their_code_and_write_nothing(hip):
    U, M, F, k = 5, 300, 8, 4
    users, news, _c, _e = wc.integer_case(U, M, F, seed=4)
    users_d, news_d = dev(users), dev(news)
    window_d = dev(wc.windows("all", U, M), torch.int32)
    ws_d = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    pos_d = torch.full((U, 65), -7, dtype=torch.int32, device="cuda")
    score_d = torch.full((U, 65), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    call = lambda **kw: _raw_call(hip, **{**dict(users_d=users_d, news_d=news_d, n_rows=M, cand_d=None, M=M, window_d=window_d, ex_d=None,
                                                 X=0, k=k, mode=0, n_splits=1, pos_d=pos_d, score_d=score_d, flags_d=flags_d, ws_d=ws_d,
                                                 ws_bytes=1 << 16, U=U, F=F), **kw})
    assert call(window_d=None) == BAD_ARG
    assert call(window_d=None, n_rows=0, M=0) == BAD_ARG  # also where the call would only fill the outputs
    assert call(k=65) == UNSUPPORTED
    assert call(users_ptr=ctypes.c_void_p(users_d.data_ptr() + 4)) == ALIGN
    need = int(hip.lib().ebn_topk_workspace_bytes(U, k, 2))
    assert call(n_splits=2, ws_bytes=need - 1) == BAD_ARG
    assert call(n_splits=2, ws_d=None) == BAD_ARG
    torch.cuda.synchronize()
    assert (pos_d == -7).all() and (score_d == 123.0).all() and (flags_d == 0).all()
    assert call(n_splits=2, ws_bytes=need) == OK  # the same call with enough workspace runs
    assert call(U=0) == OK
    torch.cuda.synchronize()
    assert (pos_d.view(-1)[:U * k] >= 0).all() and (pos_d.view(-1)[U * k:] == -7).all()
    assert call(n_rows=0, M=0) == OK  # no candidates: the outputs are filled as empty
    torch.cuda.synchronize()
    assert (pos_d.view(-1)[:U * k] == -1).all() and torch.isneginf(score_d.view(-1)[:U * k]).all()


# ------------------------------------------------------------------------------------------------ whole models
from tests.test_data_pipeline import DATA, frames  # noqa: E402,F401  (the fixture parquets under tests/golden/ebnerd)

N_IMPRESSIONS, N_CANDIDATES, TOP_N = 40, 30, 5
TWO_DAYS, SIX_HOURS = pd.Timedelta(days=2), pd.Timedelta(hours=6)


def _timed_behaviours(frames):  # noqa: F811
    """N_IMPRESSIONS rows of the fixture's behaviours frame, spread over its week, with their ``impression_time`` (which the
    fixture frame drops: it is the parquet's rows whose user has a history, in the parquet's order)"""
    from ebrec.utils._constants import DEFAULT_IMPRESSION_TIMESTAMP_COL, DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_USER_COL

    beh = frames[0]
    raw = pd.read_parquet(DATA / "behaviors.parquet", columns=[DEFAULT_USER_COL, DEFAULT_IMPRESSION_TIMESTAMP_COL, DEFAULT_INVIEW_ARTICLES_COL])
    raw = raw[raw[DEFAULT_USER_COL].isin(set(beh[DEFAULT_USER_COL]))].reset_index(drop=True)
    assert len(raw) == len(beh) and (raw[DEFAULT_USER_COL] == beh[DEFAULT_USER_COL]).all()
    assert all(sorted(a) == sorted(b) for a, b in zip(raw[DEFAULT_INVIEW_ARTICLES_COL], beh[DEFAULT_INVIEW_ARTICLES_COL]))
    beh = beh.assign(**{DEFAULT_IMPRESSION_TIMESTAMP_COL: raw[DEFAULT_IMPRESSION_TIMESTAMP_COL]})
    rows = np.argsort(beh[DEFAULT_IMPRESSION_TIMESTAMP_COL].to_numpy(), kind="stable")[np.linspace(0, len(beh) - 1, N_IMPRESSIONS).astype(int)]
    return beh.iloc[np.random.default_rng(1).permutation(rows)].reset_index(drop=True)  # not in time order: the flush sorts


def _candidates(model, loader, beh, rng, n):
    """ten articles out of the users' histories (so that the exclusion has something to exclude) and others, shuffled"""
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL

    index = model._recommend_index(loader)
    read = sorted({a for h in beh[DEFAULT_HISTORY_ARTICLE_ID_COL] for a in h} & set(index))
    cand = rng.choice(read, 10, replace=False)
    return rng.permutation(np.concatenate([cand, rng.choice(sorted(set(index) - set(cand.tolist())), n - 10, replace=False)]))


@pytest.mark.parametrize("which", ["nrms", "docvec"])
def test_model_recommend_with_a_window_is_the_full_ranking_filtered_by_time(hip, frames, which):  # noqa: F811
    """recommend(window=Freshness(pub, max_age = 2 days)) against the full ranking recommend(top_n = every candidate) filtered on
    the host by  t - 2 days <= published <= t  and cut to top_n: the same ids and the same score bits, with and without the
    history exclusion; impressions before the first article come back as fill_id / -inf."""
    from ebrec.evaluation import Freshness
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_IMPRESSION_TIMESTAMP_COL

    model, mk = {"nrms": _nrms_case, "docvec": _docvec_case}[which](frames)
    beh = _timed_behaviours(frames)
    loader = mk(beh)
    assert DEFAULT_IMPRESSION_TIMESTAMP_COL in loader.X.columns
    rng = np.random.default_rng(7)
    cand = _candidates(model, loader, beh, rng, N_CANDIDATES)
    times = beh[DEFAULT_IMPRESSION_TIMESTAMP_COL].tolist()
    assert pd.Timestamp("2023-02-23") <= min(times) and max(times) <= pd.Timestamp("2023-03-03")
    # publish times in six-hour steps from 25 February on (ties), so the earliest impressions have nothing to be offered
    pub = {int(a): pd.Timestamp("2023-02-25") + int(s) * SIX_HOURS for a, s in zip(cand.tolist(), rng.integers(0, 20, len(cand)))}
    assert len(set(pub.values())) < len(pub)
    fresh = Freshness(pub, max_age=TWO_DAYS)
    where = {int(a): j for j, a in enumerate(cand.tolist())}
    n_inside = [sum(t - TWO_DAYS <= p <= t for p in pub.values()) for t in times]
    assert min(n_inside) == 0 and max(n_inside) >= TOP_N and any(0 < n < TOP_N for n in n_inside), n_inside
    history = [set(h) for h in beh[DEFAULT_HISTORY_ARTICLE_ID_COL]]
    for exclude_history in (True, False):
        full_ids, full_sc = model.recommend(loader, cand, top_n=len(cand), return_scores=True, exclude_history=exclude_history)
        ids, sc = model.recommend(loader, cand, top_n=TOP_N, return_scores=True, exclude_history=exclude_history, window=fresh, fill_id=-9)
        assert ids.shape == sc.shape == (N_IMPRESSIONS, TOP_N) and sc.dtype == np.float32
        assert np.array_equal(model.recommend(loader, cand, top_n=TOP_N, exclude_history=exclude_history, window=fresh, fill_id=-9), ids)
        for u, t in enumerate(times):
            kept = [(a, s) for a, s in zip(full_ids[u].tolist(), full_sc[u]) if a != -1 and t - TWO_DAYS <= pub[a] <= t]
            # the documented tie rule: equal scores to the older article, then to the earlier position
            kept.sort(key=lambda e: (-e[1], pub[e[0]], where[e[0]]))
            kept = kept[:TOP_N]
            want_ids = [a for a, _ in kept] + [-9] * (TOP_N - len(kept))
            want_sc = np.array([s for _, s in kept] + [-np.inf] * (TOP_N - len(kept)), np.float32)
            assert ids[u].tolist() == want_ids, (u, ids[u], want_ids)
            assert np.array_equal(bits(sc[u]), bits(want_sc)), u
            assert not (exclude_history and set(ids[u].tolist()) & history[u])
            if n_inside[u] == 0:
                assert (ids[u] == -9).all() and np.isneginf(sc[u]).all()
        # more than one flush: each sorts its own users, the lists come back in loader order
        assert np.array_equal(model.recommend(loader, cand, top_n=TOP_N, exclude_history=exclude_history, window=fresh, fill_id=-9,
                                              users_per_call=16), ids)


def test_mmr_on_top_of_a_window(hip, frames):  # noqa: F811
    """recommend(window=W, rerank=MMR(...)) is mmr_rerank applied to recommend(window=W, top_n=pool): the pool is the window's"""
    from ebrec.evaluation import MMR, Freshness, mmr_rerank
    from ebrec.evaluation.beyond_accuracy import DeviceLookup
    from ebrec.utils._constants import DEFAULT_IMPRESSION_TIMESTAMP_COL

    POOL, LAM = 8, 0.5
    model, mk = _nrms_case(frames)
    beh = _timed_behaviours(frames)
    loader = mk(beh)
    rng = np.random.default_rng(9)
    cand = _candidates(model, loader, beh, rng, 40)
    times = beh[DEFAULT_IMPRESSION_TIMESTAMP_COL].tolist()
    # twelve articles older than every impression (a pool's worth even after the history is excluded), the rest over the week
    steps = np.concatenate([np.full(12, -4), rng.integers(0, 32, len(cand) - 12)])
    pub = {int(a): pd.Timestamp("2023-02-23") + int(s) * SIX_HOURS for a, s in zip(cand.tolist(), steps)}
    fresh = Freshness(pub)  # no oldest age: everything published up to the impression
    n_inside = [sum(p <= t for p in pub.values()) for t in times]
    assert min(n_inside) >= 12 and min(n_inside) < len(cand)
    articles = {int(a): {"emb": rng.standard_normal(8).astype(np.float32)} for a in model._recommend_index(loader)}
    lookup = DeviceLookup(articles, ["emb"])
    pool_ids, pool_sc = model.recommend(loader, cand, top_n=POOL, return_scores=True, window=fresh)
    assert (pool_ids != -1).all()
    ids, sc = model.recommend(loader, cand, top_n=TOP_N, return_scores=True, window=fresh, rerank=MMR(lookup, "emb", lam=LAM, pool=POOL))
    want_ids, want_sc = mmr_rerank(pool_ids, pool_sc, lookup, "emb", TOP_N, LAM, return_scores=True)
    assert np.array_equal(ids, want_ids) and np.array_equal(bits(sc), bits(np.asarray(want_sc, np.float32)))
    plain = model.recommend(loader, cand, top_n=TOP_N, window=fresh)
    assert not np.array_equal(ids, plain), "the case must exercise the diversity term"
    unwindowed = model.recommend(loader, cand, top_n=TOP_N, rerank=MMR(lookup, "emb", lam=LAM, pool=POOL))
    assert not np.array_equal(ids, unwindowed), "the case must exercise the window"
    for u, t in enumerate(times):
        assert all(pub[a] <= t for a in ids[u].tolist()), u


def test_npa_has_no_windowed_form(hip, frames):  # noqa: F811
    from ebrec.evaluation import Freshness
    from tests.test_npa_cached_scoring_gpu import _npa_case

    model, loader, _Pw, _hp, _V = _npa_case("fixture", frames)
    cand = sorted(model._recommend_index(loader))[:10]
    with pytest.raises(NotImplementedError, match="window= is not supported for NPAModel"):
        model.recommend_pairwise(loader, cand, top_n=5, window=Freshness({a: 1.0 for a in cand}))
