"""ebn_topk_score_f32 (csrc/ebn_topk.hip) and model.recommend() on the GPU, against the float64 restatement of
tests/recommend_cases.py and against scorer.predict."""
import ctypes

import numpy as np
import pytest
import torch

from tests import recommend_cases as rc
from tests.hip_testutil import P, S, dev

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3


def _raw_call(hip, users_d, news_d, n_rows, cand_d, M, ex_d, X, k, mode, n_splits, pos_d, score_d, flags_d, ws_d, ws_bytes, U, F,
              users_ptr=None):
    return hip.lib().ebn_topk_score_f32(users_ptr if users_ptr is not None else P(users_d), P(news_d), n_rows, P(cand_d), M, P(ex_d), X, k,
                                        mode, n_splits, P(pos_d), P(score_d), P(flags_d), P(ws_d), ws_bytes, U, F, S())


def run_topk(hip, users, news, cand_rows, exclude, k, mode=0, n_splits=0):
    """-> (pos [U, k] int32, score [U, k] float32, flags [2]) as numpy arrays"""
    U, F = users.shape
    n_rows = news.shape[0]
    M = n_rows if cand_rows is None else len(cand_rows)
    users_d, news_d = dev(users), dev(news)
    cand_d = None if cand_rows is None else dev(cand_rows, torch.int32)
    ex_d = None if exclude is None else dev(exclude, torch.int32)
    X = 0 if exclude is None else exclude.shape[1]
    pos_d = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
    score_d = torch.full((U, k), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    splits = n_splits if n_splits > 0 else int(hip.lib().ebn_topk_auto_splits(U, M))
    ws_bytes = int(hip.lib().ebn_topk_workspace_bytes(U, k, splits))
    assert ws_bytes > 0
    ws_d = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    code = _raw_call(hip, users_d, news_d, n_rows, cand_d, M, ex_d, X, k, mode, n_splits, pos_d, score_d, flags_d, ws_d, ws_bytes, U, F)
    assert code == OK, code
    torch.cuda.synchronize()
    return pos_d.cpu().numpy(), score_d.cpu().numpy(), flags_d.cpu().numpy()


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("exclude", [None, "x3", "all"])
@pytest.mark.parametrize("cand", ["null", "subset"])
@pytest.mark.parametrize("shape", rc.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_cases_equal_the_restatement(hip, shape, cand, exclude):
    """Integer-valued inputs: fp32 is exact in any order, so positions AND raw scores must equal the float64 restatement; in
    sigmoid mode the positions are the same (ranking is on the raw value) and the kept values are 1 / (1 + expf(-s)) -- expf,
    the add and the division each round once or twice: 4 ulp of fp32 relative to the float64 sigmoid."""
    U, M, F, k = shape
    users, news, cand_rows, ex = rc.integer_case(U, M, F, seed=U + M, cand=cand, exclude=exclude)
    s64 = rc.scores64(users, news, cand_rows)
    assert np.array_equal(s64, rc.scores64(users, news, cand_rows).astype(np.float32).astype(np.float64))
    want_pos, want_score, want_flags = rc.topk_reference(s64, k, cand_rows, news.shape[0], ex)
    pos, score, flags = run_topk(hip, users, news, cand_rows, ex, k, mode=0)
    assert np.array_equal(pos, want_pos)
    assert np.array_equal(score.astype(np.float64), want_score)
    assert tuple(flags) == want_flags == (0, 0)
    if exclude == "all" and M <= rc.MAX_X:
        assert (pos[0] == -1).all() and np.isneginf(score[0]).all()  # the user whose every candidate is excluded
    pos1, score1, _ = run_topk(hip, users, news, cand_rows, ex, k, mode=1)
    assert np.array_equal(pos1, want_pos)
    filled = want_pos >= 0
    want_sig = 1.0 / (1.0 + np.exp(-want_score[filled]))
    assert np.isneginf(score1[~filled]).all()
    assert (np.abs(score1[filled] - want_sig) <= 4 * 2.0 ** -23 * want_sig).all()


# ------------------------------------------------------------------------------------------------ split invariance
@pytest.mark.parametrize("shape", rc.SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_split_and_every_run_gives_the_same_bits(hip, shape):
    U, M, F, k = shape
    rng = np.random.default_rng(5)
    users, news = rng.standard_normal((U, F)).astype(np.float32), rng.standard_normal((M, F)).astype(np.float32)
    ex = rng.integers(-1, M, (U, 4)).astype(np.int32)
    runs = {s: run_topk(hip, users, news, None, ex, k, mode=1, n_splits=s) for s in (1, 2, 7, 0)}
    again = run_topk(hip, users, news, None, ex, k, mode=1, n_splits=7)
    for s, (pos, score, flags) in list(runs.items()) + [("again", again)]:
        assert np.array_equal(pos, runs[1][0]), s
        assert np.array_equal(score.view(np.int32), runs[1][1].view(np.int32)), s
        assert tuple(flags) == (0, 0)
    assert (runs[1][0] >= 0).all()


# ------------------------------------------------------------------------------------------------ rounded cases
@pytest.mark.parametrize("shape", rc.ROUNDED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_standard_normal_cases_by_properties(hip, shape):
    """Ordered lists; every returned score within b of the float64 score of the returned candidate; no admissible candidate
    left out whose float64 score exceeds the k-th returned candidate's float64 score by more than 2 b (b: the summation bound
    of the inputs, recommend_cases.summation_bound)."""
    U, M, F, k = shape
    rng = np.random.default_rng(11)
    users, news = rng.standard_normal((U, F)).astype(np.float32), rng.standard_normal((M, F)).astype(np.float32)
    ex = rng.integers(0, M, (U, 5)).astype(np.int32)
    b = rc.summation_bound(users, news)
    s64 = rc.scores64(users, news)
    pos, score, flags = run_topk(hip, users, news, None, ex, k, mode=0)
    print(f"shape {shape}: b = {b:.3e}, max |score - float64| = {np.abs(score - np.take_along_axis(s64, pos.astype(np.int64), 1)).max():.3e}")
    assert tuple(flags) == (0, 0) and (pos >= 0).all() and (pos < M).all()
    assert ((score[:, :-1] > score[:, 1:]) | ((score[:, :-1] == score[:, 1:]) & (pos[:, :-1] < pos[:, 1:]))).all()
    kept64 = np.take_along_axis(s64, pos.astype(np.int64), 1)
    assert (np.abs(score - kept64) <= b).all()
    for u in range(U):
        assert len(set(pos[u])) == k and not np.isin(pos[u], ex[u]).any()
        out = np.ones(M, bool)
        out[pos[u]] = False
        out[ex[u]] = False
        assert s64[u, out].max() <= kept64[u, -1] + 2 * b, u


# ------------------------------------------------------------------------------------------------ flags and errors
def test_rows_outside_the_table_are_skipped_and_flagged(hip):
    users, news, _c, _e = rc.integer_case(9, 40, 8, seed=2)
    cand_rows = np.arange(40, dtype=np.int32)[::-1].copy()
    cand_rows[[3, 17]] = [40, -1]  # n_rows and -1
    want_pos, want_score, want_flags = rc.topk_reference(rc.scores64(users, news, cand_rows), 6, cand_rows, 40)
    pos, score, flags = run_topk(hip, users, news, cand_rows, None, 6)
    assert want_flags == (1, 0) and tuple(flags) == (1, 0)
    assert np.array_equal(pos, want_pos) and np.array_equal(score.astype(np.float64), want_score)
    assert not np.isin(pos, [3, 17]).any()


def test_nan_scores_never_enter_a_list_and_infinities_rank_like_numbers(hip):
    users, news, _c, _e = rc.integer_case(9, 40, 8, seed=3)
    users = np.abs(users) + 1  # positive users: an infinite news component gives an infinite score, never inf - inf
    news[5] = np.nan
    news[7, 0] = np.inf
    news[8, 0] = np.inf
    news[9, 0] = -np.inf
    with np.errstate(invalid="ignore"):
        s64 = rc.scores64(users, news)
    want_pos, want_score, want_flags = rc.topk_reference(s64, 40, None, 40)
    pos, score, flags = run_topk(hip, users, news, None, None, 40)
    assert want_flags == (0, 1) and tuple(flags) == (0, 1)
    assert np.array_equal(pos, want_pos) and np.array_equal(score.astype(np.float64), want_score)
    assert (pos[:, 0] == 7).all() and (pos[:, 1] == 8).all() and (pos[:, 38] == 9).all() and (pos[:, 39] == -1).all()
    assert not (pos == 5).any()


def test_unsupported_misaligned_and_short_workspace_calls_return_their_code_and_write_nothing(hip):
    U, M, F, k = 5, 300, 8, 4
    users, news, _c, _e = rc.integer_case(U, M, F, seed=4)
    users_d, news_d = dev(users), dev(news)
    pad_d = dev(np.zeros(U * 8 + 1, np.float32))
    ex_d = dev(np.full((U, 257), -1), torch.int32)
    ws_d = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    pos_d = torch.full((U, 65), -7, dtype=torch.int32, device="cuda")
    score_d = torch.full((U, 65), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    call = lambda **kw: _raw_call(hip, **{**dict(users_d=users_d, news_d=news_d, n_rows=M, cand_d=None, M=M, ex_d=None, X=0, k=k, mode=0,
                                                 n_splits=1, pos_d=pos_d, score_d=score_d, flags_d=flags_d, ws_d=ws_d, ws_bytes=1 << 16,
                                                 U=U, F=F), **kw})
    assert call(k=65) == UNSUPPORTED
    assert call(ex_d=ex_d, X=257) == UNSUPPORTED
    assert call(users_d=pad_d, news_d=pad_d, n_rows=6, M=6, F=6) == UNSUPPORTED
    assert call(users_ptr=ctypes.c_void_p(pad_d.data_ptr() + 4)) == ALIGN
    need = int(hip.lib().ebn_topk_workspace_bytes(U, k, 2))
    assert need >= 2 * U * k * 8
    assert call(n_splits=2, ws_bytes=need - 1) == BAD_ARG
    assert call(n_splits=2, ws_d=None) == BAD_ARG
    assert call(M=M - 1) == BAD_ARG  # cand_rows NULL means M == n_rows
    torch.cuda.synchronize()
    assert (pos_d == -7).all() and (score_d == 123.0).all() and (flags_d == 0).all()
    assert call(n_splits=2, ws_bytes=need) == OK  # the same call with enough workspace runs
    assert call(U=0) == OK


def test_no_candidates_fills_the_outputs_as_empty(hip):
    users_d = dev(np.ones((3, 8), np.float32))
    pos_d = torch.full((3, 5), -7, dtype=torch.int32, device="cuda")
    score_d = torch.full((3, 5), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert _raw_call(hip, users_d, users_d, 0, None, 0, None, 0, 5, 1, 0, pos_d, score_d, flags_d, None, 0, 3, 8) == OK
    torch.cuda.synchronize()
    assert (pos_d == -1).all() and torch.isneginf(score_d).all()


# ------------------------------------------------------------------------------------------------ whole models
from tests.test_data_pipeline import frames  # noqa: E402,F401  (the fixture parquets under tests/golden/ebnerd)

N_IMPRESSIONS, N_CANDIDATES, TOP_N = 40, 30, 5


def _nrms_case(frames):  # noqa: F811
    from ebrec.models.newsrec import NRMSModel
    from ebrec.models.newsrec.dataloader import NRMSDataLoader
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL
    from tests.test_nrms_model import make_hp

    beh, _train, mapping = frames
    mk = lambda b: NRMSDataLoader(behaviors=b, article_dict=mapping, unknown_representation="zeros",
                                  history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=16, eval_mode=True)
    rng = np.random.default_rng(43)
    model = NRMSModel(make_hp(history_size=3, title_size=10), word2vec_embedding=rng.standard_normal((20, 32)).astype(np.float32), seed=3)
    return model, mk


def _docvec_case(frames):  # noqa: F811
    from ebrec.models.newsrec import NRMSDocVec
    from ebrec.models.newsrec.dataloader import NRMSDataLoader
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL
    from tests.test_docvec_model import make_hp

    beh, _train, mapping = frames
    rng = np.random.default_rng(44)
    vectors = {a: rng.standard_normal(32).astype(np.float32) for a in mapping}
    mk = lambda b: NRMSDataLoader(behaviors=b, article_dict=vectors, unknown_representation="zeros",
                                  history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=16, eval_mode=True)
    hp = make_hp(title_size=32, newsencoder_units_per_layer=[24, 16], head_num=2, head_dim=8, attention_hidden_dim=6, history_size=3)
    return NRMSDocVec(hp, seed=3), mk


def _lstur_case(user_type):
    def make(frames):  # noqa: F811
        from tests.test_cached_scoring_gpu import _lstur_case as case

        model, loader, _Pw, _hp, _V = case("fixture", user_type, frames)
        mk = lambda b: type(loader)(behaviors=b, article_dict=loader.article_dict, user_id_mapping=loader.user_id_mapping,
                                    unknown_representation="zeros", history_column=loader.history_column, batch_size=16, eval_mode=True)
        return model, mk
    return make


def _naml_case(frames):  # noqa: F811
    from tests.test_cached_scoring_gpu import _naml_case as case

    model, loader, _Pw, _hp, _V = case("fixture", frames)
    mk = lambda b: type(loader)(behaviors=b, article_dict=loader.article_dict, body_mapping=loader.body_mapping,
                                category_mapping=loader.category_mapping, subcategory_mapping=loader.subcategory_mapping,
                                unknown_representation="zeros", history_column=loader.history_column, batch_size=16, eval_mode=True)
    return model, mk


MODEL_CASES = {"nrms": _nrms_case, "docvec": _docvec_case, "lstur-ini": _lstur_case("ini"), "lstur-con": _lstur_case("con"),
               "naml": _naml_case}


@pytest.mark.parametrize("which", list(MODEL_CASES))
def test_model_recommend_agrees_with_scorer_predict(hip, frames, which):  # noqa: F811
    """recommend() against scorer.predict over a loader whose every in-view list is the candidate list: the scores of the same
    (user, article) agree within b / 4 + 2 ulp (1/4: the sigmoid's Lipschitz constant; b: the fp32 summation bound of the model's
    own user and news vectors), no candidate left out beats the fifth kept one by more than twice that, and with
    exclude_history no article of a user's history is in the user's list."""
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_LABELS_COL

    model, mk = MODEL_CASES[which](frames)
    beh = frames[0].iloc[:N_IMPRESSIONS].reset_index(drop=True)
    loader = mk(beh)
    rng = np.random.default_rng(7)
    index = model._recommend_index(loader)
    # ten articles out of the users' histories (so that the exclusion has something to exclude) and twenty others, shuffled
    read = sorted({a for h in beh[DEFAULT_HISTORY_ARTICLE_ID_COL] for a in h} & set(index))
    cand = rng.choice(read, 10, replace=False)
    cand = rng.permutation(np.concatenate([cand, rng.choice(sorted(set(index) - set(cand.tolist())), N_CANDIDATES - 10, replace=False)]))
    ids_ex, sc_ex = model.recommend(loader, cand, top_n=TOP_N, return_scores=True)
    ids_all, sc_all = model.recommend(loader, cand, top_n=TOP_N, return_scores=True, exclude_history=False)
    assert ids_ex.shape == sc_ex.shape == ids_all.shape == sc_all.shape == (N_IMPRESSIONS, TOP_N) and sc_ex.dtype == np.float32
    assert np.array_equal(model.recommend(loader, cand, top_n=TOP_N), ids_ex)

    same_users = beh.copy()
    same_users[DEFAULT_INVIEW_ARTICLES_COL] = [cand.tolist()] * N_IMPRESSIONS
    same_users[DEFAULT_LABELS_COL] = [[0] * N_CANDIDATES] * N_IMPRESSIONS
    pred = model.scorer.predict(mk(same_users)).reshape(N_IMPRESSIONS, N_CANDIDATES).astype(np.float64)

    cache, news_all = model._recommend_cache(loader)
    users = torch.cat([model._user_vectors_cached(cache, loader, i)[0] for i in range(len(loader))]).cpu().numpy()
    cand_news = news_all.cpu().numpy()[[index[c] for c in cand.tolist()]]
    tol = rc.summation_bound(users, cand_news) / 4 + 2 * 2.0 ** -24  # 2 ulp of a float32 in [0.5, 1)
    print(f"{which}: F = {users.shape[1]}, tolerance {tol:.3e}")

    col = {c: j for j, c in enumerate(cand.tolist())}
    history = [set(h) for h in beh[DEFAULT_HISTORY_ARTICLE_ID_COL]]
    assert any(history[u] & set(col) for u in range(N_IMPRESSIONS)), "the case must exercise the exclusion"
    for ids, sc, excluded in ((ids_ex, sc_ex, history), (ids_all, sc_all, [set()] * N_IMPRESSIONS)):
        for u in range(N_IMPRESSIONS):
            kept = [col[a] for a in ids[u].tolist()]
            assert len(set(kept)) == TOP_N and not set(ids[u].tolist()) & excluded[u]
            assert (np.abs(sc[u] - pred[u, kept]) <= tol).all(), (u, sc[u], pred[u, kept])
            assert (np.diff(sc[u]) <= 0).all()
            left_out = [j for c, j in col.items() if j not in kept and c not in excluded[u]]
            assert pred[u, left_out].max() <= pred[u, kept[-1]] + 2 * tol, u
    raw_ids, raw = model.recommend(loader, cand, top_n=TOP_N, return_scores=True, scores="raw")
    assert np.array_equal(raw_ids, ids_ex) and (np.abs(1 / (1 + np.exp(-raw.astype(np.float64))) - sc_ex) <= 4 * 2.0 ** -23).all()


def test_recommend_lists_go_into_the_beyond_accuracy_metrics_as_they_are(hip, frames):  # noqa: F811
    from ebrec.evaluation.beyond_accuracy import DeviceLookup, IntralistDiversity

    model, mk = _nrms_case(frames)
    loader = mk(frames[0].iloc[:N_IMPRESSIONS].reset_index(drop=True))
    ids = model.recommend(loader, None, top_n=TOP_N)  # the whole index: row 0, the unknown article, is no candidate
    assert ids.shape == (N_IMPRESSIONS, TOP_N) and np.isin(ids, list(loader.lookup_article_index)).all()
    rng = np.random.default_rng(9)
    articles = {int(a): {"emb": rng.standard_normal(8).astype(np.float32)} for a in loader.lookup_article_index}
    on_device = IntralistDiversity()(ids, lookup_dict=DeviceLookup(articles, ["emb"]), lookup_key="emb")
    on_host = IntralistDiversity()(ids, lookup_dict=articles, lookup_key="emb")
    np.testing.assert_allclose(on_device, on_host, rtol=1e-4, atol=1e-5)
