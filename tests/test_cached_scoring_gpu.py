"""Scoring LSTUR and NAML from a once-encoded article catalogue: the three kernels through the C ABI (the indexed inference GRU
bit-equal to the training GRU, the per-row AttLayer2 logit and the indexed pooling-and-scoring kernel against float64 numpy) and
scorer.predict with the cache against the per-batch path, the repeated-history layout and the float64 oracles."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from tests import lstur_oracle as lo
from tests import naml_oracle as nao
from tests.guarded import guard_in
from tests.hip_testutil import P, S, assert_close, dev, host
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)
from tests.test_lstur_gpu import _model as lstur_model
from tests.test_lstur_gpu import _params as lstur_params
from tests.test_lstur_gpu import hp_small as lstur_small
from tests.test_naml_gpu import _model as naml_model
from tests.test_naml_gpu import _params as naml_params
from tests.test_naml_gpu import hp_small as naml_small

pytestmark = pytest.mark.gpu
f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)


def idev(a, dtype=torch.int32):
    return dev(np.asarray(a), dtype)


# ---------------------------------------------------------------------------------------------- kernel (c): indexed inference GRU
@pytest.mark.parametrize("B,H,U,user_type", [(3, 1, 8, "ini"), (5, 2, 24, "con"), (16, 7, 64, "ini"), (33, 20, 400, "ini"),
                                             (33, 20, 400, "con"), (17, 50, 40, "con"), (257, 3, 36, "ini")])
def test_indexed_gru_is_bit_equal_to_the_training_gru_on_gathered_rows(hip, B, H, U, user_type):
    """The step body is shared (same tile GEMM, same gate epilogue), so the final state must equal ebn_gru_fwd_f32's Hs[H] bit for
    bit when that kernel is given the gathered gx and X rows.  B and U off the 16 x 16 tile, H from 1 to 50, both LSTUR types."""
    rng = np.random.default_rng(B * 1000 + H * 10 + U)
    F, n_rows = U, 41
    news = rng.uniform(-1, 1, (n_rows, F)).astype(np.float32)
    zero_rows = [0, 7, 40]
    news[zero_rows] = 0.0
    idx = rng.integers(0, n_rows, (B, H))
    idx[rng.random((B, H)) < 0.2] = rng.choice(zero_rows)  # masked steps: holes, left and right padding alike
    idx[0] = 0                                             # a fully masked sequence
    lim = np.sqrt(6.0 / (4 * U))
    Wk, Wr = (rng.uniform(-lim, lim, (U, 3 * U)).astype(np.float32) for _ in range(2))
    bias = rng.uniform(-0.2, 0.2, (2, 3 * U)).astype(np.float32)
    h0 = rng.uniform(-0.5, 0.5, (B, U)).astype(np.float32)
    newsd, Wkd, Wrd, bd, h0d, idxd = dev(news), dev(Wk), dev(Wr), dev(bias), dev(h0), idev(idx)
    h0p = P(h0d) if user_type == "ini" else None
    gx_all = torch.empty(n_rows, 3 * U, device="cuda")
    hip.call("ebn_gemm_f32", 0, 0, n_rows, 3 * U, F, f1, P(newsd), F, P(Wkd), 3 * U, f0, P(gx_all), 3 * U, S())
    live = (newsd != 0).any(dim=1).to(torch.int32).contiguous()
    flat = idxd.reshape(-1).long()
    gx, X = gx_all[flat].contiguous(), newsd[flat].contiguous()
    Hs, act = torch.empty(H + 1, B, U, device="cuda"), torch.empty(H, B, 4 * U, device="cuda")
    hip.call("ebn_gru_fwd_f32", P(gx), P(X), P(Wrd), P(bd), h0p, P(Hs), P(act), B, H, F, U, S())
    h_work, h_out = (torch.full((B, U), float("nan"), device="cuda") for _ in range(2))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.call("ebn_gru_infer_indexed_f32", P(gx_all), P(live), n_rows, P(idxd), P(Wrd), P(bd), h0p, P(h_work), P(h_out), B, H, U,
             P(flag), S())
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert torch.equal(h_out, Hs[H]), f"max abs diff {float((h_out - Hs[H]).abs().max()):.3e}"
    want0 = h0d[0] if user_type == "ini" else torch.zeros(U, device="cuda")
    assert torch.equal(h_out[0], want0)  # every step masked: the initial state comes out


def test_indexed_gru_flags_rows_outside_the_catalogue_and_masks_those_steps(hip):
    rng = np.random.default_rng(9)
    B, H, U, n_rows = 5, 4, 24, 12
    gx_all = dev(rng.uniform(-1, 1, (n_rows, 3 * U)).astype(np.float32))
    live = torch.ones(n_rows, dtype=torch.int32, device="cuda")
    live[3] = 0
    Wr, bias = dev(rng.uniform(-0.2, 0.2, (U, 3 * U)).astype(np.float32)), dev(rng.uniform(-0.2, 0.2, (2, 3 * U)).astype(np.float32))
    idx = rng.integers(0, n_rows, (B, H))
    clean, bad = idx.copy(), idx.copy()
    clean[2, 1], bad[2, 1] = 3, n_rows  # a masked article in one run, a row past the catalogue in the other
    clean[4, 0], bad[4, 0] = 3, -1
    outs = []
    for ix in (clean, bad):
        h_work, h_out = (torch.empty(B, U, device="cuda") for _ in range(2))
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        hip.call("ebn_gru_infer_indexed_f32", P(gx_all), P(live), n_rows, P(idev(ix)), P(Wr), P(bias), None, P(h_work), P(h_out), B, H,
                 U, P(flag), S())
        outs.append((h_out, int(flag.item())))
    assert outs[0][1] == 0 and outs[1][1] == 1
    assert torch.equal(outs[0][0], outs[1][0])
    L = hip.lib()
    ok = (P(gx_all), P(live), n_rows, P(idev(idx)), P(Wr), P(bias), None)
    hw, ho = torch.empty(B, U, device="cuda"), torch.empty(B, U, device="cuda")
    assert L.ebn_gru_infer_indexed_f32(*ok, P(hw), P(hw), B, H, U, None, S()) == -1       # one buffer for both
    assert L.ebn_gru_infer_indexed_f32(*ok, P(hw), P(ho), B, H, 6, None, S()) != 0       # U % 4
    assert L.ebn_gru_infer_indexed_f32(*ok, None, P(ho), B, H, U, None, S()) == -1
    assert L.ebn_gru_infer_indexed_f32(*ok, P(hw), P(ho), -1, H, U, None, S()) == -1


# ---------------------------------------------------------------------------------------------- kernel (a): per-row logit
@pytest.mark.parametrize("n,A", [(1, 24), (1031, 200), (77, 50)])
def test_att_logit_rows_vs_float64(hip, n, A):
    rng = np.random.default_rng(n + A)
    U = rng.uniform(-2, 2, (n, A)).astype(np.float32)  # pre-activations of O(1) rows through a glorot kernel, as in the pooling tests
    b, q = rng.uniform(-0.1, 0.1, A).astype(np.float32), rng.uniform(-0.3, 0.3, A).astype(np.float32)
    Ud, a = dev(U), torch.full((n,), float("nan"), device="cuda")
    hip.call("ebn_att_logit_rows_f32", P(Ud), P(dev(b)), P(dev(q)), P(a), n, A, S())
    want = np.exp(np.tanh(U.astype(np.float64) + b) @ q.astype(np.float64))
    assert_close(host(a), want, rtol=1e-5, atol=1e-6, what="a = exp(tanh(U + b) . q)")
    np.testing.assert_array_equal(host(Ud), U.astype(np.float64))  # the input is not modified
    assert hip.lib().ebn_att_logit_rows_f32(None, None, None, None, 5, A, S()) == -1
    assert hip.lib().ebn_att_logit_rows_f32(P(Ud), P(Ud), P(Ud), P(a), -1, A, S()) == -1


# ---------------------------------------------------------------------------------------------- kernel (b): indexed pooling + scores
LENS = [3, 0, 1, 250, 17, 0, 5, 64, 2]  # in-view lengths of one call: 0, 1 and 250 among them


def _pool_case(F, H, seed):
    rng = np.random.default_rng(seed)
    n_rows, B = 301, len(LENS)
    news = rng.uniform(-1, 1, (n_rows, F)).astype(np.float32)
    a = np.exp(rng.uniform(-3, 3, n_rows)).astype(np.float32)  # exp of the logits the pooling tests' scaling gives: finite in fp32
    his = rng.integers(0, n_rows, (B, H))
    cand = rng.integers(0, n_rows, int(np.sum(LENS)))
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    return news, a, his, cand, off


def _pool_ref(news, a, his, cand, off, sigmoid):
    n64, a64 = news.astype(np.float64), a.astype(np.float64)
    ok = (his >= 0) & (his < len(a))
    safe = np.where(ok, his, 0)
    ah = np.where(ok, a64[safe], 0.0)
    w = ah / (ah.sum(1, keepdims=True) + 1e-7)
    user = np.einsum("bh,bhf->bf", w, n64[safe])
    imp = np.repeat(np.arange(len(off) - 1), np.diff(off))
    s = np.einsum("nf,nf->n", n64[cand], user[imp])
    return user, (1.0 / (1.0 + np.exp(-s)) if sigmoid else s)


def _guarded(x):
    """x on the device between two NaN guards (tests/guarded.py): a read in front of or behind the rows poisons the result."""
    return guard_in(np.asarray(x, dtype=np.float32))[0]  # the view keeps the allocation alive


def _pool_run(hip, news_d, a_d, n_rows, his, cand, off, F, mode, want_user):
    B, H = his.shape
    scores = torch.full((max(len(cand), 1),), float("nan"), device="cuda")
    user = torch.full((B, F), float("nan"), device="cuda") if want_user else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.call("ebn_indexed_attpool_score_f32", P(news_d), P(a_d), n_rows, P(idev(his)), P(idev(cand)), P(idev(off, torch.int64)),
             len(cand), P(scores), P(user), P(flag), B, H, F, mode, S())
    torch.cuda.synchronize()
    return scores[: len(cand)], user, int(flag.item())


@pytest.mark.parametrize("H", [1, 20, 50])
@pytest.mark.parametrize("F", [400, 36])
def test_indexed_attpool_score_vs_float64(hip, F, H):
    news, a, his, cand, off = _pool_case(F, H, seed=F + H)
    news_d, a_d = _guarded(news), _guarded(a)
    for mode, want_user in ((1, True), (0, False), (0, True)):
        scores, user, flag = _pool_run(hip, news_d, a_d, len(a), his, cand, off, F, mode, want_user)
        ref_user, ref_scores = _pool_ref(news, a, his, cand, off, sigmoid=mode == 1)
        assert flag == 0
        assert_close(host(scores), ref_scores, rtol=1e-5, atol=1e-6, what=f"scores (mode {mode})")
        if want_user:
            assert_close(host(user), ref_user, rtol=1e-5, atol=1e-6, what="pooled user vector")


def test_indexed_attpool_score_out_of_range_rows_backward_offsets_and_bad_arguments(hip):
    F, H = 36, 20
    news, a, his, cand, off = _pool_case(F, H, seed=3)
    n_rows = len(a)
    news_d, a_d = _guarded(news), _guarded(a)
    base, base_user, flag = _pool_run(hip, news_d, a_d, n_rows, his, cand, off, F, 1, True)
    assert flag == 0
    # rows outside the catalogue: a history item of impression 4 (-1), one of impression 6 (n_rows), a candidate of impression 3
    his_bad, cand_bad = his.copy(), cand.copy()
    his_bad[4, 2], his_bad[6, 0] = -1, n_rows
    bad_pos = int(off[3]) + 100
    cand_bad[bad_pos] = n_rows + 1
    got, got_user, flag = _pool_run(hip, news_d, a_d, n_rows, his_bad, cand_bad, off, F, 1, True)
    assert flag == 1
    imp = np.repeat(np.arange(len(LENS)), LENS)
    untouched = torch.from_numpy((imp != 4) & (imp != 6)).cuda()
    untouched[bad_pos] = False
    assert torch.equal(got[untouched], base[untouched]), "an out-of-range row changed another impression's scores"
    assert float(got[bad_pos]) == 0.5  # sigmoid(0): the row was never read
    ref_user, ref_scores = _pool_ref(news, a, his_bad, np.where(cand_bad < n_rows, cand_bad, 0), off, sigmoid=True)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_user).all())  # nothing of the NaN guard was read
    assert_close(host(got_user), ref_user, rtol=1e-5, atol=1e-6, what="user vectors with the missing history rows skipped")
    ok = ~(host(untouched) > 0) & (np.arange(len(cand)) != bad_pos)
    assert_close(host(got)[ok], ref_scores[ok], rtol=1e-5, atol=1e-6, what="scores of the impressions with a missing history row")
    # offsets that run backwards (impression 4) or past n (the last one): empty lists, every other impression as before
    off_bad = off.copy()
    off_bad[5] = -5                               # impression 4: [254, -5) backwards; impression 5 (empty before): starts below 0
    off_bad[-1] = len(cand) + 3                   # the last impression leaves [0, n]
    scores, _u, flag = _pool_run(hip, news_d, a_d, n_rows, his, cand, off_bad, F, 1, False)
    gone = torch.from_numpy((imp == 4) | (imp == len(LENS) - 1)).cuda()
    assert flag == 0 and torch.equal(scores[~gone], base[~gone])
    assert bool(torch.isnan(scores[gone]).all())  # never written
    L = hip.lib()
    args = lambda **kw: [kw.get(k, v) for k, v in dict(news=P(news_d), a=P(a_d), n_rows=n_rows, his=P(idev(his)), cand=P(idev(cand)),
                                                      off=P(idev(off, torch.int64)), n=len(cand), scores=P(scores), user=None, flag=None,
                                                      B=len(LENS), H=H, F=F, mode=1, stream=S()).items()]
    assert L.ebn_indexed_attpool_score_f32(*args(his=None)) == -1 and L.ebn_indexed_attpool_score_f32(*args(off=None)) == -1
    assert L.ebn_indexed_attpool_score_f32(*args(B=-1)) == -1 and L.ebn_indexed_attpool_score_f32(*args(mode=2)) == -1
    assert L.ebn_indexed_attpool_score_f32(*args(F=38)) == -2 and L.ebn_indexed_attpool_score_f32(*args(H=1 << 20)) == -2
    assert L.ebn_indexed_attpool_score_f32(*args(B=0)) == 0


# ---------------------------------------------------------------------------------------------- whole models
def _synthetic_behaviors(rng, art_ids, H, n=50):
    inview = [rng.choice(np.append(art_ids, 7), int(rng.integers(1, 9))).tolist() for _ in range(n)]
    return pd.DataFrame({"user_id": rng.integers(0, 9, n), "article_id_fixed": [rng.choice(np.append(art_ids, 0), H).tolist() for _ in range(n)],
                         "article_ids_inview": inview, "labels": [[0] * len(v) for v in inview]})


ART_IDS = np.arange(500, 540)


def _lstur_case(kind, user_type, frames):  # noqa: F811
    """(model with random weights, eval loader, float64 weights, hparams, vocabulary size)"""
    from ebrec.models.newsrec.dataloader import LSTURDataLoader
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_USER_COL

    rng = np.random.default_rng(43)
    if kind == "synthetic":
        hp = type("hp", (lstur_small,), {"type": user_type})
        V = 150
        mapping = {int(a): rng.integers(1, V, hp.title_size).tolist() for a in ART_IDS}
        mapping[503] = [0] * hp.title_size  # a known article whose title is padding only: a masked GRU step
        loader = LSTURDataLoader(behaviors=_synthetic_behaviors(rng, ART_IDS, hp.history_size), article_dict=mapping,
                                 user_id_mapping={u: u + 1 for u in range(7)}, history_column="article_id_fixed",
                                 unknown_representation="zeros", eval_mode=True, batch_size=16)
    else:
        beh, _train, mapping = frames
        users = sorted(pd.unique(beh[DEFAULT_USER_COL]))
        hp = type("hp", (lstur_small,), {"type": user_type, "title_size": 10, "history_size": 3, "n_users": len(users)})
        V = 20
        loader = LSTURDataLoader(behaviors=beh.iloc[:40].reset_index(drop=True), article_dict=mapping,
                                 user_id_mapping={u: i + 1 for i, u in enumerate(users[:-3])}, unknown_representation="zeros",
                                 history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=16, eval_mode=True)
    Pw = lstur_params(hp, V, 16, seed=3)
    return lstur_model(hp, V, 16, 5, Pw), loader, Pw, hp, V


def _naml_case(kind, frames):  # noqa: F811
    from ebrec.models.newsrec.dataloader import NAMLDataLoader
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL

    rng = np.random.default_rng(47)
    if kind == "synthetic":
        hp = naml_small
        V = 150
        mapping = {int(a): rng.integers(1, V, hp.title_size).tolist() for a in ART_IDS}
        body = {int(a): rng.integers(1, V, hp.body_size).tolist() for a in ART_IDS[3:]}
        body[7] = rng.integers(1, V, hp.body_size).tolist()  # an article with a body and no title
        cats = {int(a): int(a) % hp.vert_num for a in ART_IDS[::2]}
        subcats = {int(a): int(a) % hp.subvert_num for a in ART_IDS}
        loader = NAMLDataLoader(behaviors=_synthetic_behaviors(rng, ART_IDS, hp.history_size), article_dict=mapping, body_mapping=body,
                                category_mapping=cats, subcategory_mapping=subcats, unknown_representation="zeros",
                                unknown_category_value=3, history_column="article_id_fixed", eval_mode=True, batch_size=16)
    else:
        beh, _train, mapping = frames
        hp = type("hp", (naml_small,), {"title_size": 10, "body_size": 10, "history_size": 3})
        V = 20
        cats = {a: int(a) % 6 + 1 for j, a in enumerate(sorted(mapping)) if j % 4}
        subcats = {a: int(a) % 9 for a in sorted(mapping)}
        loader = NAMLDataLoader(behaviors=beh.iloc[:40].reset_index(drop=True), article_dict=mapping, body_mapping=mapping,
                                category_mapping=cats, subcategory_mapping=subcats, unknown_representation="zeros",
                                history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=16, eval_mode=True)
    Pw = naml_params(hp, V, 16, seed=3)
    return naml_model(hp, V, 16, 5, Pw), loader, Pw, hp, V


def _runs(model, loader):
    """scorer.predict of one model over one eval loader: with the cache (twice), without it, and over the repeated-history layout"""
    assert model.scorer.cache_articles is True  # the cached path is the default
    cached = model.scorer.predict(loader)
    again = model.scorer.predict(loader)
    model.scorer.cache_articles = False
    per_batch = model.scorer.predict(loader)
    model.scorer.cache_articles = True
    repeated = np.concatenate([model.scorer.predict(loader[i][0]) for i in range(len(loader))])
    return dict(cached=cached, again=again, per_batch=per_batch, repeated=repeated, model=model, loader=loader)


@pytest.fixture(scope="module", params=[("synthetic", "ini"), ("synthetic", "con"), ("fixture", "ini"), ("fixture", "con")],
                ids=lambda p: "-".join(p))
def lstur_runs(request, frames):  # noqa: F811
    kind, user_type = request.param
    model, loader, Pw, _hp, _V = _lstur_case(kind, user_type, frames)
    out = _runs(model, loader)
    out["oracle"] = np.concatenate([lo.scorer_forward(u, h, p, Pw, user_type).reshape(-1, 1)
                                    for (u, h, p), _y in (loader[i] for i in range(len(loader)))])
    return out


@pytest.fixture(scope="module", params=["synthetic", "fixture"])
def naml_runs(request, frames):  # noqa: F811
    model, loader, Pw, _hp, _V = _naml_case(request.param, frames)
    out = _runs(model, loader)
    out["oracle"] = np.concatenate([nao.scorer_forward(xs, Pw).reshape(-1, 1) for xs, _y in (loader[i] for i in range(len(loader)))])
    return out


def _check_runs(r):
    n = sum(len(r["loader"].index_eval_batch(i)[1]) for i in range(len(r["loader"])))
    assert r["cached"].shape == r["per_batch"].shape == r["repeated"].shape == r["oracle"].shape == (n, 1) and n > 0
    for name in ("per_batch", "repeated", "oracle"):  # the figures, before anything is asserted
        print(f"cached vs {name}: max abs diff {np.abs(r['cached'].astype(np.float64) - r[name]).max():.3e}")
    assert_close(r["cached"], r["per_batch"], rtol=0, atol=2e-6, what="article cache vs per-batch")
    assert_close(r["cached"], r["repeated"], rtol=0, atol=2e-6, what="article cache vs repeated-history layout")
    assert_close(r["cached"], r["oracle"], rtol=1e-4, atol=1e-6, what="article cache vs float64 oracle")
    np.testing.assert_array_equal(r["cached"], r["again"])  # deterministic
    assert np.ptp(r["cached"]) > 1e-3  # the scores are not all alike: the comparisons above compare something


def test_lstur_cached_scores_equal_per_batch_repeated_and_oracle(hip, lstur_runs):
    _check_runs(lstur_runs)


def test_naml_cached_scores_equal_per_batch_repeated_and_oracle(hip, naml_runs):
    _check_runs(naml_runs)


def _count_calls(monkeypatch, hip):
    counts = {}
    real = hip.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(hip, "call", counting)
    return counts


def _predict_without_cache(model, loader):
    model.scorer.cache_articles = False
    try:
        return model.scorer.predict(loader)
    finally:
        model.scorer.cache_articles = True


@pytest.mark.parametrize("user_type", ["ini", "con"])
def test_lstur_predict_encodes_the_catalogue_once(hip, frames, monkeypatch, user_type):  # noqa: F811
    model, loader, _Pw, _hp, _V = _lstur_case("synthetic", user_type, frames)
    assert len(loader) >= 3
    counts = _count_calls(monkeypatch, hip)
    model.scorer.predict(loader)
    assert counts["ebn_conv1d_fwd_f32"] == 1  # one catalogue chunk, whatever the number of batches
    assert counts["ebn_gru_infer_indexed_f32"] == len(loader) and "ebn_gru_fwd_f32" not in counts
    counts.clear()
    _predict_without_cache(model, loader)
    assert counts["ebn_conv1d_fwd_f32"] == len(loader) and "ebn_gru_infer_indexed_f32" not in counts
    # chunks: one Conv1D launch per chunk, the same vectors
    tokens = np.asarray(loader.lookup_article_matrix)
    whole = model._engine.encode_catalogue(tokens)
    counts.clear()
    parts = model._engine.encode_catalogue(tokens, chunk=16)
    assert counts["ebn_conv1d_fwd_f32"] == -(-len(tokens) // 16) > 1
    assert_close(host(parts.news_all), host(whole.news_all), rtol=1e-5, atol=1e-6, what="chunked catalogue")
    assert torch.equal(parts.live, whole.live) and int(whole.live[0]) == 0  # row 0: the unknown article, a masked step


def test_naml_predict_encodes_the_catalogue_once(hip, frames, monkeypatch):  # noqa: F811
    model, loader, _Pw, _hp, _V = _naml_case("synthetic", frames)
    assert len(loader) >= 3
    counts = _count_calls(monkeypatch, hip)
    model.scorer.predict(loader)
    assert counts["ebn_conv1d_fwd_f32"] == 2  # one catalogue chunk x (title, body), whatever the number of batches
    assert counts["ebn_indexed_attpool_score_f32"] == len(loader) and counts["ebn_att_logit_rows_f32"] == 1
    assert counts["ebn_attpool_fwd_f32"] == 2  # the title and body poolings only: no user pooling launch per batch
    counts.clear()
    _predict_without_cache(model, loader)
    assert counts["ebn_conv1d_fwd_f32"] == 2 * len(loader) and "ebn_indexed_attpool_score_f32" not in counts
    t_rows, b_rows, vert, subvert = loader.article_catalogue()
    cat = (np.asarray(loader.lookup_article_matrix)[t_rows], np.asarray(loader.lookup_article_matrix_body)[b_rows], vert, subvert)
    whole = model._engine.encode_catalogue(*cat)
    counts.clear()
    parts = model._engine.encode_catalogue(*cat, chunk=16)
    assert counts["ebn_conv1d_fwd_f32"] == 2 * -(-len(t_rows) // 16) > 2
    assert_close(host(parts.news_all), host(whole.news_all), rtol=1e-5, atol=1e-6, what="chunked catalogue")
    assert_close(host(parts.a_all), host(whole.a_all), rtol=1e-5, atol=1e-6, what="chunked catalogue logits")


def test_nrms_predict_keeps_its_launches(hip, monkeypatch):
    """NRMS goes through its own hooks: none of the new entry points appears in its cached predict."""
    from ebrec.models.newsrec import NRMSModel
    from ebrec.models.newsrec.dataloader import NRMSDataLoader
    from tests.test_nrms_model import make_hp

    hp = make_hp(history_size=6, title_size=8)
    rng = np.random.default_rng(43)
    mapping = {int(a): rng.integers(1, 150, 8).tolist() for a in ART_IDS}
    loader = NRMSDataLoader(behaviors=_synthetic_behaviors(rng, ART_IDS, 6), article_dict=mapping, history_column="article_id_fixed",
                            unknown_representation="zeros", eval_mode=True, batch_size=16)
    m = NRMSModel(hp, word2vec_embedding=rng.standard_normal((150, 32)).astype(np.float32), seed=3)
    counts = _count_calls(monkeypatch, hip)
    m.scorer.predict(loader)
    assert counts["ebn_pair_score_f32"] == len(loader) and counts["ebn_gather_rows_f32"] >= len(loader)
    assert not {"ebn_gru_infer_indexed_f32", "ebn_att_logit_rows_f32", "ebn_indexed_attpool_score_f32"} & set(counts)


@pytest.mark.parametrize("which", ["lstur-ini", "lstur-con", "naml"])
def test_weights_changed_by_a_train_step_change_the_cached_scores(hip, frames, which):  # noqa: F811
    """No stale cache survives on the model: after optimizer steps the cached predict follows the new weights."""
    if which == "naml":
        model, loader, _Pw, hp, V = _naml_case("synthetic", frames)
    else:
        model, loader, _Pw, hp, V = _lstur_case("synthetic", which[-3:], frames)
    rng = np.random.default_rng(1)
    B, C, H, T = 6, 3, hp.history_size, hp.title_size
    y = np.zeros((B, C), np.int8)
    y[:, 0] = 1
    if which == "naml":
        Tb = hp.body_size
        xs = (rng.integers(1, V, (B, H, T)), rng.integers(1, V, (B, H, Tb)), rng.integers(0, hp.vert_num, (B, H, 1)),
              rng.integers(0, hp.subvert_num, (B, H, 1)), rng.integers(1, V, (B, C, T)), rng.integers(1, V, (B, C, Tb)),
              rng.integers(0, hp.vert_num, (B, C, 1)), rng.integers(0, hp.subvert_num, (B, C, 1)))
    else:
        xs = (rng.integers(0, 5, (B, 1)), rng.integers(1, V, (B, H, T)), rng.integers(1, V, (B, C, T)))
    before = model.scorer.predict(loader)
    for _ in range(3):
        model.train_step(*xs, y)
    after = model.scorer.predict(loader)
    assert np.abs(after - before).max() > 1e-5
    assert_close(after, _predict_without_cache(model, loader), rtol=0, atol=2e-6, what="cached scores after train steps vs per-batch")


def _raises_on_both_paths(model, loader, match):
    for cache in (True, False):
        model.scorer.cache_articles = cache
        try:
            with pytest.raises(IndexError, match=match):
                model.scorer.predict(loader)
        finally:
            model.scorer.cache_articles = True


def test_out_of_range_ids_in_the_catalogue_raise_like_the_per_batch_path(hip, frames):  # noqa: F811
    from ebrec.models.newsrec.dataloader import LSTURDataLoader, NAMLDataLoader

    rng = np.random.default_rng(4)
    model, _loader, _Pw, hp, V = _lstur_case("synthetic", "ini", frames)
    df = _synthetic_behaviors(rng, ART_IDS, hp.history_size)
    df.loc[0, "article_ids_inview"][0] = 500  # the bad article is in the first batch
    mapping = {int(a): rng.integers(1, V, hp.title_size).tolist() for a in ART_IDS}
    mapping[500][2] = V  # one past the table
    bad = LSTURDataLoader(behaviors=df, article_dict=mapping, user_id_mapping={}, history_column="article_id_fixed",
                          unknown_representation="zeros", eval_mode=True, batch_size=16)
    _raises_on_both_paths(model, bad, "token id")

    model, _loader, _Pw, hp, V = _naml_case("synthetic", frames)
    titles = {int(a): rng.integers(1, V, hp.title_size).tolist() for a in ART_IDS}
    bodies = {int(a): rng.integers(1, V, hp.body_size).tolist() for a in ART_IDS}
    mk = lambda t=titles, b=bodies, c={500: 1}: NAMLDataLoader(
        behaviors=df, article_dict=t, body_mapping=b, category_mapping=c, subcategory_mapping={}, unknown_representation="zeros",
        history_column="article_id_fixed", eval_mode=True, batch_size=16)
    _raises_on_both_paths(model, mk(c={500: hp.vert_num + 3}), "category id")
    bad_body = dict(bodies)
    bad_body[500] = [V] + bodies[500][1:]
    _raises_on_both_paths(model, mk(b=bad_body), "token id")
    assert np.isfinite(model.scorer.predict(mk())).all()  # the flags were reset: scoring goes on
