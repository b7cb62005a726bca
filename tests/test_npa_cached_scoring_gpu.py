"""Scoring NPA from a once-encoded article catalogue: the indexed personalised pooling (+ fused score) and the bias+tanh row kernel
through the C ABI (bit-equal to ebn_pap_fwd_f32 on the gathered rows, against float64 numpy, rows outside the catalogue, offsets
past 4 GiB, argument checks) and scorer.predict with the cache against the per-batch path, the repeated-history layout and the
float64 oracle."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from tests import npa_oracle as npo
from tests.guarded import guard_in
from tests.hip_testutil import P, S, assert_close, dev, host
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)
from tests.test_npa_gpu import _model, _params, hp_small

pytestmark = pytest.mark.gpu
f0 = ctypes.c_float(0.0)
N_ROWS = 41


def idev(a, dtype=torch.int32):
    return dev(np.asarray(a), dtype)


# ---------------------------------------------------------------------------------------------- the kernels
def _catalogue(rng, n_rows, L, F, A):
    """pre-activations U = Vd.Wa of O(1) and conv outputs Vd >= 0 of n_rows titles, the pooling's bias, and 7 query rows"""
    U = rng.uniform(-2, 2, (n_rows, L, A)).astype(np.float32)
    V = rng.uniform(0, 1, (n_rows, L, F)).astype(np.float32)
    ba = rng.uniform(-0.1, 0.1, A).astype(np.float32)
    Q = rng.uniform(-1, 1, (7, A)).astype(np.float32)
    return U, V, ba, Q


def _tanh_rows(hip, U_pre, ba_d):
    """the catalogue's Ua from the pre-activations, by the new row kernel (on a copy)"""
    Ua = U_pre.clone()
    hip.call("ebn_bias_tanh_rows_f32", P(Ua), P(ba_d), Ua.shape[0] * Ua.shape[1], Ua.shape[2], S())
    return Ua


def _indexed(hip, Ua, Vd, n_rows, rows, Q, q_idx, users=None, mode=0, want_out=True, want_scores=False):
    n_seq, (L, F), A = len(rows), Vd.shape[1:], Ua.shape[2]
    out = torch.full((n_seq, F), float("nan"), device="cuda") if want_out else None
    scores = torch.full((n_seq,), float("nan"), device="cuda") if want_scores else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.call("ebn_pap_indexed_f32", P(Ua), P(Vd), n_rows, P(idev(rows)), P(Q), P(idev(q_idx)), Q.shape[0], P(out), P(users), P(scores),
             mode, P(flag), n_seq, L, F, A, S())
    torch.cuda.synchronize()
    return out, scores, int(flag.item())


@pytest.mark.parametrize("L,F,A", [(1, 4, 1), (9, 32, 24), (30, 400, 200), (50, 36, 50), (256, 8, 7), (50, 36, 200)])
def test_indexed_pooling_is_bit_equal_to_pap_fwd_on_the_gathered_rows(hip, L, F, A):
    """Same operations in the same order: with the catalogue's Ua made by the bias+tanh row kernel, out equals ebn_pap_fwd_f32's on
    the gathered pre-activations and conv outputs bit for bit, and so does the tanh that kernel leaves in U.  A % 4 != 0 takes the
    direct reads, A % 4 == 0 the LDS-staged ones ((50, 36, 200): in two passes)."""
    rng = np.random.default_rng(L * 1000 + F + A)
    U, V, ba, Q = _catalogue(rng, N_ROWS, L, F, A)
    n_seq, n_q = 77, Q.shape[0]
    rows = rng.integers(0, N_ROWS, n_seq)
    rows[:6] = [5, 5, 5, 0, N_ROWS - 1, 5]      # one row under several queries
    q_idx = rng.integers(0, n_q, n_seq)
    q_idx[:3] = [0, 3, 6]
    q_idx[10] = n_q + 2                          # outside [0, n_q): reads row 0
    Ud, Vd, bad, Qd = dev(U), dev(V), dev(ba), dev(Q)
    flat = torch.from_numpy(rows).cuda()
    Ug, Vg = Ud[flat].contiguous(), Vd[flat].contiguous()
    out_ref, w = torch.empty(n_seq, F, device="cuda"), torch.empty(n_seq * L, device="cuda")
    hip.call("ebn_pap_fwd_f32", P(Ug), P(bad), P(Qd), P(idev(q_idx)), n_q, P(Vg), P(out_ref), P(w), None, 0, n_seq, L, F, A, None, -1,
             f0, S())
    Ua = _tanh_rows(hip, Ud, bad)
    out, _s, flag = _indexed(hip, Ua, Vd, N_ROWS, rows, Qd, q_idx)
    assert flag == 0
    assert torch.equal(Ua[flat], Ug), "the row kernel's tanh differs from the bits pap_fwd leaves in U"
    assert torch.equal(out, out_ref), f"max abs diff {float((out - out_ref).abs().max()):.3e}"
    q0 = q_idx.copy()
    q0[10] = 0
    assert torch.equal(_indexed(hip, Ua, Vd, N_ROWS, rows, Qd, q0)[0][10], out[10])
    assert torch.equal(Ud, dev(U)) and torch.equal(Vd, dev(V))  # nothing in place


def _ref64(U, V, ba, Q, rows, q_idx, users, sigmoid):
    Ua = np.tanh(U.astype(np.float64) + ba)[rows]
    s = np.einsum("nla,na->nl", Ua, Q.astype(np.float64)[q_idx])
    w = np.exp(s - s.max(1, keepdims=True))
    w /= w.sum(1, keepdims=True)
    out = np.einsum("nl,nlf->nf", w, V.astype(np.float64)[rows])
    d = np.einsum("nf,nf->n", out, users.astype(np.float64)[q_idx])
    return out, (1.0 / (1.0 + np.exp(-d)) if sigmoid else d)


@pytest.mark.parametrize("L", [30, 20, 50])
def test_indexed_pooling_and_scores_vs_float64(hip, L):
    """The shape and the tolerances of test_pap_fwd_bwd_vs_float64 (out: rtol 1e-4, atol 1e-6; the scores take the same), the three
    call forms, the catalogues between NaN guards.  User vectors of O(1/sqrt(F)) entries: scores of both signs."""
    rng = np.random.default_rng(L)
    F, A, n_seq = 400, 200, 23
    U, V, ba, Q = _catalogue(rng, N_ROWS, L, F, A)
    users = (rng.uniform(-1, 1, (Q.shape[0], F)) / np.sqrt(F)).astype(np.float32)
    rows, q_idx = rng.integers(0, N_ROWS, n_seq), rng.integers(0, Q.shape[0], n_seq)
    bad, Qd, usd = dev(ba), dev(Q), dev(users)
    Ua_plain = _tanh_rows(hip, dev(U), bad)
    assert_close(host(Ua_plain), np.tanh(U.astype(np.float64) + ba), rtol=1e-5, atol=1e-6, what="tanh(U + ba)")
    Ua, hU = guard_in(Ua_plain.cpu().numpy().reshape(N_ROWS * L, A))
    Vd, hV = guard_in(V.reshape(N_ROWS * L, F))
    Ua, Vd = Ua.view(N_ROWS, L, A), Vd.view(N_ROWS, L, F)
    for mode, want_out, want_scores in ((0, True, False), (1, False, True), (0, True, True), (1, True, True)):
        out, scores, flag = _indexed(hip, Ua, Vd, N_ROWS, rows, Qd, q_idx, usd, mode, want_out, want_scores)
        ref_out, ref_scores = _ref64(U, V, ba, Q, rows, q_idx, users, sigmoid=mode == 1)
        assert flag == 0
        if want_out:
            assert_close(host(out), ref_out, rtol=1e-4, atol=1e-6, what="out")
        if want_scores:
            assert bool(torch.isfinite(scores).all())
            assert_close(host(scores), ref_scores, rtol=1e-4, atol=1e-6, what=f"scores (mode {mode})")
    assert np.ptp(ref_scores) > 1e-2
    hU.check("Ua_all")
    hV.check("Vd_all")


def test_rows_outside_the_catalogue_are_flagged_and_never_read(hip):
    rng = np.random.default_rng(8)
    L, F, A, n_seq = 9, 32, 24, 29
    U, V, ba, Q = _catalogue(rng, N_ROWS, L, F, A)
    users = (rng.uniform(-1, 1, (Q.shape[0], F)) / np.sqrt(F)).astype(np.float32)
    Qd, usd = dev(Q), dev(users)
    Ua, _h = guard_in(_tanh_rows(hip, dev(U), dev(ba)).cpu().numpy().reshape(N_ROWS * L, A))
    Vd, _h2 = guard_in(V.reshape(N_ROWS * L, F))
    Ua, Vd = Ua.view(N_ROWS, L, A), Vd.view(N_ROWS, L, F)
    rows, q_idx = rng.integers(0, N_ROWS, n_seq), rng.integers(0, Q.shape[0], n_seq)
    bad_rows = rows.copy()
    where = [2, 11, 28]
    bad_rows[where] = [-1, N_ROWS, N_ROWS + 1]
    for mode, act0 in ((1, 0.5), (0, 0.0)):
        out0, s0, flag0 = _indexed(hip, Ua, Vd, N_ROWS, rows, Qd, q_idx, usd, mode, True, True)
        out1, s1, flag1 = _indexed(hip, Ua, Vd, N_ROWS, bad_rows, Qd, q_idx, usd, mode, True, True)
        assert flag0 == 0 and flag1 == 1
        keep = torch.ones(n_seq, dtype=torch.bool, device="cuda")
        keep[where] = False
        assert torch.equal(out1[keep], out0[keep]) and torch.equal(s1[keep], s0[keep])
        assert bool((out1[~keep] == 0).all()) and bool((s1[~keep] == act0).all())
        assert bool(torch.isfinite(out1).all()) and bool(torch.isfinite(s1).all())
    # scores alone, no flag pointer: the same scores
    s2 = torch.full((n_seq,), float("nan"), device="cuda")
    hip.call("ebn_pap_indexed_f32", P(Ua), P(Vd), N_ROWS, P(idev(bad_rows)), P(Qd), P(idev(q_idx)), Q.shape[0], None, P(usd), P(s2), 0,
             None, n_seq, L, F, A, S())
    torch.cuda.synchronize()
    assert torch.equal(s2, s1)


def test_catalogue_offsets_past_4_gib(hip):
    """Vd_all of 1100 x 256 x 4096 floats (4.6 GB, left uninitialised): row 1099 starts 4.6e9 bytes in.  Rows 0, 1 and 1099 pool to
    the bits of the same three rows in a 3-row catalogue."""
    n_rows, L, F, A = 1100, 256, 4096, 8
    try:
        Vd_all = torch.empty(n_rows, L, F, device="cuda")
    except RuntimeError as e:  # torch.cuda.OutOfMemoryError is a RuntimeError
        pytest.skip(f"no room for the 4.6 GB catalogue: {e}")
    rng = np.random.default_rng(5)
    U, V, ba, Q = _catalogue(rng, 3, L, F, A)
    Ua3, V3, Qd = _tanh_rows(hip, dev(U), dev(ba)), dev(V), dev(Q)
    Ua_all = torch.empty(n_rows, L, A, device="cuda")
    big = [0, 1, n_rows - 1]
    for j, r in enumerate(big):
        Vd_all[r].copy_(V3[j])
        Ua_all[r].copy_(Ua3[j])
    assert (n_rows - 1) * L * F * 4 > 2 ** 32
    q_idx = [2, 5, 1, 4]
    small, _s, flag_s = _indexed(hip, Ua3, V3, 3, [2, 0, 1, 2], Qd, q_idx)
    got, _s, flag = _indexed(hip, Ua_all, Vd_all, n_rows, [big[2], big[0], big[1], big[2]], Qd, q_idx)
    assert flag == 0 and flag_s == 0
    assert bool(torch.isfinite(small).all()) and float(small.abs().max()) > 0
    assert torch.equal(got, small)
    del Vd_all


def test_indexed_pooling_argument_checks(hip):
    rng = np.random.default_rng(2)
    L, F, A, n_seq = 9, 32, 24, 5
    U, V, ba, Q = _catalogue(rng, N_ROWS, L, F, A)
    Ua, Vd, Qd = _tanh_rows(hip, dev(U), dev(ba)), dev(V), dev(Q)
    users = dev(rng.uniform(-1, 1, (Q.shape[0], F)).astype(np.float32))
    rows, q_idx = idev(rng.integers(0, N_ROWS, n_seq)), idev(rng.integers(0, Q.shape[0], n_seq))
    out, scores = torch.empty(n_seq + 1, F, device="cuda"), torch.empty(n_seq, device="cuda")
    fn = hip.lib().ebn_pap_indexed_f32
    base = dict(Ua=P(Ua), Vd=P(Vd), n_rows=N_ROWS, rows=P(rows), Q=P(Qd), q_idx=P(q_idx), n_q=Q.shape[0], out=P(out), users=P(users),
                scores=P(scores), mode=1, flag=None, n_seq=n_seq, L=L, F=F, A=A, stream=S())
    rc = lambda **kw: fn(*[kw.get(k, v) for k, v in base.items()])
    assert rc() == 0
    for bad in (dict(Ua=None), dict(Vd=None), dict(rows=None), dict(Q=None), dict(q_idx=None), dict(n_seq=-1), dict(n_rows=-1),
                dict(L=0), dict(F=0), dict(A=0), dict(n_q=0), dict(out=None, scores=None), dict(users=None), dict(mode=2), dict(mode=-1)):
        assert rc(**bad) == -1, bad                        # EBN_ERR_BAD_ARG
    for bad in (dict(L=257), dict(F=4100), dict(F=30)):
        assert rc(**bad) == -2, bad                        # EBN_ERR_UNSUPPORTED
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    for bad in (dict(Ua=off(Ua)), dict(Vd=off(Vd)), dict(out=off(out))):
        assert rc(**bad) == -3, bad                        # EBN_ERR_ALIGN
    assert rc(n_seq=0) == 0 and rc(users=None, scores=None) == 0 and rc(out=None) == 0
    tanh = hip.lib().ebn_bias_tanh_rows_f32
    assert tanh(None, None, 0, A, S()) == 0 and tanh(None, P(Ua), 3, A, S()) == -1 and tanh(P(Ua), P(Ua), -1, A, S()) == -1
    assert tanh(P(Ua), P(Ua), 3, 0, S()) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the whole model
def _synthetic_behaviors(rng, art_ids, H, n=50):
    inview = [rng.choice(np.append(art_ids, 7), int(rng.integers(1, 9))).tolist() for _ in range(n)]
    return pd.DataFrame({"user_id": rng.integers(0, 9, n), "article_id_fixed": [rng.choice(np.append(art_ids, 0), H).tolist() for _ in range(n)],
                         "article_ids_inview": inview, "labels": [[0] * len(v) for v in inview]})


ART_IDS = np.arange(500, 540)


def _npa_case(kind, frames):  # noqa: F811
    """(model with random weights, eval loader, float64 weights, hparams, vocabulary size): 40 articles, 50 impressions in batches
    of 16, articles and users outside the mappings among them"""
    from ebrec.models.newsrec.dataloader import LSTURDataLoader
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_USER_COL

    rng = np.random.default_rng(43)
    if kind == "synthetic":
        hp, V = hp_small, 150
        mapping = {int(a): rng.integers(1, V, hp.title_size).tolist() for a in ART_IDS}
        loader = LSTURDataLoader(behaviors=_synthetic_behaviors(rng, ART_IDS, hp.history_size), article_dict=mapping,
                                 user_id_mapping={u: u + 1 for u in range(7)}, history_column="article_id_fixed",
                                 unknown_representation="zeros", eval_mode=True, batch_size=16)
    else:
        beh, _train, mapping = frames
        users = sorted(pd.unique(beh[DEFAULT_USER_COL]))
        hp = type("hp", (hp_small,), {"title_size": 10, "history_size": 3, "n_users": len(users)})
        V = 20
        loader = LSTURDataLoader(behaviors=beh.iloc[:40].reset_index(drop=True), article_dict=mapping,
                                 user_id_mapping={u: i + 1 for i, u in enumerate(users[:-3])}, unknown_representation="zeros",
                                 history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=16, eval_mode=True)
    Pw = _params(hp, V, 16, seed=3)
    return _model(hp, V, 16, 5, Pw), loader, Pw, hp, V


def _predict_without_cache(model, loader):
    model.scorer.cache_articles = False
    try:
        return model.scorer.predict(loader)
    finally:
        model.scorer.cache_articles = True


@pytest.fixture(scope="module", params=["synthetic", "fixture"])
def npa_runs(request, frames):  # noqa: F811
    model, loader, Pw, _hp, _V = _npa_case(request.param, frames)
    assert model.scorer.cache_articles is True  # the cached path is the default
    out = dict(loader=loader, cached=model.scorer.predict(loader), again=model.scorer.predict(loader),
               per_batch=_predict_without_cache(model, loader),
               repeated=np.concatenate([model.scorer.predict(loader[i][0]) for i in range(len(loader))]))
    out["oracle"] = np.concatenate([npo.scorer_forward(u, h, p, Pw).reshape(-1, 1) for (u, h, p), _y in (loader[i] for i in range(len(loader)))])
    return out


def test_npa_cached_scores_equal_per_batch_repeated_and_oracle(hip, npa_runs):
    r = npa_runs
    n = sum(len(r["loader"].index_eval_batch(i)[1]) for i in range(len(r["loader"])))
    assert r["cached"].shape == r["per_batch"].shape == r["repeated"].shape == r["oracle"].shape == (n, 1) and n > 0
    for name in ("per_batch", "repeated", "oracle"):  # the figures, before anything is asserted
        print(f"cached vs {name}: max abs diff {np.abs(r['cached'].astype(np.float64) - r[name]).max():.3e}")
    assert_close(r["cached"], r["per_batch"], rtol=0, atol=2e-6, what="article cache vs per-batch")
    assert_close(r["cached"], r["repeated"], rtol=0, atol=2e-6, what="article cache vs repeated-history layout")
    assert_close(r["cached"], r["oracle"], rtol=1e-4, atol=1e-6, what="article cache vs float64 oracle")
    np.testing.assert_array_equal(r["cached"], r["again"])  # deterministic
    assert np.ptp(r["cached"]) > 1e-3  # the scores are not all alike: the comparisons above compare something


def _count_calls(monkeypatch, hip):
    counts = {}
    real = hip.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(hip, "call", counting)
    return counts


def test_npa_predict_encodes_the_catalogue_once(hip, frames, monkeypatch):  # noqa: F811
    model, loader, _Pw, hp, _V = _npa_case("synthetic", frames)
    assert len(loader) >= 3
    counts = _count_calls(monkeypatch, hip)
    model.scorer.predict(loader)
    assert counts["ebn_conv1d_fwd_f32"] == 1  # one catalogue chunk, whatever the number of batches
    assert counts["ebn_pap_indexed_f32"] == 2 * len(loader) and counts["ebn_bias_tanh_rows_f32"] == 1
    assert counts["ebn_pap_fwd_f32"] == len(loader)  # the user stage only
    counts.clear()
    _predict_without_cache(model, loader)
    assert counts["ebn_conv1d_fwd_f32"] == len(loader) and "ebn_pap_indexed_f32" not in counts
    # chunks: one Conv1D launch per chunk, the same arrays
    tokens = np.asarray(loader.lookup_article_matrix)
    whole = model._engine.encode_catalogue(tokens)
    counts.clear()
    parts = model._engine.encode_catalogue(tokens, chunk=16)
    assert counts["ebn_conv1d_fwd_f32"] == -(-len(tokens) // 16) > 1
    assert tuple(whole.Vd_all.shape) == (len(tokens), hp.title_size, hp.filter_num)
    assert tuple(whole.Ua_all.shape) == (len(tokens), hp.title_size, hp.attention_hidden_dim)
    assert_close(host(parts.Vd_all), host(whole.Vd_all), rtol=1e-5, atol=1e-6, what="chunked catalogue Vd")
    assert_close(host(parts.Ua_all), host(whole.Ua_all), rtol=1e-5, atol=1e-6, what="chunked catalogue Ua")
    assert float(whole.Vd_all[0].abs().max()) > 0  # row 0, the unknown article, is a title like any other: NPA has no masking


def test_budget_below_the_catalogue_falls_back_to_the_per_batch_path(hip, frames, monkeypatch):  # noqa: F811
    model, loader, _Pw, _hp, _V = _npa_case("synthetic", frames)
    want = _predict_without_cache(model, loader)
    assert type(model).catalogue_max_bytes == 16 * 2 ** 30
    model.catalogue_max_bytes = 1
    counts = _count_calls(monkeypatch, hip)
    got = model.scorer.predict(loader)
    assert "ebn_pap_indexed_f32" not in counts and counts["ebn_conv1d_fwd_f32"] == len(loader)
    np.testing.assert_array_equal(got, want)


def test_weights_changed_by_train_steps_change_the_cached_scores(hip, frames):  # noqa: F811
    """No stale cache survives on the model: after optimizer steps the cached predict follows the new weights."""
    model, loader, _Pw, hp, V = _npa_case("synthetic", frames)
    rng = np.random.default_rng(1)
    B, C, H, T = 6, 3, hp.history_size, hp.title_size
    y = np.zeros((B, C), np.int8)
    y[:, 0] = 1
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


def test_out_of_range_ids_raise_like_the_per_batch_path(hip, frames):  # noqa: F811
    from ebrec.models.newsrec.dataloader import LSTURDataLoader

    rng = np.random.default_rng(4)
    model, clean, _Pw, hp, V = _npa_case("synthetic", frames)
    df = _synthetic_behaviors(rng, ART_IDS, hp.history_size)
    df.loc[0, "article_ids_inview"][0] = 500  # the bad article is in the first batch
    mapping = {int(a): rng.integers(1, V, hp.title_size).tolist() for a in ART_IDS}
    mk = lambda m, umap: LSTURDataLoader(behaviors=df, article_dict=m, user_id_mapping=umap, history_column="article_id_fixed",
                                         unknown_representation="zeros", eval_mode=True, batch_size=16)
    bad_title = {k: list(v) for k, v in mapping.items()}
    bad_title[500][2] = V  # one past the table
    _raises_on_both_paths(model, mk(bad_title, {}), "token id")
    _raises_on_both_paths(model, mk(mapping, {u: hp.n_users + 1 for u in range(9)}), "user index")
    assert np.isfinite(model.scorer.predict(mk(mapping, {}))).all()  # the flags were reset: scoring goes on
    assert np.isfinite(model.scorer.predict(clean)).all()
