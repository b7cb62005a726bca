"""NAML on the MI355X: the categorical-view and view-attention kernels against float64, one training step of NAMLModel against
the float64 oracle (tests/naml_oracle.py), determinism, and fit / evaluate / scorer / save / load on the fixture parquets."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nrms_numpy as on
from tests import naml_oracle as nao
from tests.hip_testutil import P, S, assert_close, dev, host
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture of the reference loader test)

pytestmark = pytest.mark.gpu

SEED = 21
f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)


@pytest.mark.parametrize("K0,K1,F", [(10, 12, 400), (12, 10, 24)])
def test_catview_fwd_bwd_vs_float64(hip, K0, K1, F):
    rng = np.random.default_rng(K0 * 100 + F)
    N, r0, r1 = 45, 7, 13  # N is not a multiple of the 16- / 32-article tiles; the two views have different tables
    ids0, ids1 = rng.integers(0, r0, N), rng.integers(0, r1, N)
    ids0[:6] = 3  # duplicate ids: their table gradients add up
    ids1[20:30] = 5
    ids0[10], ids0[11] = r0, -1  # out of range: a zero row and the flag
    t0, t1 = rng.uniform(-0.5, 0.5, (r0, K0)).astype(np.float32), rng.uniform(-0.5, 0.5, (r1, K1)).astype(np.float32)
    Wb0, Wb1 = rng.uniform(-0.5, 0.5, (K0 + 1, F)).astype(np.float32), rng.uniform(-0.5, 0.5, (K1 + 1, F)).astype(np.float32)
    dout0, dout1 = rng.normal(size=(N, F)).astype(np.float32), rng.normal(size=(N, F)).astype(np.float32)
    d = {k: dev(v) for k, v in dict(t0=t0, t1=t1, Wb0=Wb0, Wb1=Wb1, dout0=dout0, dout1=dout1).items()}
    i0, i1 = dev(ids0, torch.int32), dev(ids1, torch.int32)
    out0, out1 = torch.empty(N, F, device="cuda"), torch.empty(N, F, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.call("ebn_naml_catview_fwd_f32", P(i0), P(d["t0"]), r0, K0, P(d["Wb0"]), P(out0), P(i1), P(d["t1"]), r1, K1, P(d["Wb1"]),
             P(out1), N, F, P(flag), S())
    torch.cuda.synchronize()
    assert int(flag.item()) == 1
    grads = []
    for rep in range(2):
        part = torch.empty(int(hip.lib().ebn_naml_catview_partials_len(N, K0, K1, F)), device="cuda")
        g = [torch.full((K0 + 1, F), 7.0, device="cuda"), torch.full((r0, K0), 7.0, device="cuda"),
             torch.full((K1 + 1, F), 7.0, device="cuda"), torch.full((r1, K1), 7.0, device="cuda")]
        hip.call("ebn_naml_catview_bwd_f32", P(i0), P(d["t0"]), r0, K0, P(d["Wb0"]), P(out0), P(d["dout0"]), P(g[0]), P(g[1]), P(i1),
                 P(d["t1"]), r1, K1, P(d["Wb1"]), P(out1), P(d["dout1"]), P(g[2]), P(g[3]), P(part), part.numel(), N, F, S())
        torch.cuda.synchronize()
        grads.append([host(x) for x in g])
    for a, b in zip(*grads):
        np.testing.assert_array_equal(a, b)  # fixed summation orders: the same bits twice
    for ids, tab, Wb, out, dout, (dWb, dtab), rows in ((ids0, t0, Wb0, out0, dout0, grads[0][:2], r0),
                                                      (ids1, t1, Wb1, out1, dout1, grads[0][2:], r1)):
        K = tab.shape[1]
        ok = (ids >= 0) & (ids < rows)
        e = np.where(ok[:, None], tab.astype(np.float64)[np.clip(ids, 0, rows - 1)], 0.0)
        pre = e @ Wb[:K].astype(np.float64) + Wb[K]
        got = host(out)
        assert_close(got, np.maximum(pre, 0), rtol=1e-5, atol=1e-6, what="catview forward")
        assert (got[~ok] == np.maximum(Wb[K], 0)).all()  # an out-of-range id reads a zero row
        dY = dout.astype(np.float64) * (got > 0)  # the gate the kernel reads back from its output
        want_W = np.concatenate([e.T @ dY, dY.sum(0, keepdims=True)])
        assert_close(dWb, want_W, rtol=1e-5, atol=1e-5, what="catview dW / db")
        de = dY @ Wb[:K].astype(np.float64).T
        want_t = np.zeros((rows, K))
        for n in np.nonzero(ok)[0]:
            want_t[ids[n]] += de[n]
        assert_close(dtab, want_t, rtol=1e-5, atol=1e-5, what="catview table gradient")


@pytest.mark.parametrize("nv", [2, 4])
def test_viewatt_fwd_bwd_vs_float64(hip, nv):
    rng = np.random.default_rng(nv)
    N, F, A = 37, 400, 200
    Vw = rng.uniform(-1, 1, (nv, N, F)).astype(np.float32)
    Wa = (rng.uniform(-1, 1, (F, A)) * np.sqrt(6.0 / (F + A))).astype(np.float32)
    b, q = rng.uniform(-0.1, 0.1, A).astype(np.float32), rng.uniform(-0.3, 0.3, A).astype(np.float32)
    dnews = rng.normal(size=(N, F)).astype(np.float32)
    Vd, Wd, bd, qd, dn = dev(Vw), dev(Wa), dev(b), dev(q), dev(dnews)
    R = nv * N
    U, w, news = torch.empty(R, A, device="cuda"), torch.empty(R, device="cuda"), torch.empty(N, F, device="cuda")
    hip.call("ebn_gemm_f32", 0, 0, R, A, F, f1, P(Vd), F, P(Wd), A, f0, P(U), A, S())
    hip.call("ebn_naml_viewatt_fwd_f32", P(U), P(bd), P(qd), P(Vd), P(w), P(news), N, nv, F, A, S())
    dVw, de = torch.empty(nv, N, F, device="cuda"), torch.empty(R, device="cuda")
    hip.call("ebn_naml_viewatt_bwd_f32", P(Vd), P(w), P(dn), P(dVw), P(de), N, nv, F, S())
    part = torch.empty(int(hip.lib().ebn_attpool_partials_len(R, A)), device="cuda")
    dq, db, dWa = torch.empty(A, device="cuda"), torch.empty(A, device="cuda"), torch.empty(F, A, device="cuda")
    hip.call("ebn_attpool_bwd_dpre_f32", P(U), P(qd), P(de), P(dq), P(db), P(part), R, A, 0, S())
    hip.call("ebn_gemm_f32", 1, 0, F, A, R, f1, P(Vd), F, P(U), A, f0, P(dWa), A, S())
    hip.call("ebn_gemm_f32", 0, 1, R, F, A, f1, P(U), A, P(Wd), A, f1, P(dVw), F, S())
    torch.cuda.synchronize()
    x = torch.tensor(Vw.astype(np.float64)).permute(1, 0, 2).contiguous().requires_grad_(True)  # (N, nv, F)
    T = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in dict(W=Wa, b=b, q=q.reshape(A, 1)).items()}
    out, wref = nao.att_layer2(x, T["W"], T["b"], T["q"])
    assert_close(host(news), out.detach().numpy(), rtol=1e-5, atol=1e-6, what="view attention output")
    assert_close(host(w).reshape(nv, N), wref.detach().numpy().T, rtol=1e-5, atol=1e-7, what="view attention weights")
    (out * torch.from_numpy(dnews.astype(np.float64))).sum().backward()
    assert_close(host(dVw), x.grad.numpy().transpose(1, 0, 2), rtol=1e-4, atol=1e-5, what="d(views)")
    assert_close(host(dWa), T["W"].grad.numpy(), rtol=1e-4, atol=1e-5, what="dWa")
    assert_close(host(db), T["b"].grad.numpy(), rtol=1e-4, atol=1e-5, what="db")
    assert_close(host(dq), T["q"].grad.numpy()[:, 0], rtol=1e-4, atol=1e-5, what="dq")


class hp_small:
    title_size, body_size, history_size = 9, 11, 4
    vert_num, vert_emb_dim, subvert_num, subvert_emb_dim = 7, 10, 13, 12
    dense_activation, cnn_activation = "relu", "relu"
    attention_hidden_dim, filter_num, window_size = 24, 32, 3
    optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-3


class hp_c1:
    title_size, body_size, history_size = 30, 40, 20
    vert_num, vert_emb_dim, subvert_num, subvert_emb_dim = 100, 10, 100, 10
    dense_activation, cnn_activation = "relu", "relu"
    attention_hidden_dim, filter_num, window_size = 200, 400, 3
    optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-4


def _params(hp, V, E, seed):
    Pw = nao.random_params(V, E, hp.filter_num, hp.attention_hidden_dim, hp.window_size, hp.vert_num, hp.vert_emb_dim,
                           hp.subvert_num, hp.subvert_emb_dim, seed=seed)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in Pw.items()}


def _model(hp, V, E, seed, Pw=None):
    from ebrec.models.newsrec import NAMLModel

    m = NAMLModel(hp, word2vec_embedding=np.zeros((V, E), np.float32) if Pw is None else Pw["emb"].astype(np.float32), seed=seed)
    if Pw is not None:
        m.model.set_weights([Pw[k] for k in nao.WEIGHT_ORDER])
    return m


def _batch(hp, V, B, C, seed):
    rng = np.random.default_rng(seed)
    H, T, Tb = hp.history_size, hp.title_size, hp.body_size
    ht, hb = rng.integers(1, V, (B, H, T)), rng.integers(1, V, (B, H, Tb))
    ht[:, 0, -3:] = 0  # title padding
    hb[1, 2] = 0       # an empty body
    pt, pb = rng.integers(1, V, (B, C, T)), rng.integers(1, V, (B, C, Tb))
    hv, hs = rng.integers(0, hp.vert_num, (B, H, 1)), rng.integers(0, hp.subvert_num, (B, H, 1))
    pv, ps = rng.integers(0, hp.vert_num, (B, C, 1)), rng.integers(0, hp.subvert_num, (B, C, 1))
    hv[0] = 2  # one category over a whole history: duplicate ids in the batch
    y = np.zeros((B, C), np.int8)
    y[np.arange(B), rng.integers(0, C, B)] = 1
    return (ht, hb, hv, hs, pt, pb, pv, ps), y


@pytest.mark.parametrize("shape,loss,fused", [("small", "cross_entropy_loss", True), ("small", "log_loss", True),
                                              ("small", "cross_entropy_loss", False), ("naml-c1", "cross_entropy_loss", True),
                                              ("naml-c1", "log_loss", True)])
def test_train_step_loss_and_every_gradient_vs_oracle(hip, shape, loss, fused):
    base, V, E, B, C = (hp_small, 97, 16, 6, 3) if shape == "small" else (hp_c1, 32000, 300, 32, 5)
    hp = type("hp", (base,), {"loss": loss})
    Pw = _params(hp, V, E, seed=2)
    model = _model(hp, V, E, seed=SEED, Pw=Pw)
    eng = model._engine
    eng.fuse_user_head = fused
    xs, y = _batch(hp, V, B, C, 3)
    b = eng._stage(eng._arrays(xs[:4], "his"), eng._arrays(xs[4:], "pred"), y)
    eng._grad_kernels(b, C)
    torch.cuda.synchronize()
    loss_dev = float(eng.loss_dev.item())
    scores = host(b.scores).reshape(B, C)
    vd = {"t": host(b.Vt).reshape(b.N, hp.title_size, -1), "b": host(b.Vb).reshape(b.N, hp.body_size, -1)}

    def gate(view, pre):  # ReLU inputs within fp32 rounding of 0 take the engine's decision
        tie = np.abs(pre) <= 3e-6 * np.abs(pre).max()
        return np.where(tie, vd[view] > 0, pre > 0)

    L, _, s, g = nao.naml_loss_and_grads(xs, y, Pw, hp.dropout, on.Drop(hp.dropout, SEED, 1), loss, relu_gate=gate)
    assert abs(loss_dev - L) <= 2e-5 * max(1.0, abs(L)), (loss_dev, L)
    assert np.abs(scores - s).max() <= 1e-4 * max(1.0, np.abs(s).max()), np.abs(scores - s).max()
    pg = eng.params.g
    W, Kv, Ks = hp.window_size, hp.vert_emb_dim, hp.subvert_emb_dim
    got = {"emb": host(eng.table_acc).reshape(V, E) / 2.0 ** 40}
    for key, conv in (("t", "t_conv"), ("b", "b_conv")):
        wb = host(pg(conv))
        got[key + "_conv_W"], got[key + "_conv_b"] = wb[: W * E].reshape(W, E, -1), wb[W * E]
    for key, (aW, ab, aq) in (("t_att", ("t_aW", "t_ab", "t_aq")), ("b_att", ("b_aW", "b_ab", "b_aq")),
                              ("va", ("va_W", "va_b", "va_q")), ("u", ("u_W", "u_b", "u_q"))):
        got[key + "_W"], got[key + "_b"], got[key + "_q"] = host(pg(aW)), host(pg(ab)), host(pg(aq)).reshape(-1, 1)
    for key, K in (("v", Kv), ("s", Ks)):
        wb = host(pg(key + "_Wb"))
        got[key + "_emb"], got[key + "_W"], got[key + "_b"] = host(pg(key + "_emb")), wb[:K], wb[K]
    assert set(got) == set(g) == set(nao.WEIGHT_ORDER)
    for k in sorted(g):
        ref = np.abs(g[k]).max()
        err = np.abs(got[k] - g[k]).max()
        assert err <= 2e-4 * ref + 1e-9, f"{k}: max abs err {err:.3e} vs max |grad| {ref:.3e}"
        assert ref > 0, k
    # rows of the small tables no article names get exactly zero gradient
    used = np.zeros(hp.vert_num, bool)
    used[np.concatenate([xs[2].ravel(), xs[6].ravel()])] = True
    assert (got["v_emb"][~used] == 0).all()


def test_count_params_and_initialisers(hip):
    hp, V, E = hp_small, 50, 16
    m = _model(hp, V, E, seed=3)
    W, F, A, nv, Kv, ns, Ks = hp.window_size, hp.filter_num, hp.attention_hidden_dim, hp.vert_num, hp.vert_emb_dim, hp.subvert_num, hp.subvert_emb_dim
    want = V * E + 2 * (W * E * F + F) + 4 * (F * A + 2 * A) + nv * Kv + ns * Ks + (Kv + Ks) * F + 2 * F
    assert m.model.count_params() == want
    ws = dict(zip(nao.WEIGHT_ORDER, m.model.get_weights()))
    assert sum(w.size for w in ws.values()) == want
    for k in ("t_conv_b", "b_conv_b", "t_att_b", "b_att_b", "va_b", "u_b", "v_b", "s_b"):
        assert (ws[k] == 0).all(), k
    for k in ("v_emb", "s_emb"):
        assert np.abs(ws[k]).max() <= 0.05 and np.abs(ws[k]).max() > 0
    np.testing.assert_array_equal(ws["t_att_W"], ws["u_W"])  # glorot_uniform(seed) of one shape: identical draws


def test_graph_replay_equals_eager_and_runs_are_deterministic(hip):
    hp, V, E, B, C = hp_small, 97, 16, 6, 3
    finals = []
    for use_graph in (True, True, False):
        model = _model(hp, V, E, seed=SEED, Pw=_params(hp, V, E, seed=2))
        model._engine.use_graph = use_graph
        losses = []
        for s in range(3):
            xs, y = _batch(hp, V, B, C, 10 + s)
            losses.append(float(model.train_step(*xs, y).item()))
        torch.cuda.synchronize()
        finals.append((losses, [torch.from_numpy(np.ascontiguousarray(w)) for w in model.model.get_weights()]))
    for losses, ws in finals[1:]:
        assert losses == finals[0][0]
        for a, b in zip(finals[0][1], ws):
            assert torch.equal(a, b)


def test_fit_evaluate_scorer_save_load_and_ranges_on_fixtures(hip, tmp_path, frames):  # noqa: F811
    from ebrec.models.newsrec import NAMLModel
    from ebrec.models.newsrec.dataloader import NAMLDataLoader
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL

    beh, train, mapping = frames
    cats = {a: int(a) % 6 + 1 for j, a in enumerate(sorted(mapping)) if j % 4}
    subcats = {a: int(a) % 9 for a in sorted(mapping)}

    class hp:
        title_size, body_size, history_size = 10, 10, 3
        vert_num, vert_emb_dim, subvert_num, subvert_emb_dim = 8, 10, 9, 6
        dense_activation, cnn_activation = "relu", "relu"
        attention_hidden_dim, filter_num, window_size = 16, 24, 3
        optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-3

    loader = lambda beh_, cm=cats, **kw: NAMLDataLoader(behaviors=beh_, article_dict=mapping, body_mapping=mapping, category_mapping=cm,
                                                       subcategory_mapping=subcats, unknown_representation="zeros",
                                                       history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=16, **kw)
    model = NAMLModel(hp, vocab_size=20, word_emb_dim=16, seed=5, n_users=123)
    tr = loader(train)
    hist = model.model.fit(tr, validation_data=tr, epochs=2, verbose=0)
    losses = hist.history["loss"]
    assert len(losses) == 2 and all(np.isfinite(losses)) and np.isfinite(hist.history["val_loss"]).all()
    ev_loss = model.model.evaluate(tr, verbose=0)
    assert np.all(np.isfinite(np.asarray(ev_loss, dtype=np.float64)))

    ev = loader(beh.iloc[:40].reset_index(drop=True), eval_mode=True)
    got = model.scorer.predict(ev)
    Pw = dict(zip(nao.WEIGHT_ORDER, [w.astype(np.float64) for w in model.model.get_weights()]))
    want = np.concatenate([nao.scorer_forward(xs, Pw).reshape(-1, 1) for xs, _y in (ev[i] for i in range(len(ev)))])
    assert got.shape == want.shape == (int(beh["n"].iloc[:40].sum()), 1)
    assert_close(got, want, rtol=1e-4, atol=1e-6, what="scorer.predict vs sigmoid(cand . user)")
    xs0, _y = ev[0]
    direct = model.scorer(xs0).cpu().numpy()  # the repeated-history layout, without the compact path
    assert_close(direct, got[: len(direct)], rtol=1e-5, atol=1e-7, what="scorer on the repeated layout")
    probs = model.model.predict(xs0)
    assert probs.shape == (len(xs0[0]), 1) and np.allclose(probs, 1.0)  # softmax over one candidate

    f = tmp_path / "naml.pt"
    model.model.save_weights(f)
    other = NAMLModel(hp, vocab_size=20, word_emb_dim=16, seed=9)
    other.model.load_weights(f)
    for a, b in zip(model.model.get_weights(), other.model.get_weights()):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(other.scorer.predict(ev), got)

    bad = loader(train, cm={a: hp.vert_num + 3 for a in mapping})  # every category id >= vert_num
    with pytest.raises(IndexError, match="category id"):
        model.model.fit(bad, epochs=1, verbose=0)
    xs, y = tr[0]
    bad_tok = list(xs)
    bad_tok[1] = xs[1].copy()
    bad_tok[1][0, 0, 0] = 20
    with pytest.raises(IndexError, match="token id"):
        model.model.fit(_Loader([(tuple(bad_tok), y)]), epochs=1, verbose=0, shuffle=False)
    model.model.fit(_Loader([(xs, y)]), epochs=1, verbose=0, shuffle=False)  # the flags were reset: training goes on


def test_two_rank_process_group_raises(hip, monkeypatch):
    from ebrec.models.newsrec import NAMLModel

    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="one rank"):
        NAMLModel(hp_small, vocab_size=10, word_emb_dim=8, seed=1, process_group=object())


class _Loader:
    def __init__(self, batches):
        self.b = batches

    def __len__(self):
        return len(self.b)

    def __getitem__(self, i):
        return self.b[i]
