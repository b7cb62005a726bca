"""LSTUR on the MI355X: the masked AttLayer2 and GRU recurrence kernels against float64, one training step of LSTURModel
(both user-encoder types) against the float64 oracle (tests/lstur_oracle.py), graph replay against eager launches,
determinism, and fit / save / load / scorer on the fixture parquets."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import nrms_numpy as on
from tests import lstur_oracle as lo
from tests.hip_testutil import P, S, assert_close, dev, host
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture of the reference loader test)

pytestmark = pytest.mark.gpu

SEED = 21
f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)


# ---------------------------------------------------------------------------------------------- masked AttLayer2
@pytest.mark.parametrize("F", [64, 400])
@pytest.mark.parametrize("T", [1, 7, 30])
def test_masked_attpool_fwd_and_existing_bwd_vs_float64(hip, T, F):
    rng = np.random.default_rng(T * 1000 + F)
    n_seq, A = 41, 200
    R = n_seq * T
    Vd = rng.uniform(0, 1, (R, F)).astype(np.float32)
    Vd[rng.random(R) < 0.15] = 0.0  # rows dropped / ReLU'd to zero: masked even where the token is real
    ids = rng.integers(1, 50, (n_seq, T)).astype(np.int32)
    ids[rng.random((n_seq, T)) < 0.2] = 0
    ids[::5] = 0  # titles of padding only
    Wa = (rng.uniform(-1, 1, (F, A)) / np.sqrt(F)).astype(np.float32)
    ba, q = rng.uniform(-0.1, 0.1, A).astype(np.float32), rng.uniform(-1, 1, A).astype(np.float32)
    Vdd, Wad, bad, qd, idd = dev(Vd), dev(Wa), dev(ba), dev(q), dev(ids.reshape(-1), torch.int32)
    U = torch.empty(R, A, device="cuda")
    hip.call("ebn_gemm_f32", 0, 0, R, A, F, f1, P(Vdd), F, P(Wad), A, f0, P(U), A, S())
    out, w = torch.empty(n_seq, F, device="cuda"), torch.full((R,), float("nan"), device="cuda")
    hip.call("ebn_attpool_masked_fwd_f32", P(U), P(bad), P(qd), P(Vdd), P(idd), P(out), P(w), n_seq, T, F, A, S())
    V64 = torch.from_numpy(Vd.astype(np.float64)).reshape(n_seq, T, F).requires_grad_(True)
    W64, b64, q64 = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (Wa, ba, q.reshape(A, 1)))
    o64, w64 = lo.masked_attlayer2(V64, torch.from_numpy(ids.astype(np.int64)), W64, b64, q64)
    masked = ((ids == 0) | (Vd.reshape(n_seq, T, F) == 0).all(-1)).reshape(-1)
    assert masked.any() and (~masked).any()
    gw, go = host(w), host(out)
    assert (gw[masked] == 0).all(), "masked rows must get weight 0 exactly"
    assert (go[(ids == 0).all(1)] == 0).all(), "a title of padding only encodes to 0 exactly"
    U64 = np.tanh(Vd.astype(np.float64) @ Wa.astype(np.float64) + ba)
    assert_close(host(U), U64, rtol=1e-5, atol=1e-6, what="tanh U")
    assert_close(gw, w64.detach().numpy().reshape(-1), rtol=1e-4, atol=1e-7, what="w")
    assert_close(go, o64.detach().numpy(), rtol=1e-4, atol=1e-6, what="out")

    # the existing backward kernels are linear in w: masked rows get exactly zero gradients
    dout = rng.uniform(-1, 1, (n_seq, F)).astype(np.float32)
    (o64 * torch.from_numpy(dout.astype(np.float64))).sum().backward()
    doutd, dV, de = dev(dout), torch.empty(R, F, device="cuda"), torch.empty(R, device="cuda")
    hip.call("ebn_attpool_bwd_pool_f32", P(Vdd), P(w), P(doutd), P(dV), P(de), n_seq, T, F, S())
    dq, db = torch.empty(A, device="cuda"), torch.empty(A, device="cuda")
    part = torch.empty(max(int(hip.lib().ebn_attpool_partials_len(R, A)), 1), device="cuda")
    hip.call("ebn_attpool_bwd_dpre_f32", P(U), P(qd), P(de), P(dq), P(db), P(part), R, A, 0, S())
    dVg = torch.empty(R, F, device="cuda")
    hip.call("ebn_gemm_f32", 0, 1, R, F, A, f1, P(U), A, P(Wad), A, f0, P(dVg), F, S())
    dW = torch.empty(F, A, device="cuda")
    hip.call("ebn_gemm_f32", 1, 0, F, A, R, f1, P(Vdd), F, P(U), A, f0, P(dW), A, S())
    dV_total = host(dV) + host(dVg)
    assert (host(de)[masked] == 0).all() and (host(U)[masked] == 0).all() and (host(dV)[masked] == 0).all()
    assert (dV_total[masked] == 0).all()
    want = V64.grad.numpy().reshape(R, F)
    want[masked] = 0.0  # Keras' y = Vd * (token != 0): no gradient reaches Vd at padding
    # fp32 error scale: the same products over absolute values (ds_l = w_l (dw_l - sum w dw) cancels -- at T = 1 to ~1e-7 of
    # its terms -- so the tolerance is set by the terms, not by the result)
    w64n, V3 = w64.detach().numpy(), Vd.astype(np.float64).reshape(n_seq, T, F)
    dwa = np.abs(np.einsum("nf,nlf->nl", dout.astype(np.float64), V3))
    de_abs = w64n * (dwa + (w64n * dwa).sum(1, keepdims=True))
    dpre_abs = (de_abs.reshape(R, 1) * np.abs(q) * (1 - U64 ** 2))
    scales = {"dVd": (w64n.reshape(R, 1) * np.abs(dout).repeat(T, 0)) + dpre_abs @ np.abs(Wa).T,
              "dW": np.abs(Vd).T @ dpre_abs, "db": dpre_abs.sum(0), "dq": (de_abs.reshape(R, 1) * np.abs(U64)).sum(0)}
    for name, got, ref in (("dVd", dV_total, want), ("dW", host(dW), W64.grad.numpy()), ("db", host(db), b64.grad.numpy()),
                           ("dq", host(dq), q64.grad.numpy()[:, 0])):
        err = np.abs(got - ref).max()
        assert err <= 2e-5 * scales[name].max() + 1e-12, f"{name}: max abs err {err:.3e} vs term scale {scales[name].max():.3e}"


# ---------------------------------------------------------------------------------------------- GRU recurrence
def _gru_ref(X, h0, Wk, Wr, bias, dhH):
    """float64 autograd of the masked Keras GRU with the per-step gate pre-activations exposed: (Hs (H+1,B,U), z, r, n, ghh
    (H,B,U) each, dgx (B,H,3U), dgh (H,B,3U), dh0 (B,U))."""
    B, H, _ = X.shape
    U = Wr.shape[0]
    mask = torch.from_numpy((X != 0).any(-1))
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    G = (t64(X) @ t64(Wk) + t64(bias[0])).requires_grad_(True)
    h = t64(h0).requires_grad_(True)
    h_start, hs, ghs, zs, rs, ns, ghhs = h, [h], [], [], [], [], []
    Wr64, br = t64(Wr), t64(bias[1])
    for t in range(H):
        gh = h @ Wr64 + br
        gh.retain_grad()
        ghs.append(gh)
        gx = G[:, t]
        z = torch.sigmoid(gx[:, :U] + gh[:, :U])
        r = torch.sigmoid(gx[:, U:2 * U] + gh[:, U:2 * U])
        n = torch.tanh(gx[:, 2 * U:] + r * gh[:, 2 * U:])
        m = mask[:, t:t + 1]
        h = torch.where(m, z * h + (1 - z) * n, h)
        hs.append(h)
        for lst, v in ((zs, z), (rs, r), (ns, n), (ghhs, gh[:, 2 * U:])):
            lst.append(torch.where(m, v, torch.zeros_like(v)).detach())
    (h * t64(dhH)).sum().backward()
    st = lambda lst: torch.stack(lst).detach().numpy()
    dgh = np.stack([np.where(mask[:, t:t + 1].numpy(), g.grad.numpy(), 0.0) for t, g in enumerate(ghs)])
    return st(hs), st(zs), st(rs), st(ns), st(ghhs), G.grad.numpy(), dgh, h_start.grad.numpy()


@pytest.mark.parametrize("B,H,U", [(3, 1, 8), (5, 7, 64), (32, 20, 400), (32, 50, 400), (257, 20, 400)])
def test_gru_fwd_bwd_kernels_vs_float64(hip, B, H, U):
    rng = np.random.default_rng(B * 100 + H + U)
    F = U
    X = rng.uniform(-1, 1, (B, H, F)).astype(np.float32)
    X[rng.random((B, H)) < 0.25] = 0.0  # random masked steps (holes, left and right padding alike)
    X[0] = 0.0                          # a fully masked sequence: the output is h0, dh0 = dh_H
    lim = np.sqrt(6.0 / (4 * U))
    Wk, Wr = (rng.uniform(-lim, lim, (U, 3 * U)).astype(np.float32) for _ in range(2))
    bias = rng.uniform(-0.2, 0.2, (2, 3 * U)).astype(np.float32)
    null_h0 = H == 7  # type "con" starts from zeros: NULL h0
    h0 = np.zeros((B, U), np.float32) if null_h0 else rng.uniform(-0.5, 0.5, (B, U)).astype(np.float32)
    Xd, Wkd, Wrd, bd, h0d = dev(X.reshape(B * H, F)), dev(Wk), dev(Wr), dev(bias), dev(h0)
    gx = torch.empty(B * H, 3 * U, device="cuda")
    hip.call("ebn_gemm_f32", 0, 0, B * H, 3 * U, F, f1, P(Xd), F, P(Wkd), 3 * U, f0, P(gx), 3 * U, S())
    Hs, act = torch.full((H + 1, B, U), float("nan"), device="cuda"), torch.full((H, B, 4 * U), float("nan"), device="cuda")
    hip.call("ebn_gru_fwd_f32", P(gx), P(Xd), P(Wrd), P(bd), None if null_h0 else P(h0d), P(Hs), P(act), B, H, F, U, S())
    dhH = rng.uniform(-1, 1, (B, U)).astype(np.float32)
    dhHd = dev(dhH)
    dgx, dgh = torch.full((B * H, 3 * U), float("nan"), device="cuda"), torch.full((H, B, 3 * U), float("nan"), device="cuda")
    dh0 = torch.full((B, U), float("nan"), device="cuda")
    hip.call("ebn_gru_bwd_f32", P(dhHd), P(Xd), P(Wrd), P(Hs), P(act), P(dgx), P(dgh), P(dh0), B, H, F, U, S())
    hs, z, r, n, ghh, rdgx, rdgh, rdh0 = _gru_ref(X, h0, Wk, Wr, bias, dhH)
    gHs, gact = host(Hs), host(act).reshape(H, B, 4, U)
    # forward: O(1) values through at most 50 fp32 steps -- 1e-5 absolute
    for name, got, ref in (("Hs", gHs, hs), ("z", gact[:, :, 0], z), ("r", gact[:, :, 1], r), ("n", gact[:, :, 2], n),
                           ("gh_h", gact[:, :, 3], ghh)):
        err = np.abs(got - ref).max()
        assert err <= 1e-5, f"{name}: max abs err {err:.3e}"
    # masked steps copy h bit for bit; masked rows of the gradients are exact zeros; dh passes them unchanged
    live = (X != 0).any(-1)  # (B, H)
    for t in range(H):
        np.testing.assert_array_equal(gHs[t + 1][~live[:, t]], gHs[t][~live[:, t]])
    gdgx, gdgh = host(dgx).reshape(B, H, 3 * U), host(dgh)
    assert (gdgx[~live] == 0).all() and (gdgh[~live.T] == 0).all()
    np.testing.assert_array_equal(gHs[H][0], h0[0])
    np.testing.assert_array_equal(host(dh0)[0], dhH[0])
    # gradients: 2e-4 of the largest element (fp32 recurrences of up to 50 steps, contraction length 3U = 1200)
    for name, got, ref in (("dgx", gdgx, rdgx), ("dgh", gdgh, rdgh), ("dh0", host(dh0), rdh0)):
        err = np.abs(got - ref).max()
        assert err <= 2e-4 * np.abs(ref).max() + 1e-9, f"{name}: max abs err {err:.3e} vs max {np.abs(ref).max():.3e}"


# ---------------------------------------------------------------------------------------------- whole model
class hp_small:
    title_size, history_size, n_users, cnn_activation, type = 9, 4, 11, "relu", "ini"
    attention_hidden_dim, gru_unit, filter_num, window_size = 24, 32, 32, 3
    optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-3


class hp_c1:
    title_size, history_size, n_users, cnn_activation, type = 30, 20, 50000, "relu", "ini"
    attention_hidden_dim, gru_unit, filter_num, window_size = 200, 400, 400, 3
    optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-4


def _hp(base, user_type):
    return type("hp", (base,), {"type": user_type})


def _model(hp, V, E, seed, Pw=None):
    from ebrec.models.newsrec import LSTURModel

    m = LSTURModel(hp, word2vec_embedding=np.zeros((V, E), np.float32) if Pw is None else Pw["emb"].astype(np.float32), seed=seed)
    if Pw is not None:
        m.model.set_weights([Pw[k] for k in lo.weight_order(hp.type)])
    return m


def _params(hp, V, E, seed):
    Pw = lo.random_params(V, E, hp.n_users, hp.gru_unit, hp.attention_hidden_dim, hp.window_size, hp.type, seed=seed)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in Pw.items()}


def _batch(hp, V, B, C, seed, users):
    rng = np.random.default_rng(seed)
    his = rng.integers(1, V, (B, hp.history_size, hp.title_size))
    his[:, 0, -3:] = 0   # title padding
    his[1, 2] = 0        # a hole in the history: a masked GRU step
    his[2, :2] = 0       # left padding of the history
    his[3] = 0           # no history at all: ini -> user = long_u
    pred = rng.integers(1, V, (B, C, hp.title_size))
    pred[0, 1, 4:] = 0
    y = np.zeros((B, C), np.int8)
    y[np.arange(B), rng.integers(0, C, B)] = 1
    return np.asarray(users).reshape(B, 1), his, pred, y


def _adam_tol(g, gtol, lr, w):
    """Bound of the first Adam step's error caused by a gradient error of at most gtol (step 1: u(g) = alpha m / (sqrt v + eps)
    with m = 0.1 g, v = 0.001 g^2), plus fp32 rounding of the weight."""
    alpha = lr * np.sqrt(1 - 0.999) / (1 - 0.9)
    u = lambda x: alpha * 0.1 * x / (np.sqrt(0.001 * x * x) + 1e-7)
    return np.maximum(np.abs(u(g + gtol) - u(g)), np.abs(u(g - gtol) - u(g))) + 2e-7 * np.abs(w) + 1e-9


@pytest.mark.parametrize("user_type", ["ini", "con"])
@pytest.mark.parametrize("shape", ["small", "lstur-c1"])
def test_train_step_loss_scores_gradients_and_adam_vs_oracle(hip, shape, user_type):
    base, V, E, B, C = (hp_small, 97, 16, 6, 3) if shape == "small" else (hp_c1, 32000, 300, 32, 5)
    hp = _hp(base, user_type)
    rng = np.random.default_rng(1)
    users = rng.integers(0, hp.n_users + 1, B)
    users[1] = users[0]
    users[B - 1] = users[0]  # duplicate users: their embedding gradients must combine
    Pw = _params(hp, V, E, seed=2)
    model = _model(hp, V, E, seed=SEED, Pw=Pw)
    eng = model._engine
    user, his, pred, y = _batch(hp, V, B, C, 3, users)
    b, expand = eng._stage(user.reshape(-1), his, pred, y, False)
    eng._grad_kernels(b, C, expand)
    torch.cuda.synchronize()
    loss = float(eng.loss_dev.item())
    scores = host(b.scores).reshape(B, C)
    vd = host(b.Vd).reshape(b.N, hp.title_size, hp.filter_num)

    def gate(pre):  # ReLU inputs within fp32 rounding of 0 take the engine's decision
        tie = np.abs(pre) <= 3e-6 * np.abs(pre).max()
        return np.where(tie, vd > 0, pre > 0)

    L, _, s, g = lo.lstur_loss_and_grads(user, his, pred, y, Pw, user_type, hp.dropout, on.Drop(hp.dropout, SEED, 1), hp.loss,
                                         relu_gate=gate)
    assert abs(loss - L) <= 2e-5 * max(1.0, abs(L)), (loss, L)
    assert np.abs(scores - s).max() <= 1e-4 * max(1.0, np.abs(s).max()), np.abs(scores - s).max()
    pg = eng.params.g
    W, U = hp.window_size, hp.gru_unit
    wb = host(pg("conv_Wb"))
    fixed = lambda acc, shape: host(acc).reshape(shape) / 2.0 ** 40
    got = {"conv_W": wb[: W * E].reshape(W, E, -1), "conv_b": wb[W * E], "att_W": host(pg("att_W")), "att_b": host(pg("att_b")),
           "att_q": host(pg("att_q")).reshape(-1, 1), "gru_k": host(pg("gru_k")), "gru_r": host(pg("gru_r")),
           "gru_b": host(pg("gru_b")), "emb": fixed(eng.table_acc, (V, E)), "user_emb": fixed(eng.user_acc, (hp.n_users + 1, U))}
    if user_type == "con":
        got.update({"dense_W": host(pg("dense_W")), "dense_b": host(pg("dense_b"))})
    assert set(got) == set(g)
    for k in sorted(g):
        ref = np.abs(g[k]).max()
        err = np.abs(got[k] - g[k]).max()
        assert err <= 2e-4 * ref + 1e-9, f"{k}: max abs err {err:.3e} vs max |grad| {ref:.3e}"
    assert np.abs(g["user_emb"][users[0]]).max() > 0 and np.abs(g["gru_r"]).max() > 0
    # Keras Adam's first step over every parameter (dense buffer, word table, user table) against the oracle's gradients
    eng._optimizer_kernels()
    torch.cuda.synchronize()
    after = dict(zip(lo.weight_order(user_type), model.model.get_weights()))
    for k in sorted(g):
        w0 = Pw[k].copy()
        want = w0.copy()
        on.adam_keras_step(want, g[k], np.zeros_like(w0), np.zeros_like(w0), 1, lr=hp.learning_rate)
        tol = _adam_tol(g[k], 2e-4 * np.abs(g[k]).max() + 1e-9, hp.learning_rate, w0)
        bad = np.abs(after[k].astype(np.float64) - want) > tol
        assert not bad.any(), f"{k} after Adam: {int(bad.sum())} elements off, worst {np.abs(after[k] - want).max():.3e}"


def test_count_params_matches_keras_formula(hip):
    V, E = 50, 16
    for user_type in ("ini", "con"):
        hp = _hp(hp_small, user_type)
        m = _model(hp, V, E, seed=1)
        n, U, F, A, win = hp.n_users, hp.gru_unit, hp.filter_num, hp.attention_hidden_dim, hp.window_size
        want = V * E + (n + 1) * U + win * E * F + F + F * A + 2 * A + 3 * U * F + 3 * U * U + 6 * U
        want += 2 * U * U + U if user_type == "con" else 0
        assert m.model.count_params() == want
        assert sum(w.size for w in m.model.get_weights()) == want
    # Keras' glorot_uniform(seed) of one shape twice: the GRU's kernel and recurrent kernel start identical (F == U)
    w = dict(zip(lo.weight_order("ini"), _model(_hp(hp_small, "ini"), V, E, seed=3).model.get_weights()))
    np.testing.assert_array_equal(w["gru_k"], w["gru_r"])
    assert (w["user_emb"] == 0).all() and (w["gru_b"] == 0).all()


@pytest.mark.parametrize("user_type", ["ini", "con"])
def test_graph_replay_equals_eager_and_runs_are_deterministic(hip, user_type):
    hp, V, E, B, C = _hp(hp_small, user_type), 97, 16, 6, 3
    finals = []
    for use_graph in (True, True, False):
        model = _model(hp, V, E, seed=SEED, Pw=_params(hp, V, E, seed=2))
        model._engine.use_graph = use_graph
        losses = []
        for s in range(3):
            user, his, pred, y = _batch(hp, V, B, C, 10 + s, [1, 1, 2, 3, 5, 1])
            losses.append(float(model.train_step(user, his, pred, y).item()))
        torch.cuda.synchronize()
        finals.append((losses, [torch.from_numpy(np.ascontiguousarray(w)) for w in model.model.get_weights()]))
    for losses, ws in finals[1:]:
        assert losses == finals[0][0]
        for a, b in zip(finals[0][1], ws):
            assert torch.equal(a, b)


def test_fit_save_load_scorer_and_ranges_on_fixtures(hip, tmp_path, frames):  # noqa: F811
    from ebrec.models.newsrec import LSTURModel
    from ebrec.models.newsrec.dataloader import LSTURDataLoader
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_USER_COL

    beh, train, mapping = frames
    users = sorted(pd.unique(beh[DEFAULT_USER_COL]))
    umap = {u: i + 1 for i, u in enumerate(users[:-3])}

    class hp:
        title_size, history_size, n_users, cnn_activation, type = 10, 3, len(users), "relu", "ini"
        attention_hidden_dim, gru_unit, filter_num, window_size = 16, 24, 24, 3
        optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-3

    model = LSTURModel(hp, vocab_size=20, word_emb_dim=16, seed=5)
    tr = LSTURDataLoader(behaviors=train, article_dict=mapping, user_id_mapping=umap, history_column=DEFAULT_HISTORY_ARTICLE_ID_COL,
                         unknown_representation="zeros", batch_size=16)
    hist = model.model.fit(tr, validation_data=tr, epochs=2, verbose=0)
    losses = hist.history["loss"]
    assert len(losses) == 2 and all(np.isfinite(losses))
    assert np.abs(model._engine.user_table.cpu().numpy()).max() > 0  # the zero-initialised user table trains
    ev_loss = model.model.evaluate(tr, verbose=0)
    assert np.all(np.isfinite(np.asarray(ev_loss, dtype=np.float64)))

    f = tmp_path / "lstur.pt"
    model.model.save_weights(f)
    other = LSTURModel(hp, vocab_size=20, word_emb_dim=16, seed=9)
    other.model.load_weights(f)
    for a, b in zip(model.model.get_weights(), other.model.get_weights()):
        np.testing.assert_array_equal(a, b)

    ev = LSTURDataLoader(behaviors=beh.iloc[:40].reset_index(drop=True), article_dict=mapping, user_id_mapping=umap,
                         history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, unknown_representation="zeros", batch_size=16,
                         eval_mode=True)
    got = model.scorer.predict(ev)
    Pw = dict(zip(lo.weight_order("ini"), [w.astype(np.float64) for w in model.model.get_weights()]))
    want = np.concatenate([lo.scorer_forward(u, h, p, Pw).reshape(-1, 1) for (u, h, p), _y in (ev[i] for i in range(len(ev)))])
    assert got.shape == want.shape
    assert_close(got, want, rtol=1e-4, atol=1e-6, what="scorer.predict vs sigmoid(cand . user)")
    (u, h, pr), _y = ev[0]
    probs = model.model.predict((u, h, pr))
    assert probs.shape == (len(u), 1) and np.allclose(probs, 1.0)  # softmax over one candidate

    (u, h, pr), y = tr[0]
    bad = u.copy()
    bad[0, 0] = hp.n_users + 1
    with pytest.raises(IndexError, match="user index"):
        model.model.fit(_Loader([((bad, h, pr), y)]), epochs=1, verbose=0, shuffle=False)
    bad_tok = h.copy()
    bad_tok[0, 0, 0] = 20
    with pytest.raises(IndexError, match="token id"):
        model.model.fit(_Loader([((u, bad_tok, pr), y)]), epochs=1, verbose=0, shuffle=False)
    bad_dev = LSTURDataLoader(behaviors=train, article_dict=mapping, user_id_mapping={k: hp.n_users + 7 for k in umap},
                              history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, unknown_representation="zeros", batch_size=16)
    with pytest.raises(IndexError, match="user index"):
        model.model.fit(bad_dev, epochs=1, verbose=0)


class _Loader:
    def __init__(self, batches):
        self.b = batches

    def __len__(self):
        return len(self.b)

    def __getitem__(self, i):
        return self.b[i]
