"""NPA on the MI355X: the Conv1D and PersonalizedAttentivePooling kernels against float64, one training step of NPAModel
against the float64 oracle (tests/npa_oracle.py), determinism, and fit / save / load / scorer on the fixture parquets."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import nrms_numpy as on
from tests import npa_oracle as npo
from tests.hip_testutil import P, S, assert_close, dev, host, make_state
from tests.model_kernel_refs import SEED, STEP, _mult
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture of the reference loader test)

pytestmark = pytest.mark.gpu


def _unfold(X, T, window):
    """float64 im2col of the "same" window (test-side only): (R, E) -> (R, window*E)."""
    N = X.shape[0] // T
    Xt = X.reshape(N, T, -1)
    pl = (window - 1) // 2
    cols = []
    for j in range(window):
        s = np.zeros_like(Xt)
        lo, hi = max(0, pl - j), min(T, T + pl - j)
        s[:, lo:hi] = Xt[:, lo + j - pl:hi + j - pl]
        cols.append(s)
    return np.concatenate(cols, -1).reshape(N * T, -1)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("window", [1, 3, 5])
@pytest.mark.parametrize("T,E,F", [(30, 300, 400), (30, 1024, 400), (7, 100, 64), (1, 300, 400)])
def test_conv1d_kernels_vs_float64(hip, T, E, F, window, drop):
    rng = np.random.default_rng(T * 7 + E + window)
    n_titles = 37 if T > 1 else 1111  # R = n_titles * T is not a multiple of the 128-row tile
    R = n_titles * T
    X = rng.uniform(-1, 1, (R, E)).astype(np.float32)
    W = (rng.uniform(-1, 1, (window * E, F)) / np.sqrt(window * E)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, F).astype(np.float32)
    p_conv, p_pap = (0.2, 0.2) if drop else (0.0, 0.0)
    st = make_state(SEED, STEP) if drop else None
    stp = P(st) if drop else None
    Xd, Wd, bd = dev(X), dev(W), dev(b)
    Vd = torch.empty(R, F, device="cuda")
    hip.call("ebn_conv1d_fwd_f32", P(Xd), P(Wd), P(bd), P(Vd), n_titles, T, E, F, window, stp, 2, ctypes.c_float(p_conv), 3,
             ctypes.c_float(p_pap), S())
    A64 = _unfold(X.astype(np.float64), T, window)
    pre = A64 @ W.astype(np.float64) + b
    m = (_mult(2, p_conv, R * F) * _mult(3, p_pap, R * F)).reshape(R, F)
    want = np.maximum(pre, 0) * m
    got = host(Vd)
    scale = np.abs(A64).sum(1, keepdims=True) @ np.abs(W).max(0, keepdims=True) + 1e-3
    assert (np.abs(got - want) <= 2e-6 * scale * np.maximum(m, 1)).all(), np.abs(got - want).max()
    # the masks bit for bit: a dropped element is exactly 0; a kept one is 0 only where the ReLU blocked
    dropped = m == 0
    assert (got[dropped] == 0).all()
    clear = ~dropped & (np.abs(pre) > 1e-5 * scale)
    np.testing.assert_array_equal(got[clear] > 0, pre[clear] > 0)

    # backward: dY' = dVd / ((1-p)(1-0.2)) where Vd > 0 (the kernels' gate is the forward's own Vd)
    dVd = rng.uniform(-1, 1, (R, F)).astype(np.float32)
    gscale = (1.0 / (1 - p_conv) if p_conv else 1.0) * (1.0 / (1 - p_pap) if p_pap else 1.0)
    dYp = np.where(got > 0, dVd.astype(np.float64) * gscale, 0.0)
    dVdd = dev(dVd)
    dX = torch.empty(R, E, device="cuda")
    hip.call("ebn_conv1d_bwd_data_f32", P(dVdd), P(Vd), P(Wd), P(dX), n_titles, T, E, F, window, stp, ctypes.c_float(p_conv),
             ctypes.c_float(p_pap), S())
    dA = dYp @ W.astype(np.float64).T  # (R, window*E): scatter the window back onto its source rows
    want_dx = np.zeros((n_titles, T, E))
    pl = (window - 1) // 2
    dA3 = dA.reshape(n_titles, T, window, E)
    for j in range(window):
        lo, hi = max(0, pl - j), min(T, T + pl - j)
        want_dx[:, lo + j - pl:hi + j - pl] += dA3[:, lo:hi, j]
    sx = np.abs(dYp).sum() / R * np.abs(W).max() * window * F / 4 + 1e-6
    assert_close(host(dX), want_dx.reshape(R, E), rtol=1e-4, atol=1e-5 * sx, what="dX")

    splits = int(hip.lib().ebn_conv1d_wgrad_splits(n_titles, T, E, F, window))
    n = int(hip.lib().ebn_conv1d_wgrad_workspace_floats(n_titles, T, E, F, window, splits))
    assert n == splits * (window * E + 1) * F
    part = torch.full((n,), float("nan"), device="cuda")
    hip.call("ebn_conv1d_bwd_weight_f32", P(Xd), P(dVdd), P(Vd), P(part), splits, n_titles, T, E, F, window, stp,
             ctypes.c_float(p_conv), ctypes.c_float(p_pap), S())
    gw = host(part).reshape(splits, window * E + 1, F).sum(0)
    want_w = A64.T @ dYp
    sw = np.abs(A64).T @ np.abs(dYp) + 1e-6
    assert (np.abs(gw[: window * E] - want_w) <= 2e-6 * sw).all(), np.abs(gw[: window * E] - want_w).max()
    assert (np.abs(gw[window * E] - dYp.sum(0)) <= 2e-6 * (np.abs(dYp).sum(0) + 1e-6)).all()


@pytest.mark.parametrize("L", [30, 20, 50])
def test_pap_fwd_bwd_vs_float64(hip, L):
    rng = np.random.default_rng(L)
    n_seq, n_q, F, A = 23, 7, 400, 200
    n_drop = 9  # the first 9 sequences also get the output dropout (the next pooling's input)
    V = rng.uniform(0, 1, (n_seq * L, F)).astype(np.float32)
    Wa = (rng.uniform(-1, 1, (F, A)) / np.sqrt(F)).astype(np.float32)
    ba = rng.uniform(-0.1, 0.1, A).astype(np.float32)
    Q = rng.uniform(-1, 1, (n_q, A)).astype(np.float32)
    q_idx = rng.integers(0, n_q, n_seq).astype(np.int32)
    Vd_, Wad, bad, Qd, qi = dev(V), dev(Wa), dev(ba), dev(Q), dev(q_idx, torch.int32)
    U = torch.empty(n_seq * L, A, device="cuda")
    hip.call("ebn_gemm_f32", 0, 0, n_seq * L, A, F, ctypes.c_float(1.0), P(Vd_), F, P(Wad), A, ctypes.c_float(0.0), P(U), A, S())
    out, w, out_d = (torch.empty(n_seq, F, device="cuda"), torch.empty(n_seq * L, device="cuda"),
                     torch.empty(n_seq, F, device="cuda"))
    st = make_state(SEED, STEP)
    hip.call("ebn_pap_fwd_f32", P(U), P(bad), P(Qd), P(qi), n_q, P(Vd_), P(out), P(w), P(out_d), n_drop, n_seq, L, F, A, P(st), 4,
             ctypes.c_float(0.2), S())
    V64 = V.astype(np.float64).reshape(n_seq, L, F)
    U64 = np.tanh(V64 @ Wa.astype(np.float64) + ba)
    s = np.einsum("nla,na->nl", U64, Q.astype(np.float64)[q_idx])
    w64 = np.exp(s - s.max(1, keepdims=True))
    w64 /= w64.sum(1, keepdims=True)
    o64 = np.einsum("nl,nlf->nf", w64, V64)
    mult = _mult(4, 0.2, n_drop * F).reshape(n_drop, F)
    assert_close(host(U).reshape(n_seq, L, A), U64, rtol=1e-5, atol=1e-6, what="tanh U")
    assert_close(host(w).reshape(n_seq, L), w64, rtol=1e-4, atol=1e-7, what="w")
    assert_close(host(out), o64, rtol=1e-4, atol=1e-6, what="out")
    assert_close(host(out_d)[:n_drop], o64[:n_drop] * mult, rtol=1e-4, atol=1e-6, what="out_d")

    dout = rng.uniform(-1, 1, (n_seq, F)).astype(np.float32)
    doutd, dV, dq = dev(dout), torch.empty(n_seq * L, F, device="cuda"), torch.empty(n_seq, A, device="cuda")
    hip.call("ebn_pap_bwd_f32", P(U), P(Qd), P(qi), n_q, P(Vd_), P(w), P(doutd), P(dV), P(dq), n_drop, n_seq, L, F, A, P(st), 4,
             ctypes.c_float(0.2), S())
    d64 = dout.astype(np.float64)
    d64[:n_drop] *= mult
    dw = np.einsum("nf,nlf->nl", d64, V64)
    ds = w64 * (dw - (w64 * dw).sum(1, keepdims=True))
    assert_close(host(doutd), d64, rtol=1e-6, atol=1e-7, what="dout gated in place")
    assert_close(host(dq), np.einsum("nl,nla->na", ds, U64), rtol=1e-4, atol=1e-6, what="dq per sequence")
    assert_close(host(U).reshape(n_seq, L, A), ds[..., None] * Q.astype(np.float64)[q_idx][:, None] * (1 - U64 ** 2), rtol=1e-4,
                 atol=1e-7, what="dpre")
    assert_close(host(dV).reshape(n_seq, L, F), w64[..., None] * d64[:, None], rtol=1e-4, atol=1e-7, what="dV")
    dQ = torch.full((n_q, A), float("nan"), device="cuda")
    hip.call("ebn_pap_dq_reduce_f32", P(dq), P(qi), n_seq, P(dQ), n_q, A, S())
    want = np.zeros((n_q, A))
    np.add.at(want, q_idx, host(dq))
    assert_close(host(dQ), want, rtol=1e-6, atol=1e-7, what="dQ per query row")


# ---------------------------------------------------------------------------------------------- whole model
class hp_small:
    title_size, history_size, n_users, cnn_activation = 9, 4, 11, "relu"
    attention_hidden_dim, user_emb_dim, filter_num, window_size = 24, 20, 32, 3
    optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-3


class hp_c1:
    title_size, history_size, n_users, cnn_activation = 30, 20, 50000, "relu"
    attention_hidden_dim, user_emb_dim, filter_num, window_size = 200, 400, 400, 3
    optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-4


def _model(hp, V, E, seed, Pw=None):
    from ebrec.models.newsrec import NPAModel

    m = NPAModel(hp, word2vec_embedding=np.zeros((V, E), np.float32) if Pw is None else Pw["emb"].astype(np.float32), seed=seed)
    if Pw is not None:
        m.model.set_weights([Pw[k] for k in npo.WEIGHT_ORDER])
    return m


def _params(hp, V, E, seed):
    Pw = npo.random_params(V, E, hp.n_users, hp.user_emb_dim, hp.filter_num, hp.attention_hidden_dim, hp.window_size, seed=seed)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in Pw.items()}


def _batch(hp, V, B, C, seed, users):
    rng = np.random.default_rng(seed)
    his = rng.integers(0, V, (B, hp.history_size, hp.title_size))
    his[:, 0, -3:] = 0  # some padding
    pred = rng.integers(0, V, (B, C, hp.title_size))
    y = np.zeros((B, C), np.int8)
    y[np.arange(B), rng.integers(0, C, B)] = 1
    return np.asarray(users).reshape(B, 1), his, pred, y


@pytest.mark.parametrize("shape", ["small", "npa-c1"])
def test_train_step_loss_and_every_gradient_vs_oracle(hip, shape):
    hp, V, E, B, C = (hp_small, 97, 16, 6, 3) if shape == "small" else (hp_c1, 32000, 300, 32, 5)
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
    vd = host(b.Vd).reshape(b.N, hp.title_size, hp.filter_num)

    def gate(pre):  # ReLU inputs within fp32 rounding of 0 take the engine's decision (ReluTieGate's rule)
        tie = np.abs(pre) <= 3e-6 * np.abs(pre).max()
        return np.where(tie, vd > 0, pre > 0)

    L, _, g = npo.npa_loss_and_grads(user, his, pred, y, Pw, hp.dropout, on.Drop(hp.dropout, SEED, 1), hp.loss, relu_gate=gate)
    assert abs(loss - L) <= 2e-5 * max(1.0, abs(L)), (loss, L)
    pv = eng.params.g
    W, Ew = hp.window_size, E
    wb = host(pv("conv_Wb"))
    fixed = lambda acc, shape: host(acc).reshape(shape) / 2.0 ** 40
    got = {"conv_W": wb[: W * Ew].reshape(W, Ew, -1), "conv_b": wb[W * Ew], "n_Wq": host(pv("n_Wq")), "n_bq": host(pv("n_bq")),
           "n_Wa": host(pv("n_Wa")), "n_ba": host(pv("n_ba")), "u_Wq": host(pv("u_Wq")), "u_bq": host(pv("u_bq")),
           "u_Wa": host(pv("u_Wa")), "u_ba": host(pv("u_ba")), "emb": fixed(eng.table_acc, (V, E)),
           "user_emb": fixed(eng.user_acc, (hp.n_users + 1, hp.user_emb_dim))}
    assert set(got) == set(g)
    for k in sorted(g):
        ref = np.abs(g[k]).max()
        err = np.abs(got[k] - g[k]).max()
        assert err <= 2e-4 * ref + 1e-9, f"{k}: max abs err {err:.3e} vs max |grad| {ref:.3e}"
    assert np.abs(g["user_emb"][users[0]]).max() > 0


def test_three_steps_are_deterministic(hip):
    hp, V, E, B, C = hp_small, 97, 16, 6, 3
    finals = []
    for _ in range(2):
        model = _model(hp, V, E, seed=SEED, Pw=_params(hp, V, E, seed=2))
        for s in range(3):
            user, his, pred, y = _batch(hp, V, B, C, 10 + s, [1, 1, 2, 3, 5, 1])
            model.train_step(user, his, pred, y)
        torch.cuda.synchronize()
        finals.append([torch.from_numpy(np.ascontiguousarray(w)) for w in model.model.get_weights()])
    for a, b in zip(*finals):
        assert torch.equal(a, b)


def test_fit_save_load_scorer_and_user_range_on_fixtures(hip, tmp_path, frames):  # noqa: F811
    from ebrec.models.newsrec.dataloader import LSTURDataLoader
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_USER_COL

    beh, train, mapping = frames
    users = sorted(pd.unique(beh[DEFAULT_USER_COL]))
    umap = {u: i + 1 for i, u in enumerate(users[:-3])}

    class hp:
        title_size, history_size, n_users, cnn_activation = 10, 3, len(users), "relu"
        attention_hidden_dim, user_emb_dim, filter_num, window_size = 16, 12, 24, 3
        optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-3

    from ebrec.models.newsrec import NPAModel

    model = NPAModel(hp, vocab_size=20, word_emb_dim=16, seed=5)
    tr = LSTURDataLoader(behaviors=train, article_dict=mapping, user_id_mapping=umap, history_column=DEFAULT_HISTORY_ARTICLE_ID_COL,
                         unknown_representation="zeros", batch_size=16)
    hist = model.model.fit(tr, epochs=2, verbose=0)
    losses = hist.history["loss"]
    assert len(losses) == 2 and all(np.isfinite(losses))
    assert np.abs(model._engine.user_table.cpu().numpy()).max() > 0  # the zero-initialised user table trains

    f = tmp_path / "npa.pt"
    model.model.save_weights(f)
    other = NPAModel(hp, vocab_size=20, word_emb_dim=16, seed=9)
    other.model.load_weights(f)
    for a, b in zip(model.model.get_weights(), other.model.get_weights()):
        np.testing.assert_array_equal(a, b)

    ev = LSTURDataLoader(behaviors=beh.iloc[:40].reset_index(drop=True), article_dict=mapping, user_id_mapping=umap,
                         history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, unknown_representation="zeros", batch_size=16,
                         eval_mode=True)
    got = model.scorer.predict(ev)
    Pw = dict(zip(npo.WEIGHT_ORDER, [w.astype(np.float64) for w in model.model.get_weights()]))
    want = np.concatenate([npo.scorer_forward(u, h, p, Pw).reshape(-1, 1) for (u, h, p), _y in (ev[i] for i in range(len(ev)))])
    assert got.shape == want.shape
    assert_close(got, want, rtol=1e-4, atol=1e-6, what="scorer.predict vs sigmoid(cand . user)")
    # the same scores from the model's own encoders: the candidate vector (queried by its impression's user) dotted with the user
    (u, h, pr), _y = ev[0]
    uv, cv = model._engine._infer(u.reshape(-1), h, pr.reshape(-1, hp.title_size), np.arange(len(u)))
    np.testing.assert_allclose(got[: len(u), 0], torch.sigmoid((uv * cv).sum(1)).cpu().numpy(), rtol=1e-5, atol=1e-6)

    (u, h, pr), y = tr[0]
    bad = u.copy()
    bad[0, 0] = hp.n_users + 1
    with pytest.raises(IndexError, match="user index"):
        model.model.fit(_Loader([((bad, h, pr), y)]), epochs=1, verbose=0, shuffle=False)
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
