"""Float64 restatement of LSTUR (reference lstur.py, layers.py:55-81, 273-309) over the engine's title layout, for the LSTUR tests.

The forward is written with torch ops in float64 and differentiated by autograd; dropout masks are the build's counter stream
(oracle.nrms_numpy.dropout_keep_mask) at the engine's element indices:
  site 0  Dropout(p) of the embedded tokens   index (n*T + t)*E + e   (n: title in engine order, history first)
  site 2  Dropout(p) after the Conv1D         index (n*T + t)*F + f
Parameters are a dict of float64 numpy arrays in the engine's get_weights() order (WEIGHT_ORDER, plus CON_WEIGHT_ORDER for
type "con"): emb (V,E), user_emb (n_users+1,U), conv_W (window,E,F), conv_b (F,), att_W (F,A), att_b (A,), att_q (A,1),
gru_k (F,3U), gru_r (U,3U), gru_b (2,3U) [, dense_W (2U,U), dense_b (U,)].  Gate blocks of the GRU are [z | r | h] (Keras).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.nrms_numpy import dropout_keep_mask
from tests.npa_oracle import conv1d_same

WEIGHT_ORDER = ["emb", "user_emb", "conv_W", "conv_b", "att_W", "att_b", "att_q", "gru_k", "gru_r", "gru_b"]
CON_WEIGHT_ORDER = ["dense_W", "dense_b"]
SITE_NEWS_IN, SITE_CONV = 0, 2
KERAS_EPS = 1e-7


def weight_order(user_type: str):
    return WEIGHT_ORDER + (CON_WEIGHT_ORDER if user_type == "con" else [])


def random_params(V, E, n_users, U, A, window, user_type="ini", seed=0, user_scale=0.5):
    """filter_num == gru_unit == U (the score is cand . user)."""
    rng = np.random.default_rng(seed)
    g = lambda *s: rng.uniform(-1, 1, size=s) * np.sqrt(6.0 / (s[0] + s[-1]))
    P = {"emb": rng.uniform(-0.5, 0.5, (V, E)), "user_emb": rng.uniform(-user_scale, user_scale, (n_users + 1, U)),
         "conv_W": rng.uniform(-1, 1, (window, E, U)) * np.sqrt(6.0 / (window * (E + U))), "conv_b": rng.uniform(-0.1, 0.1, U),
         "att_W": g(U, A), "att_b": rng.uniform(-0.1, 0.1, A), "att_q": g(A, 1), "gru_k": g(U, 3 * U), "gru_r": g(U, 3 * U),
         "gru_b": rng.uniform(-0.1, 0.1, (2, 3 * U))}
    if user_type == "con":
        P.update({"dense_W": g(2 * U, U), "dense_b": rng.uniform(-0.1, 0.1, U)})
    return P


def _mask(drop, site, p, shape):
    """inverted-dropout multiplier (float64) of `site` over a tensor of `shape`, or None when off"""
    if drop is None or p <= 0:
        return None
    keep = dropout_keep_mask(drop.key(site), int(np.prod(shape)), p).reshape(shape)
    return torch.from_numpy(keep.astype(np.float64) / (1.0 - p))


def masked_attlayer2(Y: torch.Tensor, ids: torch.Tensor, W, b, q):
    """OverwriteMasking(token != 0) -> Masking() -> AttLayer2 with that mask (lstur.py:136-141, layers.py:55-81):
    Y (n,L,F), ids (n,L) -> (n,F), w (n,L).  exp is not max-subtracted; masked rows get weight 0."""
    y = Y * (ids != 0).to(Y.dtype)[..., None]
    m = (y != 0).any(-1).to(Y.dtype)
    a = torch.exp((torch.tanh(y @ W + b) @ q).squeeze(-1)) * m
    w = a / (a.sum(-1, keepdim=True) + KERAS_EPS)
    return (w[..., None] * y).sum(1), w


def gru_step(x_gates: torch.Tensor, h: torch.Tensor, Wr, br):
    """One Keras GRU step (reset_after=True): x_gates = x.kernel + input bias (B,3U), h (B,U) -> h'."""
    U = h.shape[-1]
    gh = h @ Wr + br
    z = torch.sigmoid(x_gates[:, :U] + gh[:, :U])
    r = torch.sigmoid(x_gates[:, U:2 * U] + gh[:, U:2 * U])
    n = torch.tanh(x_gates[:, 2 * U:] + r * gh[:, 2 * U:])
    return z * h + (1 - z) * n


def gru_keras(X: torch.Tensor, h0: torch.Tensor, Wk, Wr, bias, mask=None):
    """Masked Keras GRU: X (B,H,F), h0 (B,U), Wk (F,3U), Wr (U,3U), bias (2,3U) -> final state (B,U).  mask (B,H) bool or
    None; default Masking(0.0): step t of sequence b is skipped (h carried) iff X[b,t] is all zero."""
    if mask is None:
        mask = (X != 0).any(-1)
    gx = X @ Wk + bias[0]
    h = h0
    for t in range(X.shape[1]):
        h = torch.where(mask[:, t:t + 1], gru_step(gx[:, t], h, Wr, bias[1]), h)
    return h


def lstur_forward(user, his, pred, P: dict, user_type="ini", p: float = 0.0, drop=None, relu_gate=None):
    """(probs (B,C), scores (B,C), tensors of P) -- tensors with requires_grad for lstur_loss_and_grads.  drop: an
    oracle.nrms_numpy.Drop (training) or None (inference).  relu_gate(pre (N,T,F) float64 numpy) -> bool gate or None: the
    ReLU's pass/block decision, for tests that hand the engine's own choice to the oracle where pre is within rounding of 0."""
    T = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in P.items()}
    user = np.asarray(user).reshape(-1)
    his, pred = np.asarray(his), np.asarray(pred)
    B, H, L = his.shape
    C = pred.shape[1]
    ids = torch.from_numpy(np.concatenate([his.reshape(B * H, L), pred.reshape(B * C, L)]).astype(np.int64))
    N = ids.shape[0]
    X = T["emb"][ids]
    E = X.shape[-1]
    m = _mask(drop, SITE_NEWS_IN, p, (N, L, E))
    X = X * m if m is not None else X
    pre = conv1d_same(X, T["conv_W"], T["conv_b"])
    gate = relu_gate(pre.detach().numpy()) if relu_gate is not None else None
    Y = torch.relu(pre) if gate is None else pre * torch.from_numpy(np.asarray(gate, dtype=np.float64))
    F = Y.shape[-1]
    m = _mask(drop, SITE_CONV, p, (N, L, F))
    Y = Y * m if m is not None else Y
    news, _ = masked_attlayer2(Y, ids, T["att_W"], T["att_b"], T["att_q"])
    long_u = T["user_emb"][torch.from_numpy(user.astype(np.int64))]
    hist = news[: B * H].reshape(B, H, F)
    if user_type == "ini":
        uvec = gru_keras(hist, long_u, T["gru_k"], T["gru_r"], T["gru_b"])
    else:
        short = gru_keras(hist, torch.zeros_like(long_u), T["gru_k"], T["gru_r"], T["gru_b"])
        uvec = torch.cat([short, long_u], -1) @ T["dense_W"] + T["dense_b"]
    cand = news[B * H:].reshape(B, C, F)
    scores = torch.einsum("bcf,bf->bc", cand, uvec)
    return torch.softmax(scores, -1), scores, T


def lstur_loss_and_grads(user, his, pred, y, P: dict, user_type: str, p: float, drop, loss: str = "cross_entropy_loss",
                         relu_gate=None):
    """(loss, probs, scores, {name: dL/dname}) of one training step (Keras' compiled loss, batch mean)."""
    probs, s, T = lstur_forward(user, his, pred, P, user_type, p, drop, relu_gate)
    yt = torch.from_numpy(np.asarray(y, dtype=np.float64))
    if loss == "cross_entropy_loss":
        L = -(yt * torch.log_softmax(s, -1)).sum(-1).mean()
    elif loss == "log_loss":
        L = torch.nn.functional.binary_cross_entropy_with_logits(s, yt)
    else:
        raise ValueError(loss)
    L.backward()
    return float(L.detach()), probs.detach().numpy(), s.detach().numpy(), {k: t.grad.numpy() for k, t in T.items()}


def scorer_forward(user, his, pred_one, P: dict, user_type="ini"):
    """sigmoid(cand . user) of the scorer model (lstur.py:191-200), one candidate per row."""
    _probs, s, _ = lstur_forward(user, his, pred_one, P, user_type)
    return torch.sigmoid(s).detach().numpy()

