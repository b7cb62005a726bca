"""Float64 restatement of NAML (reference naml.py, layers.py:55-81) over the engine's article layout, for the NAML tests.

The forward is written with torch ops in float64 and differentiated by autograd; dropout masks are the build's counter stream
(oracle.nrms_numpy.dropout_keep_mask) at the engine's element indices (n: article in engine order, history first):
  site 0  Dropout(p) of the embedded title tokens   index (n*T + t)*E + e
  site 2  Dropout(p) after the title Conv1D          index (n*T + t)*F + f
  site 5  Dropout(p) of the embedded body tokens    index (n*Tb + t)*E + e
  site 6  Dropout(p) after the body Conv1D           index (n*Tb + t)*F + f
Parameters are a dict of float64 numpy arrays in the engine's get_weights() order (WEIGHT_ORDER); AttLayer2 q is (A, 1).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.nrms_numpy import dropout_keep_mask
from tests.npa_oracle import conv1d_same

WEIGHT_ORDER = ["emb", "t_conv_W", "t_conv_b", "t_att_W", "t_att_b", "t_att_q", "b_conv_W", "b_conv_b", "b_att_W", "b_att_b",
                "b_att_q", "v_emb", "v_W", "v_b", "s_emb", "s_W", "s_b", "va_W", "va_b", "va_q", "u_W", "u_b", "u_q"]
SITE_TITLE_IN, SITE_TITLE_CONV, SITE_BODY_IN, SITE_BODY_CONV = 0, 2, 5, 6
KERAS_EPS = 1e-7


def random_params(V, E, F, A, window, n_vert, Kv, n_sub, Ks, seed=0):
    rng = np.random.default_rng(seed)
    g = lambda *s: rng.uniform(-1, 1, size=s) * np.sqrt(6.0 / (s[0] + s[-1]))
    u = lambda *s: rng.uniform(-0.1, 0.1, s)
    conv = lambda: rng.uniform(-1, 1, (window, E, F)) * np.sqrt(6.0 / (window * (E + F)))
    return {"emb": rng.uniform(-0.5, 0.5, (V, E)), "t_conv_W": conv(), "t_conv_b": u(F), "t_att_W": g(F, A), "t_att_b": u(A),
            "t_att_q": g(A, 1), "b_conv_W": conv(), "b_conv_b": u(F), "b_att_W": g(F, A), "b_att_b": u(A), "b_att_q": g(A, 1),
            "v_emb": rng.uniform(-0.5, 0.5, (n_vert, Kv)), "v_W": g(Kv, F), "v_b": u(F),
            "s_emb": rng.uniform(-0.5, 0.5, (n_sub, Ks)), "s_W": g(Ks, F), "s_b": u(F),
            "va_W": g(F, A), "va_b": u(A), "va_q": g(A, 1), "u_W": g(F, A), "u_b": u(A), "u_q": g(A, 1)}


def _mask(drop, site, p, shape):
    """inverted-dropout multiplier (float64) of `site` over a tensor of `shape`, or None when off"""
    if drop is None or p <= 0:
        return None
    keep = dropout_keep_mask(drop.key(site), int(np.prod(shape)), p).reshape(shape)
    return torch.from_numpy(keep.astype(np.float64) / (1.0 - p))


def att_layer2(x: torch.Tensor, W, b, q):
    """AttLayer2 (layers.py:55-81): x (n, L, F) -> (n, F), w (n, L); exp without max-subtraction, / (sum + 1e-7)."""
    a = torch.exp((torch.tanh(x @ W + b) @ q)[..., 0])
    w = a / (a.sum(-1, keepdim=True) + KERAS_EPS)
    return torch.einsum("nl,nlf->nf", w, x), w


def _text_view(T, ids, key, p, drop, s_in, s_conv, relu_gate):
    X = T["emb"][torch.from_numpy(ids.astype(np.int64))]
    m = _mask(drop, s_in, p, tuple(X.shape))
    X = X * m if m is not None else X
    pre = conv1d_same(X, T[key + "_conv_W"], T[key + "_conv_b"])
    gate = relu_gate(key, pre.detach().numpy()) if relu_gate is not None else None
    Y = torch.relu(pre) if gate is None else pre * torch.from_numpy(np.asarray(gate, dtype=np.float64))
    m = _mask(drop, s_conv, p, tuple(Y.shape))
    Y = Y * m if m is not None else Y
    return att_layer2(Y, T[key + "_att_W"], T[key + "_att_b"], T[key + "_att_q"])[0]


def news_encoder(T: dict, title, body, vert, subvert, p=0.0, drop=None, relu_gate=None):
    """(N, F) news vectors of N articles: title (N,T), body (N,Tb), vert (N,), subvert (N,) integer arrays."""
    t = _text_view(T, np.asarray(title), "t", p, drop, SITE_TITLE_IN, SITE_TITLE_CONV, relu_gate)
    bo = _text_view(T, np.asarray(body), "b", p, drop, SITE_BODY_IN, SITE_BODY_CONV, relu_gate)
    v = torch.relu(T["v_emb"][torch.from_numpy(np.asarray(vert).astype(np.int64))] @ T["v_W"] + T["v_b"])
    s = torch.relu(T["s_emb"][torch.from_numpy(np.asarray(subvert).astype(np.int64))] @ T["s_W"] + T["s_b"])
    views = torch.stack([t, bo, v, s], 1)  # Concatenate(axis=-2) of the four (1, F) views
    return att_layer2(views, T["va_W"], T["va_b"], T["va_q"])[0]


def naml_forward(xs, P: dict, p: float = 0.0, drop=None, relu_gate=None):
    """(probs (B,C), scores (B,C), tensors of P) for the 8 inputs xs -- tensors with requires_grad for naml_loss_and_grads.
    drop: an oracle.nrms_numpy.Drop (training) or None (inference).  relu_gate(view "t"/"b", pre float64 numpy) -> bool gate
    or None: the Conv1D ReLU's decision, for tests that hand the engine's own choice to the oracle where pre is within rounding
    of 0."""
    T = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in P.items()}
    ht, hb, hv, hs, pt, pb, pv, ps = (np.asarray(a) for a in xs)
    B, H = ht.shape[:2]
    C = pt.shape[1]
    cat = lambda h, c, w: np.concatenate([h.reshape(B * H, w), c.reshape(B * C, w)])
    news = news_encoder(T, cat(ht, pt, ht.shape[2]), cat(hb, pb, hb.shape[2]), cat(hv, pv, 1)[:, 0], cat(hs, ps, 1)[:, 0], p,
                        drop, relu_gate)
    F = news.shape[1]
    user, _ = att_layer2(news[: B * H].reshape(B, H, F), T["u_W"], T["u_b"], T["u_q"])
    cand = news[B * H:].reshape(B, C, F)
    scores = torch.einsum("bcf,bf->bc", cand, user)
    return torch.softmax(scores, -1), scores, T


def naml_loss_and_grads(xs, y, P: dict, p: float, drop, loss: str = "cross_entropy_loss", relu_gate=None):
    """(loss, probs, scores, {name: dL/dname}) of one training step (Keras' compiled loss, batch mean)."""
    probs, s, T = naml_forward(xs, P, p, drop, relu_gate)
    yt = torch.from_numpy(np.asarray(y, dtype=np.float64))
    if loss == "cross_entropy_loss":
        L = -(yt * torch.log_softmax(s, -1)).sum(-1).mean()
    elif loss == "log_loss":
        L = torch.nn.functional.binary_cross_entropy_with_logits(s, yt)
    else:
        raise ValueError(loss)
    L.backward()
    return float(L.detach()), probs.detach().numpy(), s.detach().numpy(), {k: t.grad.numpy() for k, t in T.items()}


def scorer_forward(xs, P: dict):
    """sigmoid(cand . user) of the scorer model, one candidate per row (pred_* of shape (N, 1, .))."""
    _probs, s, _ = naml_forward(xs, P)
    return torch.sigmoid(s).detach().numpy()
