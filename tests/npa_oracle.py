"""Float64 restatement of NPA (reference npa.py, layers.py:312-339) over the engine's title layout, for the NPA tests.

The forward is written with torch ops in float64 and differentiated by autograd; dropout masks are the build's counter stream
(oracle.nrms_numpy.dropout_keep_mask) at the engine's element indices:
  site 0  Dropout(p) of the embedded tokens        index (n*T + t)*E + e   (n: title in engine order, history first)
  site 2  Dropout(p) after the Conv1D              index (n*T + t)*F + f
  site 3  Dropout(0.2) at the news pooling input   index (n*T + t)*F + f
  site 4  Dropout(0.2) at the user pooling input   index (b*H + h)*F + f
Parameters are a dict of float64 numpy arrays: emb (V,E), user_emb (n_users+1,Du), conv_W (window,E,F), conv_b (F,),
n_Wq (Du,A), n_bq (A,), n_Wa (F,A), n_ba (A,), u_Wq, u_bq, u_Wa, u_ba -- the engine's get_weights() order is WEIGHT_ORDER.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.nrms_numpy import dropout_keep_mask

WEIGHT_ORDER = ["emb", "user_emb", "conv_W", "conv_b", "n_Wq", "n_bq", "n_Wa", "n_ba", "u_Wq", "u_bq", "u_Wa", "u_ba"]
SITE_NEWS_IN, SITE_CONV, SITE_NEWS_PAP, SITE_USER_PAP = 0, 2, 3, 4
PAP_P = 0.2


def conv1d_same(X: torch.Tensor, W: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Keras Conv1D(padding="same") without activation: X (N,T,E), W (window,E,F), b (F,) -> (N,T,F).  The left pad is
    (window-1)//2 rows, the right pad the rest; padded rows are zeros."""
    N, T, E = X.shape
    win = W.shape[0]
    pl = (win - 1) // 2
    Xp = torch.cat([X.new_zeros(N, pl, E), X, X.new_zeros(N, win - 1 - pl, E)], 1)
    return sum(Xp[:, j:j + T] @ W[j] for j in range(win)) + b


def conv1d_loop(X: np.ndarray, W: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The same convolution as explicit loops (the definition the tests hold conv1d_same to)."""
    N, T, E = X.shape
    win, _, F = W.shape
    pl = (win - 1) // 2
    out = np.zeros((N, T, F))
    for n in range(N):
        for t in range(T):
            acc = b.astype(np.float64).copy()
            for j in range(win):
                s = t + j - pl
                if 0 <= s < T:
                    acc += X[n, s] @ W[j]
            out[n, t] = acc
    return out


def random_params(V, E, n_users, Du, F, A, window, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    g = lambda *s: rng.uniform(-1, 1, size=s) * np.sqrt(6.0 / (s[0] + s[-1])) * scale
    return {"emb": rng.uniform(-0.5, 0.5, (V, E)), "user_emb": rng.uniform(-0.5, 0.5, (n_users + 1, Du)),
            "conv_W": rng.uniform(-1, 1, (window, E, F)) * np.sqrt(6.0 / (window * (E + F))), "conv_b": rng.uniform(-0.1, 0.1, F),
            "n_Wq": g(Du, A), "n_bq": rng.uniform(-0.1, 0.1, A), "n_Wa": g(F, A), "n_ba": rng.uniform(-0.1, 0.1, A),
            "u_Wq": g(Du, A), "u_bq": rng.uniform(-0.1, 0.1, A), "u_Wa": g(F, A), "u_ba": rng.uniform(-0.1, 0.1, A)}


def _mask(drop, site, p, shape):
    """inverted-dropout multiplier (float64) of `site` over a tensor of `shape`, or None when off"""
    if drop is None or p <= 0:
        return None
    keep = dropout_keep_mask(drop.key(site), int(np.prod(shape)), p).reshape(shape)
    return torch.from_numpy(keep.astype(np.float64) / (1.0 - p))


def pap(V: torch.Tensor, q: torch.Tensor, Wa, ba):
    """PersonalizedAttentivePooling after its input dropout: V (n,L,F), q (n,A) -> (n,F), w (n,L)."""
    U = torch.tanh(V @ Wa + ba)
    w = torch.softmax(torch.einsum("nla,na->nl", U, q), -1)
    return torch.einsum("nl,nlf->nf", w, V), w


def npa_forward(user, his, pred, P: dict, p: float = 0.0, drop=None, relu_gate=None):
    """(probs (B,C), scores (B,C), tensors of P) -- tensors with requires_grad for npa_loss_and_grads.  drop: an
    oracle.nrms_numpy.Drop (training) or None (inference).  relu_gate(pre (N,T,F) float64 numpy) -> bool gate or None: the
    ReLU's pass/block decision, for tests that hand the engine's own choice to the oracle where pre is within rounding of 0."""
    T = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in P.items()}
    user = np.asarray(user).reshape(-1)
    his, pred = np.asarray(his), np.asarray(pred)
    B, H, L = his.shape
    C = pred.shape[1]
    ids = torch.from_numpy(np.concatenate([his.reshape(B * H, L), pred.reshape(B * C, L)]).astype(np.int64))
    imp = torch.from_numpy(np.concatenate([np.repeat(np.arange(B), H), np.repeat(np.arange(B), C)]))
    N = ids.shape[0]
    X = T["emb"][ids]
    E = X.shape[-1]
    m = _mask(drop, SITE_NEWS_IN, p, (N, L, E))
    X = X * m if m is not None else X
    pre = conv1d_same(X, T["conv_W"], T["conv_b"])
    gate = relu_gate(pre.detach().numpy()) if relu_gate is not None else None
    Y = torch.relu(pre) if gate is None else pre * torch.from_numpy(np.asarray(gate, dtype=np.float64))
    F = Y.shape[-1]
    for site, pp in ((SITE_CONV, p), (SITE_NEWS_PAP, PAP_P)):
        m = _mask(drop, site, pp, (N, L, F))
        Y = Y * m if m is not None else Y
    e = T["user_emb"][torch.from_numpy(user.astype(np.int64))]
    qn = e @ T["n_Wq"] + T["n_bq"]
    qu = e @ T["u_Wq"] + T["u_bq"]
    news, _ = pap(Y, qn[imp], T["n_Wa"], T["n_ba"])
    hist = news[: B * H].reshape(B, H, F)
    m = _mask(drop, SITE_USER_PAP, PAP_P, (B, H, F))
    hist = hist * m if m is not None else hist
    uvec, _ = pap(hist, qu, T["u_Wa"], T["u_ba"])
    cand = news[B * H:].reshape(B, C, F)
    scores = torch.einsum("bcf,bf->bc", cand, uvec)
    return torch.softmax(scores, -1), scores, T


def npa_loss_and_grads(user, his, pred, y, P: dict, p: float, drop, loss: str = "cross_entropy_loss", relu_gate=None):
    """(loss, probs, {name: dL/dname}) of one training step (Keras' compiled loss, batch mean)."""
    probs, s, T = npa_forward(user, his, pred, P, p, drop, relu_gate)
    yt = torch.from_numpy(np.asarray(y, dtype=np.float64))
    if loss == "cross_entropy_loss":
        L = -(yt * torch.log_softmax(s, -1)).sum(-1).mean()
    elif loss == "log_loss":
        L = torch.nn.functional.binary_cross_entropy_with_logits(s, yt)
    else:
        raise ValueError(loss)
    L.backward()
    return float(L.detach()), probs.detach().numpy(), {k: t.grad.numpy() for k, t in T.items()}


def scorer_forward(user, his, pred_one, P: dict):
    """sigmoid(cand . user) of the scorer model (npa.py:188-199), one candidate per row."""
    _probs, s, _ = npa_forward(user, his, pred_one, P)
    return torch.sigmoid(s).detach().numpy()
