"""Float64 references of the Fastformer, NPA-pooling and NAML model kernels (plain module: no fixtures, nothing collected).

Written from the header comments of include/ebnerd_hip.h, not from the kernels.  Every function returns a dict
`name -> (value, magnitude)`: the magnitude is the same expression with every term replaced by its absolute value (for a sum of
products `sum |a||b|`; for `ds = w (dw - sum w dw)` it is `w (|dw| + sum w |dw|)` with `|dw|` the magnitude of its own dot product),
carried through nested expressions, so that it is the scale against which the rounding of ONE float32 evaluation is judged:

    check_close:  |got - want| <= c * magnitude + TINY   element-wise, and a NaN or inf in `got` fails.

Where a function passes through tanh / exp / erf the magnitude also carries the first-order sensitivity to the rounding of the
argument (e.g. for u = tanh(x): |u| + (1 - u^2) |x|).  Backward references take what the backward KERNEL takes (the forward's saved
outputs), so a test can hand both the same float32 inputs and the comparison is of that one step alone.

The shape lists of tests/test_guarded_model_kernels_gpu.py live here as well, so that tests/test_model_kernel_refs_cpu.py can show
without a GPU which of them catch a planted defect that the earlier shapes miss."""
import math

import numpy as np

from oracle import nrms_numpy as on

TINY = 1e-30   # a subnormal-scale floor: an exact zero with a zero magnitude must still compare equal
C_SUM = 2e-6   # pure fp32 sums of products (the Conv1D weight-gradient constant of tests/test_npa_gpu.py): ~33 float32 ulps

SEED, STEP = 21, 3  # the (seed, step) of the NPA kernel tests' ebn_step_state


def _mult(site, p, n):
    """Inverted-dropout multipliers of the first n elements of `site` at (SEED, STEP)."""
    if p <= 0:
        return np.ones(n)
    return on.dropout_keep_mask(on.dropout_key(SEED, STEP, site), n, p) / (1.0 - p)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def ratio(got, want, mag):
    """max over the elements of |got - want| / (mag + TINY); inf when `got` holds a NaN / inf."""
    got, want, mag = f64(got), f64(want), f64(mag)
    assert got.shape == want.shape == mag.shape, (got.shape, want.shape, mag.shape)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        r = np.abs(got - want) / (mag + TINY)
    return float("inf") if not np.isfinite(r).all() else float(r.max())


def check_close(got, ref, c, what=""):
    """ref = (want, mag): |got - want| <= c * mag + TINY element-wise; a NaN in got FAILS (`~(err <= tol)`).  Returns max err / mag."""
    want, mag = f64(ref[0]), f64(ref[1])
    got = f64(got).reshape(want.shape)
    assert mag.shape == want.shape and (mag >= 0).all(), what
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
        tol = c * mag + TINY
        bad = ~(err <= tol)
    if bad.any():
        i = tuple(int(j) for j in np.unravel_index(int(np.argmax(bad)), bad.shape))
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} elements off ({int(np.isnan(got).sum())} NaN); first at {i}: got {got[i]!r} "
                             f"want {want[i]!r} (c * mag {tol[i]:.3e}, err / mag {err[i] / (mag[i] + TINY):.3e})")
    return ratio(got, want, mag)


# ------------------------------------------------------------------------------------------------------------ shared pieces
def _tanh(pre, mag_pre):
    u = np.tanh(pre)
    return u, np.abs(u) + (1.0 - u * u) * mag_pre


def _softmax_like(logit, mag_logit, axis, mask=None, eps=0.0, shift=False):
    """a = exp(logit) [* mask]; w = a / (sum a + eps) along `axis`.  -> w, mag_w, S (the denominator), mag_S / S."""
    z = logit - logit.max(axis, keepdims=True) if shift else logit
    a = np.exp(z)
    if mask is not None:
        a = a * mask
    scale = np.exp(-logit.max(axis, keepdims=True)) if shift else 1.0  # eps lives on the unshifted scale
    S = a.sum(axis, keepdims=True) + eps * scale
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(a > 0, a / S, 0.0)
    rel = 1.0 + mag_logit                      # relative rounding of one exp(logit): the exp itself and its argument
    relS = (w * rel).sum(axis, keepdims=True)  # ... and of the denominator
    return w, w * (rel + relS), S / scale, relS + 1.0


def _softmax_bwd(w, dw, mag_dw, axis):
    s = (w * dw).sum(axis, keepdims=True)
    ms = (w * mag_dw).sum(axis, keepdims=True)
    return w * (dw - s), w * (mag_dw + ms), s, ms


# ------------------------------------------------------------------------------------------------------------ Fastformer: LayerNorm
def ff_ln_fwd(X, bias, res, gamma, beta, eps, mode, mult=1.0):
    """mode 0: Y = mult * LN(X + bias + res[D]); mode 1: Y = LN(mult * (X + bias) + res[R, D]).  mult: [R, D] multipliers or 1."""
    X, bias, res, gamma, beta = f64(X), f64(bias), f64(res), f64(gamma), f64(beta)
    if mode == 0:
        z, mz = X + bias + res, np.abs(X) + np.abs(bias) + np.abs(res)
    else:
        z, mz = (X + bias) * mult + res, (np.abs(X) + np.abs(bias)) * mult + np.abs(res)
    mean = z.mean(-1, keepdims=True)
    d = z - mean
    rstd = 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    xhat = d * rstd
    # the row mean's rounding reaches every element; the variance sees a common shift of the row only to second order
    mxh = (mz + mz.mean(-1, keepdims=True)) * rstd + np.abs(xhat)
    y, my = gamma * xhat + beta, np.abs(gamma) * mxh + np.abs(beta)
    if mode == 0:
        y, my = y * mult, my * mult
    return dict(Y=(y, my), xhat=(xhat, mxh), rstd=(rstd[:, 0], rstd[:, 0] * (1.0 + (mxh * np.abs(xhat)).mean(-1))))


def ff_ln_bwd(dY, xhat, rstd, gamma, mode, mult=1.0):
    """-> dX, dres (mode 1), sums [3 D] = dgamma | dbeta | dbias."""
    dY, xhat, rstd, gamma = f64(dY), f64(xhat), f64(rstd).reshape(-1, 1), f64(gamma)
    R, D = dY.shape
    g = dY * mult if mode == 0 else dY
    dxh, mdxh = g * gamma, np.abs(g * gamma)
    if R:
        s1, s2 = dxh.mean(-1, keepdims=True), (dxh * xhat).mean(-1, keepdims=True)
        m1, m2 = mdxh.mean(-1, keepdims=True), (mdxh * np.abs(xhat)).mean(-1, keepdims=True)
    else:
        s1 = s2 = m1 = m2 = np.zeros((0, 1))
    dx, mdx = rstd * (dxh - s1 - xhat * s2), rstd * (mdxh + m1 + np.abs(xhat) * m2)
    out = {}
    if mode == 1:
        out["dres"] = (dx, mdx)
        dx, mdx = dx * mult, mdx * mult
    out["dX"] = (dx, mdx)
    out["sums"] = (np.concatenate([(g * xhat).sum(0), g.sum(0), dx.sum(0)]),
                   np.concatenate([np.abs(g * xhat).sum(0), np.abs(g).sum(0), mdx.sum(0)]))
    return out


def ff_colsum_finish(partials, n_parts, stride, width):
    p = f64(partials).reshape(-1)[:n_parts * stride].reshape(n_parts, stride)[:, :width]
    return dict(out=(p.sum(0), np.abs(p).sum(0)))


# ------------------------------------------------------------------------------------------------------------ Fastformer: gelu
_erf = np.vectorize(math.erf, otypes=[np.float64])


def ff_gelu_fwd(X, bias):
    X, bias = f64(X), f64(bias)
    v, mv = X + bias, np.abs(X) + np.abs(bias)
    e = _erf(v / math.sqrt(2.0)) if v.size else v
    return dict(Y=(0.5 * v * (1.0 + e), 0.5 * mv * (1.0 + np.abs(e))))


def ff_gelu_bwd(X, bias, dY):
    X, bias, dY = f64(X), f64(bias), f64(dY)
    v, mv = X + bias, np.abs(X) + np.abs(bias)
    e = _erf(v / math.sqrt(2.0)) if v.size else v
    phi = np.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
    g = 0.5 * (1.0 + e) + v * phi
    mg = 0.5 * (1.0 + np.abs(e)) + mv * phi * (2.0 + v * v)  # + the argument's rounding through g' = phi (2 - v^2)
    dX, mdX = dY * g, np.abs(dY) * mg
    return dict(dX=(dX, mdX), dbias=(dX.sum(0), mdX.sum(0)))


# ------------------------------------------------------------------------------------------------------------ Fastformer: pooling
def ff_pool_fwd(Upre, b1, w2, b2, X, mask):
    """Upre, [n, L, D] the att_fc1 product; X [n, L, D]; mask [n, L].  -> U (tanh), w [n, L], out [n, D], sinv [n]."""
    Upre, b1, w2, X, mask = f64(Upre), f64(b1), f64(w2).reshape(-1), f64(X), f64(mask)
    b2 = float(f64(b2).reshape(-1)[0])
    U, mU = _tanh(Upre + b1, np.abs(Upre) + np.abs(b1))
    logit, ml = U @ w2 + b2, mU @ np.abs(w2) + abs(b2)
    w, mw, S, relS = _softmax_like(logit, ml, 1, mask=mask, eps=1e-8)
    out, mout = np.einsum("nl,nld->nd", w, X), np.einsum("nl,nld->nd", mw, np.abs(X))
    return dict(U=(U, mU), w=(w, mw), out=(out, mout), sinv=(1.0 / S[:, 0], relS[:, 0] / S[:, 0]))


def attpool_bwd_pool(X, w, dout):
    """The direct part of an attentive pooling's backward from the saved weights: dX = w_l dout, de = w (dw - sum w dw), dw = dout . X_l.
    X [n, L, D], w [n, L], dout [n, D].  -> dX, de, and s = sum_l w_l dw_l [n] with its magnitude."""
    X, w, dout = f64(X), f64(w), f64(dout)
    dw, mdw = np.einsum("nd,nld->nl", dout, X), np.einsum("nd,nld->nl", np.abs(dout), np.abs(X))
    de, mde, s, ms = _softmax_bwd(w, dw, mdw, 1)
    dX = w[:, :, None] * dout[:, None, :]
    return dict(dX=(dX, np.abs(dX)), de=(de, mde), s=(s[:, 0], ms[:, 0]))


def ff_pool_bwd(X, w, sinv, dout):
    """+ db2n [n] = s * 1e-8 * sinv, the closed form of sum_l de_l."""
    r = attpool_bwd_pool(X, w, dout)
    k = 1e-8 * f64(sinv)
    r["db2n"] = (r["s"][0] * k, r["s"][1] * np.abs(k))
    return r


def attpool_bwd_dpre(U, q, de):
    """U [R, A] the tanh rows, de [R]: dq[k] = sum_r de_r U[r, k]; dpre = de q (1 - U^2); db[k] = sum_r dpre[r, k]."""
    U, q, de = f64(U), f64(q).reshape(-1), f64(de).reshape(-1, 1)
    dpre, mdpre = de * q * (1.0 - U * U), np.abs(de) * np.abs(q) * (1.0 + U * U)
    return dict(dq=((de * U).sum(0), np.abs(de * U).sum(0)), dpre=(dpre, mdpre), db=(dpre.sum(0), mdpre.sum(0)))


# ------------------------------------------------------------------------------------------------------------ Fastformer: head
def ff_head_fwd(user, cand, W, b):
    user, cand, W = f64(user), f64(cand), f64(W).reshape(-1)
    D = user.shape[1]
    b = float(f64(b).reshape(-1)[0])
    z, mz = user @ W[:D] + cand @ W[D:] + b, np.abs(user) @ np.abs(W[:D]) + np.abs(cand) @ np.abs(W[D:]) + abs(b)
    s = 1.0 / (1.0 + np.exp(-z))
    return dict(score=(s, s * (1.0 + (1.0 - s) * (1.0 + mz))))


def ff_head_bwd(user, cand, W, score, dscore):
    user, cand, W, s, ds = f64(user), f64(cand), f64(W).reshape(-1), f64(score), f64(dscore)
    D = user.shape[1]
    dz, mdz = ds * s * (1.0 - s), np.abs(ds) * np.abs(s) * (1.0 + np.abs(s))
    x = np.concatenate([user, cand], 1)
    return dict(duser=(dz[:, None] * W[:D], mdz[:, None] * np.abs(W[:D])), dcand=(dz[:, None] * W[D:], mdz[:, None] * np.abs(W[D:])),
                dW=(dz @ x, mdz @ np.abs(x)), db=(np.array([dz.sum()]), np.array([mdz.sum()])))


# ------------------------------------------------------------------------------------------------------------ Fastformer: attention
def _per_head(w, heads, D):
    """[n, heads, T] -> [n, T, D]: every column gets the weight of its head"""
    return np.repeat(w.transpose(0, 2, 1), D // heads, axis=2)


def ff_attn_fwd(Qraw, Kraw, bq, bk, btr, Wqa, bqa, Wka, bka, mask, heads):
    """Qraw, Kraw [n, T, D]; Wqa, Wka [heads, D]; mask [n, T].  -> Q, K, SV0, qw, kw [n, heads, T], pq, pk [n, D], AO."""
    Qraw, Kraw, bq, bk, btr, Wqa, bqa, Wka, bka, mask = (f64(a) for a in (Qraw, Kraw, bq, bk, btr, Wqa, bqa, Wka, bka, mask))
    n, T, D = Qraw.shape
    inv = 1.0 / math.sqrt(D // heads)
    am = ((1.0 - mask) * -10000.0)[:, None, :]  # [n, 1, T]
    Q, mQ = Qraw + bq, np.abs(Qraw) + np.abs(bq)
    K, mK = Kraw + bk, np.abs(Kraw) + np.abs(bk)
    lq = (np.einsum("ntd,hd->nht", Q, Wqa) + bqa[None, :, None]) * inv + am
    mlq = (np.einsum("ntd,hd->nht", mQ, np.abs(Wqa)) + np.abs(bqa)[None, :, None]) * inv + np.abs(am)
    qw, mqw, _, _ = _softmax_like(lq, mlq, 2, shift=True)
    pq, mpq = (_per_head(qw, heads, D) * Q).sum(1), (_per_head(mqw, heads, D) * mQ).sum(1)
    KP, mKP = K * pq[:, None, :], mK * mpq[:, None, :]
    lk = (np.einsum("ntd,hd->nht", KP, Wka) + bka[None, :, None]) * inv + am
    mlk = (np.einsum("ntd,hd->nht", mKP, np.abs(Wka)) + np.abs(bka)[None, :, None]) * inv + np.abs(am)
    kw, mkw, _, _ = _softmax_like(lk, mlk, 2, shift=True)
    pk, mpk = (_per_head(kw, heads, D) * KP).sum(1), (_per_head(mkw, heads, D) * mKP).sum(1)
    return dict(Q=(Q, mQ), K=(K, mK), SV0=(Q + btr, mQ + np.abs(btr)), qw=(qw, mqw), kw=(kw, mkw), pq=(pq, mpq), pk=(pk, mpk),
                AO=(pk[:, None, :] * Q, mpk[:, None, :] * mQ))


def ff_attn_bwd(Q, K, Wqa, Wka, qw, kw, pq, pk, dAO, dSV, heads):
    """From the forward's saved Q, K (biased), qw, kw, pq, pk.  -> dQ, dK [n, T, D] and
    sums [2 heads D + 3 D] = dWqa | dWka | colsum(dQ) | colsum(dK) | colsum(dSV)."""
    Q, K, Wqa, Wka, qw, kw, pq, pk, dAO = (f64(a) for a in (Q, K, Wqa, Wka, qw, kw, pq, pk, dAO))
    n, T, D = Q.shape
    hd = D // heads
    inv = 1.0 / math.sqrt(hd)
    aQ, aK, aWq, aWk, apq, apk, aA = (np.abs(a) for a in (Q, K, Wqa, Wka, pq, pk, dAO))
    heads_of = lambda x: x.reshape(n, T, heads, hd).sum(3).transpose(0, 2, 1)  # [n, T, D] -> per-head column sums [n, heads, T]
    KP, aKP = K * pq[:, None, :], aK * apq[:, None, :]
    dpk, mdpk = (dAO * Q).sum(1), (aA * aQ).sum(1)
    dkw, mdkw = heads_of(dpk[:, None, :] * KP), heads_of(mdpk[:, None, :] * aKP)
    dlk, mdlk, _, _ = _softmax_bwd(kw, dkw, mdkw, 2)
    dKP = _per_head(kw, heads, D) * dpk[:, None, :] + inv * np.einsum("nht,hd->ntd", dlk, Wka)
    mdKP = _per_head(kw, heads, D) * mdpk[:, None, :] + inv * np.einsum("nht,hd->ntd", mdlk, aWk)
    dK, mdK = dKP * pq[:, None, :], mdKP * apq[:, None, :]
    dWka, mdWka = inv * np.einsum("nht,ntd->hd", dlk, KP), inv * np.einsum("nht,ntd->hd", mdlk, aKP)
    dpq, mdpq = (dKP * K).sum(1), (mdKP * aK).sum(1)
    dqw, mdqw = heads_of(dpq[:, None, :] * Q), heads_of(mdpq[:, None, :] * aQ)
    dlq, mdlq, _, _ = _softmax_bwd(qw, dqw, mdqw, 2)
    dQ = dAO * pk[:, None, :] + _per_head(qw, heads, D) * dpq[:, None, :] + inv * np.einsum("nht,hd->ntd", dlq, Wqa)
    mdQ = aA * apk[:, None, :] + _per_head(qw, heads, D) * mdpq[:, None, :] + inv * np.einsum("nht,hd->ntd", mdlq, aWq)
    dWqa, mdWqa = inv * np.einsum("nht,ntd->hd", dlq, Q), inv * np.einsum("nht,ntd->hd", mdlq, aQ)
    if dSV is not None:
        dSV = f64(dSV)
        dQ, mdQ = dQ + dSV, mdQ + np.abs(dSV)
        cs, mcs = dSV.sum((0, 1)), np.abs(dSV).sum((0, 1))
    else:
        cs = mcs = np.zeros(D)
    return dict(dQ=(dQ, mdQ), dK=(dK, mdK),
                sums=(np.concatenate([dWqa.ravel(), dWka.ravel(), dQ.sum((0, 1)), dK.sum((0, 1)), cs]),
                      np.concatenate([mdWqa.ravel(), mdWka.ravel(), mdQ.sum((0, 1)), mdK.sum((0, 1)), mcs])))


# ------------------------------------------------------------------------------------------------------------ NPA: personalised pooling
def pap_rows(q_idx, n_q):
    """the query row of every sequence: an index outside [0, n_q) reads row 0"""
    q_idx = np.asarray(q_idx).astype(np.int64)
    return np.where((q_idx >= 0) & (q_idx < n_q), q_idx, 0)


def pap_fwd(Upre, ba, Q, q_idx, V, n_drop=0, mult=None):
    """Upre [n, L, A] = Vd . Wa; Q [n_q, A]; V [n, L, F]; mult [n_drop, F].  -> U (tanh), w [n, L], out [n, F], out_d [n_drop, F]."""
    Upre, ba, Q, V = f64(Upre), f64(ba), f64(Q), f64(V)
    q = Q[pap_rows(q_idx, Q.shape[0])]
    U, mU = _tanh(Upre + ba, np.abs(Upre) + np.abs(ba))
    s, ms = np.einsum("nla,na->nl", U, q), np.einsum("nla,na->nl", mU, np.abs(q))
    w, mw, _, _ = _softmax_like(s, ms, 1, shift=True)
    out, mout = np.einsum("nl,nlf->nf", w, V), np.einsum("nl,nlf->nf", mw, np.abs(V))
    m = np.ones((n_drop, V.shape[2])) if mult is None else f64(mult)
    return dict(U=(U, mU), w=(w, mw), out=(out, mout), out_d=(out[:n_drop] * m, mout[:n_drop] * m))


def pap_bwd(U, Q, q_idx, V, w, dout, n_drop=0, mult=None):
    """U [n, L, A] the tanh rows, w [n, L] the saved weights.  -> dout (gated), dq [n, A], dpre [n, L, A], dV [n, L, F]."""
    U, Q, V, w, d = f64(U), f64(Q), f64(V), f64(w), f64(dout).copy()
    q = Q[pap_rows(q_idx, Q.shape[0])]
    if mult is not None:
        d[:n_drop] *= f64(mult)
    dw, mdw = np.einsum("nf,nlf->nl", d, V), np.einsum("nf,nlf->nl", np.abs(d), np.abs(V))
    ds, mds, _, _ = _softmax_bwd(w, dw, mdw, 1)
    dV = w[:, :, None] * d[:, None, :]
    return dict(dout=(d, np.abs(d)), dq=(np.einsum("nl,nla->na", ds, U), np.einsum("nl,nla->na", mds, np.abs(U))),
                dpre=(ds[:, :, None] * q[:, None, :] * (1.0 - U * U), mds[:, :, None] * np.abs(q)[:, None, :] * (1.0 + U * U)),
                dV=(dV, np.abs(dV)))


def pap_dq_reduce(dq, q_idx, n_q):
    dq = f64(dq)
    rows = pap_rows(q_idx, n_q)
    out, mag = np.zeros((n_q, dq.shape[1])), np.zeros((n_q, dq.shape[1]))
    np.add.at(out, rows, dq)
    np.add.at(mag, rows, np.abs(dq))
    return dict(dQ=(out, mag))


# ------------------------------------------------------------------------------------------------------------ NAML
def _cat_rows(ids, table):
    ids, table = np.asarray(ids).astype(np.int64), f64(table)
    ok = (ids >= 0) & (ids < table.shape[0])
    return ok, np.where(ok[:, None], table[np.clip(ids, 0, table.shape[0] - 1)], 0.0)


def naml_catview_fwd(ids, table, Wb):
    """One view: out = relu(table[ids] . Wb[:K] + Wb[K]); an id outside the table reads a zero row.  Also `oob` (any id outside)."""
    Wb = f64(Wb)
    K = Wb.shape[0] - 1
    ok, e = _cat_rows(ids, table)
    pre, mag = e @ Wb[:K] + Wb[K], np.abs(e) @ np.abs(Wb[:K]) + np.abs(Wb[K])
    return dict(out=(np.maximum(pre, 0.0), mag), pre=(pre, mag), oob=bool((~ok).any()))


def naml_catview_bwd(ids, table, Wb, out, dout):
    """`out` is the FORWARD KERNEL's output: the ReLU gate is out > 0.  -> dWb [K + 1, F], dtable [rows, K]."""
    Wb, dout = f64(Wb), f64(dout)
    K = Wb.shape[0] - 1
    ok, e = _cat_rows(ids, table)
    dY = dout * (f64(out) > 0)
    de, mde = dY @ Wb[:K].T, np.abs(dY) @ np.abs(Wb[:K]).T
    rows = np.asarray(table).shape[0]
    dt, mdt = np.zeros((rows, K)), np.zeros((rows, K))
    idx = np.asarray(ids).astype(np.int64)[ok]
    np.add.at(dt, idx, de[ok])
    np.add.at(mdt, idx, mde[ok])
    return dict(dWb=(np.concatenate([e.T @ dY, dY.sum(0, keepdims=True)]), np.concatenate([np.abs(e).T @ np.abs(dY), np.abs(dY).sum(0, keepdims=True)])),
                dtable=(dt, mdt))


def naml_viewatt_fwd(Upre, b, q, Vw):
    """Upre [nv, N, A], Vw [nv, N, F].  -> U (tanh), w [nv, N], news [N, F]."""
    Upre, b, q, Vw = f64(Upre), f64(b), f64(q).reshape(-1), f64(Vw)
    U, mU = _tanh(Upre + b, np.abs(Upre) + np.abs(b))
    w, mw, _, _ = _softmax_like(U @ q, mU @ np.abs(q), 0, eps=1e-7)
    return dict(U=(U, mU), w=(w, mw), news=(np.einsum("vn,vnf->nf", w, Vw), np.einsum("vn,vnf->nf", mw, np.abs(Vw))))


def naml_viewatt_bwd(Vw, w, dnews):
    """-> dVw [nv, N, F] (the direct term), de [nv, N]."""
    r = attpool_bwd_pool(f64(Vw).transpose(1, 0, 2), f64(w).T, dnews)
    return dict(dVw=tuple(a.transpose(1, 0, 2) for a in r["dX"]), de=tuple(a.T for a in r["de"]))


# ------------------------------------------------------------------------------------------------------------ the shapes of the GPU tests
# Each list covers every value of its axis at least once: the smallest sizes at which each lane-strided loop takes no, one and a
# second trip, each limit from both sides, and each size at which the host code takes another path.
LN_CASES = [  # (R, D, mode, p)
    (1, 1, 0, 0.0), (5, 48, 1, 0.2), (37, 64, 0, 0.2), (5, 65, 1, 0.0), (37, 1024, 1, 0.2), (1, 65, 0, 0.2), (37, 48, 0, 0.0),
    (16400, 4, 1, 0.2), (16400, 4, 0, 0.0)]  # 512 workgroups of 33 rows: those from 497 on own no rows
LN_OLD = (37, 48)
COLSUM_CASES = [(1, 70, 64), (3, 70, 65), (4, 131, 129), (5, 9, 1)]  # (n_parts, stride, width), stride > width
GELU_CASES = [(1, 1), (3, 85), (1, 257), (70, 40), (33, 65), (32 * 1024 + 32, 1)]  # the last: 1024 row blocks of 33, the tail ones empty
POOL_CASES = [  # (n_seq, L, D, mask kind)
    (1, 1, 1, "ones"), (3, 64, 65, "one_dead"), (3, 65, 64, "first"), (1, 257, 257, "last"), (3, 13, 48, "one_dead"), (1, 4096, 4, "ones"),
    (3, 65, 257, "random")]
HEAD_CASES = [(1, 1), (11, 48), (5, 128), (5, 129), (11, 300)]  # (N, D)
HEAD_OLD = (11, 48)
ATTN_CASES = [  # (n_seq, T, D, heads, SV0 / dSV given, with backward)
    (2, 1, 4, 1, True, True), (3, 13, 48, 3, False, True), (2, 70, 48, 3, True, True), (3, 7, 8, 8, False, True), (2, 9, 1024, 4, True, True),
    (2, 53, 256, 16, True, False), (2, 47, 256, 16, False, True), (257, 3, 8, 2, True, True)]
PAP_CASES = [  # (n_seq, L, F, A, n_drop, out_d given, dV given)
    (1, 1, 3, 1, 0, True, True), (7, 5, 256, 63, 3, True, False), (7, 64, 257, 64, 7, True, True), (7, 65, 400, 65, 3, False, True),
    (1, 256, 3, 257, 1, True, True), (1, 1, 4096, 64, 1, True, True)]
BIAS_TANH_CASES = [(1, 1), (5, 65), (1, 257), (5, 257)]  # (n_rows, A)
CATVIEW_CASES = [  # (N, K0, K1, F, rows0, rows1, kind)
    (1, 1, 256, 1, 1, 5, "plain"), (16, 10, 12, 24, 7, 13, "oob"), (17, 256, 3, 257, 5, 1, "plain"), (32, 10, 12, 257, 7, 13, "noflag"),
    (33, 1, 256, 24, 9, 4, "all_oob"), (33, 10, 12, 1, 7, 13, "plain")]
VIEWATT_CASES = [(1, 1, 1, 1), (3, 4, 63, 64), (8, 5, 65, 65), (8, 4, 400, 1), (3, 5, 400, 64)]  # (n_views, N, F, A)
