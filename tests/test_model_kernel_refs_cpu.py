"""The float64 references of tests/model_kernel_refs.py, checked without a GPU: every backward against torch.autograd in float64 at
two shapes (1e-10 relative), and three planted defects in numpy stand-ins run through the comparator of the GPU tests -- each is
caught at one of the shapes tests/test_guarded_model_kernels_gpu.py lists and (the control aside) missed at the shape the earlier
tests used, which is the evidence that the listed shapes are the ones that matter."""
import math

import numpy as np
import pytest
import torch

from tests import model_kernel_refs as mr
from tests.guarded import guard_in

REL = 1e-10


def t64(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def same(got, want, what, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want.detach().numpy() if torch.is_tensor(want) else want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-300) if scale is None else scale
    err = float(np.abs(got - want).max())
    assert err <= REL * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("R,D,mode,p", [(5, 7, 0, 0.2), (9, 65, 1, 0.2), (4, 3, 1, 0.0), (3, 64, 0, 0.0)])
def test_layernorm_reference_vs_autograd(R, D, mode, p):
    rng = np.random.default_rng(R * 100 + D)
    X, dY = rng.normal(size=(R, D)), rng.normal(size=(R, D))
    res = rng.normal(size=(D,) if mode == 0 else (R, D))
    bias, gam, bet = (rng.normal(size=D) for _ in range(3))
    mult = (rng.random((R, D)) >= p) / (1 - p) if p > 0 else 1.0
    fwd = mr.ff_ln_fwd(X, bias, res, gam, bet, 1e-12, mode, mult)
    bwd = mr.ff_ln_bwd(dY, fwd["xhat"][0], fwd["rstd"][0], gam, mode, mult)
    x, r, b, g, be = t64(X), t64(res), t64(bias), t64(gam), t64(bet)
    m = t64(mult, False) if p > 0 else 1.0
    z = x + b + r if mode == 0 else (x + b) * m + r
    mu = z.mean(-1, keepdim=True)
    y = (z - mu) / torch.sqrt(((z - mu) ** 2).mean(-1, keepdim=True) + 1e-12) * g + be
    y = y * m if mode == 0 else y
    same(fwd["Y"][0], y, "Y")
    (y * t64(dY, False)).sum().backward()
    same(bwd["dX"][0], x.grad, "dX")
    sums = bwd["sums"][0]
    same(sums[:D], g.grad, "dgamma")
    same(sums[D:2 * D], be.grad, "dbeta")
    same(sums[2 * D:], b.grad, "dbias")
    same(bwd["dres"][0] if mode == 1 else sums[2 * D:], r.grad, "dres")


@pytest.mark.parametrize("R,C", [(4, 5), (7, 66)])
def test_gelu_reference_vs_autograd(R, C):
    rng = np.random.default_rng(R)
    X, b, dY = rng.normal(size=(R, C)) * 2, rng.normal(size=C), rng.normal(size=(R, C))
    x, bt = t64(X), t64(b)
    v = x + bt
    y = 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))
    same(mr.ff_gelu_fwd(X, b)["Y"][0], y, "Y")
    (y * t64(dY, False)).sum().backward()
    bwd = mr.ff_gelu_bwd(X, b, dY)
    same(bwd["dX"][0], x.grad, "dX")
    same(bwd["dbias"][0], bt.grad, "dbias")


@pytest.mark.parametrize("n,L,D", [(3, 5, 7), (2, 66, 4)])
def test_pooling_reference_vs_autograd(n, L, D):
    rng = np.random.default_rng(L)
    Upre, X, dout = rng.normal(size=(n, L, D)), rng.normal(size=(n, L, D)), rng.normal(size=(n, D))
    b1, w2, b2 = rng.normal(size=D) * 0.2, rng.normal(size=D) * 0.3, np.array([0.4])
    mask = (rng.random((n, L)) < 0.7).astype(np.float64)
    mask[:, 0] = 1
    mask[-1] = 0  # one dead sequence
    fwd = mr.ff_pool_fwd(Upre, b1, w2, b2, X, mask)
    u, x, b1t, w2t, b2t = t64(Upre), t64(X), t64(b1), t64(w2), t64(b2)
    e = torch.tanh(u + b1t)
    a = torch.exp(e @ w2t + b2t) * t64(mask, False)
    S = a.sum(1, keepdim=True) + 1e-8
    w = a / S
    out = (x * w.unsqueeze(2)).sum(1)
    same(fwd["out"][0], out, "out")
    same(fwd["w"][0], w, "w")
    same(fwd["sinv"][0], 1 / S[:, 0], "sinv")
    assert (fwd["out"][0][-1] == 0).all() and (fwd["w"][0][-1] == 0).all()
    (out * t64(dout, False)).sum().backward()
    bwd = mr.ff_pool_bwd(X, fwd["w"][0], fwd["sinv"][0], dout)
    same(bwd["dX"][0], x.grad, "dX (direct)")
    rest = mr.attpool_bwd_dpre(fwd["U"][0].reshape(n * L, D), w2, bwd["de"][0].reshape(-1))
    same(rest["dpre"][0].reshape(n, L, D), u.grad, "dpre")
    same(rest["dq"][0], w2t.grad, "dw2")
    same(rest["db"][0], b1t.grad, "db1")
    # autograd's d(b2) is the literal sum of de, which cancels to ~1e-8 of its terms: judged against those terms
    same(np.array([bwd["db2n"][0].sum()]), b2t.grad, "db2", scale=float(np.abs(bwd["de"][0]).sum()))
    same(np.array([bwd["db2n"][0].sum()]), np.array([bwd["de"][0].sum()]), "db2 closed form", scale=float(np.abs(bwd["de"][0]).sum()))


@pytest.mark.parametrize("N,D", [(4, 5), (6, 130)])
def test_head_reference_vs_autograd(N, D):
    rng = np.random.default_rng(D)
    u, c, W, b, ds = (rng.normal(size=s) for s in ((N, D), (N, D), (2 * D,), (1,), (N,)))
    W *= 0.2
    ut, ct, Wt, bt = t64(u), t64(c), t64(W), t64(b)
    s = torch.sigmoid(torch.cat([ut, ct], 1) @ Wt + bt)
    fwd = mr.ff_head_fwd(u, c, W, b)
    same(fwd["score"][0], s, "score")
    (s * t64(ds, False)).sum().backward()
    bwd = mr.ff_head_bwd(u, c, W, fwd["score"][0], ds)
    for k, g in (("duser", ut.grad), ("dcand", ct.grad), ("dW", Wt.grad), ("db", bt.grad)):
        same(bwd[k][0], g, k)


@pytest.mark.parametrize("n,T,D,heads,with_sv", [(2, 5, 12, 3, True), (3, 66, 8, 8, False)])
def test_attention_reference_vs_autograd(n, T, D, heads, with_sv):
    rng = np.random.default_rng(T)
    hs = D // heads
    Qr, Kr, dAO, dSV = (rng.normal(size=(n, T, D)) for _ in range(4))
    bq, bk, btr = (rng.normal(size=D) * 0.3 for _ in range(3))
    Wqa, Wka = rng.normal(size=(heads, D)) * 0.5, rng.normal(size=(heads, D)) * 0.5
    bqa, bka = rng.normal(size=heads) * 0.3, rng.normal(size=heads) * 0.3
    mask = (rng.random((n, T)) < 0.7).astype(np.float64)
    mask[:, 0] = 1
    fwd = mr.ff_attn_fwd(Qr, Kr, bq, bk, btr, Wqa, bqa, Wka, bka, mask, heads)
    tq, tk, tbq, tbk, tbtr, tWq, tWk, tbqa, tbka = (t64(a) for a in (Qr, Kr, bq, bk, btr, Wqa, Wka, bqa, bka))
    am = ((1.0 - t64(mask, False)) * -10000.0).unsqueeze(2)
    q, k = tq + tbq, tk + tbk
    a = torch.softmax((q @ tWq.T + tbqa) / math.sqrt(hs) + am, dim=1)
    pq = (a.unsqueeze(3) * q.view(n, T, heads, hs)).sum(1).reshape(n, 1, D)
    kp = k * pq
    b = torch.softmax((kp @ tWk.T + tbka) / math.sqrt(hs) + am, dim=1)
    pk = (b.unsqueeze(3) * kp.view(n, T, heads, hs)).sum(1).reshape(n, 1, D)
    ao, sv0 = pk * q, q + tbtr
    for name, want in (("AO", ao), ("SV0", sv0), ("qw", a.permute(0, 2, 1)), ("kw", b.permute(0, 2, 1)), ("pq", pq[:, 0]), ("pk", pk[:, 0])):
        same(fwd[name][0], want, name)
    loss = (ao * t64(dAO, False)).sum() + ((sv0 * t64(dSV, False)).sum() if with_sv else 0.0)
    loss.backward()
    bwd = mr.ff_attn_bwd(*(fwd[k][0] for k in ("Q", "K")), Wqa, Wka, *(fwd[k][0] for k in ("qw", "kw", "pq", "pk")), dAO, dSV if with_sv else None, heads)
    HD = heads * D
    sums = bwd["sums"][0]
    same(bwd["dQ"][0], tq.grad, "dQ")
    same(bwd["dK"][0], tk.grad, "dK")
    same(sums[:HD].reshape(heads, D), tWq.grad, "dWqa")
    same(sums[HD:2 * HD].reshape(heads, D), tWk.grad, "dWka")
    same(sums[2 * HD:2 * HD + D], tbq.grad, "dbq")
    same(sums[2 * HD + D:2 * HD + 2 * D], tbk.grad, "dbk")
    same(sums[2 * HD + 2 * D:], tbtr.grad if with_sv else np.zeros(D), "dbtr", scale=1.0)
    assert float(tbqa.grad.abs().max()) <= REL * float(tWq.grad.abs().max())  # a softmax does not see a shift


@pytest.mark.parametrize("n,L,F,A,n_drop", [(5, 4, 6, 3, 2), (3, 66, 5, 65, 3)])
def test_pap_reference_vs_autograd(n, L, F, A, n_drop):
    rng = np.random.default_rng(L)
    n_q = 4
    Upre, V, dout = rng.normal(size=(n, L, A)), rng.uniform(0, 1, (n, L, F)), rng.normal(size=(n, F))
    ba, Q = rng.normal(size=A) * 0.1, rng.normal(size=(n_q, A))
    q_idx = rng.integers(0, n_q - 1, n)  # the last query row is named by nobody
    q_idx[0], q_idx[-1] = -1, n_q        # both read row 0
    mult = (rng.random((n_drop, F)) >= 0.2) / 0.8
    fwd = mr.pap_fwd(Upre, ba, Q, q_idx, V, n_drop, mult)
    u, v, bt, Qt = t64(Upre), t64(V), t64(ba), t64(Q)
    rows = torch.as_tensor(np.where((q_idx >= 0) & (q_idx < n_q), q_idx, 0))
    U = torch.tanh(u + bt)
    w = torch.softmax((U * Qt[rows].unsqueeze(1)).sum(2), dim=1)
    out = (w.unsqueeze(2) * v).sum(1)
    same(fwd["out"][0], out, "out")
    same(fwd["out_d"][0], out[:n_drop] * t64(mult, False), "out_d")
    m_all = np.ones((n, F))
    m_all[:n_drop] = mult
    (out * t64(m_all * dout, False)).sum().backward()
    bwd = mr.pap_bwd(fwd["U"][0], Q, q_idx, V, fwd["w"][0], dout, n_drop, mult)
    same(bwd["dout"][0], m_all * dout, "gated dout")
    same(bwd["dpre"][0], u.grad, "dpre")
    same(bwd["dV"][0], v.grad, "dV (direct)")
    dQ = mr.pap_dq_reduce(bwd["dq"][0], q_idx, n_q)["dQ"][0]
    same(dQ, Qt.grad, "dQ")
    assert (dQ[n_q - 1] == 0).all()


@pytest.mark.parametrize("N,K,F,rows", [(7, 3, 5, 4), (40, 10, 66, 1)])
def test_catview_reference_vs_autograd(N, K, F, rows):
    rng = np.random.default_rng(N)
    ids = rng.integers(0, rows, N)
    ids[1], ids[2] = rows, -1
    tab, Wb, dout = rng.uniform(-0.5, 0.5, (rows, K)), rng.uniform(-0.5, 0.5, (K + 1, F)), rng.normal(size=(N, F))
    fwd = mr.naml_catview_fwd(ids, tab, Wb)
    assert fwd["oob"] and (fwd["out"][0][1] == np.maximum(Wb[K], 0)).all()
    tt, tw = t64(tab), t64(Wb)
    ok = torch.as_tensor((ids >= 0) & (ids < rows))
    e = tt[torch.as_tensor(np.clip(ids, 0, rows - 1))] * ok.unsqueeze(1)
    out = torch.relu(e @ tw[:K] + tw[K])
    same(fwd["out"][0], out, "out")
    (out * t64(dout, False)).sum().backward()
    bwd = mr.naml_catview_bwd(ids, tab, Wb, fwd["out"][0], dout)
    same(bwd["dWb"][0], tw.grad, "dWb")
    same(bwd["dtable"][0], tt.grad, "dtable")


@pytest.mark.parametrize("nv,N,F,A", [(3, 5, 6, 4), (8, 2, 66, 65)])
def test_viewatt_reference_vs_autograd(nv, N, F, A):
    rng = np.random.default_rng(nv)
    Upre, Vw, dnews = rng.normal(size=(nv, N, A)), rng.normal(size=(nv, N, F)), rng.normal(size=(N, F))
    b, q = rng.normal(size=A) * 0.1, rng.normal(size=A) * 0.3
    fwd = mr.naml_viewatt_fwd(Upre, b, q, Vw)
    u, v, bt, qt = t64(Upre), t64(Vw), t64(b), t64(q)
    a = torch.exp(torch.tanh(u + bt) @ qt)
    w = a / (a.sum(0, keepdim=True) + 1e-7)
    news = (w.unsqueeze(2) * v).sum(0)
    same(fwd["news"][0], news, "news")
    same(fwd["w"][0], w, "w")
    (news * t64(dnews, False)).sum().backward()
    bwd = mr.naml_viewatt_bwd(Vw, fwd["w"][0], dnews)
    same(bwd["dVw"][0], v.grad, "dVw (direct)")
    rest = mr.attpool_bwd_dpre(fwd["U"][0].reshape(nv * N, A), q, bwd["de"][0].reshape(-1))
    same(rest["dpre"][0].reshape(nv, N, A), u.grad, "dpre")
    same(rest["dq"][0], qt.grad, "dq")
    same(rest["db"][0], bt.grad, "db")


def test_colsum_finish_reference_and_comparator():
    p = np.arange(12, dtype=np.float64).reshape(3, 4) - 5
    r = mr.ff_colsum_finish(p, 3, 4, 3)["out"]
    np.testing.assert_array_equal(r[0], p[:, :3].sum(0))
    np.testing.assert_array_equal(r[1], np.abs(p[:, :3]).sum(0))
    mr.check_close(np.float32(r[0]), r, mr.C_SUM, "exact")
    with pytest.raises(AssertionError, match="1 NaN"):
        mr.check_close(np.array([np.nan, r[0][1], r[0][2]]), r, mr.C_SUM, "a NaN fails")
    with pytest.raises(AssertionError):  # one wrong SMALL element fails although max|err| / max|want| is tiny
        mr.check_close(np.array([1e-3, 1.0]) + np.array([1e-5, 0.0]), (np.array([1e-3, 1.0]), np.array([1e-3, 1.0])), mr.C_SUM, "small element")
    mr.check_close(np.zeros(2), (np.zeros(2), np.zeros(2)), mr.C_SUM, "exact zeros with zero magnitude")


# ------------------------------------------------------------------------------------------------------------ planted defects
def standin_ln_rowsum(X, defect):
    """Stand-in of a lane-strided row pass (64 lanes, c += 64): the row sums of X.  Defect: the loop drops its tail, c < 64 * (D // 64)."""
    R, D = X.shape
    stop = 64 * (D // 64) if defect else D
    out = np.zeros(R, np.float32)
    for lane in range(64):
        for c in range(lane, stop, 64):
            out += X[:, c]
    return out


def _ln_rowsum_case(D, defect):
    rng = np.random.default_rng(D)
    X = rng.normal(size=(5, D)).astype(np.float32) + 1
    mr.check_close(standin_ln_rowsum(X, defect), (X.astype(np.float64).sum(1), np.abs(X).astype(np.float64).sum(1)), mr.C_SUM, "row sums")


def test_defect_dropped_tail_is_caught_everywhere():
    """the control: a dropped tail of the column loop is missed at no D with D % 64 != 0, the earlier D = 48 included"""
    Ds = sorted({D for _, D, _, _ in mr.LN_CASES})
    assert 65 in Ds and mr.LN_OLD[1] == 48
    for D in Ds:
        _ln_rowsum_case(D, False)
    for D in (65, 48):
        with pytest.raises(AssertionError):
            _ln_rowsum_case(D, True)


def standin_head_dw(user, cand, score, dscore, defect):
    """Stand-in of the head backward's weight gradient: blocks of 256 columns of [user | cand].  Defect: only the first block runs."""
    N, D = user.shape
    dz = (dscore * score * (1 - score)).astype(np.float32)
    x = np.concatenate([user, cand], 1)
    dW = np.full(2 * D, np.nan, np.float32)  # the pre-fill of a guarded output
    for blk in range(1 if defect else -(-2 * D // 256)):
        for c in range(blk * 256, min(2 * D, blk * 256 + 256)):
            acc = np.float32(0)
            for n in range(N):
                acc = np.float32(acc + dz[n] * x[n, c])
            dW[c] = acc
    return dW


def _head_case(N, D, defect):
    rng = np.random.default_rng(D)
    u, c = rng.normal(size=(N, D)).astype(np.float32), rng.normal(size=(N, D)).astype(np.float32)
    s, ds = rng.uniform(0.1, 0.9, N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    ref = mr.ff_head_bwd(u, c, np.zeros(2 * D), s, ds)
    mr.check_close(standin_head_dw(u, c, s, ds, defect), ref["dW"], mr.C_SUM, "dW")


def test_defect_head_backward_first_column_block_only():
    assert mr.HEAD_OLD in mr.HEAD_CASES and (5, 129) in mr.HEAD_CASES
    for N, D in mr.HEAD_CASES:
        _head_case(N, D, False)
    _head_case(*mr.HEAD_OLD, True)  # missed at D = 48: 2 D = 96 columns are one block
    caught = []
    for N, D in mr.HEAD_CASES:
        try:
            _head_case(N, D, True)
        except AssertionError:
            caught.append(D)
    assert caught == [129, 300], caught  # 2 D > 256


def standin_ln_bwd_dbeta(dY_raw, R, D, defect):
    """Stand-in of the LayerNorm backward's dbeta partials over the operand as C sees it (flat storage, offset): min(ceil(R / 32),
    512) workgroups of rpb rows each.  Defect: a workgroup reads its first row r0 without asking whether it owns any row."""
    buf, start = dY_raw
    nb = max(1, min(-(-R // 32), 512))
    rpb = -(-max(R, 1) // nb)
    part = np.zeros((nb, D), np.float64)
    for b in range(nb):
        r0, r1 = b * rpb, min(b * rpb + rpb, R)
        rows = list(range(r0, r1))
        if defect and not rows:
            rows = [r0]
        for r in rows:
            part[b] += buf[start + r * D: start + r * D + D]
    return part.sum(0)


def _ln_bwd_case(R, D, defect):
    rng = np.random.default_rng(R)
    dY = rng.normal(size=(R, D)).astype(np.float32)
    _, h = guard_in(dY, device="cpu")
    ref = mr.ff_ln_bwd(dY, np.zeros((R, D)), np.ones(R), np.ones(D), 0)["sums"]
    with np.errstate(invalid="ignore"):
        got = standin_ln_bwd_dbeta(h.raw(), R, D, defect)
    mr.check_close(got, (ref[0][D:2 * D], ref[1][D:2 * D]), mr.C_SUM, "dbeta")
    h.check("dY")


def test_defect_layernorm_backward_reads_a_row_it_does_not_own():
    big = [(R, D) for R, D, _, _ in mr.LN_CASES if R == 16400]
    assert big and big[0] == (16400, 4)
    _ln_bwd_case(*mr.LN_OLD, False)
    _ln_bwd_case(*big[0], False)
    _ln_bwd_case(*mr.LN_OLD, True)  # missed at R = 37: both workgroups own rows
    with pytest.raises(AssertionError, match="NaN"):
        _ln_bwd_case(*big[0], True)  # workgroups 497 .. 511 start past the last row: the guard's NaN reaches dbeta
