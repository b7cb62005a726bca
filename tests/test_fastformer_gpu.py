"""Fastformer on the MI355X: every new kernel pair against float64 at shapes that are no tile multiples (twice, bit-equal), the shape
gates, and the model against what the REFERENCE computed (tests/golden/fastformer_ref_*.npz) within 4 x the reference's own float32
error: the HIP path is another float32 evaluation of the same formulas with other summation orders.

Measured on an MI355X with this fixture (E_fwd 2.6e-8, E_ref 8.3e-5, E_traj 4.8e-7 from the reference's float32 run): scores within
2.6e-8 of the float64 reference, loss within 8.0e-8, worst gradient measure 3.1e-6 (user_attention_polling.att_fc1.bias), worst
trajectory measure 1.7e-7; with per_slot masks and dropout 0.2 against the float64 oracle: scores 1.7e-8, gradients 3.2e-6.  Each
test prints its figures before it asserts."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import nrms_numpy as on
from tests import fastformer_oracle as fo
from tests.hip_testutil import P, S, dev, host
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture of the reference loader test)
from tests.test_fastformer_cpu import GOLDEN, load_golden, make_model

from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_INVIEW_ARTICLES_COL

pytestmark = pytest.mark.gpu
f32 = ctypes.c_float


def rel(got, want):
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64) if isinstance(got, np.ndarray) else host(got)
    return float(np.abs(got.reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-30))


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("mode,p", [(0, 0.0), (0, 0.2), (1, 0.0), (1, 0.2)])
def test_layernorm_pair_vs_float64(hip, mode, p):
    rng = np.random.default_rng(3 + mode)
    R, D, eps, seed, step, site = 37, 48, 1e-12, 9, 4, 2
    X, res = rng.normal(size=(R, D)).astype(np.float32), rng.normal(size=(D,) if mode == 0 else (R, D)).astype(np.float32)
    bias, gam, bet = (rng.normal(size=D).astype(np.float32) for _ in range(3))
    dY = rng.normal(size=(R, D)).astype(np.float32)
    key = on.dropout_key(seed, step, site)
    d = {k: dev(v) for k, v in dict(X=X, res=res, bias=bias, gam=gam, bet=bet, dY=dY).items()}
    outs = []
    for _ in range(2):
        Y, xh, rs = torch.empty(R, D, device="cuda"), torch.empty(R, D, device="cuda"), torch.empty(R, device="cuda")
        hip.call("ebn_ff_ln_fwd_f32", P(d["X"]), P(d["bias"]), P(d["res"]), P(d["gam"]), P(d["bet"]), f32(eps), mode, key, f32(p), P(Y), P(xh),
                 P(rs), R, D, S())
        dX, dres = torch.empty(R, D, device="cuda"), torch.zeros(R, D, device="cuda")  # mode 0 does not write dres
        part = torch.empty(int(hip.lib().ebn_ff_ln_partials_len(R, D)), device="cuda")
        n = ctypes.c_int32(0)
        hip.call("ebn_ff_ln_bwd_f32", P(d["dY"]), P(xh), P(rs), P(d["gam"]), mode, key, f32(p), P(dX), P(dres), P(part), ctypes.byref(n), R, D, S())
        sums = torch.empty(3 * D, device="cuda")
        hip.call("ebn_ff_colsum_finish_f32", P(part), n.value, 3 * D, 3 * D, P(sums), S())
        torch.cuda.synchronize()
        outs.append([host(t) for t in (Y, dX, dres, sums)])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    m = fo.drop_mult((R, D), seed, step, site, p, torch.float64, "cpu") if p > 0 else 1.0
    x, r, b, g, be = t64(X, True), t64(res, True), t64(bias, True), t64(gam, True), t64(bet, True)
    y = fo.layer_norm(x + b + r, g, be, eps) * m if mode == 0 else fo.layer_norm((x + b) * m + r, g, be, eps)
    (y * t64(dY)).sum().backward()
    Y, dX, dres, sums = outs[0]
    assert rel(Y, y.detach()) < 2e-6
    assert rel(dX, x.grad) < 1e-5
    assert rel(sums[:D], g.grad) < 1e-5 and rel(sums[D:2 * D], be.grad) < 1e-5 and rel(sums[2 * D:], b.grad) < 1e-5
    if mode == 1:
        assert rel(dres, r.grad) < 1e-5
    else:
        assert rel(sums[2 * D:], r.grad) < 1e-5  # the broadcast row's gradient is the bias gradient
    if p > 0:
        # kept fraction of the site: mode 0 drops the output itself; mode 1 drops the LayerNorm's input, visible as dX == dres * mult
        kept = float((Y != 0).mean()) if mode == 0 else float((dX != 0)[dres != 0].mean())
        assert abs(kept - (1 - p)) < 3 * math.sqrt(p * (1 - p) / (R * D)), kept


@pytest.mark.parametrize("T,D,heads,n_seq", [(13, 48, 3, 5), (1, 48, 3, 3), (30, 256, 16, 300)])
def test_attention_pair_vs_float64(hip, T, D, heads, n_seq):
    rng = np.random.default_rng(T * 7 + D)
    sc = 1.0 / math.sqrt(D)
    names = ["query", "key", "transform"]
    Pm = {}
    for nm in names:
        Pm[f"a.{nm}.weight"], Pm[f"a.{nm}.bias"] = rng.normal(size=(D, D)) * sc, rng.normal(size=D) * 0.3
    for nm in ("query_att", "key_att"):
        Pm[f"a.{nm}.weight"], Pm[f"a.{nm}.bias"] = rng.normal(size=(heads, D)) * 0.5, rng.normal(size=heads) * 0.3
    Pm = {k: v.astype(np.float32) for k, v in Pm.items()}
    Pm["a.transform.weight"] = np.eye(D, dtype=np.float32)  # the kernel stops before `transform`: identity keeps the oracle comparable
    x = rng.normal(size=(n_seq, T, D)).astype(np.float32)
    mask = (rng.random((n_seq, T)) < 0.7).astype(np.float32)
    mask[:, 0] = 1  # no all-padding sequence here: its logits are -10000 + x in float32 (ulp 1e-3), which float64 does not mimic;
    mask[-1] = 1    # the model tests cover such sequences (their pooled vectors are exactly zero)
    dout = rng.normal(size=(n_seq, T, D)).astype(np.float32)
    # float64 reference: out = AO + btr + q  (transform = identity), so d(out)/dAO = dout and dSV = dout as well
    Pt = {k: t64(v, True) for k, v in Pm.items()}
    xt = t64(x)
    q64 = (xt @ Pt["a.query.weight"].T).detach()
    k64 = (xt @ Pt["a.key.weight"].T).detach()
    qin, kin = q64.clone().requires_grad_(True), k64.clone().requires_grad_(True)

    def core2(qraw, kraw):
        n, T_, D_ = qraw.shape
        hs = D_ // heads
        am = ((1.0 - t64(mask)) * -10000.0).unsqueeze(2)
        q = qraw + Pt["a.query.bias"]
        k = kraw + Pt["a.key.bias"]
        a = torch.softmax((q @ Pt["a.query_att.weight"].T + Pt["a.query_att.bias"]) / math.sqrt(hs) + am, dim=1)
        pq = (a.unsqueeze(3) * q.view(n, T_, heads, hs)).sum(1).reshape(n, 1, D_)
        kp = k * pq
        b = torch.softmax((kp @ Pt["a.key_att.weight"].T + Pt["a.key_att.bias"]) / math.sqrt(hs) + am, dim=1)
        pk = (b.unsqueeze(3) * kp.view(n, T_, heads, hs)).sum(1).reshape(n, 1, D_)
        return pk * q, q + Pt["a.transform.bias"], a, b

    ao, sv0, a64, b64 = core2(qin, kin)
    ((ao + sv0) * t64(dout)).sum().backward()
    d = {k: dev(v) for k, v in Pm.items()}
    md, dd = dev(mask), dev(dout)
    R = n_seq * T
    outs = []
    for _ in range(2):
        Q, K = dev(q64.numpy().reshape(R, D)), dev(k64.numpy().reshape(R, D))
        AO, SV = torch.empty(R, D, device="cuda"), torch.empty(R, D, device="cuda")
        qw, kw = torch.empty(n_seq, heads, T, device="cuda"), torch.empty(n_seq, heads, T, device="cuda")
        pq, pk = torch.empty(n_seq, D, device="cuda"), torch.empty(n_seq, D, device="cuda")
        hip.call("ebn_ff_attn_fwd_f32", P(Q), P(K), P(d["a.query.bias"]), P(d["a.key.bias"]), P(d["a.transform.bias"]), P(d["a.query_att.weight"]),
                 P(d["a.query_att.bias"]), P(d["a.key_att.weight"]), P(d["a.key_att.bias"]), P(md), P(AO), P(SV), P(qw), P(kw), P(pq), P(pk),
                 n_seq, T, D, heads, S())
        dQ, dK = torch.empty(R, D, device="cuda"), torch.empty(R, D, device="cuda")
        part = torch.empty(int(hip.lib().ebn_ff_attn_partials_len(n_seq, D, heads)), device="cuda")
        n = ctypes.c_int32(0)
        hip.call("ebn_ff_attn_bwd_f32", P(Q), P(K), P(d["a.query_att.weight"]), P(d["a.key_att.weight"]), P(qw), P(kw), P(pq), P(pk), P(dd), P(dd),
                 P(dQ), P(dK), P(part), ctypes.byref(n), n_seq, T, D, heads, S())
        W = 2 * heads * D + 3 * D
        sums = torch.empty(W, device="cuda")
        hip.call("ebn_ff_colsum_finish_f32", P(part), n.value, W, W, P(sums), S())
        torch.cuda.synchronize()
        outs.append([host(t) for t in (AO, SV, qw, kw, dQ, dK, sums)])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    AO, SV, qw, kw, dQ, dK, sums = outs[0]
    HD = heads * D
    figs = dict(AO=rel(AO, ao.detach()), SV0=rel(SV, sv0.detach()), qw=rel(qw, a64.detach().permute(0, 2, 1)), kw=rel(kw, b64.detach().permute(0, 2, 1)),
                dQ=rel(dQ, qin.grad), dK=rel(dK, kin.grad), dWqa=rel(sums[:HD], Pt["a.query_att.weight"].grad),
                dWka=rel(sums[HD:2 * HD], Pt["a.key_att.weight"].grad), dbq=rel(sums[2 * HD:2 * HD + D], Pt["a.query.bias"].grad),
                dbk=rel(sums[2 * HD + D:2 * HD + 2 * D], Pt["a.key.bias"].grad), dbtr=rel(sums[2 * HD + 2 * D:], Pt["a.transform.bias"].grad))
    print("attention", (T, D, heads, n_seq), {k: f"{v:.2e}" for k, v in figs.items()})
    assert max(figs[k] for k in ("AO", "SV0", "qw", "kw")) < 1e-5, figs
    assert max(figs[k] for k in ("dQ", "dK", "dWqa", "dWka", "dbq", "dbk", "dbtr")) < 5e-5, figs
    # a softmax does not see a shift: the logit biases' float64 gradients are zero to rounding
    assert float(Pt["a.query_att.bias"].grad.abs().max()) <= 1e-10 * float(Pt["a.query_att.weight"].grad.abs().max())


def test_attention_shape_gates(hip):
    lib = hip.lib()
    t = torch.zeros(16 * 1024, device="cuda")
    n = ctypes.c_int32(0)

    def fwd(T, D, heads):
        return lib.ebn_ff_attn_fwd_f32(P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), 0, T, D, heads, S())

    def bwd(T, D, heads):
        return lib.ebn_ff_attn_bwd_f32(P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), ctypes.byref(n), 0, T, D, heads, S())

    for f in (fwd, bwd):
        assert f(30, 256, 16) == 0 and f(1, 4, 1) == 0 and f(13, 48, 3) == 0
        assert f(30, 254, 2) == -2  # D % 4
        assert f(30, 1028, 4) == -2 and f(30, 1024, 4) == -2  # D > 1024; heads * D > 4096 ... and LDS
        assert f(30, 512, 8) == -2  # heads * D fits, 30 x 516 floats of Q rows plus the rest do not fit 64 KiB of LDS
        assert f(30, 48, 5) == -1  # D % heads
        assert f(0, 48, 3) == -1
    assert fwd(53, 256, 16) == 0 and fwd(54, 256, 16) == -2  # the 64 KiB LDS edge: 277 T + 1536 floats forward,
    assert bwd(47, 256, 16) == 0 and bwd(48, 256, 16) == -2  # 324 T + 1024 floats backward
    assert lib.ebn_ff_ln_partials_len(10, 1025) == 0 and lib.ebn_ff_ln_partials_len(10, 1024) == 3 * 1024
    assert lib.ebn_ff_ln_fwd_f32(P(t), P(t), P(t), P(t), P(t), f32(1e-12), 0, 0, f32(0), P(t), None, None, 0, 1025, S()) == -2
    assert lib.ebn_ff_pool_fwd_f32(P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), 0, 4097, 8, S()) == -2
    torch.cuda.synchronize()


def test_gelu_pool_head_pairs_vs_float64(hip):
    rng = np.random.default_rng(8)
    # gelu
    R, C = 70, 40
    X, b, dY = rng.normal(size=(R, C)).astype(np.float32) * 2, rng.normal(size=C).astype(np.float32), rng.normal(size=(R, C)).astype(np.float32)
    xd, bd, dd = dev(X), dev(b), dev(dY)
    res = []
    for _ in range(2):
        Y, dX, db = torch.empty(R, C, device="cuda"), torch.empty(R, C, device="cuda"), torch.empty(C, device="cuda")
        part = torch.empty(int(hip.lib().ebn_colsum_partials_len(R, C)), device="cuda")
        hip.call("ebn_ff_gelu_fwd_f32", P(xd), P(bd), P(Y), R, C, S())
        hip.call("ebn_ff_gelu_bwd_f32", P(xd), P(bd), P(dd), P(dX), P(db), P(part), R, C, S())
        torch.cuda.synchronize()
        res.append([host(t) for t in (Y, dX, db)])
    for a, c in zip(*res):
        np.testing.assert_array_equal(a, c)
    xt, bt = t64(X, True), t64(b, True)
    v = xt + bt
    y = 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))
    (y * t64(dY)).sum().backward()
    assert rel(res[0][0], y.detach()) < 2e-6 and rel(res[0][1], xt.grad) < 1e-5 and rel(res[0][2], bt.grad) < 1e-5
    # pooling: L = 13 rows of D = 48; one sequence fully masked
    n_seq, L, D = 9, 13, 48
    Xp = rng.normal(size=(n_seq, L, D)).astype(np.float32)
    W1 = (rng.normal(size=(D, D)) / math.sqrt(D)).astype(np.float32)
    b1, w2, b2 = rng.normal(size=D).astype(np.float32) * 0.2, rng.normal(size=(1, D)).astype(np.float32) * 0.3, np.array([0.4], np.float32)
    mask = (rng.random((n_seq, L)) < 0.7).astype(np.float32)
    mask[2] = 0
    dout = rng.normal(size=(n_seq, D)).astype(np.float32)
    Pp = {"p.att_fc1.weight": t64(W1), "p.att_fc1.bias": t64(b1, True), "p.att_fc2.weight": t64(w2, True), "p.att_fc2.bias": t64(b2, True)}
    xt = t64(Xp, True)
    u64 = (xt.detach() @ Pp["p.att_fc1.weight"].T).requires_grad_(True)
    e = torch.tanh(u64 + Pp["p.att_fc1.bias"])
    a = torch.exp(e @ Pp["p.att_fc2.weight"].T + Pp["p.att_fc2.bias"]) * t64(mask).unsqueeze(2)
    a = a / (a.sum(1, keepdim=True) + 1e-8)
    out64 = (xt * a).sum(1)
    (out64 * t64(dout)).sum().backward()
    res = []
    Xd, md, dod = dev(Xp.reshape(-1, D)), dev(mask), dev(dout)
    b1d, w2d, b2d = dev(b1), dev(w2), dev(b2)
    for _ in range(2):
        U = dev(u64.detach().numpy().reshape(-1, D))
        out, w, sinv = torch.empty(n_seq, D, device="cuda"), torch.empty(n_seq, L, device="cuda"), torch.empty(n_seq, device="cuda")
        hip.call("ebn_ff_pool_fwd_f32", P(U), P(b1d), P(w2d), P(b2d), P(Xd), P(md), P(out), P(w), P(sinv), n_seq, L, D, S())
        dX, de, db2n = torch.empty(n_seq * L, D, device="cuda"), torch.empty(n_seq * L, device="cuda"), torch.empty(n_seq, device="cuda")
        hip.call("ebn_ff_pool_bwd_f32", P(Xd), P(w), P(sinv), P(dod), P(dX), P(de), P(db2n), n_seq, L, D, S())
        part = torch.empty(int(hip.lib().ebn_attpool_partials_len(n_seq * L, D)), device="cuda")
        dw2, db1, db2 = torch.empty(D, device="cuda"), torch.empty(D, device="cuda"), torch.empty(1, device="cuda")
        hip.call("ebn_attpool_bwd_dpre_f32", P(U), P(w2d), P(de), P(dw2), P(db1), P(part), n_seq * L, D, 0, S())
        hip.call("ebn_sum_f32", P(db2n), n_seq, f32(1), P(db2), 0, S())
        torch.cuda.synchronize()
        res.append([host(t) for t in (out, w, dX, U, dw2, db1, db2)])
    for x1, x2 in zip(*res):
        np.testing.assert_array_equal(x1, x2)
    out, w, dX, dpre, dw2, db1, db2 = res[0]
    assert (out[2] == 0).all() and (w[2] == 0).all()  # an all-masked sequence pools to exactly 0
    assert rel(out, out64.detach()) < 2e-6 and rel(w, a.detach().squeeze(2)) < 2e-6
    direct = (a.detach() * t64(dout).unsqueeze(1)).reshape(-1, D)  # dX without the path through att_fc1 (a GEMM of the caller)
    assert rel(dX, direct) < 1e-5
    assert rel(dpre, u64.grad.reshape(-1, D)) < 2e-5 and rel(dw2, Pp["p.att_fc2.weight"].grad) < 2e-5 and rel(db1, Pp["p.att_fc1.bias"].grad) < 2e-5
    g = float(Pp["p.att_fc2.weight"].grad.abs().max())
    assert abs(db2[0] - float(Pp["p.att_fc2.bias"].grad)) < 1e-6 * g  # the closed form of a sum that cancels to ~1e-8 of its terms
    # head
    N, D = 11, 48
    u, c, W, bb, ds = (rng.normal(size=s).astype(np.float32) for s in ((N, D), (N, D), (1, 2 * D), (1,), (N,)))
    W *= 0.2
    ut, ct, Wt, bt = t64(u, True), t64(c, True), t64(W, True), t64(bb, True)
    s64 = torch.sigmoid(torch.cat([ut, ct], 1) @ Wt.T + bt).squeeze(1)
    (s64 * t64(ds)).sum().backward()
    ud, cd, Wd, bd, dsd = dev(u), dev(c), dev(W), dev(bb), dev(ds)
    res = []
    for _ in range(2):
        sc = torch.empty(N, device="cuda")
        hip.call("ebn_ff_head_fwd_f32", P(ud), P(cd), P(Wd), P(bd), P(sc), N, D, S())
        du, dc, dW, db = torch.empty(N, D, device="cuda"), torch.empty(N, D, device="cuda"), torch.empty(2 * D, device="cuda"), torch.empty(1, device="cuda")
        hip.call("ebn_ff_head_bwd_f32", P(ud), P(cd), P(Wd), P(sc), P(dsd), P(du), P(dc), P(dW), P(db), N, D, S())
        torch.cuda.synchronize()
        res.append([host(t) for t in (sc, du, dc, dW, db)])
    for x1, x2 in zip(*res):
        np.testing.assert_array_equal(x1, x2)
    sc, du, dc, dW, db = res[0]
    assert rel(sc, s64.detach()) < 2e-6 and rel(du, ut.grad) < 1e-5 and rel(dc, ct.grad) < 1e-5 and rel(dW, Wt.grad) < 1e-5 and rel(db, bt.grad) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- the model
def golden_model(**kw):
    z, names, cfg = load_golden()
    if "p" in kw:
        cfg = SimpleNamespace(**{**vars(cfg), "hidden_dropout_prob": kw.pop("p")})
    model = make_model(cfg, z["word_dim"].item(), **kw)
    model.load_state_dict({n: torch.as_tensor(z["param." + n]) for n in names}, strict=True)
    model = model.cuda()
    hist, cand, y = torch.as_tensor(z["hist"]).cuda(), torch.as_tensor(z["cand"]).cuda(), torch.as_tensor(z["labels"]).cuda()
    return z, names, cfg, model, hist, cand, y


def grads_of(model, hist, cand, y):
    model.zero_grad()
    score = model(hist, cand)
    loss = torch.nn.BCELoss()(score, y)
    loss.backward()
    return score, loss, {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}


def test_model_against_the_reference_fixture(hip):
    z, names, cfg, model, hist, cand, y = golden_model()
    model.train()
    score, loss, g = grads_of(model, hist, cand, y)
    E_fwd, E_ref, G = z["E_fwd"].item(), z["E_ref"].item(), z["G"].item()
    e_fwd = float(np.abs(host(score) - z["f64.score"]).max())
    e_loss = abs(loss.item() - z["f64.loss"].item())
    per = {n: fo.measure(host(g[n]), z["f64.grad." + n], G) for n in names}
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    print(f"fixture: |score - ref64| = {e_fwd:.3g} (E_fwd {E_fwd:.3g}), |loss - ref64| = {e_loss:.3g}, worst gradient measures {worst} (E_ref {E_ref:.3g})")
    assert e_fwd <= 4 * E_fwd
    assert e_loss <= 4 * max(E_fwd, abs(z["f32.loss"].item() - z["f64.loss"].item()))
    assert max(per.values()) <= 4 * E_ref, worst
    assert float(g["news_encoder.position_embeddings.weight"][1:].abs().max()) == 0.0
    # exact zeros: the padded-slot-0 user and the all-padding candidate
    with torch.no_grad():
        user = model.user_encoder(hist)
    assert float(user[1].abs().max()) == 0.0 and float(user[0].abs().max()) > 0
    assert np.abs(host(user) - z["f64.user"]).max() <= 4 * np.abs(z["f32.user"].astype(np.float64) - z["f64.user"]).max()
    N, H = hist.shape[:2]
    with torch.no_grad():  # the news vectors themselves: history slots first, then the candidates
        _, _, (_, NV) = model._engine.forward(hist, cand, 0.0, model._keys(0), False, model.token_mask)
    assert float(NV[N * H + 4].abs().max()) == 0.0 and float(NV[N * H + 3].abs().max()) > 0  # the all-padding candidate: exactly zero
    assert float(NV[1 * H:2 * H].abs().max()) == 0.0  # every slot of sample 1 under its all-zero slot-0 token mask
    assert float(NV[2 * H + 3].abs().max()) > 0  # sample 2's padded slot 3 is encoded under slot 0's mask; the history mask drops it
    W, b = host(model.output_layer.weight)[0], host(model.output_layer.bias)[0]
    D = cfg.hidden_size
    want4 = 1 / (1 + math.exp(-(float(host(user)[4] @ W[:D]) + b)))  # candidate 4 is all padding: only the user half and the bias
    assert abs(float(score[4].item()) - want4) < 1e-6


def test_three_sgd_steps_against_the_reference_trajectory(hip):
    z, names, cfg, model, hist, cand, y = golden_model()
    traj = np.load(GOLDEN / "fastformer_ref_traj.npz")
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    for _ in range(3):
        opt.zero_grad()
        torch.nn.BCELoss()(model(hist, cand), y).backward()
        opt.step()
    G, E = z["G"].item(), z["E_traj"].item()
    sd = model.state_dict()
    per = {n: fo.measure(host(sd[n]), traj["f64.traj." + n], G) for n in names}
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    print(f"trajectory: worst measures {worst} (E_traj {E:.3g})")
    assert max(per.values()) <= 4 * E, worst


def test_accumulation_frozen_table_and_determinism(hip):
    z, names, cfg, model, hist, cand, y = golden_model()
    model.train()
    _, _, g1 = grads_of(model, hist, cand, y)
    _, _, g1b = grads_of(model, hist, cand, y)
    for n in names:
        assert torch.equal(g1[n], g1b[n]), n  # the same bits twice
    y2 = 1 - y
    _, _, g2 = grads_of(model, hist, cand, y2)
    model.zero_grad()
    torch.nn.BCELoss()(model(hist, cand), y).backward()
    torch.nn.BCELoss()(model(hist, cand), y2).backward()
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, g1[n] + g2[n]), n
    model.word_embedding.weight.requires_grad_(False)
    _, _, gf = grads_of(model, hist, cand, y)
    assert gf["word_embedding.weight"] is None
    for n in names:
        if n != "word_embedding.weight":
            assert torch.equal(gf[n], g1[n]), n
    model.eval()
    with torch.no_grad():
        a, b = model(hist, cand), model(hist, cand)
    assert torch.equal(a, b) and not a.requires_grad


def test_per_slot_mask_and_dropout_against_the_oracle(hip):
    p, seed = 0.2, 5
    z, names, cfg, model, hist, cand, y = golden_model(p=p, token_mask="per_slot", seed=seed)
    model.train()
    model.dropout_step = 6
    score, loss, g = grads_of(model, hist, cand, y)  # draws at step 7
    assert model.dropout_step == 7
    Pt = {n: torch.tensor(z["param." + n], dtype=torch.float64, requires_grad=True) for n in names}
    s64 = fo.forward(Pt, hist.cpu(), cand.cpu(), cfg.num_attention_heads, cfg.layer_norm_eps, "per_slot", drop=(p, seed, 7))
    l64 = torch.nn.BCELoss()(s64, y.cpu().double())
    l64.backward()
    G = max(float(Pt[n].grad.abs().max()) for n in names if Pt[n].grad is not None)
    per = {n: fo.measure(host(g[n]), Pt[n].grad.numpy() if Pt[n].grad is not None else np.zeros(Pt[n].shape), G) for n in names}
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    e_fwd = float(np.abs(host(score) - s64.detach().numpy()).max())
    print(f"per_slot + dropout: |score - oracle64| = {e_fwd:.3g}, worst gradient measures {worst}")
    # no reference run exists for this configuration.  Scores: 16 float32 ulps of 1.0 (a sigmoid output behind a few hundred rounded
    # operations); gradients: the fixture's 4 x E_ref, the same float32 arithmetic with masks multiplied in
    assert e_fwd <= 16 * 2.0 ** -24 and max(per.values()) <= 4 * z["E_ref"].item(), worst
    # kept fraction of EACH of the 1 + 2 * layers sites, at the model's own keys of step 7 and its own element count R * D
    N, H, T = hist.shape
    R, D = N * (H + 1) * T, cfg.hidden_size
    keys = model._keys(7)
    bound = 3 * math.sqrt(p * (1 - p) / (R * D))
    with torch.no_grad():
        _, saved, _ = model._engine.forward(hist, cand, p, keys, True, "per_slot")
    kept = {0: float((saved["layers"][0][0] != 0).float().mean())}  # site 0 drops the embedding LayerNorm's output
    rng = np.random.default_rng(1)
    dY, xh = dev(rng.normal(size=(R, D))), dev(rng.normal(size=(R, D)))
    ones_r, ones_d = torch.ones(R, device="cuda"), torch.ones(D, device="cuda")
    for site in range(1, len(keys)):  # mode 1 sites drop the LayerNorm's input: dX == dres * mult
        dX, dres = torch.empty(R, D, device="cuda"), torch.empty(R, D, device="cuda")
        part = torch.empty(int(hip.lib().ebn_ff_ln_partials_len(R, D)), device="cuda")
        n = ctypes.c_int32(0)
        hip.call("ebn_ff_ln_bwd_f32", P(dY), P(xh), P(ones_r), P(ones_d), 1, keys[site], f32(p), P(dX), P(dres), P(part), ctypes.byref(n), R, D, S())
        torch.cuda.synchronize()
        kept[site] = float((dX != 0)[dres != 0].float().mean())
    print(f"kept fractions per site {kept} (1 - p = {1 - p}, 3 sigma = {bound:.4f})")
    assert len(kept) == 1 + 2 * cfg.num_hidden_layers and all(abs(v - (1 - p)) < bound for v in kept.values()), kept
    assert len(set(kept.values())) > 1  # the sites draw different masks
    model.dropout_step = 6
    score2, _, g2 = grads_of(model, hist, cand, y)
    assert torch.equal(score, score2) and all(torch.equal(g[n], g2[n]) for n in names)  # the same step counter, the same bits
    score3, _, _ = grads_of(model, hist, cand, y)
    assert not torch.equal(score, score3)  # the next step draws other masks


def test_unsupported_shape_names_the_limit(hip):
    cfg = SimpleNamespace(hidden_size=512, num_attention_heads=16, num_hidden_layers=1, intermediate_size=64, max_position_embeddings=4,
                          hidden_dropout_prob=0.0, layer_norm_eps=1e-12, initializer_range=0.02, hidden_act="gelu", pooler_type="weightpooler",
                          vocab_size=30)
    model = make_model(cfg, 16).cuda()
    with pytest.raises(ValueError, match="heads \\* hidden_size <= 4096"):
        model(torch.ones(2, 3, 8, dtype=torch.int32, device="cuda"), torch.ones(2, 1, 8, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()


def test_backward_limit_is_reported_by_the_forward_and_stale_backwards_raise(hip):
    # T = 50 at hidden 256 / 16 heads fits the forward's LDS bound (T <= 53) but not the backward's (T <= 47)
    cfg = SimpleNamespace(hidden_size=256, num_attention_heads=16, num_hidden_layers=1, intermediate_size=64, max_position_embeddings=4,
                          hidden_dropout_prob=0.0, layer_norm_eps=1e-12, initializer_range=0.02, hidden_act="gelu", pooler_type="weightpooler",
                          vocab_size=30)
    model = make_model(cfg, 16).cuda()
    hist, cand = torch.ones(2, 3, 50, dtype=torch.int32, device="cuda"), torch.ones(2, 1, 50, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        assert model(hist, cand).shape == (2, 1)
    with pytest.raises(ValueError, match="backward"):
        model(hist, cand)
    hist, cand = hist[:, :, :12].contiguous(), cand[:, :, :12].contiguous()
    loss = model(hist, cand).sum()
    with torch.no_grad():
        model.output_layer.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()
    loss = model(hist, cand).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        loss.backward()
    torch.cuda.synchronize()


def test_train_and_evaluate_end_to_end(hip, frames, tmp_path):  # noqa: F811
    from torch.utils.data import DataLoader

    from ebrec.models.fastformer import FastformerDataset, evaluate, train

    beh, train_df, mapping = frames
    cfg = SimpleNamespace(hidden_size=48, num_attention_heads=3, num_hidden_layers=1, intermediate_size=64, max_position_embeddings=4,
                          hidden_dropout_prob=0.1, layer_norm_eps=1e-12, initializer_range=0.05, hidden_act="gelu", pooler_type="weightpooler",
                          vocab_size=20)
    torch.manual_seed(0)
    model = make_model(cfg, 16).cuda()
    mk = lambda df, sh: DataLoader(FastformerDataset(behaviors=df, history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, article_dict=mapping,
                                                     batch_size=64, shuffle=sh, seed=1, device="cuda"))
    from ebrec.utils._constants import DEFAULT_LABELS_COL

    one = train_df[[sum(l) == 1 for l in train_df[DEFAULT_LABELS_COL]]]  # one click per impression and equal in-view lengths: the
    val = one.iloc[160:224]                                              # reference's AUC helper cuts the flat list into equal sublists
    assert len(val) == 64
    path = tmp_path / "ckpt" / "ff.pt"
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model = train(model, mk(one.iloc[:160], True), torch.nn.BCELoss(), torch.optim.Adam(model.parameters(), lr=1e-3), num_epochs=2,
                  val_dataloader=mk(val, False), state_dict_path=str(path), patience=2, gradient_accumulation_steps=2, tqdm_disable=True,
                  monitor_metric="auc")
    assert path.exists()
    best = torch.load(path)
    assert all(torch.equal(best[k].cuda(), v) for k, v in model.state_dict().items())  # the best state is what the model holds
    assert any(not torch.equal(before[k], v) for k, v in model.state_dict().items())
    outs, labels, loss = evaluate(model, mk(val, False), torch.nn.BCELoss(), tqdm_disable=True)
    n = sum(len(l) for l in val[DEFAULT_INVIEW_ARTICLES_COL])
    assert outs.shape == (n, 1) and labels.shape == (n, 1) and math.isfinite(loss)
    assert float(outs.min()) > 0 and float(outs.max()) < 1
