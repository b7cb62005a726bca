"""Fastformer_wu on the MI355X: the positional embedding LayerNorm and the class-head pair against float64 at shapes that are no tile
multiples (twice, bit-equal) and on guard-banded operands, the model against what the REFERENCE computed
(tests/golden/fastformer_wu_ref_*.npz) within 4 x the reference's own float32 error -- the HIP path is another float32 evaluation of
the same formulas with other summation orders -- training behaviour, the stand-alone StandardFastformerEncoder, the attention
default, the error paths and a toy task end to end.  Each test prints its figures before it asserts (`pytest -s`).

Measured on an MI355X with this fixture (E_fwd 8.1e-7 relative to the largest logit, E_ref 1.3e-4, E_traj 1.8e-6 from the reference's
float32 run): logits within 5.5e-7, loss within 1.1e-7 (reference float32: 3.5e-7), worst gradient measure 4.3e-6
(fastformer_model.encoders.0.attention.self.query.weight), worst trajectory measure 4.6e-6 (embedding_transform.bias; the bound is
7.3e-6); a loss on the logits alone 3.2e-6; dropout 0.2 against the float64 oracle: logits 8.0e-7, gradients 9.6e-6; the stand-alone
encoder: output 4.6e-7, gradients 2.7e-6 (input_embs); attention="auto" at T = 64, hidden 256 / 16 heads (the streamed pair): logits
2.0e-7, gradients 1.0e-5.  Kernels against float64, the largest over all cases: positional LayerNorm Y 1.5e-7, dX 1.4e-7, dgamma
1.3e-7, dbeta 1.0e-7, dbias 1.8e-7, dpos 1.6e-7; class head logits 1.1e-7, loss 8.2e-8, dX 3.5e-7, dW 1.6e-7, db 2.9e-7 (logits of
+-100: loss 2.8e-8).  The toy task goes from a loss of 1.403 to 0.003 in 30 Adam steps."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import nrms_numpy as on
from tests import fastformer_oracle as fo
from tests import fastformer_wu_oracle as fw
from tests.guarded import assert_values
from tests.hip_testutil import P, S, dev, host
from tests.test_fastformer_wu_cpu import GOLDEN, load_golden, make_model
from tests.test_guarded_model_kernels_gpu import G as Guarded

pytestmark = pytest.mark.gpu
f32 = ctypes.c_float


def rel(got, want):
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64) if isinstance(got, np.ndarray) else host(got)
    assert np.isfinite(got).all()
    return float(np.abs(got.reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-30))


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


# ---------------------------------------------------------------------------------------------------------------- kernels
# T and n_seq * T no multiples of the 4 rows per workgroup, D no multiple of 64, the D limit; bias = NULL once
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("n_seq,T,D,with_bias", [(5, 7, 48, True), (3, 1, 48, True), (1, 13, 68, False), (9, 6, 1024, True)])
def test_positional_layernorm_vs_float64(hip, n_seq, T, D, with_bias, p):
    rng = np.random.default_rng(n_seq * 100 + T)
    R, eps, seed, step, site = n_seq * T, 1e-12, 9, 4, 0
    X, dY = rng.normal(size=(R, D)).astype(np.float32), rng.normal(size=(R, D)).astype(np.float32)
    pos = np.full((T + 3, D), np.nan, np.float32)  # rows >= T must never be read
    pos[:T] = rng.normal(size=(T, D))
    bias, gam, bet = (rng.normal(size=D).astype(np.float32) for _ in range(3))
    key = on.dropout_key(seed, step, site)
    d = {k: dev(v) for k, v in dict(X=X, pos=pos, bias=bias, gam=gam, bet=bet, dY=dY).items()}
    bias_d = d["bias"] if with_bias else None
    outs = []
    for _ in range(2):
        Y, xh, rs = torch.empty(R, D, device="cuda"), torch.empty(R, D, device="cuda"), torch.empty(R, device="cuda")
        hip.call("ebn_ff_ln_pos_fwd_f32", P(d["X"]), P(bias_d), P(d["pos"]), P(d["gam"]), P(d["bet"]), f32(eps), key, f32(p), P(Y), P(xh), P(rs),
                 n_seq, T, D, S())
        dX = torch.empty(R, D, device="cuda")
        part = torch.empty(int(hip.lib().ebn_ff_ln_partials_len(R, D)), device="cuda")
        n = ctypes.c_int32(0)
        hip.call("ebn_ff_ln_bwd_f32", P(d["dY"]), P(xh), P(rs), P(d["gam"]), 0, key, f32(p), P(dX), None, P(part), ctypes.byref(n), R, D, S())
        sums, dpos = torch.empty(3 * D, device="cuda"), torch.empty(T, D, device="cuda")
        hip.call("ebn_ff_colsum_finish_f32", P(part), n.value, 3 * D, 3 * D, P(sums), S())
        hip.call("ebn_ff_colsum_finish_f32", P(dX), n_seq, T * D, T * D, P(dpos), S())
        torch.cuda.synchronize()
        outs.append([host(t) for t in (Y, dX, sums, dpos)])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    m = fo.drop_mult((R, D), seed, step, site, p, torch.float64, "cpu") if p > 0 else 1.0
    x, ps, b, g, be = t64(X, True), t64(pos[:T], True), t64(bias if with_bias else 0 * bias, True), t64(gam, True), t64(bet, True)
    y = fo.layer_norm((x + b).view(n_seq, T, D) + ps, g, be, eps).view(R, D) * m
    (y * t64(dY)).sum().backward()
    Y, dX, sums, dpos = outs[0]
    figs = dict(Y=rel(Y, y.detach()), dX=rel(dX, x.grad), dgamma=rel(sums[:D], g.grad), dbeta=rel(sums[D:2 * D], be.grad),
                dbias=rel(sums[2 * D:], b.grad), dpos=rel(dpos, ps.grad))
    print("positional LayerNorm", (n_seq, T, D, with_bias, p), {k: f"{v:.2e}" for k, v in figs.items()})
    assert figs["Y"] < 2e-6
    assert max(figs[k] for k in ("dX", "dgamma", "dbeta", "dbias", "dpos")) < 1e-5, figs
    if p > 0:
        kept = float((Y != 0).mean())  # the site drops the output itself
        print("kept fraction", kept)
        assert abs(kept - (1 - p)) < 3 * math.sqrt(p * (1 - p) / (R * D)), kept


def test_positional_layernorm_gates(hip):
    lib = hip.lib()
    t = torch.zeros(16 * 1024, device="cuda")
    call = lambda n_seq, T, D: lib.ebn_ff_ln_pos_fwd_f32(P(t), None, P(t), P(t), P(t), f32(1e-12), 0, f32(0), P(t), None, None, n_seq, T, D, S())
    assert call(0, 3, 48) == 0 and call(2, 3, 1024) == 0
    assert call(2, 3, 1028) == -2
    assert call(2, 0, 48) == -1 and call(-1, 3, 48) == -1
    torch.cuda.synchronize()


def cls_run(hip, X, W, b, targets, dloss, dscore):
    """one forward + backward of the class-head pair -> dict of host arrays (and the flag)"""
    N, D = X.shape
    C = W.shape[0]
    Xd, Wd, bd, td = dev(X), dev(W), dev(b), dev(targets, torch.int64)
    logits, prob = torch.empty(N, C, device="cuda"), torch.empty(N, C, device="cuda")
    rowloss, loss, flag = torch.empty(N, device="cuda"), torch.empty(1, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.call("ebn_ff_cls_fwd_f32", P(Xd), P(Wd), P(bd), P(td), P(logits), P(prob), P(rowloss), P(loss), P(flag), N, D, C, S())
    dX = torch.empty(N, D, device="cuda")
    part = torch.empty(int(hip.lib().ebn_ff_cls_partials_len(N, D, C)), device="cuda")
    n = ctypes.c_int32(0)
    dl = None if dloss is None else dev(np.array([dloss], np.float32))
    ds = None if dscore is None else dev(dscore)
    hip.call("ebn_ff_cls_bwd_f32", P(Xd), P(Wd), P(prob), P(td), P(dl), P(ds), P(dX), P(part), ctypes.byref(n), N, D, C, S())
    width = C * D + C
    assert n.value == min(-(-N // 32), 128) and n.value * width == part.numel()
    sums = torch.empty(width, device="cuda")
    hip.call("ebn_ff_colsum_finish_f32", P(part), n.value, width, width, P(sums), S())
    torch.cuda.synchronize()
    return dict(logits=host(logits), loss=host(loss), dX=host(dX), dW=host(sums[:C * D]).reshape(C, D), db=host(sums[C * D:]), flag=int(flag.item()))


def cls_ref(X, W, b, targets, dloss, dscore, valid=None):
    """float64: the loss is the sum over the `valid` rows (default all) of their cross-entropy terms, over N"""
    N, C = X.shape[0], W.shape[0]
    x, w, bb = t64(X, True), t64(W, True), t64(b, True)
    score = x @ w.T + bb
    valid = np.ones(N, bool) if valid is None else valid
    tt = torch.as_tensor(np.where(valid, targets, 0))
    m = score.max(1, keepdim=True).values
    rows = (score - m).exp().sum(1).log() + m.squeeze(1) - score.gather(1, tt.view(-1, 1)).squeeze(1)
    loss = (rows * torch.as_tensor(valid.astype(np.float64))).sum() / N
    total = (0.0 if dloss is None else dloss) * loss + (0.0 if dscore is None else (score * t64(dscore)).sum())
    total.backward()
    return dict(logits=score.detach().numpy(), loss=np.array([loss.item()]), dX=x.grad.numpy(), dW=w.grad.numpy(), db=bb.grad.numpy())


def cls_data(N, D, C, logit_scale=None):
    rng = np.random.default_rng(N * 13 + D + C)
    X, W = rng.normal(size=(N, D)).astype(np.float32), (rng.normal(size=(C, D)) / math.sqrt(D)).astype(np.float32)
    b = rng.normal(size=C).astype(np.float32) * 0.3
    if logit_scale is not None:  # logits reach +-logit_scale: exp overflows float32 without the max-subtraction
        X *= np.float32(logit_scale / np.abs(X.astype(np.float64) @ W.astype(np.float64).T).max())
    targets = rng.integers(0, C, N)
    targets[:min(N, C)] = np.arange(C)[:min(N, C)]
    dscore = rng.normal(size=(N, C)).astype(np.float32)
    return X, W, b, targets, dscore


# one row, N no multiple of the 4 rows per forward workgroup, more than two 32-row tiles (three backward workgroups), D no
# multiple of 64, the D limit, C no power of two; the last case's logits reach +-100
@pytest.mark.parametrize("N,D,C,logit_scale", [(11, 48, 4, None), (1, 48, 4, None), (70, 68, 7, None), (5, 1024, 4, None), (11, 48, 4, 100.0)])
def test_class_head_pair_vs_float64(hip, N, D, C, logit_scale):
    X, W, b, targets, dscore = cls_data(N, D, C, logit_scale)
    for what, dl, ds in (("dloss", 0.7, None), ("dscore", None, dscore), ("both", 0.7, dscore)):
        a, a2 = cls_run(hip, X, W, b, targets, dl, ds), cls_run(hip, X, W, b, targets, dl, ds)
        for k in a:
            np.testing.assert_array_equal(a[k], a2[k])
        want = cls_ref(X, W, b, targets, dl, ds)
        figs = {k: rel(a[k], want[k]) for k in want}
        print("class head", (N, D, C, logit_scale, what), {k: f"{v:.2e}" for k, v in figs.items()}, "max |logit|", float(np.abs(want["logits"]).max()))
        assert a["flag"] == 0
        if logit_scale is not None:
            assert np.abs(want["logits"]).max() > 0.99 * logit_scale and np.isfinite(a["loss"]).all()
        assert figs["logits"] < 2e-6 and figs["loss"] < 2e-6, figs
        assert max(figs[k] for k in ("dX", "dW", "db")) < 1e-5, figs


@pytest.mark.parametrize("bad", [-1, 4, -100])
def test_class_head_flags_a_target_outside_the_classes(hip, bad):
    N, D, C = 11, 48, 4
    X, W, b, targets, dscore = cls_data(N, D, C)
    targets = targets.copy()
    targets[6] = bad
    valid = np.arange(N) != 6
    a = cls_run(hip, X, W, b, targets, 0.7, dscore)
    want = cls_ref(X, W, b, targets, 0.7, dscore, valid)  # the row removed from the loss's sum, N still dividing it
    figs = {k: rel(a[k], want[k]) for k in want}
    print("class head, target", bad, {k: f"{v:.2e}" for k, v in figs.items()})
    assert a["flag"] == 1
    assert figs["logits"] < 2e-6 and figs["loss"] < 2e-6 and max(figs[k] for k in ("dX", "dW", "db")) < 1e-5, figs


def test_class_head_gates(hip):
    lib = hip.lib()
    t = torch.zeros(80 * 1024, device="cuda")
    n = ctypes.c_int32(0)
    fwd = lambda N, D, C: lib.ebn_ff_cls_fwd_f32(P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), N, D, C, S())
    bwd = lambda N, D, C: lib.ebn_ff_cls_bwd_f32(P(t), P(t), P(t), P(t), None, None, P(t), P(t), ctypes.byref(n), N, D, C, S())
    for f in (fwd, bwd):
        assert f(0, 48, 4) == 0 and f(2, 1024, 64) == 0 and f(2, 48, 1) == 0
        assert f(2, 1028, 4) == -2 and f(2, 48, 65) == -2
        assert f(2, 48, 0) == -1 and f(-1, 48, 4) == -1
    assert lib.ebn_ff_cls_partials_len(70, 68, 7) == 3 * (7 * 68 + 7) and lib.ebn_ff_cls_partials_len(0, 48, 4) == 4 * 48 + 4
    assert lib.ebn_ff_cls_partials_len(10 ** 6, 48, 4) == 128 * (4 * 48 + 4) and lib.ebn_ff_cls_partials_len(2, 48, 65) == 0
    torch.cuda.synchronize()


def test_new_entries_on_guard_banded_offset_operands(hip):
    """Both new entries with every operand between guards (tests/guarded.py) and deliberately misaligned by 1..3 floats: nothing
    outside the stated extents is written, every output element is, NaN guards never reach a result."""
    rng = np.random.default_rng(77)
    # positional LayerNorm: the position table is handed over with exactly T rows, NaN behind them
    n_seq, T, D, p = 5, 7, 65, 0.2
    R = n_seq * T
    X, pos = rng.normal(size=(R, D)).astype(np.float32), rng.normal(size=(T, D)).astype(np.float32)
    bias, gam, bet = (rng.normal(size=D).astype(np.float32) for _ in range(3))
    key = on.dropout_key(3, 1, 0)
    g = Guarded()
    Y, xh, rs = g.o((R, D), "Y", offset=1), g.o((R, D), "xhat", offset=3), g.o((R,), "rstd", offset=2)
    hip.call("ebn_ff_ln_pos_fwd_f32", P(g.i(X, "X", offset=1)), P(g.i(bias, "bias", offset=2)), P(g.i(pos, "pos", offset=3)), P(g.i(gam, "gamma", offset=1)),
             P(g.i(bet, "beta", offset=1)), f32(1e-12), key, f32(p), P(Y), P(xh), P(rs), n_seq, T, D, S())
    g.check()
    m = fo.drop_mult((R, D), 3, 1, 0, p, torch.float64, "cpu")
    z = (t64(X) + t64(bias)).view(n_seq, T, D) + t64(pos)
    want_xh = fo.layer_norm(z, torch.ones(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64), 1e-12).view(R, D)
    assert_values(host(Y), (want_xh * t64(gam) + t64(bet)) * m, 2e-6, 2e-6, "guarded ln_pos Y")
    assert_values(host(xh), want_xh, 2e-6, 2e-6, "guarded ln_pos xhat")
    g = Guarded()
    XY = g.io(X, "X = Y", offset=2)  # Y aliases X, no bias, inference
    hip.call("ebn_ff_ln_pos_fwd_f32", P(XY), None, P(g.i(pos, "pos", offset=1)), P(g.i(gam, "gamma")), P(g.i(bet, "beta")), f32(1e-12), key, f32(0.0),
             P(XY), None, None, n_seq, T, D, S())
    g.check()
    want = fo.layer_norm(t64(X).view(n_seq, T, D) + t64(pos), t64(gam), t64(bet), 1e-12).view(R, D)
    assert_values(host(XY), want, 2e-6, 2e-6, "guarded ln_pos, Y aliases X")
    # class head: 70 rows = three backward workgroups of <= 32 rows; int64 targets as guarded int32 pairs whose guards are out of range
    N, D, C = 70, 65, 7
    X, W, b, targets, dscore = cls_data(N, D, C)
    g = Guarded()
    tg = g.i(np.asarray(targets, np.int64).view(np.int32), "targets", fill=0x7FFFFFFF, offset=2)
    logits, prob, rowloss = g.o((N, C), "logits", offset=1), g.o((N, C), "prob", offset=3), g.o((N,), "rowloss", offset=1)
    loss, flag = g.o((1,), "loss", offset=2), g.io(np.zeros(1, np.float32), "flag", offset=3)  # a zero word: the flag
    Xg, Wg = g.i(X, "X", offset=3), g.i(W, "W", offset=1)
    hip.call("ebn_ff_cls_fwd_f32", P(Xg), P(Wg), P(g.i(b, "b", offset=2)), P(tg), P(logits), P(prob), P(rowloss), P(loss), P(flag), N, D, C, S())
    g.check()
    assert int(flag.view(torch.int32).item()) == 0
    want = cls_ref(X, W, b, targets, 0.7, dscore)
    assert_values(host(logits), want["logits"], 2e-6, 2e-6, "guarded cls logits")
    assert_values(host(loss), want["loss"], 2e-6, 2e-6, "guarded cls loss")
    g = Guarded()
    dX = g.o((N, D), "dX", offset=1)
    part = g.scratch(hip.lib().ebn_ff_cls_partials_len(N, D, C), "partials")
    n = ctypes.c_int32(-1)
    tg = g.i(np.asarray(targets, np.int64).view(np.int32), "targets", fill=0x7FFFFFFF, offset=0)
    hip.call("ebn_ff_cls_bwd_f32", P(g.i(X, "X", offset=2)), P(g.i(W, "W", offset=3)), P(g.i(host(prob).astype(np.float32), "prob", offset=1)), P(tg),
             P(g.i(np.array([0.7], np.float32), "dloss", offset=3)), P(g.i(dscore, "dscore", offset=1)), P(dX), P(part), ctypes.byref(n), N, D, C, S())
    sums = g.o((C * D + C,), "sums", offset=1)
    hip.call("ebn_ff_colsum_finish_f32", P(part), n.value, C * D + C, C * D + C, P(sums), S())
    g.check()
    assert n.value == 3
    scale = np.abs(want["dW"]).max()
    assert_values(host(dX), want["dX"], 1e-5, 1e-5 * np.abs(want["dX"]).max(), "guarded cls dX")
    assert_values(host(sums)[:C * D].reshape(C, D), want["dW"], 1e-5, 1e-5 * scale, "guarded cls dW")
    assert_values(host(sums)[C * D:], want["db"], 1e-5, 1e-5 * np.abs(want["db"]).max(), "guarded cls db")


# ---------------------------------------------------------------------------------------------------------------- the model
def golden_model(**kw):
    z, names, cfg = load_golden()
    if "p" in kw:
        cfg = SimpleNamespace(**{**vars(cfg), "hidden_dropout_prob": kw.pop("p")})
    model = make_model(cfg, z["word_dim"].item(), **kw)
    model.load_state_dict({n: torch.as_tensor(z["param." + n]) for n in names}, strict=True)
    model = model.cuda()
    return z, names, cfg, model, torch.as_tensor(z["ids"]).cuda(), torch.as_tensor(z["targets"]).cuda()


def grads_of(model, ids, targets):
    model.zero_grad()
    loss, score = model(ids, targets)
    loss.backward()
    return score, loss, {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}


def test_model_against_the_reference_fixture(hip):
    z, names, cfg, model, ids, targets = golden_model()
    model.train()
    score, loss, g = grads_of(model, ids, targets)
    E_fwd, E_ref, G = z["E_fwd"].item(), z["E_ref"].item(), z["G"].item()
    top = float(np.abs(z["f64.score"]).max())
    e_fwd = float(np.abs(host(score) - z["f64.score"]).max()) / top
    e_loss = abs(loss.item() - z["f64.loss"].item())
    per = {n: fo.measure(host(g[n]), z["f64.grad." + n], G) for n in names}
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    print(f"fixture: measure(score) = {e_fwd:.3g} (E_fwd {E_fwd:.3g}), |loss - ref64| = {e_loss:.3g} (|loss32 - loss64| "
          f"{abs(z['f32.loss'].item() - z['f64.loss'].item()):.3g}), worst gradient measures {worst} (E_ref {E_ref:.3g})")
    assert tuple(score.shape) == (ids.shape[0], 4) and loss.dim() == 0
    assert e_fwd <= 4 * E_fwd
    assert e_loss <= 4 * max(E_fwd * top, abs(z["f32.loss"].item() - z["f64.loss"].item()))
    assert max(per.values()) <= 4 * E_ref, worst
    T = ids.shape[1]
    dpos = g["fastformer_model.position_embeddings.weight"]
    assert float(dpos[T:].abs().max()) == 0.0 and float(dpos[T - 1].abs().max()) > 0  # rows >= T: exact zeros
    # the all-padding sequence pools to an exact zero vector: its logits are the head's bias, bit for bit
    assert torch.equal(score[4], model.output_layer.bias.detach())
    model.eval()
    with torch.no_grad():
        l2, s2 = model(ids, targets)
    assert torch.equal(s2, score) and torch.equal(l2, loss) and not s2.requires_grad


def test_three_sgd_steps_against_the_reference_trajectory(hip):
    z, names, cfg, model, ids, targets = golden_model()
    traj = np.load(GOLDEN / "fastformer_wu_ref_traj.npz")
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    for _ in range(3):
        opt.zero_grad()
        model(ids, targets)[0].backward()
        opt.step()
    G, E = z["G"].item(), z["E_traj"].item()
    sd = model.state_dict()
    per = {n: fo.measure(host(sd[n]), traj["f64.traj." + n], G) for n in names}
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    print(f"trajectory: worst measures {worst} (E_traj {E:.3g})")
    assert max(per.values()) <= 4 * E, worst


def test_determinism_accumulation_and_the_frozen_table(hip, monkeypatch):
    from ebrec import _hip

    z, names, cfg, model, ids, targets = golden_model()
    model.train()
    scatters = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (scatters.append(name) if "scatter" in name else None, real(name, *a))[1])
    _, _, g1 = grads_of(model, ids, targets)
    assert scatters == ["ebn_embedding_grad_scatter_fixed"]
    _, _, g1b = grads_of(model, ids, targets)
    for n in names:
        assert torch.equal(g1[n], g1b[n]), n  # the same bits twice
    t2 = (targets + 1) % 4
    _, _, g2 = grads_of(model, ids, t2)
    model.zero_grad()
    model(ids, targets)[0].backward()
    model(ids, t2)[0].backward()
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, g1[n] + g2[n]), n
    # both outputs are differentiable: a loss on the logits alone, and on both
    model.zero_grad()
    loss, score = model(ids, targets)
    (loss + 0.5 * (score ** 2).sum()).backward()
    gboth = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    model.zero_grad()
    (0.5 * (model(ids, targets)[1] ** 2).sum()).backward()
    Pt = {n: torch.tensor(z["param." + n], dtype=torch.float64, requires_grad=True) for n in names}
    l64, s64 = fw.forward(Pt, ids.cpu(), targets.cpu(), cfg.num_attention_heads, cfg.layer_norm_eps)
    (0.5 * (s64 ** 2).sum()).backward()
    G = max(float(Pt[n].grad.abs().max()) for n in names)
    per = {n: fo.measure(host(p.grad), Pt[n].grad.numpy(), G) for n, p in model.named_parameters()}
    print("score-only loss: worst gradient measure", max(per.values()))
    assert max(per.values()) <= 4 * z["E_ref"].item()
    per = {n: fo.measure(host(gboth[n]), host(g1[n]) + Pt[n].grad.numpy(), G) for n in names}
    assert max(per.values()) <= 4 * z["E_ref"].item()
    # a frozen word table: no gradient, no scatter launch, every other gradient the same bits
    del scatters[:]
    model.word_embedding.weight.requires_grad_(False)
    _, _, gf = grads_of(model, ids, targets)
    assert gf["word_embedding.weight"] is None and scatters == []
    for n in names:
        if n != "word_embedding.weight":
            assert torch.equal(gf[n], g1[n]), n


def test_dropout_against_the_oracle(hip):
    p, seed = 0.2, 5
    z, names, cfg, model, ids, targets = golden_model(p=p, seed=seed)
    model.train()
    model.dropout_step = 6
    score, loss, g = grads_of(model, ids, targets)  # draws at step 7
    assert model.dropout_step == 7
    Pt = {n: torch.tensor(z["param." + n], dtype=torch.float64, requires_grad=True) for n in names}
    l64, s64 = fw.forward(Pt, ids.cpu(), targets.cpu(), cfg.num_attention_heads, cfg.layer_norm_eps, drop=(p, seed, 7))
    l64.backward()
    G = max(float(Pt[n].grad.abs().max()) for n in names if Pt[n].grad is not None)
    per = {n: fo.measure(host(g[n]), Pt[n].grad.numpy() if Pt[n].grad is not None else np.zeros(Pt[n].shape), G) for n in names}
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    e_fwd = float(np.abs(host(score) - s64.detach().numpy()).max() / s64.detach().abs().max())
    print(f"dropout {p}: measure(score) = {e_fwd:.3g}, |loss - oracle64| = {abs(loss.item() - l64.item()):.3g}, worst gradient measures {worst}")
    assert e_fwd <= 4 * z["E_fwd"].item() and max(per.values()) <= 4 * z["E_ref"].item(), worst
    nodrop = fw.forward(Pt, ids.cpu(), targets.cpu(), cfg.num_attention_heads, cfg.layer_norm_eps)[1]
    assert float((nodrop - s64).detach().abs().max()) > 1e-3  # the masks matter
    model.dropout_step = 6
    score2, _, g2 = grads_of(model, ids, targets)
    assert torch.equal(score, score2) and all(torch.equal(g[n], g2[n]) for n in names)  # the same step counter, the same bits
    score3, _, _ = grads_of(model, ids, targets)
    assert not torch.equal(score, score3)  # the next step draws other masks
    model.eval()
    with torch.no_grad():
        model(ids, targets)
    assert model.dropout_step == 8  # an eval forward draws nothing


def test_stand_alone_encoder_against_the_oracle(hip):
    from ebrec.models.fastformer import StandardFastformerEncoder

    z, names, cfg = load_golden()
    pre = "fastformer_model."
    rng = np.random.default_rng(4)
    torch.manual_seed(3)
    enc = StandardFastformerEncoder(cfg, pooler_count=2)
    state = {n[len(pre):]: torch.as_tensor(z["param." + n]) for n in names if n.startswith(pre)}
    for k, v in enc.state_dict().items():
        if k.startswith("poolers.1."):
            state[k] = v.clone() + (0.2 * torch.randn_like(v) if k.endswith("bias") else 0)
    enc.load_state_dict(state, strict=True)
    enc = enc.cuda().train()
    N, T = z["ids"].shape
    D = cfg.hidden_size
    x = rng.normal(size=(N, T, D)).astype(np.float32)
    mask = (z["ids"] != 0).astype(np.float32)
    dout = rng.normal(size=(N, D)).astype(np.float32)
    E_fwd, E_ref = z["E_fwd"].item(), z["E_ref"].item()
    for index in (0, 1):
        enc.zero_grad()
        xd = dev(x).requires_grad_(True)
        out = enc(xd, dev(mask), pooler_index=index)
        (out * dev(dout)).sum().backward()
        Pt = {k: v.double().requires_grad_(True) for k, v in state.items()}
        x64 = t64(x, True)
        o64 = fw.encoder(x64, t64(mask), Pt, cfg.num_attention_heads, cfg.layer_norm_eps, "", index)
        (o64 * t64(dout)).sum().backward()
        other = f"poolers.{1 - index}."
        assert all((Pt[k].grad is None) == k.startswith(other) for k in Pt)
        G = max(float(x64.grad.abs().max()), max(float(v.grad.abs().max()) for v in Pt.values() if v.grad is not None))
        per = {k: fo.measure(host(p.grad), Pt[k].grad.numpy(), G) for k, p in enc.named_parameters() if not k.startswith(other)}
        per["input_embs"] = fo.measure(host(xd.grad), x64.grad.numpy(), G)
        e_fwd = float(np.abs(host(out) - o64.detach().numpy()).max() / o64.detach().abs().max())
        worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
        print(f"stand-alone encoder, pooler {index}: measure(out) = {e_fwd:.3g}, worst gradient measures {worst}")
        assert tuple(out.shape) == (N, D) and float(out[4].abs().max()) == 0.0  # the all-padding sequence
        assert e_fwd <= 4 * E_fwd and max(per.values()) <= 4 * E_ref, worst
        assert all(p.grad is None for k, p in enc.named_parameters() if k.startswith(other))  # the other pooler was not used
        assert float(enc.position_embeddings.weight.grad[T:].abs().max()) == 0.0
    with torch.no_grad():
        assert not torch.equal(enc(dev(x), dev(mask), 0), enc(dev(x), dev(mask), 1))


def test_auto_attention_takes_the_streamed_pair_for_a_long_text(hip):
    # hidden 256 / 16 heads, T = 64: past the resident pair's T <= 47 when training
    cfg = SimpleNamespace(hidden_size=256, num_attention_heads=16, num_hidden_layers=1, intermediate_size=64, max_position_embeddings=64,
                          hidden_dropout_prob=0.0, layer_norm_eps=1e-12, initializer_range=0.05, hidden_act="gelu", pooler_type="weightpooler",
                          vocab_size=30)
    z, _, _ = load_golden()
    torch.manual_seed(1)
    model = make_model(cfg, 16)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("bias") or "LayerNorm.weight" in name:
                p.add_(torch.randn_like(p) * 0.2)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rng = np.random.default_rng(2)
    N, T = 3, 64
    ids = rng.integers(1, cfg.vocab_size, (N, T))
    ids[1, 40:] = 0
    targets = np.array([2, 0, 3])
    model = model.cuda().train()
    eng = model.fastformer_model._engine
    assert model.attention == "auto" and eng.attention_kind(T, True) == "streamed" and eng.attention_kind(12, True) == "resident"
    score, loss, g = grads_of(model, torch.as_tensor(ids).cuda(), torch.as_tensor(targets).cuda())
    Pt = {k: v.double().requires_grad_(True) for k, v in state.items()}
    l64, s64 = fw.forward(Pt, torch.as_tensor(ids), torch.as_tensor(targets), cfg.num_attention_heads, cfg.layer_norm_eps)
    l64.backward()
    G = max(float(v.grad.abs().max()) for v in Pt.values())
    per = {k: fo.measure(host(g[k]), Pt[k].grad.numpy(), G) for k in Pt}
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    e_fwd = float(np.abs(host(score) - s64.detach().numpy()).max() / s64.detach().abs().max())
    print(f"auto at T = 64, hidden 256 / 16 heads: measure(score) = {e_fwd:.3g}, |loss - oracle64| = {abs(loss.item() - l64.item()):.3g}, "
          f"worst gradient measures {worst}")
    assert e_fwd <= 4 * z["E_fwd"].item() and max(per.values()) <= 4 * z["E_ref"].item(), worst
    resident = make_model(cfg, 16, attention="resident")
    resident.load_state_dict(state, strict=True)
    resident = resident.cuda().train()
    before = hip.lib().ebn_launch_count()
    with pytest.raises(ValueError, match="backward"):  # in the forward, not inside loss.backward()
        resident(torch.as_tensor(ids).cuda(), torch.as_tensor(targets).cuda())
    assert hip.lib().ebn_launch_count() == before
    torch.cuda.synchronize()


def test_error_paths(hip):
    z, names, cfg, model, ids, targets = golden_model()
    lib = hip.lib()
    long_ids = torch.ones(2, cfg.max_position_embeddings + 1, dtype=torch.int32, device="cuda")
    before = lib.ebn_launch_count()
    with pytest.raises(IndexError, match="max_position_embeddings"):
        model(long_ids, torch.zeros(2, dtype=torch.int64, device="cuda"))
    assert lib.ebn_launch_count() == before  # known on the host: nothing was launched
    full = torch.ones(2, cfg.max_position_embeddings, dtype=torch.int32, device="cuda")  # T = max_position_embeddings itself runs
    assert model(full, torch.zeros(2, dtype=torch.int64, device="cuda"))[1].shape == (2, 4)
    for bad in (4, -100):
        t = targets.clone()
        t[2] = bad
        with pytest.raises(IndexError, match="target"):
            model(ids, t)
    bad_ids = ids.clone()
    bad_ids[0, 0] = cfg.vocab_size
    with pytest.raises(IndexError, match="token id"):
        model(bad_ids, targets)
    loss, _ = model(ids, targets)
    with torch.no_grad():
        model.output_layer.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()
    loss, _ = model(ids, targets)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        loss.backward()
    with pytest.raises(RuntimeError):  # a CPU tensor next to a model on the GPU
        model(ids.cpu(), targets)
    torch.cuda.synchronize()


def test_toy_task_end_to_end(hip):
    cfg = SimpleNamespace(hidden_size=48, num_attention_heads=3, num_hidden_layers=1, intermediate_size=64, max_position_embeddings=8,
                          hidden_dropout_prob=0.0, layer_norm_eps=1e-12, initializer_range=0.05, hidden_act="gelu", pooler_type="weightpooler",
                          vocab_size=20)
    torch.manual_seed(0)
    model = make_model(cfg, 16).cuda().train()
    rng = np.random.default_rng(0)
    ids = rng.integers(1, cfg.vocab_size, (64, 8))
    ids[::3, 5:] = 0
    targets = torch.as_tensor(ids[:, 0] % 4).cuda()  # the class is the first token id mod 4
    ids = torch.as_tensor(ids).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss, _ = model(ids, targets)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        last, score = model(ids, targets)
    acc = float((score.argmax(1) == targets).float().mean())
    print(f"toy task: loss {losses[0]:.4f} -> {last.item():.4f} after 30 Adam steps, accuracy {acc:.2f}")
    assert math.isfinite(last.item()) and last.item() < losses[0]
