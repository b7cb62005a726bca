"""The streamed Fastformer attention pair (csrc/ebn_fastformer_streamed.hip) and `Fastformer(..., attention=...)` on the MI355X.

Kernel pair: against the float64 formulation of tests/test_fastformer_gpu.py at shapes the resident pair refuses, twice with equal
bits.  The bound is not a constant: the same formulation is evaluated in float32 torch on the CPU, its relative error against
float64 is taken per quantity (E32), and the HIP result -- another float32 evaluation with other summation orders -- must stay within
4 x E32 (the margin tests/test_fastformer_gpu.py gives the model); at the shapes shared with that file also within its 1e-5 / 5e-5.
Guard bands (tests/guarded.py), gates, the model at hidden 768 / 12 heads against the float64 oracle within 4 x the float32 oracle's
own error, the reference fixtures with attention="streamed", the reference's 500-token fixture, and attention="auto".

Every test prints its figures before it asserts (`pytest -s`).  The measured figures are in DESIGN.md section 12."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import fastformer_oracle as fo
from tests.guarded import guard_in, guard_out
from tests.hip_testutil import P, S, dev, host
from tests.test_fastformer_cpu import GOLDEN, make_model
from tests.test_fastformer_streamed_cpu import load_long

pytestmark = pytest.mark.gpu
f32 = ctypes.c_float
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
SHARED_SHAPES = {(13, 48, 3, 5), (1, 48, 3, 3), (30, 256, 16, 300)}  # those of test_fastformer_gpu.test_attention_pair_vs_float64
FWD_KEYS, GRAD_KEYS = ("AO", "SV0", "qw", "kw"), ("dQ", "dK", "dWqa", "dWka", "dbq", "dbk", "dbtr")


def rel(got, want):
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64) if isinstance(got, np.ndarray) else host(got)
    return float(np.abs(got.reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-30))


# ---------------------------------------------------------------------------------------------------------------- kernel pair
def attn_data(T, D, heads, n_seq, all_padding=None):
    """float32 operands of one call; Qr / Kr are x.Wq^T / x.Wk^T rounded to float32, so every evaluation starts from the same bits"""
    rng = np.random.default_rng(T * 7 + D)
    d = dict(bq=rng.normal(size=D) * 0.3, bk=rng.normal(size=D) * 0.3, btr=rng.normal(size=D) * 0.3, Wqa=rng.normal(size=(heads, D)) * 0.5,
             bqa=rng.normal(size=heads) * 0.3, Wka=rng.normal(size=(heads, D)) * 0.5, bka=rng.normal(size=heads) * 0.3)
    x = rng.normal(size=(n_seq, T, D))
    d["Qr"] = x @ (rng.normal(size=(D, D)) / math.sqrt(D)).T
    d["Kr"] = x @ (rng.normal(size=(D, D)) / math.sqrt(D)).T
    d["dout"] = rng.normal(size=(n_seq, T, D))
    d = {k: v.astype(np.float32) for k, v in d.items()}
    mask = (rng.random((n_seq, T)) < 0.7).astype(np.float32)
    mask[:, 0] = 1  # no all-padding sequence where values are compared: its logits are -10000 + x in float32 (ulp 1e-3), which float64
    mask[-1] = 1    # does not mimic
    if all_padding is not None:
        mask[all_padding] = 0
    d["mask"] = mask
    return d


def core2(d, heads, dtype):
    """the float64 formulation of test_attention_pair_vs_float64 in `dtype`: out = AO + SV0 with transform = identity, so dAO = dSV = dout.
    -> every quantity the pair leaves, as float64 numpy"""
    t = lambda a, grad=False: torch.tensor(np.asarray(a, np.float64), dtype=dtype, requires_grad=grad)
    qin, kin = t(d["Qr"], True), t(d["Kr"], True)
    bq, bk, btr, Wqa, bqa, Wka, bka = (t(d[k], True) for k in ("bq", "bk", "btr", "Wqa", "bqa", "Wka", "bka"))
    n, T, D = qin.shape
    hs = D // heads
    am = ((1.0 - t(d["mask"])) * -10000.0).unsqueeze(2)
    q, k = qin + bq, kin + bk
    a = torch.softmax((q @ Wqa.T + bqa) / math.sqrt(hs) + am, dim=1)
    pq = (a.unsqueeze(3) * q.view(n, T, heads, hs)).sum(1).reshape(n, 1, D)
    kp = k * pq
    b = torch.softmax((kp @ Wka.T + bka) / math.sqrt(hs) + am, dim=1)
    pk = (b.unsqueeze(3) * kp.view(n, T, heads, hs)).sum(1).reshape(n, 1, D)
    ao, sv0 = pk * q, q + btr
    ((ao + sv0) * t(d["dout"])).sum().backward()
    out = dict(AO=ao, SV0=sv0, qw=a.permute(0, 2, 1), kw=b.permute(0, 2, 1), dQ=qin.grad, dK=kin.grad, dWqa=Wqa.grad, dWka=Wka.grad, dbq=bq.grad,
               dbk=bk.grad, dbtr=btr.grad, dbqa=bqa.grad)
    return {k_: v.detach().double().numpy() for k_, v in out.items()}


def run_pair(hip, d, T, D, heads, n_seq):
    """one forward + backward of the streamed pair and the two logit-weight GEMMs -> dict of host arrays"""
    lib = hip.lib()
    R = n_seq * T
    Q, K = dev(d["Qr"].reshape(R, D)), dev(d["Kr"].reshape(R, D))
    c = {k: dev(d[k]) for k in ("bq", "bk", "btr", "Wqa", "bqa", "Wka", "bka", "mask", "dout")}
    AO, SV = torch.empty(R, D, device="cuda"), torch.empty(R, D, device="cuda")
    qw, kw = torch.empty(n_seq, heads, T, device="cuda"), torch.empty(n_seq, heads, T, device="cuda")
    pq, pk = torch.empty(n_seq, D, device="cuda"), torch.empty(n_seq, D, device="cuda")
    hip.call("ebn_ff_attn_streamed_fwd_f32", P(Q), P(K), P(c["bq"]), P(c["bk"]), P(c["btr"]), P(c["Wqa"]), P(c["bqa"]), P(c["Wka"]), P(c["bka"]),
             P(c["mask"]), P(AO), P(SV), P(qw), P(kw), P(pq), P(pk), n_seq, T, D, heads, S())
    dQ, dK = torch.empty(R, D, device="cuda"), torch.empty(R, D, device="cuda")
    n_dl = int(lib.ebn_ff_attn_streamed_dlogits_len(n_seq, T, heads))
    assert n_dl == R * heads and int(lib.ebn_ff_attn_streamed_kp_len(n_seq, T, D)) == R * D
    d1, d2, kp = torch.empty(R, heads, device="cuda"), torch.empty(R, heads, device="cuda"), torch.empty(R, D, device="cuda")
    part = torch.empty(int(lib.ebn_ff_attn_streamed_partials_len(n_seq, D)), device="cuda")
    n = ctypes.c_int32(0)
    hip.call("ebn_ff_attn_streamed_bwd_f32", P(Q), P(K), P(c["Wqa"]), P(c["Wka"]), P(qw), P(kw), P(pq), P(pk), P(c["dout"]), P(c["dout"]), P(dQ),
             P(dK), P(d1), P(d2), P(kp), P(part), ctypes.byref(n), n_seq, T, D, heads, S())
    assert n.value == min(n_seq, 256) and part.numel() == n.value * 3 * D
    sums = torch.empty(3 * D, device="cuda")
    hip.call("ebn_ff_colsum_finish_f32", P(part), n.value, 3 * D, 3 * D, P(sums), S())
    inv = f32(1.0 / math.sqrt(D // heads))
    n_ws = int(lib.ebn_gemm_workspace_floats(heads, D, R))
    ws = torch.empty(max(n_ws, 1), device="cuda")
    dWqa, dWka = torch.empty(heads, D, device="cuda"), torch.empty(heads, D, device="cuda")
    for dl, x, out in ((d1, Q, dWqa), (d2, kp, dWka)):
        hip.call("ebn_gemm_f32_ws", 1, 0, heads, D, R, inv, P(dl), heads, P(x), D, f32(0), P(out), D, P(ws), n_ws, S())
    torch.cuda.synchronize()
    got = dict(AO=AO, SV0=SV, qw=qw, kw=kw, pq=pq, pk=pk, dQ=dQ, dK=dK, d1=d1, d2=d2, kp=kp, dWqa=dWqa, dWka=dWka, dbq=sums[:D], dbk=sums[D:2 * D],
               dbtr=sums[2 * D:], Q=Q, K=K)
    return {k: t.detach().cpu().numpy().copy() for k, t in got.items()}


@pytest.mark.parametrize("T,D,heads,n_seq", [
    (13, 48, 3, 5), (1, 48, 3, 3),  # the old non-multiples
    (30, 256, 16, 300),             # the resident pair's own flagship shape (the third shape shared with test_fastformer_gpu.py)
    (30, 768, 12, 7),               # the target shape
    (70, 1024, 16, 3),              # max D, heads * D = 16384, T across a 64-lane boundary
    (500, 24, 4, 2),                # long T: many passes of every t += 64 and t += waves loop, ragged tail; head size 6 (no 16-byte slices)
    (512, 768, 12, 2),              # the required T edge
    (9, 68, 68, 4),                 # head size 1, heads * D > 4096 with a tiny D, heads past the register-held weight column
    (5, 16, 2, 300),                # more sequences than the workgroup cap: each workgroup walks several
])
def test_streamed_pair_vs_float64(hip, T, D, heads, n_seq):
    d = attn_data(T, D, heads, n_seq)
    want, w32 = core2(d, heads, torch.float64), core2(d, heads, torch.float32)
    runs = [run_pair(hip, d, T, D, heads, n_seq) for _ in range(2)]
    for k in runs[0]:
        assert np.array_equal(runs[0][k].view(np.int32), runs[1][k].view(np.int32)), f"{k} differs between two runs"
    got = runs[0]
    E32 = {k: rel(w32[k], want[k]) for k in FWD_KEYS + GRAD_KEYS}
    figs = {k: rel(got[k], want[k]) for k in FWD_KEYS + GRAD_KEYS}
    print("streamed attention", (T, D, heads, n_seq), {k: f"{figs[k]:.2e} (E32 {E32[k]:.2e})" for k in figs})
    assert np.array_equal(got["Q"], (d["Qr"] + d["bq"]).reshape(got["Q"].shape)) and np.array_equal(got["K"], (d["Kr"] + d["bk"]).reshape(got["K"].shape))
    for k in figs:
        assert figs[k] <= 4 * E32[k], (k, figs[k], E32[k])
    if (T, D, heads, n_seq) in SHARED_SHAPES:
        assert max(figs[k] for k in FWD_KEYS) < 1e-5 and max(figs[k] for k in GRAD_KEYS) < 5e-5, figs
    # a softmax does not see a shift: the logit biases' float64 gradients are zero to rounding
    assert float(np.abs(want["dbqa"]).max()) <= 1e-10 * float(np.abs(want["dWqa"]).max())


# ---------------------------------------------------------------------------------------------------------------- guard bands
class Guards:
    """the guarded operands of one call (tests/guarded.py): NaN around inputs, canaries around and a pre-fill inside outputs"""

    def __init__(self):
        self.h = []

    def i(self, x, name):
        v, h = guard_in(x)
        self.h.append((name, h))
        return v

    def o(self, shape, name, values=None):
        v, h = guard_out(shape)
        if values is not None:  # an in-place operand: an output with a payload
            h.fill_payload(np.asarray(values).reshape(h.rows, h.width))
        self.h.append((name, h))
        return v

    def check(self):
        torch.cuda.synchronize()
        for name, h in self.h:
            h.check(name)


@pytest.mark.parametrize("T,D,heads,n_seq", [(13, 48, 3, 5), (30, 768, 12, 3)])
def test_streamed_pair_between_guard_bands(hip, T, D, heads, n_seq):
    lib = hip.lib()
    d = attn_data(T, D, heads, n_seq, all_padding=1)
    R = n_seq * T
    g = Guards()
    Q, K = g.o((R, D), "Q", d["Qr"]), g.o((R, D), "K", d["Kr"])
    o = dict(AO=g.o((R, D), "AO"), SV0=g.o((R, D), "SV0"), qw=g.o((n_seq * heads, T), "qw"), kw=g.o((n_seq * heads, T), "kw"), pq=g.o((n_seq, D), "pq"),
             pk=g.o((n_seq, D), "pk"))
    rc = lib.ebn_ff_attn_streamed_fwd_f32(P(Q), P(K), P(g.i(d["bq"], "bq")), P(g.i(d["bk"], "bk")), P(g.i(d["btr"], "btr")), P(g.i(d["Wqa"], "Wqa")),
                                          P(g.i(d["bqa"], "bqa")), P(g.i(d["Wka"], "Wka")), P(g.i(d["bka"], "bka")), P(g.i(d["mask"], "mask")), P(o["AO"]),
                                          P(o["SV0"]), P(o["qw"]), P(o["kw"]), P(o["pq"]), P(o["pk"]), n_seq, T, D, heads, S())
    assert rc == OK
    g.check()  # inputs untouched, no canary disturbed, every output (the in-place Q and K included) written
    assert np.array_equal(Q.cpu().numpy(), (d["Qr"] + d["bq"]).reshape(R, D)) and np.array_equal(K.cpu().numpy(), (d["Kr"] + d["bk"]).reshape(R, D))
    for k, t in o.items():
        assert bool(torch.isfinite(t).all()), k
    for k in ("qw", "kw"):
        assert float((o[k].sum(1) - 1).abs().max()) <= 1e-6, k  # the all-padding sequence's softmaxes included
    saved = {k: t.cpu().numpy().copy() for k, t in dict(Q=Q, K=K, **o).items()}
    g = Guards()
    b = dict(dQ=g.o((R, D), "dQ"), dK=g.o((R, D), "dK"), d1=g.o((R, heads), "d1"), d2=g.o((R, heads), "d2"), kp=g.o((R, D), "kp"),
             part=g.o((int(lib.ebn_ff_attn_streamed_partials_len(n_seq, D)),), "partials"))
    n = ctypes.c_int32(-1)
    rc = lib.ebn_ff_attn_streamed_bwd_f32(P(g.i(saved["Q"], "Q")), P(g.i(saved["K"], "K")), P(g.i(d["Wqa"], "Wqa")), P(g.i(d["Wka"], "Wka")),
                                          P(g.i(saved["qw"], "qw")), P(g.i(saved["kw"], "kw")), P(g.i(saved["pq"], "pq")), P(g.i(saved["pk"], "pk")),
                                          P(g.i(d["dout"], "dAO")), P(g.i(d["dout"][::-1].copy(), "dSV")), P(b["dQ"]), P(b["dK"]), P(b["d1"]), P(b["d2"]),
                                          P(b["kp"]), P(b["part"]), ctypes.byref(n), n_seq, T, D, heads, S())
    assert rc == OK and n.value == n_seq
    g.check()  # every scratch buffer has exactly its *_len elements: all written, nothing beside them
    for k, t in b.items():
        assert bool(torch.isfinite(t).all()), k
    assert np.array_equal(b["kp"].cpu().numpy(), saved["K"] * np.repeat(saved["pq"], T, axis=0))


# ---------------------------------------------------------------------------------------------------------------- gates
def test_streamed_gates(hip):
    lib = hip.lib()
    t = torch.zeros(16 * 1024, device="cuda")
    n = ctypes.c_int32(0)
    sup = lib.ebn_ff_attn_streamed_supported

    def fwd(T, D, heads):
        return lib.ebn_ff_attn_streamed_fwd_f32(P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), 0, T, D, heads,
                                                S())

    def bwd(T, D, heads):
        return lib.ebn_ff_attn_streamed_bwd_f32(P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t),
                                                ctypes.byref(n), 0, T, D, heads, S())

    for T, D, heads, code in [(30, 768, 12, OK), (512, 768, 12, OK), (30, 1024, 16, OK), (30, 512, 8, OK), (30, 1028, 4, UNSUPPORTED),
                              (30, 254, 2, UNSUPPORTED), (30, 48, 5, BAD_ARG), (0, 48, 3, BAD_ARG)]:
        assert sup(T, D, heads, 0) == code and sup(T, D, heads, 1) == code, (T, D, heads)
        assert fwd(T, D, heads) == code and bwd(T, D, heads) == code, (T, D, heads)
    # the 64 KiB LDS edge at 768 / 12: 13 T + 1536 floats forward (T <= 1142), 24 T + 3072 floats backward (T <= 554)
    assert sup(1142, 768, 12, 0) == OK and fwd(1142, 768, 12) == OK and sup(1143, 768, 12, 0) == UNSUPPORTED and fwd(1143, 768, 12) == UNSUPPORTED
    assert sup(554, 768, 12, 1) == OK and bwd(554, 768, 12) == OK and sup(555, 768, 12, 1) == UNSUPPORTED and bwd(555, 768, 12) == UNSUPPORTED
    assert sup(555, 768, 12, 0) == OK and fwd(555, 768, 12) == OK  # the backward's bound is the tighter one
    # and at 1024 / 16: 17 T + 2048 forward (T <= 843), 32 T + 4096 backward (T <= 384)
    assert sup(843, 1024, 16, 0) == OK and sup(844, 1024, 16, 0) == UNSUPPORTED and sup(384, 1024, 16, 1) == OK and sup(385, 1024, 16, 1) == UNSUPPORTED
    assert lib.ebn_ff_attn_streamed_partials_len(0, 768) == 3 * 768 and lib.ebn_ff_attn_streamed_partials_len(300, 768) == 256 * 3 * 768
    assert lib.ebn_ff_attn_streamed_partials_len(-1, 768) == 0 and lib.ebn_ff_attn_streamed_dlogits_len(7, 30, 12) == 7 * 30 * 12
    assert lib.ebn_ff_attn_streamed_kp_len(7, 30, 768) == 7 * 30 * 768
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the model
def cfg_of(hidden, heads, layers=1, p=0.0):
    return SimpleNamespace(hidden_size=hidden, num_attention_heads=heads, num_hidden_layers=layers, intermediate_size=64, max_position_embeddings=4,
                           hidden_dropout_prob=p, layer_norm_eps=1e-12, initializer_range=0.1, hidden_act="gelu", pooler_type="weightpooler",
                           vocab_size=30)


def lively_state(cfg, word_dim, seed):
    """a float32 state_dict off the trivial initial values (biases and LayerNorm weights perturbed), so that every gradient path carries signal"""
    torch.manual_seed(seed)
    model = make_model(cfg, word_dim)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("bias") or "LayerNorm.weight" in name:
                p.add_(torch.randn_like(p) * 0.2)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def batch_of(N, H, T, vocab, seed):
    rng = np.random.default_rng(seed)
    hist, cand = rng.integers(1, vocab, (N, H, T)), rng.integers(1, vocab, (N, 1, T))
    for n in range(N):
        for h in range(H):
            hist[n, h, rng.integers(T // 2, T + 1):] = 0
        cand[n, 0, rng.integers(T // 2, T + 1):] = 0
    hist[1, 2] = 0  # one padded history slot
    y = (np.arange(N) % 2).astype(np.float32).reshape(N, 1)
    return torch.as_tensor(hist.astype(np.int32)), torch.as_tensor(cand.astype(np.int32)), torch.as_tensor(y)


def grads_of(model, hist, cand, y):
    model.zero_grad()
    score = model(hist, cand)
    loss = torch.nn.BCELoss()(score, y)
    loss.backward()
    return score, loss, {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}


def oracle_run(state, hist, cand, y, heads, dtype, token_mask, drop):
    Pt = {n: v.detach().to(dtype).clone().requires_grad_(True) for n, v in state.items()}
    s = fo.forward(Pt, hist, cand, heads, 1e-12, token_mask, drop=drop)
    loss = torch.nn.BCELoss()(s, y.to(dtype))
    loss.backward()
    g = {n: (Pt[n].grad.double().numpy() if Pt[n].grad is not None else np.zeros(tuple(Pt[n].shape))) for n in Pt}
    return s.detach().double().numpy(), float(loss.item()), g


def check_against_oracle(model, state, hist, cand, y, heads, token_mask, drop, what):
    """scores, loss and every parameter gradient of one training-mode step against the float64 oracle, within 4 x the float32 oracle's error"""
    names = list(state)
    s64, l64, g64 = oracle_run(state, hist, cand, y, heads, torch.float64, token_mask, drop)
    s32, l32, g32 = oracle_run(state, hist, cand, y, heads, torch.float32, token_mask, drop)
    G = max(float(np.abs(g64[n]).max()) for n in names)
    E_fwd, E_loss = float(np.abs(s32 - s64).max()), abs(l32 - l64)
    E_ref = max(fo.measure(g32[n], g64[n], G) for n in names)
    score, loss, g = grads_of(model, hist.cuda(), cand.cuda(), y.cuda())
    e_fwd, e_loss = float(np.abs(host(score) - s64).max()), abs(loss.item() - l64)
    per = {n: fo.measure(host(g[n]), g64[n], G) for n in names}
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    print(f"{what}: |score - oracle64| = {e_fwd:.3g} (E_fwd {E_fwd:.3g}), |loss - oracle64| = {e_loss:.3g} (float32 oracle {E_loss:.3g}), worst gradient "
          f"measures {worst} (E_ref {E_ref:.3g})")
    assert e_fwd <= 4 * E_fwd
    assert e_loss <= 4 * max(E_fwd, E_loss)
    assert max(per.values()) <= 4 * E_ref, worst
    return score, g


@pytest.mark.parametrize("p,token_mask", [(0.0, "first_slot"), (0.2, "per_slot")])
def test_model_at_768_12_against_the_oracle(hip, p, token_mask):
    cfg, seed = cfg_of(768, 12, p=p), 5
    state = lively_state(cfg, 16, 3)
    hist, cand, y = batch_of(2, 3, 30, cfg.vocab_size, 11)
    model = make_model(cfg, 16, attention="streamed", token_mask=token_mask, seed=seed)
    model.load_state_dict(state, strict=True)
    model = model.cuda().train()
    model.dropout_step = 6  # a step with dropout draws at step 7
    check_against_oracle(model, state, hist, cand, y, 12, token_mask, (p, seed, 7) if p > 0 else None, f"768 / 12, dropout {p}, {token_mask}")
    assert model.dropout_step == (7 if p > 0 else 6)
    with torch.no_grad():
        assert model.user_encoder(hist.cuda()).shape == (2, 768)  # follows the same choice


def golden_streamed():
    from tests.test_fastformer_cpu import load_golden

    z, names, cfg = load_golden()
    model = make_model(cfg, z["word_dim"].item(), attention="streamed")
    model.load_state_dict({n: torch.as_tensor(z["param." + n]) for n in names}, strict=True)
    hist, cand, y = torch.as_tensor(z["hist"]).cuda(), torch.as_tensor(z["cand"]).cuda(), torch.as_tensor(z["labels"]).cuda()
    return z, names, model.cuda().train(), hist, cand, y


def fixture_check(z, names, score, loss, g, what):
    E_fwd, E_ref, G = z["E_fwd"].item(), z["E_ref"].item(), z["G"].item()
    e_fwd = float(np.abs(host(score) - z["f64.score"]).max())
    e_loss = abs(loss.item() - z["f64.loss"].item())
    per = {n: fo.measure(host(g[n]), z["f64.grad." + n], G) for n in names}
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    print(f"{what}: |score - ref64| = {e_fwd:.3g} (E_fwd {E_fwd:.3g}), |loss - ref64| = {e_loss:.3g}, worst gradient measures {worst} (E_ref {E_ref:.3g})")
    assert e_fwd <= 4 * E_fwd
    assert e_loss <= 4 * max(E_fwd, abs(z["f32.loss"].item() - z["f64.loss"].item()))
    assert max(per.values()) <= 4 * E_ref, worst


def test_streamed_model_against_the_reference_fixture(hip):
    z, names, model, hist, cand, y = golden_streamed()
    score, loss, g = grads_of(model, hist, cand, y)
    fixture_check(z, names, score, loss, g, "fixture, streamed")
    with torch.no_grad():
        user = model.user_encoder(hist)
    assert float(user[1].abs().max()) == 0.0 and float(user[0].abs().max()) > 0  # the padded-slot-0 user: exactly zero
    assert np.abs(host(user) - z["f64.user"]).max() <= 4 * np.abs(z["f32.user"].astype(np.float64) - z["f64.user"]).max()


def test_streamed_three_sgd_steps_against_the_reference_trajectory(hip):
    z, names, model, hist, cand, y = golden_streamed()
    traj = np.load(GOLDEN / "fastformer_ref_traj.npz")
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    for _ in range(3):
        opt.zero_grad()
        torch.nn.BCELoss()(model(hist, cand), y).backward()
        opt.step()
    G, E = z["G"].item(), z["E_traj"].item()
    sd = model.state_dict()
    per = {n: fo.measure(host(sd[n]), traj["f64.traj." + n], G) for n in names}
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:3]
    print(f"trajectory, streamed: worst measures {worst} (E_traj {E:.3g})")
    assert max(per.values()) <= 4 * E, worst


def test_streamed_model_against_the_long_title_reference(hip):
    z, names, cfg = load_long()
    hist, cand, y = torch.as_tensor(z["hist"]).cuda(), torch.as_tensor(z["cand"]).cuda(), torch.as_tensor(z["labels"]).cuda()
    state = {n: torch.as_tensor(z["param." + n]) for n in names}
    model = make_model(cfg, z["word_dim"].item(), attention="streamed")
    model.load_state_dict(state, strict=True)
    model = model.cuda().train()
    score, loss, g = grads_of(model, hist, cand, y)
    fixture_check(z, names, score, loss, g, "500-token fixture, streamed")
    resident = make_model(cfg, z["word_dim"].item())
    resident.load_state_dict(state, strict=True)
    with pytest.raises(ValueError, match="attention=\"auto\""):  # T = 500 is past the resident forward's T <= 492 at hidden 24 / 4 heads
        resident.cuda()(hist, cand)
    torch.cuda.synchronize()


def test_auto_is_the_resident_pair_where_it_fits_and_the_streamed_pair_beyond(hip):
    # hidden 256 / 16 heads, T = 12: the resident pair takes both directions -> the default model's bits
    cfg = cfg_of(256, 16)
    state = lively_state(cfg, 16, 4)
    hist, cand, y = (t.cuda() for t in batch_of(2, 3, 12, cfg.vocab_size, 12))
    out = {}
    for kind in ("resident", "auto"):
        model = make_model(cfg, 16, attention=kind)
        model.load_state_dict(state, strict=True)
        model = model.cuda().train()
        assert model._engine.attention_kind(12, True) == "resident"
        out[kind] = grads_of(model, hist, cand, y)
    assert torch.equal(out["resident"][0], out["auto"][0])
    for n in state:
        assert torch.equal(out["resident"][2][n], out["auto"][2][n]), n
    # hidden 512 / 16 heads, T = 8 (the shape of test_unsupported_shape_names_the_limit): the default raises, auto runs the streamed pair
    cfg = cfg_of(512, 16)
    state = lively_state(cfg, 16, 6)
    hist, cand, y = batch_of(2, 3, 8, cfg.vocab_size, 13)
    default = make_model(cfg, 16)
    default.load_state_dict(state, strict=True)
    with pytest.raises(ValueError, match="heads \\* hidden_size <= 4096"):
        default.cuda()(hist.cuda(), cand.cuda())
    model = make_model(cfg, 16, attention="auto")
    model.load_state_dict(state, strict=True)
    model = model.cuda().train()
    assert model._engine.attention_kind(8, True) == "streamed" and model._engine.attention_kind(8, False) == "streamed"
    check_against_oracle(model, state, hist, cand, y, 16, "first_slot", None, "512 / 16, auto")
    torch.cuda.synchronize()
