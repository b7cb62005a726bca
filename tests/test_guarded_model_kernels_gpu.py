"""The Fastformer, NPA-pooling and NAML model kernels on guard-banded operands at their edge shapes, against the float64 references
of tests/model_kernel_refs.py.

Every operand goes through tests/guarded.py (dense rows: ld = width): float inputs sit between NaN guards, integer inputs between
HARMFUL values (a catview id outside its table raises the flag; a q_idx guard names an extra last row of Q that holds NaN), outputs
are pre-filled and sit between canaries, in-place operands are outputs with a payload, scratch is poisoned.  After each call every
handle is checked, every output is compared element-wise -- |got - want| <= c * mag + 1e-30 with `mag` the reference's magnitude
array; a NaN fails -- and a second run must give the same bits where the header promises a fixed summation order.  A backward
kernel gets the float64 forward's outputs rounded to float32, and its reference gets the same arrays: each kernel is judged on its
own step.  The shapes (tests/model_kernel_refs.py) are the smallest at which each lane-strided loop takes no, one and a second trip
and each limit is touched from both sides; tests/test_model_kernel_refs_cpu.py shows which planted defects only they catch.

LIMIT (tests/guarded.py): an over-read whose value a select discards is not seen.

The constant c:
  * C_SUM = 2e-6 for outputs that are one level of fp32 sums and products of the kernel's inputs (and for the LayerNorm pair, whose
    only other operations, the division and the square root, are correctly rounded; its magnitudes carry the row mean's rounding);
  * for outputs behind tanhf / expf / erff or a softmax normalisation (forward `a / sum a`, backward `w (dw - sum w dw)` and what is
    computed from it): 4 x the largest err / mag measured on an MI355X over all shapes of this file (libm differs by a few ulps
    between ROCm releases), never above what the earlier test of the kernel allowed (1e-4 for the pap and NAML outputs, 1e-5 for
    the Fastformer forward outputs, 5e-5 for the Fastformer gradients).

MI355X, 2026-10-19, on top of commit fd57118; max err / mag over all shapes of this file, and the c in force:
  output      max err/mag  c
  ln.Y        8.941e-08   C_SUM = 2e-6
  ln.xhat     9.119e-08   C_SUM = 2e-6
  ln.rstd     4.860e-08   C_SUM = 2e-6
  ln.dX       1.664e-07   C_SUM = 2e-6
  ln.dres     1.654e-07   C_SUM = 2e-6
  ln.sums     1.029e-07   C_SUM = 2e-6
  colsum.out  9.957e-08   C_SUM = 2e-6
  gelu.Y      1.495e-07   6.0e-07   (cap 1e-05)
  gelu.dX     1.362e-07   5.5e-07   (cap 5e-05)
  gelu.dbias  8.421e-08   3.4e-07   (cap 5e-05)
  pool.U      9.374e-08   3.8e-07   (cap 1e-05)
  pool.w      4.266e-08   1.8e-07   (cap 1e-05)
  pool.out    1.928e-08   7.8e-08   (cap 1e-05)
  pool.sinv   1.275e-08   5.1e-08   (cap 1e-05)
  pool.dX     5.945e-08   C_SUM = 2e-6
  pool.de     9.088e-08   3.7e-07   (cap 5e-05)
  pool.db2n   5.841e-08   2.4e-07   (cap 5e-05)
  dpre.dq     1.662e-07   C_SUM = 2e-6
  dpre.dpre   1.259e-07   C_SUM = 2e-6
  dpre.db     4.782e-08   C_SUM = 2e-6
  head.score  4.715e-08   1.9e-07   (cap 1e-05)
  head.duser  1.226e-07   C_SUM = 2e-6
  head.dcand  1.253e-07   C_SUM = 2e-6
  head.dW     4.844e-08   C_SUM = 2e-6
  head.db     9.041e-09   C_SUM = 2e-6
  attn.Q      5.960e-08   C_SUM = 2e-6
  attn.K      5.960e-08   C_SUM = 2e-6
  attn.SV0    1.100e-07   C_SUM = 2e-6
  attn.qw     4.797e-08   2.0e-07   (cap 1e-05)
  attn.kw     1.683e-08   6.8e-08   (cap 1e-05)
  attn.pq     3.307e-08   1.4e-07   (cap 1e-05)
  attn.pk     8.409e-09   3.4e-08   (cap 1e-05)
  attn.AO     9.207e-09   3.7e-08   (cap 1e-05)
  attn.dQ     9.649e-08   3.9e-07   (cap 5e-05)
  attn.dK     1.433e-07   5.8e-07   (cap 5e-05)
  attn.sums   9.236e-08   3.7e-07   (cap 5e-05)
  pap.U       9.562e-08   3.9e-07   (cap 0.0001)
  pap.w       1.747e-08   7.0e-08   (cap 0.0001)
  pap.out     1.504e-08   6.1e-08   (cap 0.0001)
  pap.out_d   1.084e-08   4.4e-08   (cap 0.0001)
  pap.dout    5.960e-08   C_SUM = 2e-6
  pap.dV      1.169e-07   C_SUM = 2e-6
  pap.dq      7.335e-08   3.0e-07   (cap 0.0001)
  pap.dpre    1.172e-07   4.7e-07   (cap 0.0001)
  pap.dQ      8.155e-08   C_SUM = 2e-6
  cat.out     1.203e-07   C_SUM = 2e-6
  cat.dWb     2.063e-07   C_SUM = 2e-6
  cat.dtable  8.317e-08   C_SUM = 2e-6
  va.U        8.565e-08   3.5e-07   (cap 0.0001)
  va.w        4.249e-08   1.7e-07   (cap 0.0001)
  va.news     7.125e-08   2.9e-07   (cap 0.0001)
  va.dVw      5.933e-08   C_SUM = 2e-6
  va.de       1.609e-08   6.5e-08   (cap 0.0001)
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import nrms_numpy as on
from tests import fastformer_oracle as fo
from tests import model_kernel_refs as mr
from tests.guarded import guard_in, guard_out, poison
from tests.hip_testutil import P, S, host, make_state

pytestmark = pytest.mark.gpu
f32 = ctypes.c_float
NAN = float("nan")
OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3
CAP_FF_FWD, CAP_FF_GRAD, CAP_PAP_NAML = 1e-5, 5e-5, 1e-4

# c per output: mr.C_SUM, or 4 x the measured maximum of err / mag (the table above), capped
C = {
    # LayerNorm pair, colsum_finish: fp32 sums, correctly rounded division and square root
    "ln.Y": mr.C_SUM, "ln.xhat": mr.C_SUM, "ln.rstd": mr.C_SUM, "ln.dX": mr.C_SUM, "ln.dres": mr.C_SUM, "ln.sums": mr.C_SUM, "colsum.out": mr.C_SUM,
    # gelu: erff / expf
    "gelu.Y": min(6.0e-07, CAP_FF_FWD), "gelu.dX": min(5.5e-07, CAP_FF_GRAD), "gelu.dbias": min(3.4e-07, CAP_FF_GRAD),
    # pooling: tanhf, expf, a normalisation
    "pool.U": min(3.8e-07, CAP_FF_FWD), "pool.w": min(1.8e-07, CAP_FF_FWD), "pool.out": min(7.8e-08, CAP_FF_FWD), "pool.sinv": min(5.1e-08, CAP_FF_FWD),
    "pool.dX": mr.C_SUM, "pool.de": min(3.7e-07, CAP_FF_GRAD), "pool.db2n": min(2.4e-07, CAP_FF_GRAD), "dpre.dq": mr.C_SUM, "dpre.dpre": mr.C_SUM, "dpre.db": mr.C_SUM,
    # head: expf in the sigmoid; the backward is sums of products of its inputs
    "head.score": min(1.9e-07, CAP_FF_FWD), "head.duser": mr.C_SUM, "head.dcand": mr.C_SUM, "head.dW": mr.C_SUM, "head.db": mr.C_SUM,
    # attention: two softmaxes forward, their backwards nested
    "attn.Q": mr.C_SUM, "attn.K": mr.C_SUM, "attn.SV0": mr.C_SUM, "attn.qw": min(2.0e-07, CAP_FF_FWD), "attn.kw": min(6.8e-08, CAP_FF_FWD), "attn.pq": min(1.4e-07, CAP_FF_FWD),
    "attn.pk": min(3.4e-08, CAP_FF_FWD), "attn.AO": min(3.7e-08, CAP_FF_FWD), "attn.dQ": min(3.9e-07, CAP_FF_GRAD), "attn.dK": min(5.8e-07, CAP_FF_GRAD), "attn.sums": min(3.7e-07, CAP_FF_GRAD),
    # NPA personalised pooling
    "pap.U": min(3.9e-07, CAP_PAP_NAML), "pap.w": min(7.0e-08, CAP_PAP_NAML), "pap.out": min(6.1e-08, CAP_PAP_NAML), "pap.out_d": min(4.4e-08, CAP_PAP_NAML), "pap.dout": mr.C_SUM, "pap.dV": mr.C_SUM,
    "pap.dq": min(3.0e-07, CAP_PAP_NAML), "pap.dpre": min(4.7e-07, CAP_PAP_NAML), "pap.dQ": mr.C_SUM,
    # NAML: the categorical views are sums behind a ReLU; the view attention is tanhf, expf and a normalisation
    "cat.out": mr.C_SUM, "cat.dWb": mr.C_SUM, "cat.dtable": mr.C_SUM,
    "va.U": min(3.5e-07, CAP_PAP_NAML), "va.w": min(1.7e-07, CAP_PAP_NAML), "va.news": min(2.9e-07, CAP_PAP_NAML), "va.dVw": mr.C_SUM, "va.de": min(6.5e-08, CAP_PAP_NAML),
}
MEASURED = {}  # output -> the largest err / mag of this session (printed by every comparison: `pytest -s`)


def cmp(got, ref, key, what=""):
    """print err / mag, then assert |got - want| <= C[key] * mag + TINY element-wise"""
    got = host(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    r = mr.ratio(got.reshape(np.shape(ref[0])), ref[0], ref[1])
    MEASURED[key] = max(MEASURED.get(key, 0.0), r)
    print(f"ERRMAG {key} {r:.3e} {what}")
    mr.check_close(got, ref, C[key], f"{key} {what}")


def r32(a):
    """a float64 reference value as the float32 array a kernel is handed"""
    return np.asarray(a, np.float64).astype(np.float32)


class G:
    """the guarded operands of one call sequence"""

    def __init__(self):
        self.h = []

    def i(self, x, name, fill=NAN, offset=0):
        v, h = guard_in(x, fill=fill, offset=offset)
        self.h.append((name, h))
        return v

    def o(self, shape, name, dtype=torch.float32, offset=0):
        v, h = guard_out(shape, dtype=dtype, offset=offset)
        self.h.append((name, h))
        return v

    def io(self, values, name, offset=0):
        """an in-place operand: an output with a payload"""
        values = np.asarray(values)
        shape = values.shape if values.ndim <= 2 else (int(np.prod(values.shape[:-1])), values.shape[-1])
        v, h = guard_out(shape, offset=offset)
        h.fill_payload(values.reshape(shape))
        self.h.append((name, h))
        return v

    def scratch(self, n, name):
        """scratch of exactly n floats whose every element the kernel must write: canaries around it, a pre-fill inside"""
        return self.o((max(int(n), 1),), name) if n > 0 else poison(torch.empty(1, device="cuda"))

    def check(self):
        torch.cuda.synchronize()
        for name, h in self.h:
            h.check(name)

    def untouched(self):
        torch.cuda.synchronize()
        for name, h in self.h:
            h.check_untouched(name)


def same_bits(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{what}: {k} differs between two runs"


def bits(**tensors):
    return {k: t.detach().cpu().contiguous().numpy().copy() for k, t in tensors.items()}


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_data(R, D, mode, p, seed=9, step=4, site=2):
    rng = np.random.default_rng(R * 31 + D + mode)
    X, dY = rng.normal(size=(R, D)).astype(np.float32), rng.normal(size=(R, D)).astype(np.float32)
    res = rng.normal(size=(D,) if mode == 0 else (R, D)).astype(np.float32)
    bias, gam, bet = (rng.normal(size=D).astype(np.float32) for _ in range(3))
    key = on.dropout_key(seed, step, site)
    mult = fo.drop_mult((R, D), seed, step, site, p, torch.float64, "cpu").numpy() if p > 0 else 1.0
    return X, dY, res, bias, gam, bet, key, mult


@pytest.mark.parametrize("R,D,mode,p", mr.LN_CASES)
def test_layernorm_pair(hip, R, D, mode, p):
    X, dY, res, bias, gam, bet, key, mult = _ln_data(R, D, mode, p)
    eps = 1e-12
    fwd = mr.ff_ln_fwd(X, bias, res, gam, bet, eps, mode, mult)
    xh32, rs32 = r32(fwd["xhat"][0]), r32(fwd["rstd"][0])
    bwd = mr.ff_ln_bwd(dY, xh32, rs32, gam, mode, mult)
    runs = []
    for rep in range(2):
        g = G()
        Y, xh, rs = g.o((R, D), "Y"), g.o((R, D), "xhat"), g.o((R,), "rstd")
        hip.call("ebn_ff_ln_fwd_f32", P(g.i(X, "X")), P(g.i(bias, "bias")), P(g.i(res, "res")), P(g.i(gam, "gamma")), P(g.i(bet, "beta")), f32(eps),
                 mode, key, f32(p), P(Y), P(xh), P(rs), R, D, S())
        g.check()
        g = G()
        dX = g.o((R, D), "dX")
        dres = g.o((R, D), "dres") if mode == 1 else None
        part = g.scratch(hip.lib().ebn_ff_ln_partials_len(R, D), "partials")
        sums = g.o((3 * D,), "sums")
        n = ctypes.c_int32(-1)
        hip.call("ebn_ff_ln_bwd_f32", P(g.i(dY, "dY")), P(g.i(xh32, "xhat")), P(g.i(rs32, "rstd")), P(g.i(gam, "gamma")), mode, key, f32(p), P(dX),
                 P(dres), P(part), ctypes.byref(n), R, D, S())
        hip.call("ebn_ff_colsum_finish_f32", P(part), n.value, 3 * D, 3 * D, P(sums), S())
        g.check()
        assert n.value == min(-(-R // 32), 512) and n.value * 3 * D == part.numel()
        if R == 16400:  # 512 workgroups of 33 rows: those from 497 on own no rows and write zero partials
            tail = part.view(512, 3 * D)[497:]
            assert n.value == 512 and bool((tail == 0).all()) and bool((part.view(512, 3 * D)[496] != 0).any())
        runs.append(bits(Y=Y, xhat=xh, rstd=rs, dX=dX, sums=sums, **({"dres": dres} if mode == 1 else {})))
    same_bits(runs[0], runs[1], "LayerNorm")
    what = f"R={R} D={D} mode={mode} p={p}"
    for k in ("Y", "xhat", "rstd"):
        cmp(runs[0][k], fwd[k], "ln." + k, what)
    for k in ("dX", "sums") + (("dres",) if mode == 1 else ()):
        cmp(runs[0][k], bwd[k], "ln." + k, what)
    if p > 0 and R * D >= 1000:  # the masks themselves: a dropped element is exactly 0
        dropped = mult == 0
        assert (runs[0]["Y" if mode == 0 else "dX"][dropped] == 0).all() and 0.1 < dropped.mean() < 0.3


def test_layernorm_inference_and_aliasing(hip):
    R, D, mode, p = 5, 65, 1, 0.2
    X, dY, res, bias, gam, bet, key, mult = _ln_data(R, D, mode, p)
    fwd = mr.ff_ln_fwd(X, bias, res, gam, bet, 1e-12, mode, mult)
    g = G()
    Y = g.o((R, D), "Y")  # xhat = rstd = NULL: inference
    hip.call("ebn_ff_ln_fwd_f32", P(g.i(X, "X")), P(g.i(bias, "bias")), P(g.i(res, "res")), P(g.i(gam, "gamma")), P(g.i(bet, "beta")), f32(1e-12),
             mode, key, f32(p), P(Y), None, None, R, D, S())
    g.check()
    cmp(Y, fwd["Y"], "ln.Y", "xhat = rstd = NULL")
    g = G()
    XY, xh, rs = g.io(X, "X = Y"), g.o((R, D), "xhat"), g.o((R,), "rstd")  # Y aliases X
    hip.call("ebn_ff_ln_fwd_f32", P(XY), P(g.i(bias, "bias")), P(g.i(res, "res")), P(g.i(gam, "gamma")), P(g.i(bet, "beta")), f32(1e-12), mode, key,
             f32(p), P(XY), P(xh), P(rs), R, D, S())
    g.check()
    cmp(XY, fwd["Y"], "ln.Y", "Y aliases X")
    cmp(xh, fwd["xhat"], "ln.xhat", "Y aliases X")
    assert np.array_equal(host(XY), host(Y))  # and the same bits as the run with its own Y


def test_layernorm_backward_of_no_rows(hip):
    D = 48
    z = np.zeros((1, D), np.float32)
    g = G()
    dX, dres = g.o((1, D), "dX"), g.o((1, D), "dres")
    n_len = int(hip.lib().ebn_ff_ln_partials_len(0, D))
    assert n_len == 3 * D
    part, sums = g.scratch(n_len, "partials"), g.o((3 * D,), "sums")
    n = ctypes.c_int32(-1)
    hip.call("ebn_ff_ln_bwd_f32", P(g.i(z, "dY")), P(g.i(z, "xhat")), P(g.i(z[0, :1], "rstd")), P(g.i(np.ones(D, np.float32), "gamma")), 1, 0,
             f32(0.0), P(dX), P(dres), P(part), ctypes.byref(n), 0, D, S())
    hip.call("ebn_ff_colsum_finish_f32", P(part), n.value, 3 * D, 3 * D, P(sums), S())
    torch.cuda.synchronize()
    assert n.value == 1
    for name, h in g.h:
        (h.check_untouched if name in ("dX", "dres") else h.check)(name)
    assert bool((sums == 0).all()) and bool((part == 0).all())


@pytest.mark.parametrize("n_parts,stride,width", mr.COLSUM_CASES)
def test_colsum_finish_strided(hip, n_parts, stride, width):
    rng = np.random.default_rng(n_parts)
    x = rng.normal(size=(n_parts, width)).astype(np.float32)
    runs = []
    for rep in range(2):
        g = G()
        v, h = guard_in(x, ld=stride)  # the bands between the rows hold NaN
        g.h.append(("partials", h))
        out = g.o((width,), "out")
        hip.call("ebn_ff_colsum_finish_f32", P(v), n_parts, stride, width, P(out), S())
        g.check()
        runs.append(bits(out=out))
    same_bits(runs[0], runs[1], "colsum_finish")
    cmp(runs[0]["out"], mr.ff_colsum_finish(x, n_parts, width, width)["out"], "colsum.out", f"n_parts={n_parts} stride={stride} width={width}")


# ---------------------------------------------------------------------------------------------------------------- gelu
@pytest.mark.parametrize("R,C_", mr.GELU_CASES)
def test_gelu_pair(hip, R, C_):
    rng = np.random.default_rng(R + C_)
    X, b, dY = rng.normal(size=(R, C_)).astype(np.float32) * 2, rng.normal(size=C_).astype(np.float32), rng.normal(size=(R, C_)).astype(np.float32)
    runs = []
    for rep in range(2):
        g = G()
        Y, dX, db = g.o((R, C_), "Y"), g.o((R, C_), "dX"), g.o((C_,), "dbias")
        xd, bd = g.i(X, "X"), g.i(b, "bias")
        part = poison(torch.empty(int(hip.lib().ebn_colsum_partials_len(R, C_)), device="cuda"))
        hip.call("ebn_ff_gelu_fwd_f32", P(xd), P(bd), P(Y), R, C_, S())
        hip.call("ebn_ff_gelu_bwd_f32", P(xd), P(bd), P(g.i(dY, "dY")), P(dX), P(db), P(part), R, C_, S())
        g.check()
        runs.append(bits(Y=Y, dX=dX, dbias=db))
    same_bits(runs[0], runs[1], "gelu")
    what = f"R={R} C={C_}"
    cmp(runs[0]["Y"], mr.ff_gelu_fwd(X, b)["Y"], "gelu.Y", what)
    bwd = mr.ff_gelu_bwd(X, b, dY)
    cmp(runs[0]["dX"], bwd["dX"], "gelu.dX", what)
    cmp(runs[0]["dbias"], bwd["dbias"], "gelu.dbias", what)


# ---------------------------------------------------------------------------------------------------------------- pooling
def _pool_mask(kind, n_seq, L, rng):
    m = (rng.random((n_seq, L)) < 0.7).astype(np.float32)
    m[:, 0] = 1
    if kind == "ones":
        m[:] = 1
    elif kind == "one_dead":
        m[1] = 0
    elif kind in ("first", "last"):
        m[:] = 0
        m[:, 0 if kind == "first" else L - 1] = 1
    return m


@pytest.mark.parametrize("n_seq,L,D,kind", mr.POOL_CASES)
def test_pooling_pair(hip, n_seq, L, D, kind):
    rng = np.random.default_rng(L * 7 + D)
    Upre, X = rng.normal(size=(n_seq, L, D)).astype(np.float32), rng.normal(size=(n_seq, L, D)).astype(np.float32)
    b1, w2 = rng.normal(size=D).astype(np.float32) * 0.2, (rng.normal(size=D) * 0.3 / math.sqrt(max(D / 48, 1))).astype(np.float32)
    b2, dout = np.array([0.4], np.float32), rng.normal(size=(n_seq, D)).astype(np.float32)
    mask = _pool_mask(kind, n_seq, L, rng)
    fwd = mr.ff_pool_fwd(Upre, b1, w2, b2, X, mask)
    U32, w32, sinv32 = r32(fwd["U"][0]), r32(fwd["w"][0]), r32(fwd["sinv"][0])
    bwd = mr.ff_pool_bwd(X, w32, sinv32, dout)
    de32 = r32(bwd["de"][0])
    rest = mr.attpool_bwd_dpre(U32.reshape(-1, D), w2, de32.reshape(-1))
    R = n_seq * L
    runs = []
    for rep in range(2):
        g = G()
        U, out, w, sinv = g.io(Upre, "U"), g.o((n_seq, D), "out"), g.o((n_seq, L), "w"), g.o((n_seq,), "sinv")
        hip.call("ebn_ff_pool_fwd_f32", P(U), P(g.i(b1, "b1")), P(g.i(w2, "w2")), P(g.i(b2, "b2")), P(g.i(X, "X")), P(g.i(mask, "mask")), P(out), P(w),
                 P(sinv), n_seq, L, D, S())
        g.check()
        g = G()
        dX, de, db2n = g.o((R, D), "dX"), g.o((R,), "de"), g.o((n_seq,), "db2n")
        hip.call("ebn_ff_pool_bwd_f32", P(g.i(X, "X")), P(g.i(w32, "w")), P(g.i(sinv32, "sinv")), P(g.i(dout, "dout")), P(dX), P(de), P(db2n), n_seq,
                 L, D, S())
        g.check()
        g = G()
        Ut, dw2, db1 = g.io(U32, "U (tanh)"), g.o((D,), "dw2"), g.o((D,), "db1")
        part = poison(torch.empty(int(hip.lib().ebn_attpool_partials_len(R, D)), device="cuda"))
        hip.call("ebn_attpool_bwd_dpre_f32", P(Ut), P(g.i(w2, "w2")), P(g.i(de32, "de")), P(dw2), P(db1), P(part), R, D, 0, S())
        g.check()
        runs.append(bits(U=U, out=out, w=w, sinv=sinv, dX=dX, de=de, db2n=db2n, dpre=Ut, dq=dw2, db=db1))
    same_bits(runs[0], runs[1], "pooling")
    what = f"n_seq={n_seq} L={L} D={D} mask={kind}"
    got = runs[0]
    for k in ("U", "w", "out", "sinv"):
        cmp(got[k], fwd[k], "pool." + k, what)
    for k in ("dX", "de", "db2n"):
        cmp(got[k], bwd[k], "pool." + k, what)
    for k in ("dq", "dpre", "db"):
        cmp(got[k], rest[k], "dpre." + k, what)
    dead = mask.sum(1) == 0
    assert (got["out"][dead] == 0).all() and (got["w"][dead] == 0).all()  # an all-masked sequence pools to exactly 0
    assert (got["w"][mask == 0] == 0).all()
    if kind in ("first", "last"):
        np.testing.assert_allclose(got["out"], X[:, 0 if kind == "first" else L - 1], rtol=1e-6, atol=1e-7)  # the one live token, weight 1 - 1e-8 / a


def test_pooling_refuses_4097_rows(hip):
    lib, D = hip.lib(), 4
    g = G()
    z = np.zeros((2, D), np.float32)
    args = [g.io(z, "U"), g.i(z[0], "b1"), g.i(z[0], "w2"), g.i(z[0, :1], "b2"), g.i(z, "X"), g.i(z[0], "mask"), g.o((1, D), "out"), g.o((2,), "w"),
            g.o((1,), "sinv")]
    assert lib.ebn_ff_pool_fwd_f32(*(P(a) for a in args), 1, 4097, D, S()) == UNSUPPORTED
    argb = [g.i(z, "X"), g.i(z[0], "w"), g.i(z[0, :1], "sinv"), g.i(z[0], "dout"), g.o((2, D), "dX"), g.o((2,), "de"), g.o((1,), "db2n")]
    assert lib.ebn_ff_pool_bwd_f32(*(P(a) for a in argb), 1, 4097, D, S()) == UNSUPPORTED
    g.untouched()


# ---------------------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("N,D", mr.HEAD_CASES)
def test_head_pair(hip, N, D):
    rng = np.random.default_rng(N * 13 + D)
    u, c, W, bb, ds = (rng.normal(size=s).astype(np.float32) for s in ((N, D), (N, D), (2 * D,), (1,), (N,)))
    W *= np.float32(0.2)
    fwd = mr.ff_head_fwd(u, c, W, bb)
    s32 = r32(fwd["score"][0])
    bwd = mr.ff_head_bwd(u, c, W, s32, ds)
    runs = []
    for rep in range(2):
        g = G()
        sc = g.o((N,), "score")
        hip.call("ebn_ff_head_fwd_f32", P(g.i(u, "user")), P(g.i(c, "cand")), P(g.i(W, "W")), P(g.i(bb, "b")), P(sc), N, D, S())
        g.check()
        g = G()
        du, dc, dW, db = g.o((N, D), "duser"), g.o((N, D), "dcand"), g.o((2 * D,), "dW"), g.o((1,), "db")
        hip.call("ebn_ff_head_bwd_f32", P(g.i(u, "user")), P(g.i(c, "cand")), P(g.i(W, "W")), P(g.i(s32, "score")), P(g.i(ds, "dscore")), P(du), P(dc),
                 P(dW), P(db), N, D, S())
        g.check()
        runs.append(bits(score=sc, duser=du, dcand=dc, dW=dW, db=db))
    same_bits(runs[0], runs[1], "head")
    cmp(runs[0]["score"], fwd["score"], "head.score", f"N={N} D={D}")
    for k in ("duser", "dcand", "dW", "db"):
        cmp(runs[0][k], bwd[k], "head." + k, f"N={N} D={D}")


def test_head_backward_of_no_rows(hip):
    D = 129
    z = np.zeros((1, D), np.float32)
    g = G()
    du, dc, dW, db = g.o((1, D), "duser"), g.o((1, D), "dcand"), g.o((2 * D,), "dW"), g.o((1,), "db")
    hip.call("ebn_ff_head_bwd_f32", P(g.i(z, "user")), P(g.i(z, "cand")), P(g.i(np.ones(2 * D, np.float32), "W")), P(g.i(z[0, :1], "score")),
             P(g.i(z[0, :1], "dscore")), P(du), P(dc), P(dW), P(db), 0, D, S())
    torch.cuda.synchronize()
    for name, h in g.h:
        (h.check_untouched if name in ("duser", "dcand") else h.check)(name)
    assert bool((dW == 0).all()) and bool((db == 0).all())


# ---------------------------------------------------------------------------------------------------------------- attention
def _attn_data(n_seq, T, D, heads, seed=0):
    rng = np.random.default_rng(T * 7 + D + seed)
    d = dict(Qr=rng.normal(size=(n_seq, T, D)), Kr=rng.normal(size=(n_seq, T, D)), bq=rng.normal(size=D) * 0.3, bk=rng.normal(size=D) * 0.3,
             btr=rng.normal(size=D) * 0.3, Wqa=rng.normal(size=(heads, D)) * 0.5, bqa=rng.normal(size=heads) * 0.3,
             Wka=rng.normal(size=(heads, D)) * 0.5, bka=rng.normal(size=heads) * 0.3, dAO=rng.normal(size=(n_seq, T, D)),
             dSV=rng.normal(size=(n_seq, T, D)))
    d = {k: v.astype(np.float32) for k, v in d.items()}
    mask = (rng.random((n_seq, T)) < 0.7).astype(np.float32)
    mask[:, 0] = 1  # every sequence compared by value keeps a live token: float64 does not mimic the -10000 + x logits of an all-padding one
    mask[-1] = 1
    d["mask"] = mask
    return d


def _attn_fwd_call(lib, g, d, n_seq, T, D, heads, with_sv, q_offset=0, Q0=None, K0=None):
    R = n_seq * T
    Q = g.io(d["Qr"] if Q0 is None else Q0, "Q", offset=q_offset)
    K = g.io(d["Kr"] if K0 is None else K0, "K")
    o = dict(Q=Q, K=K, AO=g.o((R, D), "AO"), SV0=g.o((R, D), "SV0") if with_sv else None, qw=g.o((n_seq * heads, T), "qw"),
             kw=g.o((n_seq * heads, T), "kw"), pq=g.o((n_seq, D), "pq"), pk=g.o((n_seq, D), "pk"))
    rc = lib.ebn_ff_attn_fwd_f32(P(Q), P(K), P(g.i(d["bq"], "bq")), P(g.i(d["bk"], "bk")), P(g.i(d["btr"], "btr")), P(g.i(d["Wqa"], "Wqa")),
                                 P(g.i(d["bqa"], "bqa")), P(g.i(d["Wka"], "Wka")), P(g.i(d["bka"], "bka")), P(g.i(d["mask"], "mask")), P(o["AO"]),
                                 P(o["SV0"]), P(o["qw"]), P(o["kw"]), P(o["pq"]), P(o["pk"]), n_seq, T, D, heads, S())
    return rc, o


def _attn_bwd_call(lib, g, d, saved, n_seq, T, D, heads, with_sv, q_offset=0):
    R, W = n_seq * T, 2 * heads * D + 3 * D
    o = dict(dQ=g.o((R, D), "dQ"), dK=g.o((R, D), "dK"), part=g.scratch(lib.ebn_ff_attn_partials_len(n_seq, D, heads), "partials"))
    n = ctypes.c_int32(-1)
    rc = lib.ebn_ff_attn_bwd_f32(P(g.i(saved["Q"], "Q", offset=q_offset)), P(g.i(saved["K"], "K")), P(g.i(d["Wqa"], "Wqa")), P(g.i(d["Wka"], "Wka")),
                                 P(g.i(saved["qw"], "qw")), P(g.i(saved["kw"], "kw")), P(g.i(saved["pq"], "pq")), P(g.i(saved["pk"], "pk")),
                                 P(g.i(d["dAO"], "dAO")), P(g.i(d["dSV"], "dSV")) if with_sv else None, P(o["dQ"]), P(o["dK"]), P(o["part"]),
                                 ctypes.byref(n), n_seq, T, D, heads, S())
    if rc == OK:
        o["sums"] = g.o((W,), "sums")
        assert lib.ebn_ff_colsum_finish_f32(P(o["part"]), n.value, W, W, P(o["sums"]), S()) == OK
    return rc, o, n.value


@pytest.mark.parametrize("n_seq,T,D,heads,with_sv,with_bwd", mr.ATTN_CASES)
def test_attention_pair(hip, n_seq, T, D, heads, with_sv, with_bwd):
    lib = hip.lib()
    d = _attn_data(n_seq, T, D, heads)
    fwd = mr.ff_attn_fwd(d["Qr"], d["Kr"], d["bq"], d["bk"], d["btr"], d["Wqa"], d["bqa"], d["Wka"], d["bka"], d["mask"], heads)
    saved = {k: r32(fwd[k][0]) for k in ("Q", "K", "qw", "kw", "pq", "pk")}
    fkeys = ("Q", "K", "AO", "qw", "kw", "pq", "pk") + (("SV0",) if with_sv else ())
    runs = []
    for rep in range(2):
        g = G()
        rc, o = _attn_fwd_call(lib, g, d, n_seq, T, D, heads, with_sv)
        assert rc == OK
        g.check()
        run = bits(**{k: o[k] for k in fkeys})
        if with_bwd:
            g = G()
            rc, ob, n_parts = _attn_bwd_call(lib, g, d, saved, n_seq, T, D, heads, with_sv)
            assert rc == OK and n_parts == min(n_seq, 256)  # n_seq = 257: workgroup 0 walks sequences 0 and 256
            g.check()
            run.update(bits(dQ=ob["dQ"], dK=ob["dK"], sums=ob["sums"]))
        runs.append(run)
    same_bits(runs[0], runs[1], "attention")
    what = f"n_seq={n_seq} T={T} D={D} heads={heads} SV={with_sv}"
    for k in fkeys:
        cmp(runs[0][k], fwd[k], "attn." + k, what)
    if with_bwd:
        bwd = mr.ff_attn_bwd(saved["Q"], saved["K"], d["Wqa"], d["Wka"], saved["qw"], saved["kw"], saved["pq"], saved["pk"], d["dAO"],
                             d["dSV"] if with_sv else None, heads)
        for k in ("dQ", "dK", "sums"):
            cmp(runs[0][k], bwd[k], "attn." + k, what)
        if not with_sv:
            assert (runs[0]["sums"][-D:] == 0).all()  # colsum(dSV) of no dSV


def test_attention_all_padding_sequence_stays_finite(hip):
    lib = hip.lib()
    n_seq, T, D, heads = 2, 13, 48, 3
    d = _attn_data(n_seq, T, D, heads)
    d["mask"][1] = 0
    g = G()
    rc, o = _attn_fwd_call(lib, g, d, n_seq, T, D, heads, True)
    assert rc == OK
    g.check()
    for k in ("Q", "K", "AO", "SV0", "qw", "kw", "pq", "pk"):
        assert bool(torch.isfinite(o[k]).all()), k
    for k in ("qw", "kw"):
        assert float((o[k].sum(1) - 1).abs().max()) <= 1e-6, k
    saved = {k: host(o[k]).astype(np.float32) for k in ("Q", "K", "qw", "kw", "pq", "pk")}
    g = G()
    rc, ob, _ = _attn_bwd_call(lib, g, d, saved, n_seq, T, D, heads, True)
    assert rc == OK
    g.check()
    for k in ("dQ", "dK", "sums"):
        assert bool(torch.isfinite(ob[k]).all()), k


def test_attention_refusals_write_nothing(hip):
    lib = hip.lib()
    n_seq, T, D, heads = 2, 13, 48, 3
    d = _attn_data(n_seq, T, D, heads)
    fwd = mr.ff_attn_fwd(d["Qr"], d["Kr"], d["bq"], d["bk"], d["btr"], d["Wqa"], d["bqa"], d["Wka"], d["bka"], d["mask"], heads)
    saved = {k: r32(fwd[k][0]) for k in ("Q", "K", "qw", "kw", "pq", "pk")}
    g = G()
    rc, _ = _attn_fwd_call(lib, g, d, n_seq, T, D, heads, True, q_offset=1)  # Q one float off a 16-byte boundary
    assert rc == ALIGN
    rc, _, _ = _attn_bwd_call(lib, g, d, saved, n_seq, T, D, heads, True, q_offset=1)
    assert rc == ALIGN
    g.untouched()
    # one row past the 64 KiB LDS edges, with sequences to run (n_seq = 0 would return before the launch anyway)
    for T_, bwd_ in ((54, False), (48, True)):
        d = _attn_data(2, T_, 256, 16)
        g = G()
        if bwd_:
            z = {k: np.zeros(s, np.float32) for k, s in dict(Q=(2 * T_, 256), K=(2 * T_, 256), qw=(32, T_), kw=(32, T_), pq=(2, 256), pk=(2, 256)).items()}
            rc, _, _ = _attn_bwd_call(lib, g, d, z, 2, T_, 256, 16, True)
        else:
            rc, _ = _attn_fwd_call(lib, g, d, 2, T_, 256, 16, True)
        assert rc == UNSUPPORTED, (T_, bwd_)
        g.untouched()


# ---------------------------------------------------------------------------------------------------------------- NPA pooling
def _pap_data(n_seq, L, F, A, n_live_q=3):
    """Q has n_live_q rows that sequences name, one row nobody names, and a LAST row of NaN: the harmful value of the q_idx guards"""
    rng = np.random.default_rng(L * 5 + F + A)
    n_q = n_live_q + 2
    V = rng.uniform(0, 1, (n_seq, L, F)).astype(np.float32)
    Wa = (rng.uniform(-1, 1, (F, A)) / np.sqrt(F)).astype(np.float32)
    ba = rng.uniform(-0.1, 0.1, A).astype(np.float32)
    Q = rng.uniform(-1, 1, (n_q, A)).astype(np.float32)
    Q[n_q - 1] = np.nan
    q_idx = rng.integers(0, n_live_q, n_seq).astype(np.int32)
    q_idx[0] = -1  # outside [0, n_q): reads row 0
    if n_seq > 2:
        q_idx[2], q_idx[3] = n_q, 0
    dout = rng.uniform(-1, 1, (n_seq, F)).astype(np.float32)
    return V, Wa, ba, Q, q_idx, dout, n_q


@pytest.mark.parametrize("n_seq,L,F,A,n_drop,with_out_d,with_dV", mr.PAP_CASES)
def test_pap_pair(hip, n_seq, L, F, A, n_drop, with_out_d, with_dV):
    V, Wa, ba, Q, q_idx, dout, n_q = _pap_data(n_seq, L, F, A)
    R, p, site = n_seq * L, 0.2, 4
    st = make_state(mr.SEED, mr.STEP)
    mult = mr._mult(site, p, n_drop * F).reshape(n_drop, F) if n_drop else np.ones((0, F))
    g = G()
    Upre = g.o((R, A), "U = V . Wa")
    hip.call("ebn_gemm_f32", 0, 0, R, A, F, f32(1.0), P(g.i(V, "V")), F, P(g.i(Wa, "Wa")), A, f32(0.0), P(Upre), A, S())
    g.check()
    Upre = host(Upre).astype(np.float32).reshape(n_seq, L, A)  # the GEMM has its own guarded tests: its product is this test's input
    assert np.abs(Upre - V.astype(np.float64) @ Wa.astype(np.float64)).max() <= 1e-5
    fwd = mr.pap_fwd(Upre, ba, Q, q_idx, V, n_drop, mult)
    U32, w32 = r32(fwd["U"][0]), r32(fwd["w"][0])
    bwd = mr.pap_bwd(U32, Q, q_idx, V, w32, dout, n_drop, mult)
    dq32 = r32(bwd["dq"][0])
    red = mr.pap_dq_reduce(dq32, q_idx, n_q)
    guard_q = n_q - 1  # the NaN row
    runs = []
    for rep in range(2):
        g = G()
        U, out, w = g.io(Upre, "U"), g.o((n_seq, F), "out"), g.o((R,), "w")
        out_d = g.o((max(n_drop, 1), F), "out_d") if with_out_d else None
        hip.call("ebn_pap_fwd_f32", P(U), P(g.i(ba, "ba")), P(g.i(Q, "Q")), P(g.i(q_idx, "q_idx", fill=guard_q)), n_q, P(g.i(V, "V")), P(out), P(w),
                 P(out_d), n_drop, n_seq, L, F, A, P(st), site, f32(p), S())
        torch.cuda.synchronize()
        for name, h in g.h:
            (h.check_untouched if name == "out_d" and n_drop == 0 else h.check)(name)
        run = bits(U=U, out=out, w=w, **({"out_d": out_d[:n_drop]} if with_out_d else {}))
        g = G()
        Ut, dd, dq = g.io(U32, "U (tanh)"), g.io(dout, "dout"), g.o((n_seq, A), "dq")
        dV = g.o((R, F), "dV") if with_dV else None
        hip.call("ebn_pap_bwd_f32", P(Ut), P(g.i(Q, "Q")), P(g.i(q_idx, "q_idx", fill=guard_q)), n_q, P(g.i(V, "V")), P(g.i(w32, "w")), P(dd), P(dV),
                 P(dq), n_drop, n_seq, L, F, A, P(st), site, f32(p), S())
        g.check()
        g = G()
        dQ = g.o((n_q, A), "dQ")
        hip.call("ebn_pap_dq_reduce_f32", P(g.i(dq32, "dq")), P(g.i(q_idx, "q_idx", fill=guard_q)), n_seq, P(dQ), n_q, A, S())
        g.check()
        run.update(bits(dout=dd, dq=dq, dpre=Ut, dQ=dQ, **({"dV": dV} if with_dV else {})))
        runs.append(run)
    same_bits(runs[0], runs[1], "pap")
    what = f"n_seq={n_seq} L={L} F={F} A={A} n_drop={n_drop}"
    got = runs[0]
    for k in ("U", "w", "out") + (("out_d",) if with_out_d else ()):
        cmp(got[k], fwd[k], "pap." + k, what)
    for k in ("dout", "dq", "dpre") + (("dV",) if with_dV else ()):
        cmp(got[k], bwd[k], "pap." + k, what)
    cmp(got["dQ"], red["dQ"], "pap.dQ", what)
    # rows -1 and n_q behave exactly as row 0 in all three kernels: the same call with those indices replaced gives the same bits
    named = set(mr.pap_rows(q_idx, n_q).tolist())
    for row in range(n_q):
        if row not in named:
            assert (got["dQ"][row] == 0).all(), row  # zeros written over the pre-fill (row n_q - 2 is never named, nor is the NaN row)
    assert n_q - 2 not in named and n_q - 1 not in named
    g = G()
    qi0 = mr.pap_rows(q_idx, n_q).astype(np.int32)
    U, out, w = g.io(Upre, "U"), g.o((n_seq, F), "out"), g.o((R,), "w")
    hip.call("ebn_pap_fwd_f32", P(U), P(g.i(ba, "ba")), P(g.i(Q, "Q")), P(g.i(qi0, "q_idx", fill=guard_q)), n_q, P(g.i(V, "V")), P(out), P(w), None, 0,
             n_seq, L, F, A, None, -1, f32(0.0), S())
    Ut, dd, dq, dQ = g.io(U32, "U (tanh)"), g.io(got["dout"], "dout"), g.o((n_seq, A), "dq"), g.o((n_q, A), "dQ")
    hip.call("ebn_pap_bwd_f32", P(Ut), P(g.i(Q, "Q")), P(g.i(qi0, "q_idx", fill=guard_q)), n_q, P(g.i(V, "V")), P(g.i(w32, "w")), P(dd), None, P(dq), 0,
             n_seq, L, F, A, None, -1, f32(0.0), S())
    hip.call("ebn_pap_dq_reduce_f32", P(g.i(dq32, "dq")), P(g.i(qi0, "q_idx", fill=guard_q)), n_seq, P(dQ), n_q, A, S())
    g.check()
    same_bits({k: got[k] for k in ("out", "w", "dq", "dpre", "dQ")}, bits(out=out, w=w, dq=dq, dpre=Ut, dQ=dQ), "q_idx -1 / n_q against row 0")


def test_pap_refuses_257_rows_and_4097_columns(hip):
    lib = hip.lib()
    z = np.zeros((2, 4), np.float32)
    qi = np.zeros(1, np.int32)
    for L, F in ((257, 4), (1, 4097)):
        g = G()
        rc = lib.ebn_pap_fwd_f32(P(g.io(z, "U")), P(g.i(z[0], "ba")), P(g.i(z, "Q")), P(g.i(qi, "q_idx", fill=0)), 2, P(g.i(z, "V")), P(g.o((1, 4), "out")),
                                 P(g.o((2,), "w")), P(g.o((1, 4), "out_d")), 1, 1, L, F, 4, None, -1, f32(0.0), S())
        assert rc == UNSUPPORTED, (L, F)
        rc = lib.ebn_pap_bwd_f32(P(g.io(z, "U")), P(g.i(z, "Q")), P(g.i(qi, "q_idx", fill=0)), 2, P(g.i(z, "V")), P(g.i(z[0], "w")), P(g.io(z[:1], "dout")),
                                 P(g.o((2, 4), "dV")), P(g.o((1, 4), "dq")), 1, 1, L, F, 4, None, -1, f32(0.0), S())
        assert rc == UNSUPPORTED, (L, F)
        g.untouched()


@pytest.mark.parametrize("n_rows,A", mr.BIAS_TANH_CASES)
def test_bias_tanh_rows_equals_pap_forward_bits(hip, n_rows, A):
    rng = np.random.default_rng(A)
    L, F = n_rows, 3
    Upre, ba = (rng.normal(size=(n_rows, A)) * 2).astype(np.float32), rng.uniform(-0.5, 0.5, A).astype(np.float32)
    V, Q = rng.uniform(0, 1, (L, F)).astype(np.float32), rng.uniform(-1, 1, (1, A)).astype(np.float32)
    g = G()
    U1, U2 = g.io(Upre, "U of pap_fwd"), g.io(Upre, "U of bias_tanh_rows")
    hip.call("ebn_pap_fwd_f32", P(U1), P(g.i(ba, "ba")), P(g.i(Q, "Q")), P(g.i(np.zeros(1, np.int32), "q_idx", fill=0)), 1, P(g.i(V, "V")),
             P(g.o((1, F), "out")), P(g.o((L,), "w")), None, 0, 1, L, F, A, None, -1, f32(0.0), S())
    hip.call("ebn_bias_tanh_rows_f32", P(U2), P(g.i(ba, "ba")), n_rows, A, S())
    g.check()
    same_bits(bits(U=U1), bits(U=U2), "bias_tanh_rows against pap_fwd")
    pre = Upre.astype(np.float64) + ba
    cmp(U2, mr._tanh(pre, np.abs(Upre).astype(np.float64) + np.abs(ba)), "pap.U", f"bias_tanh_rows n_rows={n_rows} A={A}")


# ---------------------------------------------------------------------------------------------------------------- NAML categorical views
def _cat_data(N, K0, K1, F, r0, r1, kind):
    rng = np.random.default_rng(N * 3 + K0 + F)
    ids = [rng.integers(0, r, N).astype(np.int32) for r in (r0, r1)]
    if N >= 6:
        ids[0][:3] = ids[0][5]  # duplicate ids: their table gradients add up
    if kind == "oob":
        ids[0][1], ids[1][N - 1] = r0, -1
    if kind == "all_oob":
        ids[0][:] = r0 + np.arange(N)
    tabs = [rng.uniform(-0.5, 0.5, (r, K)).astype(np.float32) for r, K in ((r0, K0), (r1, K1))]
    Wbs = [rng.uniform(-0.5, 0.5, (K + 1, F)).astype(np.float32) for K in (K0, K1)]
    douts = [rng.normal(size=(N, F)).astype(np.float32) for _ in range(2)]
    return ids, tabs, Wbs, douts


@pytest.mark.parametrize("N,K0,K1,F,r0,r1,kind", mr.CATVIEW_CASES)
def test_catview_pair(hip, N, K0, K1, F, r0, r1, kind):
    ids, tabs, Wbs, douts = _cat_data(N, K0, K1, F, r0, r1, kind)
    rows, Ks = (r0, r1), (K0, K1)
    fwd = [mr.naml_catview_fwd(ids[v], tabs[v], Wbs[v]) for v in range(2)]
    want_flag = int(fwd[0]["oob"] or fwd[1]["oob"])
    assert want_flag == (kind in ("oob", "all_oob"))
    runs = []
    for rep in range(2):
        g = G()
        # an id guard outside the table: an over-read of the ids raises the flag (and would read a zero row, never an address)
        i = [g.i(ids[v], f"ids{v}", fill=rows[v] + 7) for v in range(2)]
        t = [g.i(tabs[v], f"table{v}") for v in range(2)]
        W = [g.i(Wbs[v], f"Wb{v}") for v in range(2)]
        out = [g.o((N, F), f"out{v}") for v in range(2)]
        flag = None
        if kind != "noflag":
            flag = g.o((1,), "oob_flag", dtype=torch.int32)
            flag.zero_()
            g.h[-1][1].fill_payload(np.zeros(1, np.int32))
        hip.call("ebn_naml_catview_fwd_f32", P(i[0]), P(t[0]), r0, K0, P(W[0]), P(out[0]), P(i[1]), P(t[1]), r1, K1, P(W[1]), P(out[1]), N, F, P(flag),
                 S())
        g.check()
        if flag is not None:
            assert int(flag.item()) == want_flag  # 0 with every id in range: no id guard was read
        o32 = [host(out[v]).astype(np.float32) for v in range(2)]
        g = G()
        i = [g.i(ids[v], f"ids{v}", fill=rows[v] + 7) for v in range(2)]
        dW = [g.o((Ks[v] + 1, F), f"dWb{v}") for v in range(2)]
        dt = [g.o((rows[v], Ks[v]), f"dtable{v}") for v in range(2)]
        n_part = int(hip.lib().ebn_naml_catview_partials_len(N, K0, K1, F))
        part = g.scratch(n_part, "partials")
        a = [(P(i[v]), P(g.i(tabs[v], f"table{v}")), rows[v], Ks[v], P(g.i(Wbs[v], f"Wb{v}")), P(g.i(o32[v], f"out{v}")), P(g.i(douts[v], f"dout{v}")),
              P(dW[v]), P(dt[v])) for v in range(2)]
        hip.call("ebn_naml_catview_bwd_f32", *a[0], *a[1], P(part), n_part, N, F, S())
        g.check()
        runs.append(bits(out0=out[0], out1=out[1], dWb0=dW[0], dtable0=dt[0], dWb1=dW[1], dtable1=dt[1]))
    same_bits(runs[0], runs[1], "catview")
    got = runs[0]
    for v in range(2):
        what = f"view {v}: N={N} K={Ks[v]} F={F} rows={rows[v]} {kind}"
        cmp(got[f"out{v}"], fwd[v]["out"], "cat.out", what)
        bwd = mr.naml_catview_bwd(ids[v], tabs[v], Wbs[v], got[f"out{v}"], douts[v])  # the gate is the kernel's own forward output
        cmp(got[f"dWb{v}"], bwd["dWb"], "cat.dWb", what)
        cmp(got[f"dtable{v}"], bwd["dtable"], "cat.dtable", what)
        unnamed = np.setdiff1d(np.arange(rows[v]), ids[v])
        assert (got[f"dtable{v}"][unnamed] == 0).all()  # rows no id names: exact zeros over the pre-fill
    if kind == "all_oob":
        assert (got["out0"] == np.maximum(Wbs[0][K0], 0)).all() and (got["dtable0"] == 0).all() and (got["dWb0"][:K0] == 0).all()


def test_catview_refuses_257_columns(hip):
    lib = hip.lib()
    z = np.zeros((2, 4), np.float32)
    for K0, K1 in ((257, 4), (4, 257)):
        g = G()
        i = [g.i(np.zeros(1, np.int32), f"ids{v}", fill=9) for v in range(2)]
        flag = g.o((1,), "oob_flag", dtype=torch.int32)
        rc = lib.ebn_naml_catview_fwd_f32(P(i[0]), P(g.i(z, "table0")), 1, K0, P(g.i(z, "Wb0")), P(g.o((1, 4), "out0")), P(i[1]), P(g.i(z, "table1")), 1, K1,
                                          P(g.i(z, "Wb1")), P(g.o((1, 4), "out1")), 1, 4, P(flag), S())
        assert rc == UNSUPPORTED
        part = g.o((64,), "partials")
        a = [(P(i[v]), P(g.i(z, "table")), 1, K, P(g.i(z, "Wb")), P(g.i(z[0], "out")), P(g.i(z[0], "dout")), P(g.o((2, 4), "dWb")), P(g.o((1, 4), "dtable")))
             for v, K in enumerate((K0, K1))]
        assert lib.ebn_naml_catview_bwd_f32(*a[0], *a[1], P(part), 64, 1, 4, S()) == UNSUPPORTED
        assert lib.ebn_naml_catview_partials_len(1, K0, K1, 4) == 0
        g.untouched()


# ---------------------------------------------------------------------------------------------------------------- NAML view attention
@pytest.mark.parametrize("nv,N,F,A", mr.VIEWATT_CASES)
def test_viewatt_pair(hip, nv, N, F, A):
    rng = np.random.default_rng(nv * 11 + F + A)
    Vw, Upre = rng.uniform(-1, 1, (nv, N, F)).astype(np.float32), rng.normal(size=(nv, N, A)).astype(np.float32)
    b, q = rng.uniform(-0.1, 0.1, A).astype(np.float32), (rng.uniform(-0.3, 0.3, A) / math.sqrt(max(A / 64, 1))).astype(np.float32)
    dnews = rng.normal(size=(N, F)).astype(np.float32)
    R = nv * N
    fwd = mr.naml_viewatt_fwd(Upre, b, q, Vw)
    U32, w32 = r32(fwd["U"][0]), r32(fwd["w"][0])
    bwd = mr.naml_viewatt_bwd(Vw, w32, dnews)
    de32 = r32(bwd["de"][0])
    rest = mr.attpool_bwd_dpre(U32.reshape(R, A), q, de32.reshape(-1))
    runs = []
    for rep in range(2):
        g = G()
        U, w, news = g.io(Upre, "U"), g.o((nv, N), "w"), g.o((N, F), "news")
        hip.call("ebn_naml_viewatt_fwd_f32", P(U), P(g.i(b, "b")), P(g.i(q, "q")), P(g.i(Vw, "Vw")), P(w), P(news), N, nv, F, A, S())
        g.check()
        g = G()
        dVw, de = g.o((R, F), "dVw"), g.o((nv, N), "de")
        hip.call("ebn_naml_viewatt_bwd_f32", P(g.i(Vw, "Vw")), P(g.i(w32, "w")), P(g.i(dnews, "dnews")), P(dVw), P(de), N, nv, F, S())
        g.check()
        g = G()
        Ut, dq, db = g.io(U32, "U (tanh)"), g.o((A,), "dq"), g.o((A,), "db")
        part = poison(torch.empty(int(hip.lib().ebn_attpool_partials_len(R, A)), device="cuda"))
        hip.call("ebn_attpool_bwd_dpre_f32", P(Ut), P(g.i(q, "q")), P(g.i(de32, "de")), P(dq), P(db), P(part), R, A, 0, S())
        g.check()
        runs.append(bits(U=U, w=w, news=news, dVw=dVw, de=de, dpre=Ut, dq=dq, db=db))
    same_bits(runs[0], runs[1], "view attention")
    what = f"n_views={nv} N={N} F={F} A={A}"
    for k in ("U", "w", "news"):
        cmp(runs[0][k], fwd[k], "va." + k, what)
    for k in ("dVw", "de"):
        cmp(runs[0][k], bwd[k], "va." + k, what)
    for k in ("dq", "dpre", "db"):
        cmp(runs[0][k], rest[k], "dpre." + k, what)


def test_viewatt_refuses_nine_views(hip):
    lib = hip.lib()
    z = np.zeros((9, 4), np.float32)
    g = G()
    rc = lib.ebn_naml_viewatt_fwd_f32(P(g.io(z, "U")), P(g.i(z[0], "b")), P(g.i(z[0], "q")), P(g.i(z, "Vw")), P(g.o((9,), "w")), P(g.o((1, 4), "news")), 1, 9,
                                      4, 4, S())
    assert rc == UNSUPPORTED
    rc = lib.ebn_naml_viewatt_bwd_f32(P(g.i(z, "Vw")), P(g.i(z[:, 0], "w")), P(g.i(z[0], "dnews")), P(g.o((9, 4), "dVw")), P(g.o((9,), "de")), 1, 9, 4, S())
    assert rc == UNSUPPORTED
    g.untouched()
