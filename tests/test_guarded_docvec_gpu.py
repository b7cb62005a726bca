"""The fused NRMSDocVec launches (csrc/ebn_docvec.hip: dvn_panel_kernel in five instantiations, dvn_dbn_apply_kernel,
dvn_stage_gather_kernel) through the C ABI on guard-banded operands, stage by stage against the float64 references of
tests/docvec_kernel_refs.py.

ebn_dvn_fwd_train_f32 and then ebn_dvn_bwd_f32 are called with an ebn_dvn_args whose every operand goes through tests/guarded.py: float
inputs (X0, W, b, gamma, beta, dNE) sit between NaN guards, every output (R, Xn, NE, dY, dP, ggamma, gbeta) is pre-filled and sits
between canaries, the in-place operands (moving_mean, moving_var, loss, range_flag) are outputs with a payload, and `stat` is a guarded
output with a ZERO payload (its contract is zero: it is not poisoned).  After the pair of calls every handle is checked, every output is
compared element-wise -- |got - want| <= C_SUM * mag + 1e-30, a NaN fails -- with the stage of the launch that wrote it computed in
float64 from the launch's own earlier outputs (docvec_kernel_refs.check_step: the table of stages and magnitudes is there), range_flag
is 0, and the whole chain is held to oracle.nrms_numpy at the bounds of tests/test_docvec_model.py.  The ReLU gate of every backward
stage is the kernel's own R > 0: no tie is excluded.  The cases (docvec_kernel_refs.CASES) are the smallest shapes at which each loop of
the kernels takes no, one and a second trip and each clamp is touched from both sides; tests/test_docvec_kernel_refs_cpu.py shows
planted defects that only they catch.

Bit claims stay bit claims: two runs from identical inputs give identical bits in every output and in `stat`; the zero patterns of Xn
and dY are the dropout mask (indexed by global row); dP[n_layers] is dNE gated by NE > 0.

The `stat` contract (include/ebnerd_hip.h): zero before the first call; the BACKWARD accumulators are re-zeroed by the first forward
launch, the FORWARD ones by the last backward launch.  So after a complete forward + backward the forward block is all-zero bits and
the backward block still holds the step's column sums -- the last launch reads them, no launch behind it could clear them -- until the
next forward call clears it: asserted as the forward block zero after the pair, the backward block zero after the forward call of a
step that started on a used scratch, and that step equal, bit for bit, to the same step on a freshly zeroed scratch.  The mean | istd
block of an empty call site is untouched (it keeps what an earlier step with rows in that site left there).

A refused call writes nothing: each refusal returns its code and leaves every handle untouched, `stat` included -- both calls validate
everything in front of their first launch, and a float4 / 64-bit operand moved by 4 bytes is EBN_ERR_ALIGN.

ebn_docvec_stage_gather_f32: ids between harmful guards (a row outside the table raises the flag), row counts on both sides of one
block's share (512 float4 items), an id outside the table (flag, zero row), n1 = 0 with a NULL second segment, and the label-only call
n0 = n1 = 0 with both segments NULL (labels copied, step advanced, nothing else written).

NOT covered: the int-overflow limits (MAX_TILES = 4096 row tiles, 2^29 elements) need far more than a few seconds; the range-flag path
keeps its model-level test; ebn_dvn_finale_f32 its float64 kernel-level test in tests/test_hip_kernels.py.  LIMIT (tests/guarded.py):
an over-read whose value a select discards is not seen.

The constant is C_SUM = 2e-6 for EVERY output: all are fp32 sums of products plus a correctly rounded division and square root.

MI355X, 2026-10-20, on top of commit 8039a3c; max err / mag over all cases of this file (no kernel defect found: all cases pass):
  output           max err/mag  c
  dvn.R            1.621e-07   C_SUM = 2e-6
  dvn.mean         4.825e-07   C_SUM = 2e-6
  dvn.istd         5.663e-07   C_SUM = 2e-6
  dvn.Xn           1.642e-07   C_SUM = 2e-6
  dvn.NE           1.356e-07   C_SUM = 2e-6
  dvn.moving_mean  1.177e-07   C_SUM = 2e-6
  dvn.moving_var   1.609e-07   C_SUM = 2e-6
  dvn.dY           1.711e-07   C_SUM = 2e-6
  dvn.ggamma       8.027e-08   C_SUM = 2e-6
  dvn.gbeta        1.289e-07   C_SUM = 2e-6
  dvn.dP           1.969e-06   C_SUM = 2e-6   (`reload`, layer 0, row 32 only; every other case and row: at most 1.5e-07)
  dvn.loss         3.870e-08   C_SUM = 2e-6
  dvn.l2_part      8.496e-08   C_SUM = 2e-6
dvn.dP at `reload`: row 32 is the ONE row of the candidate site.  BatchNormalization over a single row annihilates its gradient, so
dP[1][32] is rounding noise and dY[0][32] = dP[1][32] . W[1]^T is of the order 1e-9: a few thousand units of the 2^-40 grid of the
backward accumulators (measured: -2992, -137, ... units).  dP[0][32] = k (dy - s1) with s1 the fixed-point column sum of that one row
is then the quantisation residue itself, |dy - s1| <= 2^-41, times k = gamma istd = 31.6: 1.4e-11 where float64 gives 0.  That is
exactly the derived absolute term of the reference (tiles 2^-41 per column sum), which is all the magnitude holds there -- err / mag
approaches C_SUM over the 516 columns by construction and cannot pass it (the slack 2 C_SUM |dy| exceeds the one float32 rounding of
k s1, 6e-8 |k dy|).  An absolute error of 1.4e-11 on a gradient that is mathematically zero, bounded by derivation: not a defect.
The whole module (60 tests) runs in 3.2 s; no case takes more than half a second.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import docvec_kernel_refs as dk
from tests.hip_testutil import P, S, assert_close, make_state, read_state
from tests.test_guarded_training_tail_gpu import FLAT, G

pytestmark = pytest.mark.gpu
OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3
MEASURED = {}


def cmp(key, got, ref, what=""):
    """print err / mag, then assert |got - want| <= C_SUM * mag + TINY element-wise"""
    r = dk.ratio(np.asarray(got, np.float64).reshape(np.shape(ref[0])), ref[0], ref[1])
    MEASURED[key] = max(MEASURED.get(key, 0.0), r)
    print(f"ERRMAG {key} {r:.3e} {what}")
    dk.check_close(got, ref, dk.C_SUM, f"{key} {what}")


def state():
    return make_state(seed=dk.SEED, step=dk.STEP)


def out_names(L):
    per = ("R", "Xn", "dY", "dP", "ggamma", "gbeta", "moving_mean", "moving_var")
    return [f"{k}{l}" for l in range(L) for k in per] + ["NE", f"dP{L}", "loss", "range_flag", "stat"]


def operands(hip, shape, p, l2, inp, stat0=None, off=()):
    """-> (G, ebn_dvn_args) over guarded operands.  `off`: names moved by 4 bytes."""
    n0, n1, din, units, e_out = shape
    L, n = len(units), n0 + n1
    g, a = G(), hip.DvnArgs()
    o = lambda name: 1 if name in off else 0
    a.n_layers, a.din, a.e_out, a.n0, a.n1, a.drop_p, a.l2 = L, din, e_out, n0, n1, p, l2
    for l, u in enumerate(units):
        a.units[l] = u
    a.X0 = g.i(inp["X0"], "X0", offset=o("X0")).data_ptr()
    for l in range(L + 1):
        a.W[l], a.b[l] = g.i(inp["W"][l], f"W{l}", offset=o(f"W{l}")).data_ptr(), g.i(inp["b"][l], f"b{l}").data_ptr()
    for l, u in enumerate(units):
        a.gamma[l], a.beta[l] = g.i(inp["gamma"][l], f"gamma{l}").data_ptr(), g.i(inp["beta"][l], f"beta{l}").data_ptr()
        a.moving_mean[l], a.moving_var[l] = g.io(inp["mm"][l], f"moving_mean{l}").data_ptr(), g.io(inp["mv"][l], f"moving_var{l}").data_ptr()
        a.R[l], a.Xn[l] = g.o((n, u), f"R{l}", offset=o(f"R{l}")).data_ptr(), g.o((n, u), f"Xn{l}").data_ptr()
        a.dY[l], a.dP[l] = g.o((n, u), f"dY{l}").data_ptr(), g.o((n, u), f"dP{l}").data_ptr()
        a.ggamma[l], a.gbeta[l] = g.o((u,), f"ggamma{l}").data_ptr(), g.o((u,), f"gbeta{l}").data_ptr()
    a.NE, a.dNE = g.o((n, e_out), "NE").data_ptr(), g.i(inp["dNE"], "dNE", offset=o("dNE")).data_ptr()
    a.dP[L] = g.o((n, e_out), f"dP{L}").data_ptr()
    a.loss, a.range_flag = g.io(np.array([dk.LOSS0], np.float32), "loss").data_ptr(), g.flag("range_flag").data_ptr()
    stat = np.zeros(dk.stat_floats(units), np.float32) if stat0 is None else np.asarray(stat0, np.float32)
    a.stat = g.io(stat, "stat", offset=o("stat"), guard=FLAT).data_ptr()
    return g, a


def outputs(g, L):
    """name -> the payload as the calls left it (float32; range_flag int32)"""
    torch.cuda.synchronize()
    return {k: g.h[k].payload().cpu().numpy() for k in out_names(L)}


def run_pair(hip, shape, p, l2, inp, stat0=None, between=None):
    g, a = operands(hip, shape, p, l2, inp, stat0)
    assert int(hip.lib().ebn_dvn_supported(ctypes.byref(a))) == 1
    assert int(hip.lib().ebn_dvn_stat_floats(ctypes.byref(a))) == dk.stat_floats(shape[3])
    st = state()
    assert hip.lib().ebn_dvn_fwd_train_f32(ctypes.byref(a), P(st), S()) == OK
    if between is not None:
        torch.cuda.synchronize()
        between(g)
    assert hip.lib().ebn_dvn_bwd_f32(ctypes.byref(a), P(st), S()) == OK
    g.check()
    return g, outputs(g, len(shape[3]))


def same_bits(a, b, names, what):
    for k in names:
        assert np.array_equal(np.asarray(a[k]).view(np.int32), np.asarray(b[k]).view(np.int32)), f"{what}: {k} differs"


# ---------------------------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("p,l2", dk.P_L2)
@pytest.mark.parametrize("name", list(dk.CASES))
def test_every_stage_of_the_pair_against_float64(hip, name, p, l2):
    shape = dk.CASES[name]
    n0, n1, din, units, e_out = shape
    inp = dk.case_inputs(*shape)
    what = f"{name} p {p} l2 {l2}"
    _, out = run_pair(hip, shape, p, l2, inp)
    dk.check_step(out, inp, n0, n1, units, p, l2, cmp=cmp, what=what)
    dk.chain_check(out, inp, n0, n1, units, p, l2, assert_close, what=what)
    _, again = run_pair(hip, shape, p, l2, inp)  # "bitwise reproducible run to run"
    same_bits(out, again, out_names(len(units)), f"{what}: a second run from identical inputs")


# ---------------------------------------------------------------------------------------------------------------- the stat contract
@pytest.mark.parametrize("name", list(dk.CASES))
def test_a_step_on_a_used_scratch_is_the_step_on_a_zero_scratch(hip, name):
    shape = dk.CASES[name]
    n0, n1, din, units, e_out = shape
    L, p, l2 = len(units), 0.2, 1e-4
    # the step in front: other data, rows in BOTH call sites (the scratch layout depends on the widths only)
    prev_shape = shape if n0 and n1 else (3, 2, din, units, e_out)
    _, prev = run_pair(hip, prev_shape, p, l2, dk.case_inputs(*prev_shape, seed=5))
    used = prev["stat"]
    views = [dk.stat_view(used, units, l) for l in range(L)]
    assert not any(v["fwd"].any() for v in views), "the forward accumulators are not all-zero bits after a complete step"
    assert any(v["bwd"].any() for v in views) and all(v["istd"].all() for v in views)  # both sites' blocks were written

    def after_forward(g):  # the first forward launch re-zeroes the backward accumulators of every layer
        now = g.h["stat"].payload().cpu().numpy()
        assert not any(dk.stat_view(now, units, l)["bwd"].any() for l in range(L)), "backward accumulators not re-zeroed by the forward call"

    inp = dk.case_inputs(*shape)
    _, a = run_pair(hip, shape, p, l2, inp, stat0=used, between=after_forward)
    _, b = run_pair(hip, shape, p, l2, inp)
    dk.check_step(a, inp, n0, n1, units, p, l2, stat0=used, cmp=cmp, what=f"{name} on a used scratch")  # (the empty site's block == `used`'s)
    same_bits(a, b, [k for k in out_names(L) if k != "stat"], f"{name}: used scratch against zero scratch")
    sa, sb = a["stat"].copy(), b["stat"].copy()
    for l in range(L):
        for s, rows in enumerate((n0, n1)):
            if rows == 0:  # untouched: `used`'s in a, zero in b
                va, vb, vu = dk.stat_view(sa, units, l), dk.stat_view(sb, units, l), views[l]
                for k in ("mean", "istd"):
                    assert np.array_equal(va[k][s].view(np.int32), vu[k][s].view(np.int32)) and not vb[k][s].view(np.int32).any()
                    va[k][s] = 0
    assert np.array_equal(sa.view(np.int32), sb.view(np.int32)), f"{name}: stat after a step on a used scratch differs from the zero-scratch one"


# ---------------------------------------------------------------------------------------------------------------- refusals
REFUSE_SHAPE = (5, 3, 8, [8, 12], 8)
REFUSALS = {  # name -> (shape, names moved by 4 bytes, change to the argument block, code, the calls that must refuse)
    "hidden_width_1028": ((5, 3, 8, [1028, 12], 8), (), None, UNSUPPORTED, ("fwd", "bwd")),
    "width_30": ((5, 3, 8, [30, 12], 8), (), None, UNSUPPORTED, ("fwd", "bwd")),
    "no_rows": (REFUSE_SHAPE, (), lambda a: (setattr(a, "n0", 0), setattr(a, "n1", 0)), BAD_ARG, ("fwd", "bwd")),
    "five_layers": (REFUSE_SHAPE, (), lambda a: setattr(a, "n_layers", 5), UNSUPPORTED, ("fwd", "bwd")),
    "drop_p_1": (REFUSE_SHAPE, (), lambda a: setattr(a, "drop_p", 1.0), BAD_ARG, ("fwd", "bwd")),
    "null_W_last": (REFUSE_SHAPE, (), lambda a: a.W.__setitem__(2, None), BAD_ARG, ("fwd", "bwd")),
    "null_gamma_0": (REFUSE_SHAPE, (), lambda a: a.gamma.__setitem__(0, None), BAD_ARG, ("fwd", "bwd")),
    "misaligned_X0": (REFUSE_SHAPE, ("X0",), None, ALIGN, ("fwd",)),
    "misaligned_W1": (REFUSE_SHAPE, ("W1",), None, ALIGN, ("fwd", "bwd")),
    "misaligned_R0": (REFUSE_SHAPE, ("R0",), None, ALIGN, ("fwd", "bwd")),
    "misaligned_dNE": (REFUSE_SHAPE, ("dNE",), None, ALIGN, ("bwd",)),
    "misaligned_stat": (REFUSE_SHAPE, ("stat",), None, ALIGN, ("fwd", "bwd")),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_refused_call_returns_its_code_and_writes_nothing(hip, name):
    shape, off, change, code, calls = REFUSALS[name]
    inp = dk.case_inputs(*shape)
    for call in calls:
        g, a = operands(hip, shape, 0.2, 1e-4, inp, off=off)
        for k in off:
            assert g.h[k].view.data_ptr() % 16 == 4
        if change is not None:
            change(a)
        if code != ALIGN and name not in ("null_W_last", "null_gamma_0"):
            assert int(hip.lib().ebn_dvn_supported(ctypes.byref(a))) == 0 and int(hip.lib().ebn_dvn_stat_floats(ctypes.byref(a))) == 0
        fn = hip.lib().ebn_dvn_fwd_train_f32 if call == "fwd" else hip.lib().ebn_dvn_bwd_f32
        assert fn(ctypes.byref(a), P(state()), S()) == code, (name, call)
        g.untouched()


# ---------------------------------------------------------------------------------------------------------------- the step prologue
N_TABLE = 11


def _gather(hip, n0, n1, din, n_lab, oob=False, null_idx1=False):
    rng = np.random.default_rng(100 * n0 + n1 + din)
    matrix = rng.standard_normal((N_TABLE, din)).astype(np.float32)
    ids = rng.integers(0, N_TABLE, n0 + n1).astype(np.int32)
    if n0 + n1:
        ids[0], ids[-1] = 0, N_TABLE - 1
    if oob:
        ids[(n0 + n1) // 2], ids[(n0 + n1) // 3] = N_TABLE, -1
    lab = rng.random(max(n_lab, 1)).astype(np.float32)[:n_lab]
    g = G()
    # an id guard is a row outside the table: an over-read id raises the flag of the clean run
    i0 = g.i(ids[:n0], "idx0", fill=N_TABLE + 3, guard=FLAT) if n0 else None
    i1 = g.i(ids[n0:], "idx1", fill=N_TABLE + 3, guard=FLAT) if n1 and not null_idx1 else None
    ls, ld = (g.i(lab, "labels_src"), g.o((n_lab,), "labels_dst")) if n_lab else (None, None)
    X0 = g.o((max(n0 + n1, 1), din), "X0")
    st = make_state(seed=9, step=4, lr=1e-3)
    rc = hip.lib().ebn_docvec_stage_gather_f32(P(i0) if n0 else None, n0, P(i1) if i1 is not None else None, n1, P(ls) if n_lab else None,
                                               P(ld) if n_lab else None, n_lab, P(g.i(matrix, "matrix")), N_TABLE, din, P(X0), P(g.flag()), P(st),
                                               0.9, 0.999, S())
    assert rc == OK
    torch.cuda.synchronize()
    got = read_state(st)
    assert got.step == 5 and got.drop_key[8] == dk.on.dropout_key(9, 5, 8)
    if n_lab:
        assert np.array_equal(g.bits("labels_dst"), lab.view(np.int32))
    return g, ids, matrix


@pytest.mark.parametrize("oob", [False, True])
@pytest.mark.parametrize("n0,n1,din", [(300, 211, 4), (300, 212, 4), (300, 213, 4), (0, 513, 4), (40, 24, 32), (40, 25, 32), (1, 0, 4)])
def test_stage_gather_both_sides_of_a_block(hip, n0, n1, din, oob):
    g, ids, matrix = _gather(hip, n0, n1, din, n_lab=n1, oob=oob)
    g.check()
    ok = (ids >= 0) & (ids < N_TABLE)
    want = np.where(ok[:, None], matrix[np.clip(ids, 0, N_TABLE - 1)], np.float32(0))
    assert np.array_equal(g.bits("X0"), want.view(np.int32)) and int(g.get("flag")[0]) == int(oob) and ok.all() != oob


def test_stage_gather_with_an_empty_null_second_segment(hip):
    g, ids, matrix = _gather(hip, 513, 0, 4, n_lab=7, null_idx1=True)
    g.check()
    assert np.array_equal(g.bits("X0"), matrix[ids].view(np.int32)) and int(g.get("flag")[0]) == 0


@pytest.mark.parametrize("n_lab", [5, 300])
def test_stage_gather_label_only_call_copies_the_labels_advances_the_step_and_writes_nothing_else(hip, n_lab):
    g, _, _ = _gather(hip, 0, 0, 8, n_lab=n_lab)  # both segments NULL; _gather checked the labels and the step state
    g.check(but=("X0",))  # X0 keeps its pre-fill: no row was gathered
    assert int(g.get("flag")[0]) == 0


def test_zz_report_measured_constants(hip):
    """last in the module: the err / mag table of this session (`pytest -s`); the constant in force is C_SUM for every row"""
    for k in sorted(MEASURED):
        print(f"TABLE {k:18s} {MEASURED[k]:.3e}   C_SUM = 2e-6")
    assert MEASURED and all(v <= dk.C_SUM for v in MEASURED.values())
