"""ebn_mmr_rerank_f32, ebn_dpp_rerank_f32, ebn_calibrated_rerank_f32 and ebn_label_target_f32 on guard-banded operands
(tests/guarded_eval.py) at the smallest shapes that reach each edge of the kernels: two users per workgroup with an odd U, the
last table row with D % 32 != 0, D at the limit, k - 1 Cholesky slots on both sides of a chunk of four, C on both sides of the
two ballot halves, a target that is positive in the last element of its allocation.

References and bounds are the existing ones, unchanged: rerank_cases.mmr_reference held to EQUALITY where the float32 and float64
restatements agree bit for bit on the host (asserted, not assumed) and rerank_cases.check_greedy / tolerance elsewhere;
dpp_cases.check_greedy_dpp; calibrate_cases.check_greedy / tolerance and target_reference with the (H + 2) ulp bound of
tests/test_calibrate_gpu.py.  Every case runs twice and at a second pointer offset: the bits must be equal.
tests/test_guarded_eval_cpu.py plants the defects these operands exist to show."""
import numpy as np
import pytest

from tests import calibrate_cases as cc
from tests import dpp_cases as dc
from tests import guarded_eval as ge
from tests import rerank_cases as rr
from tests.hip_testutil import P as PTR, S

pytestmark = pytest.mark.gpu

# (U, P, D, k): 1x1; two users per workgroup, odd U, D off the slab, k = P; P = 32 on the edge; the first one-user size; the
# largest P and k; k > P; D % 32 != 0 just below the limit; D at the limit
POOL_SHAPES = [(1, 1, 4, 1), (3, 31, 36, 31), (3, 32, 36, 5), (2, 33, 36, 10), (1, 64, 64, 64), (2, 5, 8, 64), (2, 64, 8188, 10), (1, 40, 8192, 3)]
DPP_SLOT_SHAPES = [(U, P, 36, k) for (U, P) in ((3, 32), (2, 33)) for k in (1, 2, 5, 6)]  # k - 1 = 0, 1, 4, 5 Cholesky slots
A32 = float(np.float32(cc.ALPHA))


def shape_id(s):
    return "x".join(map(str, s))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def call_pool(hip, entry, ops, lam):
    code = getattr(hip.lib(), entry)(PTR(ops.table), ops.n_rows, ops.D, PTR(ops.rows), PTR(ops.rel), ops.P, ops.k, lam, PTR(ops.sel),
                                     PTR(ops.obj), PTR(ops.flags), ops.U, S())
    assert code == 0, code
    import torch

    torch.cuda.synchronize()


def three_runs(make, run, check, n):
    """the case at offset 0, again at offset 0, and at pointer offset 1 + n % 3: every run checked, the bits equal"""
    out = []
    for off in (0, 0, 1 + n % 3):
        ops = make(off)
        run(ops)
        out.append(check(ops))
    for sel, obj in out[1:]:
        assert np.array_equal(sel, out[0][0]) and np.array_equal(bits(obj), bits(out[0][1])), "two runs / two pointer offsets differ in their bits"


# ------------------------------------------------------------------------------------------------ MMR
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=shape_id)
def test_mmr_on_guarded_operands(hip, shape):
    U, P, D, k = shape
    unit, rows, rel = ge.name_both_ends(*rr.exact_case(U, P, D, seed=U + P))
    for n, lam in enumerate((0.0, 0.5, 1.0)):
        want = rr.mmr_reference(unit, rows, rel, k, lam)
        exact = ge.mmr_float32_equals(unit, rows, rel, k, lam, want)
        assert exact or D > 768, "exact_case is exact up to D = 768"
        tol = rr.tolerance(unit, lam)
        print(f"MMR {shape} lam {lam}: {'exact on the host: held to equality' if exact else f'greedy property, tol = {tol:.3e}'}")
        three_runs(lambda off: ge.PoolOps(unit, rows, rel, k, off=off), lambda ops: call_pool(hip, "ebn_mmr_rerank_f32", ops, lam),
                   lambda ops: ge.check_pool_result(ops, want[2], want=want[:2] if exact else None,
                                                    greedy=None if exact else lambda sel, obj: rr.check_greedy(unit, rows, rel, sel, obj, lam, tol)),
                   n + U + P)


def test_mmr_rounded_rows_by_the_greedy_property(hip):
    """standard-normal unit rows at the two widths whose last slab is partial, two users per workgroup with an odd U"""
    for n, (U, P, D, k) in enumerate(((3, 31, 36, 31), (3, 32, 8188, 5))):
        unit, rows, rel = ge.name_both_ends(*rr.rounded_case(U, P, D, seed=11))
        lam32 = float(np.float32(0.3))
        tol = rr.tolerance(unit, 0.3)
        three_runs(lambda off: ge.PoolOps(unit, rows, rel, k, off=off), lambda ops: call_pool(hip, "ebn_mmr_rerank_f32", ops, 0.3),
                   lambda ops: ge.check_pool_result(ops, (0, 0), greedy=lambda sel, obj: rr.check_greedy(unit, rows, rel, sel, obj, lam32, tol)), n)


# ------------------------------------------------------------------------------------------------ DPP
def dpp_inputs(U, P, D):
    """dpp_cases.dpp_case up to the document-vector width.  Beyond it the pools and relevances of dpp_case over rows that ARE unit
    vectors in dyadic numbers (rerank_cases.exact_unit_table over 32 columns, spread over the first and the last 16 of D, so both
    ends of every row are read): every dot product is exact in fp32 in any order -- asserted on the host, the float32 and float64
    similarity matrices are equal -- and the kernel's Gram stage has no rounding of its own.

    Why not standard-normal rows at every D: dpp_cases.tolerances takes its delta from the error of the float32 NUMPY restatement
    (E32, pairwise sums), with a floor of 2^-20.  The kernel forms a dot product as ONE fp32 fma chain over D, as its contract says;
    at D = 8188 that chain is off by up to 3.1e-6 on a row's dot product with itself (emulated on the host; numpy: 2.3e-7), so d2
    starts 1.6e-6 off.  Measured on an MI355X with dpp_case(2, 64, 8188): every guard intact, flags (0, 0), the picks greedy, but
    |out_obj - float64| = 1.654e-6 against tol = 1.489e-6 at user 0, round 2.  That is the chain's rounding, not a wrong read; the
    bound stays as it is, and the widths beyond 768 are held to it on inputs whose Gram stage is exact."""
    if D <= 768:
        return ge.name_both_ends(*dc.dpp_case(U, P, D, seed=11))
    _, rows, rel = dc.dpp_case(U, P, 32, seed=11)
    small = rr.exact_unit_table(4 * P, 32, np.random.default_rng(D))
    unit = np.zeros((4 * P, D), np.float32)
    unit[:, :16], unit[:, D - 16:] = small[:, :16], small[:, 16:]
    unit, rows, rel = ge.name_both_ends(unit, rows, rel)
    for u in range(U):
        present = dc.present_mask(rows[u], rel[u], len(unit))
        s32, s64 = (dc.similarity(unit, rows[u], present, dt)[0] for dt in (np.float32, np.float64))
        assert np.array_equal(s32.astype(np.float64), s64), "the Gram stage of this case is not exact in fp32"
    return unit, rows, rel


@pytest.mark.parametrize("shape", POOL_SHAPES + DPP_SLOT_SHAPES, ids=shape_id)
def test_dpp_on_guarded_operands(hip, shape):
    U, P, D, k = shape
    unit, rows, rel = dpp_inputs(U, P, D)
    for n, lam in enumerate((0.3, 1.0)):
        def greedy(sel, obj):
            gap, err, e32 = dc.check_greedy_dpp(unit, rows, rel, sel, obj, lam)
            print(f"DPP {shape} lam {lam}: E32 = {e32:.3e}, worst shortfall {gap:.3e}, worst |obj - float64| {err:.3e}")
            present = np.stack([dc.present_mask(rows[u], rel[u], len(unit)) for u in range(U)])
            assert ((sel >= 0).sum(1) == np.minimum(present.sum(1), k)).all()  # full length: spanned entries are clamped, not dropped

        three_runs(lambda off: ge.PoolOps(unit, rows, rel, k, off=off), lambda ops: call_pool(hip, "ebn_dpp_rerank_f32", ops, lam),
                   lambda ops: ge.check_pool_result(ops, (0, 0), greedy=greedy), n + U + k)


# ------------------------------------------------------------------------------------------------ calibrated re-ranking
def call_cal(hip, ops, C, stride, lam):
    code = hip.lib().ebn_calibrated_rerank_f32(PTR(ops.table), ops.n_rows, C, PTR(ops.rows), PTR(ops.rel), ops.P, PTR(ops.target), stride, ops.k,
                                               lam, cc.ALPHA, PTR(ops.sel), PTR(ops.obj), PTR(ops.flags), ops.U, S())
    assert code == 0, code
    import torch

    torch.cuda.synchronize()


@pytest.mark.parametrize("P", [1, 33, 64])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 127, 128])
def test_calibrated_on_guarded_operands(hip, C, P):
    """The last user's target is positive in label C - 1: with a row per user tgt[C - 1] is the last element of the allocation,
    with ONE row for all (target_stride 0) that user's row is the whole allocation.  W sits at pointer offsets 0 to 3."""
    U, k, H, lam = 3, 10, 20, 0.5
    W, rows, rel, hist = cc.exact_case(U, P, C, H, seed=U + P + C)
    W, rows, rel = ge.name_both_ends(W, rows, rel)
    p = cc.target_reference(W, hist)[0].astype(np.float32)
    p[U - 1] = p[0]  # exact_case leaves the last of three users an empty history
    p[U - 1, C - 1] = max(p[U - 1, C - 1], np.float32(0.25))  # used as given, not renormalised
    tol = cc.tolerance(lam, C, k)
    for n, (stride, target) in enumerate(((C, p), (0, p[U - 1]))):
        assert target.reshape(-1)[-1] > 0

        def greedy(sel, obj):
            gap, err = cc.check_greedy(W, rows, rel, target, sel, obj, lam, tol, A32)
            print(f"calibrated C {C} P {P} stride {stride}: tol = {tol:.3e}, worst shortfall {gap:.3e}, worst |obj - float64| {err:.3e}")

        three_runs(lambda off: ge.PoolOps(W, rows, rel, k, off=off, table_off=(off + n + C) % 4, target=target),
                   lambda ops: call_cal(hip, ops, C, stride, lam), lambda ops: ge.check_pool_result(ops, (0, 0), greedy=greedy), n + C + P)


# ------------------------------------------------------------------------------------------------ the history target
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("H", [1, 64, 256])
def test_label_target_on_guarded_operands(hip, H, weighted):
    """W in NaN, the history rows inside a valid row, the weights inside 3e18, the target in canaries; C = 65 takes both label
    halves of a lane, the last history slot names the last table row.  One-hot rows and dyadic weights whose sum is a power of two:
    the (H + 2) ulp bound of tests/test_calibrate_gpu.py."""
    import torch

    from tests.guarded import guard_in, guard_out

    U, C, n_rows = 3, 65, 40
    rng = np.random.default_rng(H + C)
    W = cc.label_table(n_rows, C, rng)
    hist = rng.integers(0, n_rows, (U, H)).astype(np.int32)
    hist[0, 0], hist[U - 1, H - 1] = 0, n_rows - 1
    W[n_rows - 1], W[n_rows - 1, C - 1] = 0.0, 1.0  # the last label of the last row: the last element of the table
    if H > 1:
        hist[1, H // 2] = -1  # the padding: silent
    weights = cc.dyadic_weights(H, rng) if weighted else None
    want, flag0 = cc.target_reference(W, hist, weights)
    assert flag0 == 0
    out = []
    for off in (0, 0, 1 + H % 3):
        W_d, h_W = guard_in(W, fill=ge.NAN, offset=off, guard=ge.table_guard(C))
        hist_d, h_hist = guard_in(hist.reshape(-1), fill=1, offset=off, guard=ge.GUARD)
        w_d, h_w = guard_in(weights, fill=ge.BIG, offset=off, guard=ge.GUARD) if weighted else (None, None)
        t_d, h_t = guard_out((U * C,), offset=off, guard=ge.GUARD)
        f_d, h_f = ge.zeroed_flags(2, "cuda")
        code = hip.lib().ebn_label_target_f32(PTR(W_d), n_rows, C, PTR(hist_d), H, PTR(w_d), PTR(t_d), PTR(f_d), U, S())
        assert code == 0, code
        torch.cuda.synchronize()
        for name, h in (("W", h_W), ("hist_rows", h_hist), ("hist_w", h_w), ("target", h_t), ("flags", h_f)):
            if h is not None:
                h.check(name)
        got = h_t.payload().cpu().numpy().reshape(U, C)
        assert h_f.payload().cpu().tolist() == [0, 0]
        assert (np.abs(got - want) <= (H + 2) * 2.0 ** -23 * want).all(), float(np.abs(got - want).max())  # false for a NaN
        out.append(got)
    assert np.array_equal(bits(out[0]), bits(out[1])) and np.array_equal(bits(out[0]), bits(out[2]))
