"""The hand-tiled kernels on padded, guard-banded operands (tests/guarded.py): every input sits behind and in front of NaN (or
a harmful integer), every output inside canaries with a NaN pre-fill, every workspace is poisoned.  Results are compared with
the float64 reference and the tolerance of the kernel's existing test; then every buffer's guards are checked, and flags must
stay 0.  Each layout runs twice: "pad4" (+4 floats per row, distinct pads per operand where the ABI has several leading
dimensions, 16-byte aligned pointers: the vector / MFMA paths) and "pad1" (+1 float, or a pointer moved by 4 bytes where the
ABI has no leading dimension: the scalar path, or the entry point's EBN_ERR_ALIGN / EBN_ERR_UNSUPPORTED with nothing written).
For GEMM and attention the pad4 payload must also be BIT-IDENTICAL to a tight-layout call (the summation order is a function
of the shape, not of the strides).

GEMM branch -> shape (M, N, K), asserted through ebn_gemm_plan as (bm, bn, splits); every shape has a ragged last tile in M and
N and a partial last K slab:
    32 x 32 small, one 128-deep slab        (37, 20, 12)        (32, 32, 1)
    32 x 32 small, two slabs                (130, 70, 130)      (32, 32, 1)    no extent is a multiple of 4: scalar loads
    32 x 32 small, two slabs, float4 loads  (132, 68, 132)      (32, 32, 1)    gemm_small_vec_kernel in pad4, all layouts
    64 x 64 tiles                           (96, 100, 4100)     (64, 64, 1)    no workspace
    64 x 64 split-K + splitk_reduce_kernel  (96, 100, 4100)     (64, 64, 52)   with workspace
    128 x 64 tiles                          (24636, 92, 20)     (128, 64, 1)
    128 x 128 tiles                         (19132, 348, 20)    (128, 128, 1)
    256 x 64 tiles                          (22972, 284, 20)    (256, 64, 1)
    direct 16 x 16 (tA = 0, beta = 0)       (4099, 68, 72)      (32, 32, 1)    see below
    direct TN K-chunked (tA = 1, tB = 0)    (72, 72, 12300)     (64, 64, 60)   with workspace: 49 chunks of 256 + a 12-deep tail
                                            (52, 132, 8204)     (64, 64, 57)   with workspace: 33 chunks, all column groups narrow
    scalar-load kernels                     the pad1 variant of every shape above
The plan does not name the two LDS-free kernels of ebn_gemm_direct.hip.  The TN form is pinned through ebn_gemm_f32_partials,
which reports the number of slices it wrote: the TN kernel's chunk count (49, 33) differs from the planner's split count (60,
57), so the assertion fails when the shape stops taking that kernel.  ((72, 72, 4100) does NOT take it: two tiles give 64 chunks
of 128 rows, below the kernel's 256-row minimum.)  For the 16 x 16 form nothing host-visible tells the kernels apart:
ebn_gemm_direct_wanted takes (4099, 68, 72) today (M >= 4096, 48 <= N <= 512, 32 <= K <= 2048, K % 4 == 0; five column blocks
in one group), and a change to that predicate would silently move the case onto the 32 x 32 tiles -- still a checked case, but
no longer this branch.
No entry of test_hip_kernels.GEMM_SHAPES plans to the 128 x 64, 128 x 128 or 256 x 64 tile (the planner's time model prefers
the 64 x 64 tile for all of them), so those three shapes are the smallest outputs (M, N = 64 i - 4, K = 20: one full 16-deep
slab + a 4-wide tail) for which ebn_gemm_plan returns the tile.  They are the large cases of this module: 9 to 27 MB of output,
and 25 MB per guard for the transposed A (guards are 256 * ld elements, tests/guarded.py).

LIMIT: an over-read whose value is discarded by a select never reaches an output and is not detected (tests/guarded.py).
Zero-scratch contracts are not poisoned: none of the entry points below has one (ebn_dvn_fwd_train_f32's `stat`, the documented
case, belongs to the DocVec kernels: tests/test_guarded_docvec_gpu.py holds them, with `stat` as a guarded zero payload)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import nrms_numpy as on
from tests import lstur_oracle as lo
from tests import recommend_cases as rc
from tests.guarded import PREFILL_F32, assert_values, guard_in, guard_out, poison
from tests.hip_testutil import P, S, dev, gemm, host, make_state
from tests.test_hip_kernels import _qkv_case
from tests.test_lstur_gpu import _gru_ref
from tests.test_npa_gpu import SEED as CONV_SEED
from tests.test_npa_gpu import STEP as CONV_STEP
from tests.test_npa_gpu import _mult, _unfold

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3
VARIANTS = ["pad4", "pad1"]
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
ALPHA_BETA = [(1.0, 0.0), (0.5, 1.0), (2.0, -0.5)]
cf = ctypes.c_float


def _pad(variant, i=0):
    """the i-th distinct pad of a variant: pad4 -> 4, 8, 12, ... (multiples of 4); pad1 -> 1, 2, 3, 5, 6, 7, ... (never one)"""
    return 4 * (i + 1) if variant == "pad4" else (1, 2, 3, 5, 6, 7)[i]


def _dev(a):
    return dev(np.array(a))  # a writable copy: the shared reference arrays are read-only


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_all(**handles):
    torch.cuda.synchronize()
    for name, h in handles.items():
        h.check(name)


def _untouched(**handles):
    torch.cuda.synchronize()
    for name, h in handles.items():
        h.check_untouched(name)


def _plan(hip, M, N, K, ws_floats):
    bm, bn, sp = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert hip.lib().ebn_gemm_plan(M, N, K, ws_floats, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(sp)) == OK
    return bm.value, bn.value, sp.value


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ============================================================================================================ GEMM family
@functools.lru_cache(maxsize=None)
def _gemm_data(M, N, K):
    """op(A) [M, K], op(B) [K, N], C0 [M, N] in fp32 and the float64 product: computed once per shape, shared, read-only"""
    rng = np.random.default_rng(M * 131 + N * 17 + K)
    opA, opB, C0 = (rng.standard_normal(s).astype(np.float32) for s in ((M, K), (K, N), (M, N)))
    return _frozen(opA, opB, C0, opA.astype(np.float64) @ opB.astype(np.float64))


GEMM_BRANCHES = [("small32-1slab", (37, 20, 12), False, (32, 32, 1)), ("small32-2slabs", (130, 70, 130), False, (32, 32, 1)),
                 ("small32-2slabs-vec", (132, 68, 132), False, (32, 32, 1)),
                 ("tile64", (96, 100, 4100), False, (64, 64, 1)), ("splitk64", (96, 100, 4100), True, (64, 64, 52)),
                 ("tile128x64", (24636, 92, 20), False, (128, 64, 1)), ("tile128x128", (19132, 348, 20), False, (128, 128, 1)),
                 ("tile256x64", (22972, 284, 20), False, (256, 64, 1))]


def _run_gemm_cases(hip, shape, use_ws, want_plan, tA, tB, variant, alpha_beta, pad_a=None, pad_b=None):
    M, N, K = shape
    n_ws = int(hip.lib().ebn_gemm_workspace_floats(M, N, K)) if use_ws else 0
    assert (n_ws > 0) == use_ws
    assert _plan(hip, M, N, K, n_ws) == want_plan
    opA, opB, C0, ref = _gemm_data(M, N, K)
    A, B = (opA.T if tA else opA), (opB.T if tB else opB)
    pa, pb, pc = (_pad(variant) if pad_a is None else pad_a), (_pad(variant) if pad_b is None else pad_b), _pad(variant)
    lda, ldb, ldc = A.shape[1] + pa, B.shape[1] + pb, N + pc
    Ad, ha = guard_in(A, ld=lda)
    Bd, hb = guard_in(B, ld=ldb)
    tight = variant == "pad4" and pad_a is None and pad_b is None
    At, Bt = (_dev(A), _dev(B)) if tight else (None, None)
    for alpha, beta in alpha_beta:
        what = f"gemm {M}x{N}x{K} tA={tA} tB={tB} a={alpha} b={beta} {variant}"
        Cd, hc = guard_out((M, N), ld=ldc)
        if beta != 0:
            hc.fill_payload(C0)  # beta == 0: the payload stays NaN -- C must not be read
        ws = poison(torch.empty(n_ws, device="cuda")) if use_ws else None
        if use_ws and beta != 0:  # ebn_gemm_f32_site: the same launcher behind a third entry point (`site` is ignored)
            hip.call("ebn_gemm_f32_site", tA, tB, M, N, K, alpha, P(Ad), lda, P(Bd), ldb, beta, P(Cd), ldc, P(ws), n_ws, 3, S())
        else:                     # ebn_gemm_f32 without, ebn_gemm_f32_ws with a workspace
            gemm(tA, tB, M, N, K, alpha, Ad, lda, Bd, ldb, beta, Cd, ldc, ws)
        got = hc.payload()
        assert_values(host(got), alpha * ref + beta * C0, rtol=2e-6, atol=1e-5 + 3e-7 * K, what=what)
        _check_all(C=hc)
        if tight:
            Ct = _dev(C0) if beta != 0 else _nan(M, N)
            gemm(tA, tB, M, N, K, alpha, At, A.shape[1], Bt, B.shape[1], beta, Ct, N, poison(torch.empty(n_ws, device="cuda")) if use_ws else None)
            assert _bits_equal(got, Ct), what + ": padded and tight layouts differ in bits"
    _check_all(A=ha, B=hb)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("tA,tB", LAYOUTS)
@pytest.mark.parametrize("name,shape,use_ws,want_plan", GEMM_BRANCHES, ids=[b[0] for b in GEMM_BRANCHES])
def test_gemm_every_dispatch_branch(hip, name, shape, use_ws, want_plan, tA, tB, variant):
    """ebn_gemm_f32 / ebn_gemm_f32_ws: one shape per branch of gemm_dispatch (module docstring), all four layouts, the three
    (alpha, beta) pairs; against float64 at test_gemm_all_layouts' tolerance.  pad4 is bit-identical to the tight layout."""
    _run_gemm_cases(hip, shape, use_ws, want_plan, tA, tB, variant, ALPHA_BETA)


@pytest.mark.parametrize("variant", VARIANTS + ["A-pad4-B-pad1"])
@pytest.mark.parametrize("tB", [0, 1])
def test_gemm_direct_16x16_kernels(hip, tB, variant):
    """(4099, 68, 72), A not transposed, beta = 0: the LDS-free 16 x 16-block kernel in both B layouts (float4 fragments of a
    [N][K] B, dword rows of a [K][N] B -- the latter also with an unaligned B: variant A-pad4-B-pad1).  The beta != 0 pairs of
    the same shape run on the 32 x 32 tiles."""
    if variant == "A-pad4-B-pad1":
        _run_gemm_cases(hip, (4099, 68, 72), False, (32, 32, 1), 0, tB, "pad4", [(1.0, 0.0), (2.0, 0.0)], pad_a=4, pad_b=1)
    else:
        _run_gemm_cases(hip, (4099, 68, 72), False, (32, 32, 1), 0, tB, variant, [(1.0, 0.0), (2.0, 0.0)] + ALPHA_BETA[1:])


TN_DIRECT = [((72, 72, 12300), 49, (64, 64, 60)), ((52, 132, 8204), 33, (64, 64, 57))]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape,chunks,want_plan", TN_DIRECT, ids=["72x72x12300", "52x132x8204"])
def test_gemm_direct_tn_kernel(hip, shape, chunks, want_plan, variant):
    """The K-chunked 16 x 16-block kernel (transposed A, workspace given): ebn_gemm_f32_partials must report the TN kernel's
    chunk count, which is not the planner's split count -- the selection is asserted, not assumed -- and write exactly that many
    slices; then the three (alpha, beta) pairs through ebn_gemm_f32_ws / _site with the combining pass.  The kernel loads by
    dwords: pad1 takes it too."""
    M, N, K = shape
    assert chunks != want_plan[2]
    opA, opB, _, ref = _gemm_data(M, N, K)
    n_ws = int(hip.lib().ebn_gemm_partials_workspace_floats(M, N, K))
    assert n_ws == max(chunks, want_plan[2]) * M * N
    lda, ldb = M + _pad(variant, 0), N + _pad(variant, 1)
    (Ad, ha), (Bd, hb), (wsd, hw) = guard_in(opA.T, ld=lda), guard_in(opB, ld=ldb), guard_out((n_ws,))
    n = ctypes.c_int32(-1)
    hip.call("ebn_gemm_f32_partials", 1, 0, M, N, K, cf(0.5), P(Ad), lda, P(Bd), ldb, P(wsd), n_ws, ctypes.byref(n), S())
    assert n.value == chunks, f"{n.value} slices: not the direct TN kernel's {chunks} chunks"
    got = hw.payload()
    assert_values(host(got[: chunks * M * N]).reshape(chunks, M, N).sum(0), 0.5 * ref, rtol=2e-6, atol=1e-5 + 3e-7 * K, what="sum of the TN chunks")
    assert bool((got[chunks * M * N:].view(torch.int32) == PREFILL_F32).all()), "slices past the reported count were written"
    hw.prefilled = False  # (only the reported slices are outputs)
    _check_all(A=ha, B=hb, workspace=hw)
    _run_gemm_cases(hip, shape, True, want_plan, 1, 0, variant, ALPHA_BETA)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M,N,K", [(5, 7, 3), (130, 70, 33)])
def test_split_precision_gemm_guarded(hip, M, N, K, variant):
    """ebn_gemm_f32_prec(precision = 1): its workspace (bf16 planes, zero padding written by the kernels themselves, split-K
    partials) is poisoned.  (1, 1, 1), the smallest shape of the existing test, has no second row for a stride to act on: the
    next two of GEMM_SHAPES with more than one row stand in."""
    opA, opB, C0, ref = _gemm_data(M, N, K)
    nbytes = int(hip.lib().ebn_gemm_prec_workspace_bytes(M, N, K, 1))
    for tA, tB in LAYOUTS:
        A, B = (opA.T if tA else opA), (opB.T if tB else opB)
        lda, ldb, ldc = A.shape[1] + _pad(variant, 0), B.shape[1] + _pad(variant, 1), N + _pad(variant, 2)
        (Ad, ha), (Bd, hb) = guard_in(A, ld=lda), guard_in(B, ld=ldb)
        for alpha, beta in ALPHA_BETA:
            Cd, hc = guard_out((M, N), ld=ldc)
            if beta != 0:
                hc.fill_payload(C0)
            ws = poison(torch.empty(nbytes // 4 + 64, device="cuda"))
            hip.call("ebn_gemm_f32_prec", tA, tB, M, N, K, cf(alpha), P(Ad), lda, P(Bd), ldb, cf(beta), P(Cd), ldc, P(ws), nbytes, 1, S())
            assert_values(host(hc.payload()), alpha * ref + beta * C0, rtol=2e-6, atol=1e-5 + 3e-7 * K,
                         what=f"split gemm {M}x{N}x{K} tA={tA} tB={tB} a={alpha} b={beta} {variant}")
            _check_all(C=hc)
        _check_all(A=ha, B=hb)


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_partials_guarded(hip, variant):
    """ebn_gemm_f32_partials at (0, 0, 64, 64, 16): the slices land in the (guarded, NaN pre-filled) workspace; their sum is the
    product (float64, GEMM tolerance); pad4 gives the bits of the tight call."""
    M, N, K, alpha = 64, 64, 16, 0.5
    opA, opB, _, ref = _gemm_data(M, N, K)
    n_ws = int(hip.lib().ebn_gemm_partials_workspace_floats(M, N, K))
    assert n_ws == M * N
    lda, ldb = K + _pad(variant, 0), N + _pad(variant, 1)
    (Ad, ha), (Bd, hb), (wsd, hw) = guard_in(opA, ld=lda), guard_in(opB, ld=ldb), guard_out((n_ws,))
    n = ctypes.c_int32(-1)
    hip.call("ebn_gemm_f32_partials", 0, 0, M, N, K, cf(alpha), P(Ad), lda, P(Bd), ldb, P(wsd), n_ws, ctypes.byref(n), S())
    assert n.value == 1
    got = hw.payload().reshape(n.value, M, N)
    assert_values(host(got).sum(0), alpha * ref, rtol=2e-6, atol=1e-5 + 3e-7 * K, what="sum of the partial slices")
    _check_all(A=ha, B=hb, workspace=hw)
    if variant == "pad4":
        wt, nt = _nan(n_ws), ctypes.c_int32(-1)
        hip.call("ebn_gemm_f32_partials", 0, 0, M, N, K, cf(alpha), P(_dev(opA)), K, P(_dev(opB)), N, P(wt), n_ws, ctypes.byref(nt), S())
        assert nt.value == n.value and _bits_equal(got.reshape(-1), wt)


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_rowmap_guarded(hip, variant):
    """ebn_gemm_f32_rowmap at (256, 132, 40), V = 1000: ids guarded with V (a read of the guard raises oob_flag), table / B
    padded.  Unaligned leading dimensions are EBN_ERR_UNSUPPORTED with nothing written."""
    M, N, K, V = 256, 132, 40, 1000
    rng = np.random.default_rng(M + N)
    table, B = rng.standard_normal((V, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    ids = rng.integers(0, V, M).astype(np.int32)
    ids[0], ids[1], ids[-1] = 0, V - 1, ids[2]
    ldt, ldb, ldc = K + _pad(variant, 0), N + _pad(variant, 1), N + _pad(variant, 2)
    (td, ht), (Bd, hb), (idd, hi) = guard_in(table, ld=ldt), guard_in(B, ld=ldb), guard_in(ids, fill=V)
    (Cd, hc), (fd, hf) = guard_out((M, N), ld=ldc), guard_out((1,), dtype=torch.int32)
    hf.fill_payload([0])
    code = hip.lib().ebn_gemm_f32_rowmap(P(idd), V, M, N, K, P(td), ldt, P(Bd), ldb, P(Cd), ldc, P(fd), S())
    if variant == "pad1":
        assert code == UNSUPPORTED
        return _untouched(table=ht, B=hb, ids=hi, C=hc, flag=hf)
    assert code == OK
    ref = table[ids].astype(np.float64) @ B.astype(np.float64)
    assert_values(host(hc.payload()), ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max(), what="row-mapped product")
    assert int(hf.payload().item()) == 0
    _check_all(table=ht, B=hb, ids=hi, C=hc, flag=hf)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("use_ws", [False, True])
def test_gemm_rank1_guarded(hip, use_ws, variant):
    """ebn_gemm_f32_rank1, C = alpha A.B^T + row_scale[m] seq_rows[m / L, n], at the AttLayer2 shape (3 x 20 rows, E = 256,
    A = 200) of test_attpool_forward_and_backward (the smallest one whose K is a multiple of 4: the epilogue kernel), restated
    in float64 at that test's dX tolerance; pad1 takes the fill kernel + the scalar-load GEMM."""
    n_seq, L, N, K = 3, 20, 256, 200
    M = n_seq * L
    rng = np.random.default_rng(21)
    A = np.tanh(rng.standard_normal((M, K))).astype(np.float32)
    B = (on.glorot_uniform((N, K), rng) * 2).astype(np.float32)
    rs, sr = rng.random(M).astype(np.float32), rng.standard_normal((n_seq, N)).astype(np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64).T + rs[:, None].astype(np.float64) * np.repeat(sr.astype(np.float64), L, axis=0)
    lda, ldb, ldc, lds = K + _pad(variant, 0), K + _pad(variant, 1), N + _pad(variant, 2), N + _pad(variant, 3)
    (Ad, ha), (Bd, hb), (rsd, hr), (srd, hs) = guard_in(A, ld=lda), guard_in(B, ld=ldb), guard_in(rs), guard_in(sr, ld=lds)
    Cd, hc = guard_out((M, N), ld=ldc)
    n_ws = max(int(hip.lib().ebn_gemm_workspace_floats(M, N, K)), 1) if use_ws else 0
    ws = poison(torch.empty(n_ws, device="cuda")) if use_ws else None
    hip.call("ebn_gemm_f32_rank1", M, N, K, cf(1.0), P(Ad), lda, P(Bd), ldb, P(Cd), ldc, P(rsd), P(srd), lds, L, P(ws), n_ws, S())
    assert_values(host(hc.payload()), ref, rtol=3e-5, atol=1e-5, what=f"rank-1 epilogue ws={use_ws} {variant}")
    _check_all(A=ha, B=hb, row_scale=hr, seq_rows=hs, C=hc)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("use_ws", [False, True])
def test_dense_relu_forward_guarded(hip, use_ws, variant):
    """ebn_dense_relu_fwd_f32 at (37, 20, 12) -- the smallest shape of its test that reaches the bias epilogue (K % 4 == 0);
    pad1: plain product + row-by-row bias / ReLU over the strided C."""
    M, N, K = 37, 20, 12
    rng = np.random.default_rng(M + N + K)
    A, B, b = (x.astype(np.float32) for x in (rng.standard_normal((M, K)), rng.standard_normal((K, N)) / np.sqrt(K), rng.standard_normal(N) * 0.3))
    want = np.maximum(A.astype(np.float64) @ B.astype(np.float64) + b, 0)
    lda, ldb, ldc = K + _pad(variant, 0), N + _pad(variant, 1), N + _pad(variant, 2)
    (Ad, ha), (Bd, hb), (bd, hbias), (Cd, hc) = guard_in(A, ld=lda), guard_in(B, ld=ldb), guard_in(b), guard_out((M, N), ld=ldc)
    n_ws = max(int(hip.lib().ebn_gemm_workspace_floats(M, N, K)), 1) if use_ws else 0
    ws = poison(torch.empty(n_ws, device="cuda")) if use_ws else None
    hip.call("ebn_dense_relu_fwd_f32", M, N, K, P(Ad), lda, P(Bd), ldb, P(bd), P(Cd), ldc, P(ws), n_ws, S())
    got = host(hc.payload())
    assert_values(got, want, rtol=2e-6, atol=1e-5 + 3e-7 * K, what=f"dense relu ws={use_ws} {variant}")
    assert (got >= 0).all()
    _check_all(A=ha, B=hb, bias=hbias, C=hc)


@pytest.mark.parametrize("variant", VARIANTS)
def test_dense_backward_pair_guarded(hip, variant):
    """ebn_dense_bwd_pair_f32 at (250, 76, 36), beta = 0.5 -- the smallest aligned shape of its test: one launch for both
    products in pad4, two scalar-load GEMMs in pad1 -- and with beta = 0 over a NaN dW."""
    R, K_in, N_out = 250, 76, 36
    rng = np.random.default_rng(R * 7 + K_in * 3 + N_out)
    X, dY, W, dW0 = (rng.standard_normal(s).astype(np.float32) for s in ((R, K_in), (R, N_out), (K_in, N_out), (K_in, N_out)))
    ldx, lddy, ldw, lddw, lddx = (w + _pad(variant, i) for i, w in enumerate((K_in, N_out, N_out, N_out, K_in)))
    (Xd, hx), (dYd, hy), (Wd, hw) = guard_in(X, ld=ldx), guard_in(dY, ld=lddy), guard_in(W, ld=ldw)
    n = max(int(hip.lib().ebn_gemm_workspace_floats(K_in, N_out, R)), int(hip.lib().ebn_gemm_workspace_floats(R, K_in, N_out)), 1)
    for beta in (0.5, 0.0):
        (dWd, hdw), (dXd, hdx) = guard_out((K_in, N_out), ld=lddw), guard_out((R, K_in), ld=lddx)
        if beta != 0:
            hdw.fill_payload(dW0)
        ws = poison(torch.empty(n, device="cuda"))
        hip.call("ebn_dense_bwd_pair_f32", R, K_in, N_out, P(Xd), ldx, P(dYd), lddy, P(Wd), ldw, cf(beta), P(dWd), lddw, P(dXd), lddx, P(ws), n, S())
        assert_values(host(hdw.payload()), X.astype(np.float64).T @ dY.astype(np.float64) + beta * dW0, rtol=2e-6, atol=1e-5 + 3e-7 * R, what="pair dW")
        assert_values(host(hdx.payload()), dY.astype(np.float64) @ W.astype(np.float64).T, rtol=2e-6, atol=1e-5 + 3e-7 * N_out, what="pair dX")
        _check_all(dW=hdw, dX=hdx)
    _check_all(X=hx, dY=hy, W=hw)


@pytest.mark.parametrize("variant", VARIANTS)
def test_tn_group_guarded(hip, variant):
    """ebn_gemm_tn_group_f32 on [(48, 40, 96), (20, 36, 96)] with column sums and the L2 term; unaligned leading dimensions
    are EBN_ERR_UNSUPPORTED with nothing written."""
    from ebrec import _hip

    shapes = [(48, 40, 96), (20, 36, 96)]
    rng = np.random.default_rng(len(shapes) * 7 + shapes[0][0])
    probs = (_hip.TnProblem * len(shapes))()
    ins, outs, want = {}, {}, []
    for i, (M, N, K) in enumerate(shapes):
        A, B, W = (rng.standard_normal(s).astype(np.float32) for s in ((K, M), (K, N), (M, N)))
        lda, ldb, ldc = M + _pad(variant, 0), N + _pad(variant, 1), N + _pad(variant, 2)
        (Ad, ha), (Bd, hb), (Wd, hw) = guard_in(A, ld=lda), guard_in(B, ld=ldb), guard_in(W, ld=ldc)
        (Cd, hc), (csd, hcs) = guard_out((M, N), ld=ldc), guard_out((N,))
        q = probs[i]
        q.M, q.N, q.K, q.A, q.lda, q.B, q.ldb, q.C, q.ldc = M, N, K, Ad.data_ptr(), lda, Bd.data_ptr(), ldb, Cd.data_ptr(), ldc
        lam = 0.25 if i == 0 else 0.0
        q.colsum = csd.data_ptr()
        if lam:
            q.l2_W, q.two_lambda = Wd.data_ptr(), lam
        ins.update({f"A{i}": ha, f"B{i}": hb, f"W{i}": hw})
        outs.update({f"C{i}": hc, f"colsum{i}": hcs})
        want.append((A.astype(np.float64).T @ B.astype(np.float64) + lam * W, B.astype(np.float64).sum(0)))
    code = hip.lib().ebn_gemm_tn_group_f32(probs, len(shapes), S())
    if variant == "pad1":
        assert code == UNSUPPORTED
        return _untouched(**ins, **outs)
    assert code == OK
    for i, (c_ref, cs_ref) in enumerate(want):
        assert_values(host(outs[f"C{i}"].payload()), c_ref, rtol=2e-5, atol=2e-5 * np.abs(c_ref).max(), what=f"C of problem {i}")
        assert_values(host(outs[f"colsum{i}"].payload()), cs_ref, rtol=2e-5, atol=2e-5 * max(1.0, np.abs(cs_ref).max()), what=f"column sums {i}")
    _check_all(**ins, **outs)


# ============================================================================================================ attention
ATTN_GUARDED = [(3, 17, 2, 16),                   # MFMA
                (2, 32, 2, 16), (1, 5, 3, 32),    # one-wave <32> when unaligned
                (2, 50, 4, 16),                   # MFMA / one-wave <64> (the fallback shape of the saturated-softmax test)
                (3, 65, 3, 16),                   # long
                (2, 64, 2, 32)]                   # forward and backward route differently
SEED_A, STEP_A = 5, 2


@functools.lru_cache(maxsize=None)
def _attn_ref(n_seq, L, h, d, p):
    """qkv, dY (fp32) and the float64 forward output / backward gradient, dropout mask indexed by LOGICAL element"""
    E = h * d
    qkv, Qh, Kh, Vh, Pm = _qkv_case(n_seq, L, h, d, 11)
    O = (Pm.transpose(0, 1, 3, 2) @ Vh).transpose(0, 2, 1, 3).reshape(n_seq, L, E)
    rng = np.random.default_rng(13)
    dY = rng.standard_normal((n_seq * L, E)).astype(np.float32)
    w = rng.random(n_seq * L).astype(np.float32)
    dpool = rng.standard_normal((n_seq, E)).astype(np.float32)
    mult = np.ones(O.size) if p == 0 else on.dropout_keep_mask(on.dropout_key(SEED_A, STEP_A, 1), O.size, p) / (1 - p)
    O = O * mult.reshape(O.shape)

    def grads(dy):
        dOh = (dy.astype(np.float64).reshape(n_seq, L, E) * mult.reshape(n_seq, L, E)).reshape(n_seq, L, h, d).transpose(0, 2, 1, 3)
        dVh = Pm @ dOh
        dP = Vh @ dOh.transpose(0, 1, 3, 2)
        dS = Pm * (dP - (Pm * dP).sum(-1, keepdims=True))
        back = lambda Z: Z.transpose(0, 2, 1, 3).reshape(n_seq * L, E)
        return np.concatenate([back(dS @ Kh / np.sqrt(d)), back(dS.transpose(0, 1, 3, 2) @ Qh / np.sqrt(d)), back(dVh)], 1)

    full = (dY.astype(np.float64) + w[:, None].astype(np.float64) * np.repeat(dpool.astype(np.float64), L, axis=0)).astype(np.float32)
    return _frozen(qkv.reshape(n_seq * L, 3 * E), dY, w, dpool, full, O.reshape(n_seq * L, E), grads(dY), grads(full))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("n_seq,L,h,d", ATTN_GUARDED)
def test_attention_forward_backward_and_pooled_backward(hip, n_seq, L, h, d, p, variant):
    """ebn_attn_fwd_f32 / ebn_attn_bwd_f32 / ebn_attn_bwd_pooled_f32 with every leading dimension padded by a DIFFERENT amount
    (a stride swap cannot cancel), against float64 at the tolerances of test_attention_forward_is_transposed_softmax_times_v,
    test_attention_backward and test_attention_backward_with_the_pooling_term_folded_in.  pad4: bit-identical to the tight
    layout.  The pooled backward is MFMA only: unaligned strides and unsupported shapes are EBN_ERR_UNSUPPORTED, nothing written."""
    E, R = h * d, n_seq * L
    qkv, dY, w, dpool, full, O, dq_ref, dq_full_ref = _attn_ref(n_seq, L, h, d, p)
    ld_qkv, ld_out, ld_dout, ld_dqkv, ld_pool = (wd + _pad(variant, i) for i, wd in enumerate((3 * E, E, E, 3 * E, E)))
    st = make_state(seed=SEED_A, step=STEP_A)
    tight = variant == "pad4"
    (qd, hq), (od, ho) = guard_in(qkv, ld=ld_qkv), guard_out((R, E), ld=ld_out)
    hip.call("ebn_attn_fwd_f32", P(qd), ld_qkv, P(od), ld_out, n_seq, L, h, d, P(st), 1, cf(p), S())
    assert_values(host(ho.payload()), O, rtol=2e-5, atol=2e-6, what="attn fwd")
    _check_all(qkv=hq, out=ho)
    (dyd, hdy), (gd, hg) = guard_in(dY, ld=ld_dout), guard_out((R, 3 * E), ld=ld_dqkv)
    hip.call("ebn_attn_bwd_f32", P(qd), ld_qkv, P(dyd), ld_dout, P(gd), ld_dqkv, n_seq, L, h, d, P(st), 1, cf(p), S())
    assert_values(host(hg.payload()), dq_ref, rtol=3e-5, atol=5e-6, what="attn bwd")
    _check_all(qkv=hq, dout=hdy, dqkv=hg)
    if tight:
        ot, gt, qt = _nan(R, E), _nan(R, 3 * E), _dev(qkv)
        hip.call("ebn_attn_fwd_f32", P(qt), 3 * E, P(ot), E, n_seq, L, h, d, P(st), 1, cf(p), S())
        hip.call("ebn_attn_bwd_f32", P(qt), 3 * E, P(_dev(dY)), E, P(gt), 3 * E, n_seq, L, h, d, P(st), 1, cf(p), S())
        assert _bits_equal(ho.payload(), ot), "forward: padded and tight layouts differ in bits"
        assert _bits_equal(hg.payload(), gt), "backward: padded and tight layouts differ in bits"
    # the pooled backward against the plain one on dout + w (x) dpool (rounded to fp32), as its own test does
    (wd_, hw), (dpd, hdp), (pg, hpg) = guard_in(w), guard_in(dpool, ld=ld_pool), guard_out((R, 3 * E), ld=ld_dqkv)
    code = hip.lib().ebn_attn_bwd_pooled_f32(P(qd), ld_qkv, P(dyd), ld_dout, P(wd_), P(dpd), ld_pool, P(pg), ld_dqkv, n_seq, L, h, d,
                                             P(st), 1, cf(p), S())
    if not tight or not hip.lib().ebn_attn_bwd_pooled_supported(L, d):
        assert code == UNSUPPORTED
        return _untouched(qkv=hq, dout=hdy, pool_w=hw, pool_dout=hdp, dqkv=hpg)
    assert code == OK
    (fd, hfull), (pl, hpl) = guard_in(full, ld=ld_dout), guard_out((R, 3 * E), ld=ld_dqkv)
    hip.call("ebn_attn_bwd_f32", P(qd), ld_qkv, P(fd), ld_dout, P(pl), ld_dqkv, n_seq, L, h, d, P(st), 1, cf(p), S())
    assert_values(host(hpl.payload()), dq_full_ref, rtol=3e-5, atol=5e-6, what="attn bwd of the folded gradient")
    assert_values(host(hpg.payload()), host(hpl.payload()), rtol=2e-5, atol=2e-5, what="pooled attn bwd")
    _check_all(qkv=hq, dout=hdy, pool_w=hw, pool_dout=hdp, dqkv=hpg, full=hfull, dqkv_plain=hpl)
    pt = _nan(R, 3 * E)
    hip.call("ebn_attn_bwd_pooled_f32", P(_dev(qkv)), 3 * E, P(_dev(dY)), E, P(_dev(w)), P(_dev(dpool)), E, P(pt), 3 * E, n_seq, L, h, d, P(st), 1, cf(p), S())
    assert _bits_equal(hpg.payload(), pt), "pooled backward: padded and tight layouts differ in bits"


# ============================================================================================================ top-k
@pytest.mark.parametrize("variant", ["aligned", "users+4B"])
@pytest.mark.parametrize("n_splits", [1, 2])
@pytest.mark.parametrize("shape", [(65, 257, 36, 10), (3, 7, 4, 10)], ids=lambda s: "x".join(map(str, s)))
def test_topk_guarded(hip, shape, n_splits, variant):
    """ebn_topk_score_f32 on the integer cases (exact): users / news_all guarded with NaN (flags[1] stays 0), cand_rows with n_rows
    (flags[0] stays 0), exclude with the row of the first / last user's best candidate in front / behind (an over-read drops it
    from that user's list), outputs in canaries, workspace poisoned.  A users pointer moved by 4 bytes: EBN_ERR_ALIGN, nothing
    written."""
    U, M, F, k = shape
    users, news, cand_rows, ex = rc.integer_case(U, M, F, seed=U + M, cand="subset", exclude="x3")
    n_rows = news.shape[0]
    s64 = rc.scores64(users, news, cand_rows)
    want_pos, want_score, want_flags = rc.topk_reference(s64, k, cand_rows, n_rows, ex)
    assert want_flags == (0, 0)
    (ud, hu), (nd, hn) = guard_in(users, offset=0 if variant == "aligned" else 1), guard_in(news)
    (cd, hcr), (ed, he) = guard_in(cand_rows, fill=n_rows), guard_in(ex, fill=-1)
    he.set_guards(int(cand_rows[want_pos[0, 0]]), int(cand_rows[want_pos[U - 1, 0]]))
    (pd_, hp), (sd, hs), (fd, hf) = guard_out((U, k), dtype=torch.int32), guard_out((U, k)), guard_out((2,), dtype=torch.int32)
    hf.fill_payload([0, 0])
    ws_bytes = int(hip.lib().ebn_topk_workspace_bytes(U, k, n_splits))
    assert ws_bytes > 0
    ws = poison(torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"))
    code = hip.lib().ebn_topk_score_f32(P(ud), P(nd), n_rows, P(cd), M, P(ed), ex.shape[1], k, 0, n_splits, P(pd_), P(sd), P(fd), P(ws),
                                        ws_bytes, U, F, S())
    handles = dict(users=hu, news_all=hn, cand_rows=hcr, exclude=he, out_pos=hp, out_score=hs, flags=hf)
    if variant != "aligned":
        assert code == ALIGN
        return _untouched(**handles)
    assert code == OK
    torch.cuda.synchronize()
    assert tuple(hf.payload().tolist()) == (0, 0)
    assert np.array_equal(hp.payload().cpu().numpy(), want_pos)
    assert np.array_equal(hs.payload().cpu().numpy().astype(np.float64), want_score)
    _check_all(**handles)


# ============================================================================================================ LSTUR
GRU_SHAPES = [(3, 1, 8), (17, 3, 36), (5, 2, 132)]  # partial sequence tile; partial unit tile after two full ones, K below one
#                                                     128 slab; one full slab plus a 4-wide tail


@functools.lru_cache(maxsize=None)
def _gru_case(B, H, U):
    rng = np.random.default_rng(B * 100 + H + U)
    X = rng.uniform(-1, 1, (B, H, U)).astype(np.float32)
    X[rng.random((B, H)) < 0.25] = 0.0
    X[0] = 0.0
    lim = np.sqrt(6.0 / (4 * U))
    Wk, Wr = (rng.uniform(-lim, lim, (U, 3 * U)).astype(np.float32) for _ in range(2))
    bias = rng.uniform(-0.2, 0.2, (2, 3 * U)).astype(np.float32)
    h0 = rng.uniform(-0.5, 0.5, (B, U)).astype(np.float32)
    dhH = rng.uniform(-1, 1, (B, U)).astype(np.float32)
    gx = (X.reshape(B * H, U).astype(np.float64) @ Wk.astype(np.float64)).astype(np.float32)
    return _frozen(X, Wk, Wr, bias, h0, dhH, gx) + (_gru_ref(X, h0, Wk, Wr, bias, dhH),)


@pytest.mark.parametrize("variant", ["aligned", "X+4B"])
@pytest.mark.parametrize("B,H,U", GRU_SHAPES)
def test_gru_forward_backward_guarded(hip, B, H, U, variant):
    """ebn_gru_fwd_f32 / ebn_gru_bwd_f32 against the float64 autograd of test_gru_fwd_bwd_kernels_vs_float64, at its tolerances.
    An X moved by 4 bytes is EBN_ERR_ALIGN with nothing written."""
    X, Wk, Wr, bias, h0, dhH, gx, (hs, z, r, n, ghh, rdgx, rdgh, rdh0) = _gru_case(B, H, U)
    F = U
    off = 0 if variant == "aligned" else 1
    (gxd, hgx), (Xd, hx), (Wd, hw), (bd, hb), (h0d, hh0) = (guard_in(gx), guard_in(X.reshape(B * H, F), offset=off), guard_in(Wr), guard_in(bias),
                                                           guard_in(h0))
    (Hsd, hHs), (actd, hact) = guard_out((H + 1, B, U)), guard_out((H, B, 4 * U))
    code = hip.lib().ebn_gru_fwd_f32(P(gxd), P(Xd), P(Wd), P(bd), P(h0d), P(Hsd), P(actd), B, H, F, U, S())
    ins = dict(gx=hgx, X=hx, Wrec=hw, bias=hb, h0=hh0)
    if variant != "aligned":
        assert code == ALIGN
        (a, ha), (b_, hb2), (c, hc) = guard_out((B * H, 3 * U)), guard_out((H, B, 3 * U)), guard_out((B, U))
        assert hip.lib().ebn_gru_bwd_f32(P(h0d), P(Xd), P(Wd), P(Hsd), P(actd), P(a), P(b_), P(c), B, H, F, U, S()) == ALIGN
        return _untouched(**ins, Hs=hHs, act=hact, dgx=ha, dgh=hb2, dh0=hc)
    assert code == OK
    gHs, gact = host(hHs.payload()).reshape(H + 1, B, U), host(hact.payload()).reshape(H, B, 4, U)
    for name, got, ref in (("Hs", gHs, hs), ("z", gact[:, :, 0], z), ("r", gact[:, :, 1], r), ("n", gact[:, :, 2], n), ("gh_h", gact[:, :, 3], ghh)):
        assert np.abs(got - ref).max() <= 1e-5, f"{name}: max abs err {np.abs(got - ref).max():.3e}"
    _check_all(**ins, Hs=hHs, act=hact)
    (dhd, hdh), (Hsi, hHsi), (acti, hacti) = guard_in(dhH), guard_in(hHs.payload().cpu().numpy()), guard_in(hact.payload().cpu().numpy())
    (dgxd, hdgx), (dghd, hdgh), (dh0d, hdh0) = guard_out((B * H, 3 * U)), guard_out((H, B, 3 * U)), guard_out((B, U))
    hip.call("ebn_gru_bwd_f32", P(dhd), P(Xd), P(Wd), P(Hsi), P(acti), P(dgxd), P(dghd), P(dh0d), B, H, F, U, S())
    live = (X != 0).any(-1)
    gdgx, gdgh, gdh0 = host(hdgx.payload()).reshape(B, H, 3 * U), host(hdgh.payload()).reshape(H, B, 3 * U), host(hdh0.payload())
    assert (gdgx[~live] == 0).all() and (gdgh[~live.T] == 0).all()
    for name, got, ref in (("dgx", gdgx, rdgx), ("dgh", gdgh, rdgh), ("dh0", gdh0, rdh0)):
        err = np.abs(got - ref).max()
        assert err <= 2e-4 * np.abs(ref).max() + 1e-9, f"{name}: max abs err {err:.3e} vs max {np.abs(ref).max():.3e}"
    _check_all(dhH=hdh, X=hx, Wrec=hw, Hs=hHsi, act=hacti, dgx=hdgx, dgh=hdgh, dh0=hdh0)


@pytest.mark.parametrize("variant", ["aligned", "Wrec+4B"])
@pytest.mark.parametrize("B,H,U", GRU_SHAPES)
def test_indexed_gru_guarded(hip, B, H, U, variant):
    """ebn_gru_infer_indexed_f32: his_idx guarded with n_rows (a read raises oob), live_all with 1, gx_all with NaN; bit-equal to
    ebn_gru_fwd_f32's Hs[H] on the gathered rows (the assertion of its existing test)."""
    rng = np.random.default_rng(B * 1000 + H * 10 + U)
    n_rows = 41
    news = rng.uniform(-1, 1, (n_rows, U)).astype(np.float32)
    zero_rows = [0, 7, 40]
    news[zero_rows] = 0.0
    idx = rng.integers(0, n_rows, (B, H)).astype(np.int32)
    idx[rng.random((B, H)) < 0.2] = rng.choice(zero_rows)
    idx[0] = 0
    lim = np.sqrt(6.0 / (4 * U))
    Wk, Wr = (rng.uniform(-lim, lim, (U, 3 * U)).astype(np.float32) for _ in range(2))
    bias = rng.uniform(-0.2, 0.2, (2, 3 * U)).astype(np.float32)
    h0 = rng.uniform(-0.5, 0.5, (B, U)).astype(np.float32)
    gx_all = (news.astype(np.float64) @ Wk.astype(np.float64)).astype(np.float32)
    live = (news != 0).any(1).astype(np.int32)
    (gd, hg), (ld_, hl), (idd, hi) = guard_in(gx_all), guard_in(live, fill=1), guard_in(idx, fill=n_rows)
    (Wd, hw), (bd, hb), (h0d, hh0) = guard_in(Wr, offset=0 if variant == "aligned" else 1), guard_in(bias), guard_in(h0)
    (hwk, hhw), (hout, hho), (fd, hf) = guard_out((B, U)), guard_out((B, U)), guard_out((1,), dtype=torch.int32)
    hf.fill_payload([0])
    hhw.prefilled = False  # h_work is scratch: with H == 1 nothing is written to it
    code = hip.lib().ebn_gru_infer_indexed_f32(P(gd), P(ld_), n_rows, P(idd), P(Wd), P(bd), P(h0d), P(hwk), P(hout), B, H, U, P(fd), S())
    handles = dict(gx_all=hg, live_all=hl, his_idx=hi, Wrec=hw, bias=hb, h0=hh0, h_work=hhw, h_out=hho, oob_flag=hf)
    if variant != "aligned":
        assert code == ALIGN
        return _untouched(**handles)
    assert code == OK
    flat = idx.reshape(-1)
    Hs, act = _nan(H + 1, B, U), _nan(H, B, 4 * U)
    hip.call("ebn_gru_fwd_f32", P(_dev(gx_all[flat])), P(_dev(news[flat])), P(_dev(Wr)), P(_dev(bias)), P(_dev(h0)), P(Hs), P(act), B, H, U, U, S())
    torch.cuda.synchronize()
    assert int(hf.payload().item()) == 0
    assert _bits_equal(hho.payload(), Hs[H]), f"max abs diff {float((hho.payload() - Hs[H]).abs().max()):.3e}"
    _check_all(**handles)


@pytest.mark.parametrize("variant", ["aligned", "X+4B"])
@pytest.mark.parametrize("T", [1, 7])
def test_masked_attpool_guarded(hip, T, variant):
    """ebn_attpool_masked_fwd_f32 at F = 64: ids guarded with 1 (a live token) and X with NaN -- a masked-row over-read un-masks a
    NaN row.  No alignment rule: an X moved by 4 bytes must give the same result."""
    F, n_seq, A = 64, 41, 200
    rng = np.random.default_rng(T * 1000 + F)
    R = n_seq * T
    Vd = rng.uniform(0, 1, (R, F)).astype(np.float32)
    Vd[rng.random(R) < 0.15] = 0.0
    ids = rng.integers(1, 50, (n_seq, T)).astype(np.int32)
    ids[rng.random((n_seq, T)) < 0.2] = 0
    ids[::5] = 0
    Wa = (rng.uniform(-1, 1, (F, A)) / np.sqrt(F)).astype(np.float32)
    ba, q = rng.uniform(-0.1, 0.1, A).astype(np.float32), rng.uniform(-1, 1, A).astype(np.float32)
    U0 = (Vd.astype(np.float64) @ Wa.astype(np.float64)).astype(np.float32)
    (Ud, hU), (outd, ho), (wd, hwt) = guard_out((R, A)), guard_out((n_seq, F)), guard_out((R,))
    hU.fill_payload(U0)
    (Xd, hx), (idd, hi), (bd, hb), (qd, hq) = guard_in(Vd, offset=0 if variant == "aligned" else 1), guard_in(ids.reshape(-1), fill=1), guard_in(ba), guard_in(q)
    hip.call("ebn_attpool_masked_fwd_f32", P(Ud), P(bd), P(qd), P(Xd), P(idd), P(outd), P(wd), n_seq, T, F, A, S())
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    o64, w64 = lo.masked_attlayer2(t64(Vd).reshape(n_seq, T, F), torch.from_numpy(ids.astype(np.int64)), t64(Wa), t64(ba), t64(q.reshape(A, 1)))
    masked = ((ids == 0) | (Vd.reshape(n_seq, T, F) == 0).all(-1)).reshape(-1)
    gw, go = host(hwt.payload()), host(ho.payload())
    assert (gw[masked] == 0).all(), "masked rows must get weight 0 exactly"
    assert (go[(ids == 0).all(1)] == 0).all()
    assert_values(host(hU.payload()), np.tanh(Vd.astype(np.float64) @ Wa.astype(np.float64) + ba), rtol=1e-5, atol=1e-6, what="tanh U")
    assert_values(gw, w64.numpy().reshape(-1), rtol=1e-4, atol=1e-7, what="w")
    assert_values(go, o64.numpy(), rtol=1e-4, atol=1e-6, what="out")
    _check_all(U=hU, out=ho, w=hwt, X=hx, ids=hi, b=hb, q=hq)


# ============================================================================================================ Conv1D
@pytest.mark.parametrize("variant", ["aligned", "X+4B"])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("T,E,F", [(7, 100, 64), (1, 300, 400)])
def test_conv1d_guarded(hip, T, E, F, drop, variant):
    """ebn_conv1d_fwd_f32 / _bwd_data_f32 / _bwd_weight_f32, window 3 (halo rows at both ends of every title, T = 1: nothing but
    halo), with the assertions of test_conv1d_kernels_vs_float64; the weight-gradient slices land in a NaN pre-filled, guarded
    workspace.  An X moved by 4 bytes is EBN_ERR_ALIGN with nothing written."""
    window = 3
    rng = np.random.default_rng(T * 7 + E + window)
    n_titles = 37 if T > 1 else 1111
    R = n_titles * T
    X = rng.uniform(-1, 1, (R, E)).astype(np.float32)
    W = (rng.uniform(-1, 1, (window * E, F)) / np.sqrt(window * E)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, F).astype(np.float32)
    dVd = rng.uniform(-1, 1, (R, F)).astype(np.float32)
    p_conv, p_pap = (0.2, 0.2) if drop else (0.0, 0.0)
    st = make_state(CONV_SEED, CONV_STEP) if drop else None
    stp = P(st) if drop else None
    (Xd, hx), (Wd, hw), (bd, hb), (Vo, hv) = guard_in(X, offset=0 if variant == "aligned" else 1), guard_in(W), guard_in(b), guard_out((R, F))
    L = hip.lib()
    code = L.ebn_conv1d_fwd_f32(P(Xd), P(Wd), P(bd), P(Vo), n_titles, T, E, F, window, stp, 2, cf(p_conv), 3, cf(p_pap), S())
    splits = int(L.ebn_conv1d_wgrad_splits(n_titles, T, E, F, window))
    n = int(L.ebn_conv1d_wgrad_workspace_floats(n_titles, T, E, F, window, splits))
    assert n == splits * (window * E + 1) * F
    if variant != "aligned":
        assert code == ALIGN
        (dd, hd), (pd_, hp) = guard_in(dVd), guard_out((n,))
        assert L.ebn_conv1d_bwd_weight_f32(P(Xd), P(dd), P(dd), P(pd_), splits, n_titles, T, E, F, window, stp, cf(p_conv), cf(p_pap), S()) == ALIGN
        return _untouched(X=hx, W=hw, bias=hb, Vd=hv, dVd=hd, partials=hp)
    assert code == OK
    A64 = _unfold(X.astype(np.float64), T, window)
    pre = A64 @ W.astype(np.float64) + b
    m = (_mult(2, p_conv, R * F) * _mult(3, p_pap, R * F)).reshape(R, F)
    want = np.maximum(pre, 0) * m
    got = host(hv.payload())
    scale = np.abs(A64).sum(1, keepdims=True) @ np.abs(W).max(0, keepdims=True) + 1e-3
    assert (np.abs(got - want) <= 2e-6 * scale * np.maximum(m, 1)).all(), np.abs(got - want).max()
    dropped = m == 0
    assert (got[dropped] == 0).all()
    clear = ~dropped & (np.abs(pre) > 1e-5 * scale)
    np.testing.assert_array_equal(got[clear] > 0, pre[clear] > 0)
    _check_all(X=hx, W=hw, bias=hb, Vd=hv)

    gscale = (1.0 / (1 - p_conv) if p_conv else 1.0) * (1.0 / (1 - p_pap) if p_pap else 1.0)
    dYp = np.where(got > 0, dVd.astype(np.float64) * gscale, 0.0)
    (dd, hd), (vi, hvi), (dX, hdx) = guard_in(dVd), guard_in(hv.payload().cpu().numpy()), guard_out((R, E))
    hip.call("ebn_conv1d_bwd_data_f32", P(dd), P(vi), P(Wd), P(dX), n_titles, T, E, F, window, stp, cf(p_conv), cf(p_pap), S())
    dA3 = (dYp @ W.astype(np.float64).T).reshape(n_titles, T, window, E)
    want_dx = np.zeros((n_titles, T, E))
    pl = (window - 1) // 2
    for j in range(window):
        lo_, hi_ = max(0, pl - j), min(T, T + pl - j)
        want_dx[:, lo_ + j - pl:hi_ + j - pl] += dA3[:, lo_:hi_, j]
    sx = np.abs(dYp).sum() / R * np.abs(W).max() * window * F / 4 + 1e-6
    assert_values(host(hdx.payload()), want_dx.reshape(R, E), rtol=1e-4, atol=1e-5 * sx, what="dX")
    _check_all(dVd=hd, Vd=hvi, W=hw, dX=hdx)

    part, hp = guard_out((n,))
    hip.call("ebn_conv1d_bwd_weight_f32", P(Xd), P(dd), P(vi), P(part), splits, n_titles, T, E, F, window, stp, cf(p_conv), cf(p_pap), S())
    gw = host(hp.payload()).reshape(splits, window * E + 1, F).sum(0)
    want_w = A64.T @ dYp
    sw = np.abs(A64).T @ np.abs(dYp) + 1e-6
    assert (np.abs(gw[: window * E] - want_w) <= 2e-6 * sw).all(), np.abs(gw[: window * E] - want_w).max()
    assert (np.abs(gw[window * E] - dYp.sum(0)) <= 2e-6 * (np.abs(dYp).sum(0) + 1e-6)).all()
    _check_all(X=hx, dVd=hd, Vd=hvi, partials=hp)
