"""The guard-band harness (tests/guarded.py) on the CPU: a healthy stand-in "kernel" passes, and each planted defect -- the bugs
the guarded GPU tests exist to find -- makes handle.check() or the value comparison fail.  The stand-ins are numpy loops over
the operands as C sees them (flat storage + element offset + leading dimension); no GPU code is made to misbehave."""
import numpy as np
import pytest
import torch

from tests.guarded import CANARY, assert_values, guard_in, guard_len, guard_out, poison

M, N, K = 5, 6, 7
DEFECTS = ["write_past_end", "write_padding", "unwritten", "overread_zero_multiplier", "width_for_ld"]


def standin_gemm(a, a0, lda, b, b0, ldb, c, c0, ldc, alpha, beta, defect=None):
    """C[M,N] = alpha * A[M,K] . B[K,N] (+ beta * C when beta != 0; C is not read otherwise), row by row."""
    Bm = np.stack([b[b0 + k * ldb: b0 + k * ldb + N] for k in range(K)]).astype(np.float64)
    a_stride = K if defect == "width_for_ld" else lda
    for m in range(M):
        row = alpha * (a[a0 + m * a_stride: a0 + m * a_stride + K].astype(np.float64) @ Bm)
        if defect == "overread_zero_multiplier" and m == M - 1:
            with np.errstate(invalid="ignore"):
                row = row + 0.0 * (a[a0 + M * lda: a0 + M * lda + K].astype(np.float64) @ Bm)  # one row past the end
        if beta != 0:
            row = row + beta * c[c0 + m * ldc: c0 + m * ldc + N]
        n_store = N - 1 if (defect == "unwritten" and m == M - 1) else N
        c[c0 + m * ldc: c0 + m * ldc + n_store] = row[:n_store].astype(np.float32)
    if defect == "write_past_end":
        c[c0 + M * ldc] = 0.0
    if defect == "write_padding":
        c[c0 + 2 * ldc + N] = 0.0


def _run(defect, pad, beta=0.0):
    rng = np.random.default_rng(3)
    A, B = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    _, ha = guard_in(A, ld=K + pad, device="cpu")
    _, hb = guard_in(B, ld=N + pad, device="cpu")
    _, hc = guard_out((M, N), ld=N + pad, device="cpu")
    if beta != 0:
        hc.fill_payload(C0)
    (a, a0), (b, b0), (c, c0) = ha.raw(), hb.raw(), hc.raw()
    standin_gemm(a, a0, K + pad, b, b0, N + pad, c, c0, N + pad, 0.5, beta, defect)
    got = hc.payload().numpy().astype(np.float64)
    want = 0.5 * A.astype(np.float64) @ B.astype(np.float64) + beta * C0
    assert_values(got, want, rtol=2e-6, atol=1e-5, what="stand-in product")  # the comparison of the GPU tests: a NaN fails it
    for h, name in ((ha, "A"), (hb, "B"), (hc, "C")):
        h.check(name)


@pytest.mark.parametrize("beta", [0.0, -0.5])
@pytest.mark.parametrize("pad", [0, 1, 4])
def test_a_healthy_stand_in_passes(pad, beta):
    _run(None, pad, beta)


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_planted_defect_is_caught(defect):
    pad = 4
    with pytest.raises(AssertionError):
        _run(defect, pad)


def test_the_value_comparison_fails_on_nan_and_inf():
    want = np.ones((3, 4))
    assert_values(want + 1e-7, want)
    for poisoned in (np.nan, np.inf, -np.inf, 2.0):
        got = want.copy()
        got[1, 2] = poisoned
        with pytest.raises(AssertionError, match=r"first at \(1, 2\)"):
            assert_values(got, want, what="one bad element")
    with pytest.raises(AssertionError):
        assert_values(np.ones(3), np.ones(4))


@pytest.mark.parametrize("defect", ["overread_zero_multiplier", "unwritten"])
def test_a_nan_that_reaches_the_output_fails_the_value_comparison_itself(defect):
    """not only check(): the over-read of a NaN guard under a zero multiplier and the output left at its NaN pre-fill are
    caught by assert_values before any canary is looked at"""
    with pytest.raises(AssertionError, match="stand-in product.*NaN"):
        _run(defect, 4)


def test_messages_name_the_place():
    _, h = guard_out((M, N), ld=N + 4, device="cpu")
    c, c0 = h.raw()
    c[c0:c0 + M * (N + 4)].reshape(M, N + 4)[:, :N] = 1.0
    h.check()
    c[c0 + 2 * (N + 4) + N + 1] = 0.0
    with pytest.raises(AssertionError, match=rf"padding column {N + 1} of row 2"):
        h.check()
    c[c0 + 2 * (N + 4) + N + 1] = np.array([CANARY], np.int32).view(np.float32)[0]
    h.check()
    c[c0 - 1] = 0.0
    with pytest.raises(AssertionError, match="in front"):
        h.check()
    _, h = guard_out((M, N), device="cpu")
    c, c0 = h.raw()
    c[c0:c0 + M * N] = 1.0
    c[c0 + M * N + 2] = 0.0
    with pytest.raises(AssertionError, match="behind the operand .2 elements"):
        h.check()
    _, h = guard_out((M, N), device="cpu")
    c, c0 = h.raw()
    c[c0:c0 + M * N - 1] = 1.0
    with pytest.raises(AssertionError, match=rf"never written; first: payload element \({M - 1}, {N - 1}\)"):
        h.check()


def test_layout_alignment_offsets_and_integer_operands():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    v, h = guard_in(x, ld=8, device="cpu")
    assert v.data_ptr() % 16 == 0 and v.stride() == (8, 1) and torch.equal(v, torch.from_numpy(x))
    flat, s = h.raw()
    assert s >= guard_len(8) and len(flat) - (s + 3 * 8) >= guard_len(8) and guard_len(8) == 4096 and guard_len(100) == 25600
    assert np.isnan(flat[:s]).all() and np.isnan(flat[s + 24:]).all() and np.isnan(flat[s:s + 24].reshape(3, 8)[:, 4:]).all()
    v1, h1 = guard_in(x, ld=5, device="cpu", offset=1)
    assert v1.data_ptr() % 16 == 4 and torch.equal(v1, torch.from_numpy(x))
    ids, hi = guard_in(np.array([3, 1, 2], np.int32), fill=99, device="cpu")
    flat, s = hi.raw()
    assert ids.dtype == torch.int32 and ids.tolist() == [3, 1, 2] and (flat[:s] == 99).all() and (flat[s + 3:] == 99).all()
    flat[s + 1] = 7  # a kernel that writes into an input
    with pytest.raises(AssertionError, match=r"payload element \(0, 1\)"):
        hi.check("ids")
    o, ho = guard_out((2, 3), dtype=torch.int32, device="cpu")
    with pytest.raises(AssertionError, match="never written"):
        ho.check()
    o.fill_(0)
    ho.check()
    assert torch.isnan(poison(torch.zeros(5))).all()
    assert torch.isnan(poison(torch.zeros(8, dtype=torch.uint8)).view(torch.float32)).all()
