"""The six ebn_ba_* entry points on guard-banded operands (tests/guarded_eval.py): the table and the scalar column in NaN, the id
arrays inside a VALID row number, the int64 offsets as int32 word pairs inside zero words, the distance matrix of the subset sums
in NaN, every output in canaries with a pre-filled payload.

Shapes: the widths on both sides of every template switch (D % 4, the 64-wide slab, the register form of the cross mean at 256,
512, 768, 1024 and its hand-over to the tiled form at 1028), the table 16-byte aligned and at pointer offset 1 with D % 4 == 0
(the scalar-load branch of the dispatch), list lengths on both sides of the wave-per-list form (10 | 11) and of the 16-wide tile,
once with a length-10 list at the end of the id array and once with a length-17 one.

References and bounds are the existing ones of tests/test_beyond_accuracy_gpu.py, unchanged: the package's float64 host path
under dist_tol(D) (check_dist), check_mean for the list means, 2^-22 for the unit rows and 2 * 2^-20 for the subset sums.
tests/test_guarded_eval_cpu.py plants the defects these operands exist to show."""
import numpy as np
import pytest
import torch

from tests import guarded_eval as ge
from tests.guarded import guard_in, guard_out
from tests.hip_testutil import P, S
from tests.test_beyond_accuracy_gpu import check_dist, check_mean, host_diversity, host_serendipity

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 60, 64, 68, 256, 260, 512, 768, 1024, 1028]
N_ROWS = 40
LAST_10 = [33, 0, 17, 1, 32, 2, 16, 11, 15, 10]  # the wave-per-list form owns the end of the id array
LAST_17 = [10, 32, 0, 16, 1, 33, 15, 2, 11, 17]  # the tiled form does
assert sorted(LAST_10) == sorted(LAST_17) == [0, 1, 2, 10, 11, 15, 16, 17, 32, 33]


def unit32(vec):
    """unit rows in float32, a zero row divided by 1 (what ebn_ba_unit_rows_f32 leaves, up to rounding)"""
    nrm = np.sqrt((vec * vec).sum(1, keepdims=True, dtype=np.float32))
    nrm[nrm == 0] = 1
    return (vec / nrm).astype(np.float32)


def table(D, seed):
    rng = np.random.default_rng(seed)
    vec = (rng.standard_normal((N_ROWS, D)) + 0.5).astype(np.float32)
    vec[5] = 0.0
    vec[9] = vec[8]
    return vec


def id_lists(lengths, seed):
    """lists of the given lengths over rows [0, N_ROWS): the table's first and last row are named, two ids of the longest list
    are missing (-1 and N_ROWS)"""
    rng = np.random.default_rng(seed)
    lists = [rng.integers(0, N_ROWS, n) for n in lengths]
    longest = int(np.argmax(lengths))
    lists[longest][:4] = [0, N_ROWS - 1, -1, N_ROWS]
    lists[-1][-1] = N_ROWS - 1  # the last id of the array names the last row
    return lists


def guarded_lists(lists):
    ids, off = ge.csr(lists)
    ids_d, h_ids = guard_in(ids, fill=1, guard=ge.GUARD)
    off_d, h_off = ge.words_in(off, 0)
    return ids_d, off_d, len(ids), [("ids", h_ids), ("offsets", h_off)]


def intralist(hip, unit, lists, form, table_off):
    ops = ge.ListOps(unit, lists, table_off=table_off)
    hip.call("ebn_ba_intralist_f32", P(ops.table), ops.n_rows, ops.D, P(ops.ids), ops.n_ids, P(ops.off), ops.n_lists, form, P(ops.out), S())
    torch.cuda.synchronize()
    return ops


def cross(hip, unit, R, H, form, table_off, want, D, what):
    unit_d, h_unit = guard_in(unit, fill=ge.NAN, offset=table_off, guard=ge.table_guard(D))
    ids_r, off_r, n_r, h_r = guarded_lists(R)
    ids_h, off_h, n_h, h_h = guarded_lists(H)
    out, h_out = guard_out((len(R),), guard=ge.GUARD)
    hip.call("ebn_ba_cross_f32", P(unit_d), N_ROWS, D, P(ids_r), n_r, P(off_r), P(ids_h), n_h, P(off_h), len(R), form, P(out), S())
    torch.cuda.synchronize()
    for name, h in [("unit", h_unit), ("out", h_out)] + [(f"{n}_r", h) for n, h in h_r] + [(f"{n}_h", h) for n, h in h_h]:
        h.check(name)
    check_dist(h_out.payload().cpu().numpy().astype(np.float64), want, D, what)


@pytest.mark.parametrize("D", WIDTHS)
def test_intralist_and_cross_on_guarded_operands(hip, D):
    vec = table(D, seed=D)
    unit = unit32(vec)
    A, B = id_lists(LAST_10, seed=D + 1), id_lists(LAST_17, seed=D + 2)
    want = {"last 10": host_diversity(vec, A), "last 17": host_diversity(vec, B)}
    want_ab, want_ba = host_serendipity(vec, A, B), host_serendipity(vec, B, A)
    assert np.isnan(want["last 10"]).sum() == 2 and np.isnan(want_ab).sum() == 2  # lengths 0 and 1 / an empty side, nothing else
    for table_off in (0, 1):  # offset 1: 4-byte aligned, the scalar-load forms whatever D % 4 is
        for form in (0, 1):
            for name, lists in (("last 10", A), ("last 17", B)):
                what = f"intralist D {D} table offset {table_off} form {form}, {name}"
                ops = intralist(hip, unit, lists, form, table_off)
                ge.check_list_values(ops, want[name], lambda got, ref: check_dist(got, ref, D, what))
            cross(hip, unit, A, B, form, table_off, want_ab, D, f"cross D {D} table offset {table_off} form {form}, A x B")
            cross(hip, unit, B, A, form, table_off, want_ba, D, f"cross D {D} table offset {table_off} form {form}, B x A")


@pytest.mark.parametrize("D", [3, 68, 260])
@pytest.mark.parametrize("m", [1, 15, 16, 17, 33])
def test_pairdist_on_guarded_operands(hip, m, D):
    vec = table(D, seed=D + m)
    unit = unit32(vec)
    rng = np.random.default_rng(m)
    ids = rng.integers(0, N_ROWS, m).astype(np.int32)
    ids[0], ids[-1] = 0, N_ROWS - 1
    if m > 2:
        ids[1] = N_ROWS  # missing
    ok = (ids >= 0) & (ids < N_ROWS)
    v = vec.astype(np.float64)[np.where(ok, ids, 0)]
    nrm = np.sqrt((v * v).sum(1, keepdims=True))
    nrm[nrm == 0] = 1.0
    u = v / nrm
    want = np.clip(1.0 - u @ u.T, 0.0, 2.0)
    np.fill_diagonal(want, 0.0)
    want[~ok, :], want[:, ~ok] = np.nan, np.nan
    for table_off in (0, 1):
        unit_d, h_unit = guard_in(unit, fill=ge.NAN, offset=table_off, guard=ge.table_guard(D))
        ids_d, h_ids = guard_in(ids, fill=1, guard=ge.GUARD)
        out, h_out = guard_out((m * m,), guard=ge.GUARD)
        hip.call("ebn_ba_pairdist_f32", P(unit_d), N_ROWS, D, P(ids_d), m, P(out), S())
        torch.cuda.synchronize()
        for name, h in (("unit", h_unit), ("ids", h_ids), ("out", h_out)):
            h.check(name)
        got = h_out.payload().cpu().numpy().astype(np.float64).reshape(m, m)
        check_dist(got, want, D, f"pairdist m {m} D {D} table offset {table_off}")
        assert (np.diag(got)[ok] == 0.0).all()


@pytest.mark.parametrize("n_rows", [1, 4, 5])
@pytest.mark.parametrize("D", [1, 63, 64, 65])
def test_unit_rows_on_guarded_operands(hip, D, n_rows):
    rng = np.random.default_rng(D + n_rows)
    vec = (rng.standard_normal((n_rows, D)) + 0.5).astype(np.float32)
    if n_rows > 1:
        vec[1] = 0.0
    want = vec.astype(np.float64)
    nrm = np.sqrt((want * want).sum(1, keepdims=True))
    nrm[nrm == 0] = 1.0
    want = want / nrm
    for off in (0, 1):
        src, h_src = guard_in(vec, fill=ge.NAN, offset=off, guard=ge.table_guard(D))
        dst, h_dst = guard_out((n_rows, D), offset=off, guard=ge.table_guard(D))
        hip.call("ebn_ba_unit_rows_f32", P(src), P(dst), n_rows, D, S())
        torch.cuda.synchronize()
        h_src.check("src")
        h_dst.check("dst")
        got = h_dst.payload().cpu().numpy().astype(np.float64)
        assert (np.abs(got - want) <= 2.0 ** -22).all(), (off, float(np.abs(got - want).max()))  # the bound of test_unit_rows; false for a NaN
        if n_rows > 1:
            assert (got[1] == 0.0).all()


@pytest.mark.parametrize("n_subsets", [1, 4, 5])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65])
def test_subset_sums_on_guarded_operands(hip, k, n_subsets):
    """distances in multiples of 1/64: every sum is exact in fp32 in any order, the division is the one rounding"""
    m = 70
    rng = np.random.default_rng(k + n_subsets)
    dist = (rng.integers(0, 129, (m, m)) / 64.0).astype(np.float32)
    subsets = np.stack([rng.choice(m, k, replace=False) for _ in range(n_subsets)]).astype(np.int32)
    subsets[0, 0], subsets[-1, -1] = 0, m - 1  # dist[0, ...] and dist[m - 1, ...]: both ends of the matrix
    if k >= 63:
        subsets[0, 5], subsets[-1, 7] = m, -1  # skipped
    want = []
    for s in subsets:
        v = [i for i in s if 0 <= i < m]
        want.append(sum(float(dist[a, b]) for ia, a in enumerate(v) for ib, b in enumerate(v) if ia != ib) / (len(v) * (len(v) - 1)) if len(v) >= 2 else np.nan)
    want = np.array(want)
    dist_d, h_dist = guard_in(dist, fill=ge.NAN, guard=ge.table_guard(m))
    sub_d, h_sub = guard_in(subsets.reshape(-1), fill=1, guard=ge.GUARD)
    out, h_out = guard_out((n_subsets,), guard=ge.GUARD)
    hip.call("ebn_ba_subset_sums_f32", P(dist_d), m, P(sub_d), k, n_subsets, P(out), S())
    torch.cuda.synchronize()
    for name, h in (("dist", h_dist), ("subsets", h_sub), ("out", h_out)):
        h.check(name)
    got = h_out.payload().cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert k == 1 or np.nanmax(np.abs(got - want)) <= 2.0 * 2.0 ** -20  # the bound of test_list_mean_and_subset_sums_through_the_abi


@pytest.mark.parametrize("transform", [0, 1], ids=["mean", "neg_log2"])
@pytest.mark.parametrize("last", [65, 0, 1], ids=lambda n: f"last{n}")
def test_list_mean_on_guarded_operands(hip, last, transform):
    rng = np.random.default_rng(3 + last)
    values = rng.uniform(1e-4, 1.0, N_ROWS).astype(np.float32)
    lengths = [n for n in (0, 1, 63, 64, 65) if n != last] + [last]
    lists = [rng.integers(0, N_ROWS, n) for n in lengths]
    lists[2][:3] = [0, N_ROWS, -1]
    lists[3][-1] = N_ROWS - 1
    if last:
        lists[-1][-1] = N_ROWS - 1
    want, scale = ge.list_mean_reference(values, lists, transform)
    ops = ge.ListOps(values, lists)
    hip.call("ebn_ba_list_mean_f32", P(ops.table), N_ROWS, P(ops.ids), ops.n_ids, P(ops.off), ops.n_lists, transform, P(ops.out), S())
    torch.cuda.synchronize()
    ge.check_list_values(ops, want, lambda got, ref: check_mean(got, ref, scale, f"list mean, transform {transform}, last length {last}"))
