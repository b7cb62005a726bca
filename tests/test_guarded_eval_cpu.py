"""Proof, without a GPU, that the guarded tests of the evaluation and re-ranking kernels would fail on the errors they exist to
find.  The operands are the ones of tests/test_guarded_rerank_gpu.py, tests/test_guarded_beyond_gpu.py and
tests/test_guarded_rank_metrics_gpu.py built on the host (tests/guarded_eval.py, device="cpu"); a numpy stand-in of each kernel
family's index walk runs over them as C sees them (Handle.raw()); the result goes through the SAME check_* helpers the GPU tests
call.  The clean stand-in passes; each planted defect raises.  No GPU code is made to misbehave.

One limit, the harness's own (tests/guarded.py): a read whose value is discarded cannot be seen.  The pool of the missing user of a
half-empty workgroup is such a read when only the loads lose their `u < U` guard; the stand-in has ONE guard for a user's
loads and stores, and the planted defect drops it: the phantom user's pool is walked and its picks land behind out_sel."""
import numpy as np
import pytest
import torch

from tests import guarded_eval as ge
from tests import ranking_cases as rc
from tests import rerank_cases as rr
from tests.guarded import CANARY, PREFILL_I32
from tests.test_beyond_accuracy_gpu import check_mean

LAM = 0.5
POOL_DEFECTS = ["pool_entry_P", "phantom_user", "table_round32", "store_k_plus_1", "flags2"]
# (U, P, D, k): two users per workgroup with the last workgroup half empty and D off the 32-deep slab; one user per workgroup
POOL_SHAPES = [(3, 31, 36, 5), (2, 33, 36, 10)]


def _pool(shape, defect, off=0):
    U, P, D, k = shape
    unit, rows, rel = ge.name_both_ends(*rr.exact_case(U, P, D, seed=U + P))
    want = rr.mmr_reference(unit, rows, rel, k, LAM)
    ops = ge.PoolOps(unit, rows, rel, k, device="cpu", off=off)
    ge.standin_mmr(ops, LAM, defect)
    ge.check_pool_result(ops, want[2], want=want[:2])


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("shape", POOL_SHAPES + [(1, 1, 4, 1), (2, 5, 8, 64)], ids=lambda s: "x".join(map(str, s)))
def test_the_clean_pool_walk_passes(shape, off):
    _pool(shape, None, off)


# one user per workgroup (P > 32) has no half-empty workgroup: the phantom user is planted at two users per workgroup only
@pytest.mark.parametrize("shape,defect", [(s, d) for s in POOL_SHAPES for d in POOL_DEFECTS if d != "phantom_user" or s[1] <= 32],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_every_planted_pool_defect_is_caught(shape, defect):
    with pytest.raises(AssertionError):
        _pool(shape, defect)


def test_the_pool_defects_are_caught_by_the_means_the_guards_promise():
    """entry P of the LAST user is the guard: relevance 3e18 on a valid row wins round 0 (a pick >= P); the rounded-up last table
    row reads NaN (flags[1]); k + 1 stores and flags[2] disturb a canary"""
    shape = (2, 33, 36, 10)
    for defect, match in (("pool_entry_P", "a pick outside the pool"), ("table_round32", "flags"), ("store_k_plus_1", "out_sel.*canary.*behind"),
                          ("flags2", "flags.*canary.*behind")):
        with pytest.raises(AssertionError, match=match):
            _pool(shape, defect)
    with pytest.raises(AssertionError, match="out_sel.*canary.*behind"):
        _pool((3, 31, 36, 5), "phantom_user")


def test_the_float32_walk_tells_exact_cases_from_rounded_ones():
    unit, rows, rel = ge.name_both_ends(*rr.exact_case(3, 32, 36, seed=1))
    assert ge.mmr_float32_equals(unit, rows, rel, 5, 0.25, rr.mmr_reference(unit, rows, rel, 5, 0.25))
    unit, rows, rel = ge.name_both_ends(*rr.rounded_case(3, 32, 36, seed=1))
    want = rr.mmr_reference(unit, rows, rel, 32, 0.3)
    assert not np.array_equal(want[1], want[1].astype(np.float32)) and not ge.mmr_float32_equals(unit, rows, rel, 32, 0.3, want)


# ------------------------------------------------------------------------------------------------ id lists
def _list_mean(defect, transform=0, last=17):
    rng = np.random.default_rng(5)
    values = rng.uniform(0.1, 1.0, 40).astype(np.float32)
    lists = [rng.integers(0, 40, n) for n in (0, 1, 63, 64, 65, 10, last)]
    ops = ge.ListOps(values, lists, device="cpu")
    ge.standin_list_mean(ops, transform, defect)
    want, scale = ge.list_mean_reference(values, lists, transform)
    ge.check_list_values(ops, want, lambda got, ref: check_mean(got, ref, scale, "stand-in list mean"))


@pytest.mark.parametrize("transform", [0, 1])
def test_the_clean_id_walk_passes_and_an_id_read_past_the_end_is_caught(transform):
    _list_mean(None, transform)
    with pytest.raises(AssertionError):
        _list_mean("id_past_end", transform)


def test_an_offset_read_past_the_end_runs_backwards():
    """the int64 offsets sit inside zero words: offsets[n_lists + 1] is 0, below the last list's end"""
    ops = ge.ListOps(np.ones(4, np.float32), [[0, 1], [2]], device="cpu")
    off = ge.raw_as(ops.h["offsets"], np.int64)
    assert off[:3].tolist() == [0, 2, 3] and off[3] == 0 and ge.raw_as(ops.h["ids"], np.int32)[:5].tolist() == [0, 1, 2, 1, 1]


# ------------------------------------------------------------------------------------------------ ranking metrics
RANK_LENS = [5, 16, 0, 17, 2, 64, 1, 15, 65, 300, 16]  # the last list, of the 16-lane form, ends at n_items


def _rank(defect, n_lists=len(RANK_LENS)):
    lens = (RANK_LENS * (n_lists // len(RANK_LENS) + 1))[-n_lists:]
    labels, scores, off = ge.rank_case(lens, seed=2)
    blocks = -(-n_lists // ge.RM_LPB)
    ops = ge.RankOps(labels, scores, off, ws_bytes=blocks * (16 * 8 + 3 * 8), device="cpu")
    ge.standin_rank_metrics(ops, defect)
    ge.check_metric_result(ops, ge.rank_reference(labels, scores, off), "stand-in")


@pytest.mark.parametrize("n_lists", [len(RANK_LENS), 257])
def test_the_clean_rank_metrics_walk_passes(n_lists):
    _rank(None, n_lists)


@pytest.mark.parametrize("defect", ["short_reads_16", "workspace_one_more"])
def test_every_planted_rank_metrics_defect_is_caught(defect):
    with pytest.raises(AssertionError):
        _rank(defect)


def test_the_rank_metrics_defects_are_caught_by_the_means_the_guards_promise():
    with pytest.raises(AssertionError, match="workspace.*canary.*behind"):
        _rank("workspace_one_more", 257)
    labels, scores, off = ge.rank_case([3, 16, 5], seed=1, ties=())
    ops = ge.RankOps(labels, scores, off, ws_bytes=152, device="cpu")
    ge.standin_rank_metrics(ops, "short_reads_16")
    assert ops.metric_results()[1].tolist() == [0, 0, 2], "only the last list reads the NaN behind the scores"
    ge.check_byte_tail(ops.h["flags"], 3, "flags")
    ge.raw_as(ops.h["flags"], np.uint8)[3] = 0  # byte 3 of the flags' only word: a flag stored for one list too many
    with pytest.raises(AssertionError, match="bytes behind element 2"):
        ge.check_byte_tail(ops.h["flags"], 3, "flags")


# ------------------------------------------------------------------------------------------------ the word views
def test_word_views_of_byte_int64_and_float64_operands():
    lab, h = ge.words_in(np.array([1, 0, 1, 0, 0, 1], np.uint8), ge.LABEL_WORD, device="cpu")
    assert lab.dtype == torch.int32 and lab.numel() == 2 and lab.data_ptr() % 16 == 0
    raw = ge.raw_as(h, np.uint8)
    assert raw[:6].tolist() == [1, 0, 1, 0, 0, 1] and (raw[6:64] == 1).all()
    flat, start = h.raw()
    assert (flat[:start] == ge.LABEL_WORD).all()
    s, hs = ge.words_in(np.array([0.25, 0.5]), ge.F64_NAN_WORD, device="cpu")
    d = ge.raw_as(hs, np.float64)
    assert d[:2].tolist() == [0.25, 0.5] and np.isnan(d[2:10]).all() and s.data_ptr() % 16 == 0
    assert ge.read_words(hs, np.float64, 2).tolist() == [0.25, 0.5]
    o, ho = ge.words_out(5, device="cpu")
    assert o.numel() == 2
    with pytest.raises(AssertionError, match="never written"):
        ho.check("bytes")
    ge.raw_as(ho, np.uint8)[:5] = 0
    ho.check("bytes")
    ge.check_byte_tail(ho, 5, "bytes")
    assert ge.read_words(ho, np.uint8, 8).tolist() == [0] * 5 + [PREFILL_I32 & 0xFF] * 3
    ge.raw_as(ho, np.uint8)[8] = 0
    with pytest.raises(AssertionError, match="behind the operand"):
        ho.check("bytes")
    f, hf = ge.zeroed_flags(2, "cpu")
    assert f.tolist() == [0, 0]
    hf.check("flags")
    flat, start = hf.raw()
    assert flat[start + 2] == np.array([CANARY], np.uint32).view(np.int32)[0]
    flat[start + 1] = 1
    hf.check("flags")
