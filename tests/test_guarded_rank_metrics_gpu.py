"""ebn_rank_metrics (f32 and f64 scores, form 0 and 1, with and without per_list) and ebn_list_ranks on guard-banded operands
(tests/guarded_eval.py): f32 scores in NaN, f64 scores as int32 word pairs inside 0x7FF00000 words (two of them are a NaN: an
over-read score raises flag bit 1), the uint8 labels packed four to an int32 word inside 0x01010101 (an over-read label is a
positive), the int64 offsets inside zero words (an over-read offset makes a list run backwards), sums / counters / per_list /
flags / ranks in canaries with a pre-filled payload, the flags -- a BYTE array -- with the unused bytes of their last word
compared by hand, the workspace poisoned, in canaries and passed at EXACTLY ebn_rank_metrics_workspace_bytes(n_lists).

Every case holds all sixteen list lengths on both sides of the four forms (<= 16, <= 64, LDS-resident <= 1024, tiled); the case
decides which form owns the LAST list, the one that ends at n_items, and n_lists of 255, 256, 257 sit on both sides of a
workgroup of 256 lists.  References: ranking_cases.counting_values / flags_numpy and rank_predictions_by_score under the existing
REL / mean_tol (close, check_sums of tests/test_device_metrics_gpu.py).  tests/test_guarded_eval_cpu.py plants the defects."""
import functools

import numpy as np
import pytest
import torch

from tests import guarded_eval as ge
from tests.hip_testutil import P, S

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500]
# (n_lists, length of the last list): the 16-lane form, the tiled form, the LDS-resident form, one wave, the 16-lane form again
CASES = [(1, 16), (1, 2500), (255, 2500), (256, 1024), (257, 64), (301, 15)]


@functools.lru_cache(maxsize=None)
def case(n_lists, last):
    """-> (labels, scores float32, offsets, reference): `last` at the end, the other fifteen lengths permuted in front of it
    behind short filler lists; computed once, shared by every run, left unchanged"""
    rng = np.random.default_rng(n_lists + last)
    if n_lists == 1:
        lens = [last]
    else:
        rest = [n for n in LENGTHS if n != last]
        assert len(rest) == 15
        lens = rng.integers(0, 21, n_lists - 16).tolist() + rng.permutation(rest).tolist() + [last]
    assert len(lens) == n_lists and lens[-1] == last
    labels, scores, off = ge.rank_case(lens, seed=n_lists)
    for a in (labels, scores, off):
        a.setflags(write=False)
    return labels, scores, off, ge.rank_reference(labels, scores, off)


def call_metrics(hip, ops, form):
    hip.call("ebn_rank_metrics", P(ops.scores), 1 if ops.f64 else 0, P(ops.labels), ops.n_items, P(ops.off), ops.n_lists, P(ops.kinds),
             P(ops.params), ops.n_slots, form, P(ops.sums), P(ops.flags), P(ops.counters), P(ops.per_list), P(ops.ws), ops.ws_bytes, S())
    torch.cuda.synchronize()


@pytest.mark.parametrize("n_lists,last", CASES, ids=lambda v: str(v))
def test_rank_metrics_on_guarded_operands(hip, n_lists, last):
    labels, scores, off, ref = case(n_lists, last)
    ws_bytes = int(hip.lib().ebn_rank_metrics_workspace_bytes(n_lists))
    assert ws_bytes == -(-n_lists // 256) * (16 * 8 + 3 * 8)
    assert (n_lists % 4 != 0) or n_lists == 256, "the flags end inside a word in every case but the one on the workgroup edge"
    sums = {}
    for f64 in (False, True):
        for form in (0, 1):
            for per_list in (True, False):
                ops = ge.RankOps(labels, scores, off, ws_bytes, f64=f64, per_list=per_list)
                call_metrics(hip, ops, form)
                what = f"{n_lists} lists, last {last}, {'f64' if f64 else 'f32'}, form {form}, per_list {per_list}"
                sums[f64, form, per_list] = ge.check_metric_result(ops, ref, what)
            assert sums[f64, form, True].tobytes() == sums[f64, form, False].tobytes(), "the sums depend on per_list"


@pytest.mark.parametrize("n_lists,last", CASES, ids=lambda v: str(v))
def test_list_ranks_on_guarded_operands(hip, n_lists, last):
    labels, scores, off, _ = case(n_lists, last)
    for f64 in (False, True):
        for form in (0, 1):
            ops = ge.RankOps(labels, scores, off, 152, f64=f64, per_list=False)
            hip.call("ebn_list_ranks", P(ops.scores), 1 if f64 else 0, ops.n_items, P(ops.off), n_lists, form, P(ops.ranks), P(ops.rank_flags), S())
            torch.cuda.synchronize()
            ge.check_rank_result(ops, labels, scores, off, f"{n_lists} lists, last {last}, {'f64' if f64 else 'f32'}, form {form}")
