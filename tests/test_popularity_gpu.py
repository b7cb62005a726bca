"""ebn_window_counts_i32 (csrc/ebn_popularity.hip) through the C ABI on guard-banded operands, against the brute force of
tests/popularity_cases.py, and the host classes on the device.

Every input sits inside poison (tests/guarded.py; the int64 operands as pairs of int32 words): event times of -2 (before every
window of the small cases, so an over-read would have to be counted by an unbounded window or shift a search), row / list offsets
of 0, rows of 1, list times of 0 -- values that are safe as addresses and wrong as results.  `counts` sits in a canary buffer with
ld = n_items + 3, pre-filled: the canaries and the padding columns survive, every payload element is written, and the counts
EQUAL the brute force as integers."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from tests import guarded
from tests import popularity_cases as pc

pytestmark = pytest.mark.gpu

OK, BAD_ARG = 0, -1
PAD = 3


def _guard_i64(x, fill):
    """an int64 operand as int32 words inside guards of `fill` words -> (device pointer, handle)"""
    words = np.ascontiguousarray(np.asarray(x, np.int64)).view(np.int32)
    view, h = guarded.guard_in(words, fill=fill)
    assert view.data_ptr() % 16 == 0
    return ctypes.c_void_p(view.data_ptr()), h


def _ages(max_ages):
    return [int(a) for a in max_ages] + [-1] * (8 - len(max_ages))  # the unused arguments are ignored, whatever they hold


def _run(hip, c, pad=PAD):
    """one guarded call -> counts [W, n] as a numpy array"""
    n, W = len(c["item_rows"]), len(c["max_ages"])
    ev, h_ev = _guard_i64(c["event_times"], -2)
    off, h_off = _guard_i64(c["row_offsets"], 0)
    loff, h_loff = _guard_i64(c["list_offsets"], 0)
    lt, h_lt = _guard_i64(c["list_times"], 0)
    rows, h_rows = guarded.guard_in(np.asarray(c["item_rows"], np.int32), fill=1)
    out, h_out = guarded.guard_out((W, n), ld=n + pad, dtype=torch.int32)
    rc = hip.lib().ebn_window_counts_i32(ev, off, len(c["row_offsets"]) - 1, hip.ptr(rows), n, loff, lt, len(c["list_times"]), W,
                                         *_ages(c["max_ages"]), c["min_age"], ctypes.c_void_p(out.data_ptr()), n + pad, hip.stream_handle())
    assert rc == OK, rc
    torch.cuda.synchronize()
    for h, what in ((h_ev, "event_times"), (h_off, "row_offsets"), (h_loff, "list_offsets"), (h_lt, "list_times"), (h_rows, "item_rows")):
        h.check(what)
    h_out.check("counts")
    return h_out.payload().cpu().numpy().reshape(W, n)


@pytest.mark.parametrize("name", pc.NAMES)
def test_counts_equal_the_brute_force(hip, name):
    c, want = pc.case(name)
    got = _run(hip, c)
    assert got.dtype == np.int32 and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} counts differ"


def test_two_runs_and_another_leading_dimension_give_the_same_counts(hip):
    c, want = pc.case("eight_windows")
    assert np.array_equal(_run(hip, c), want) and np.array_equal(_run(hip, c, pad=0), want) and np.array_equal(_run(hip, c, pad=61), want)


def test_argument_checks_return_codes_and_launch_nothing(hip):
    L = hip.lib()
    c, _ = pc.case("items_257")
    n, W, n_rows, n_lists = len(c["item_rows"]), 3, len(c["row_offsets"]) - 1, len(c["list_times"])
    ev, _h1 = _guard_i64(c["event_times"], -2)
    off, _h2 = _guard_i64(c["row_offsets"], 0)
    loff, _h3 = _guard_i64(c["list_offsets"], 0)
    lt, _h4 = _guard_i64(c["list_times"], 0)
    rows_t, _h5 = guarded.guard_in(np.asarray(c["item_rows"], np.int32), fill=1)
    rows = hip.ptr(rows_t)
    out, h_out = guarded.guard_out((8, n), ld=n + PAD, dtype=torch.int32)
    O, ld, st = ctypes.c_void_p(out.data_ptr()), n + PAD, hip.stream_handle()
    a = [30, 7, 60, 0, 0, 0, 0, 0]
    call = L.ebn_window_counts_i32
    before = L.ebn_launch_count()
    assert call(ev, off, n_rows, rows, n, loff, lt, n_lists, 0, *a, 0, O, ld, st) == BAD_ARG          # no window
    assert call(ev, off, n_rows, rows, n, loff, lt, n_lists, 9, *a, 0, O, ld, st) == BAD_ARG          # more than EBN_WC_MAX_WINDOWS
    assert call(ev, off, n_rows, rows, n, loff, lt, n_lists, -1, *a, 0, O, ld, st) == BAD_ARG
    assert call(ev, off, n_rows, rows, n, loff, lt, n_lists, W, *a, 0, O, n - 1, st) == BAD_ARG       # ld < n_items
    assert call(ev, off, n_rows, rows, -1, loff, lt, n_lists, W, *a, 0, O, ld, st) == BAD_ARG
    assert call(ev, off, n_rows, rows, n, loff, lt, -1, W, *a, 0, O, ld, st) == BAD_ARG
    assert call(ev, off, -1, rows, n, loff, lt, n_lists, W, *a, 0, O, ld, st) == BAD_ARG
    assert call(ev, off, n_rows, rows, n, loff, lt, 0, W, *a, 0, O, ld, st) == BAD_ARG                # items but no list
    assert call(ev, off, n_rows, rows, 2 ** 31, loff, lt, n_lists, W, *a, 0, O, 2 ** 31, st) == BAD_ARG
    assert call(ev, off, n_rows, rows, n, loff, lt, n_lists, W, *a, -1, O, ld, st) == BAD_ARG         # min_age < 0
    for w in range(W):
        bad = list(a)
        bad[w] = -1
        assert call(ev, off, n_rows, rows, n, loff, lt, n_lists, W, *bad, 0, O, ld, st) == BAD_ARG    # a max_age < 0
    assert call(None, off, n_rows, rows, n, loff, lt, n_lists, W, *a, 0, O, ld, st) == BAD_ARG
    assert call(ev, None, n_rows, rows, n, loff, lt, n_lists, W, *a, 0, O, ld, st) == BAD_ARG
    assert call(ev, off, n_rows, None, n, loff, lt, n_lists, W, *a, 0, O, ld, st) == BAD_ARG
    assert call(ev, off, n_rows, rows, n, None, lt, n_lists, W, *a, 0, O, ld, st) == BAD_ARG
    assert call(ev, off, n_rows, rows, n, loff, None, n_lists, W, *a, 0, O, ld, st) == BAD_ARG
    assert call(ev, off, n_rows, rows, n, loff, lt, n_lists, W, *a, 0, None, ld, st) == BAD_ARG
    assert call(None, None, 0, None, 0, None, None, 0, W, *a, 0, None, 0, st) == OK                   # no items: nothing to do
    assert call(ev, off, n_rows, rows, 0, loff, lt, n_lists, W, *a, 0, O, ld, st) == OK
    assert L.ebn_launch_count() == before
    torch.cuda.synchronize()
    h_out.check_untouched("counts")
    # a table without rows is a legal call: every item is unknown and counts 0, the event pointers are not needed
    assert call(None, None, 0, rows, n, loff, lt, n_lists, W, *a, 0, O, ld, st) == OK
    torch.cuda.synchronize()
    assert L.ebn_launch_count() == before + 1
    assert not h_out.payload()[:W].any() and bool((h_out.payload()[W:] == guarded.PREFILL_I32).all())


def test_recent_popularity_on_the_device_equals_the_host_path(hip):
    from pathlib import Path

    from ebrec.models import PopularityIndex, RecentPopularity

    golden = Path(__file__).resolve().parent / "golden" / "ebnerd"
    behaviors, history = pd.read_parquet(golden / "behaviors.parquet"), pd.read_parquet(golden / "history.parquet")
    windows = [pd.Timedelta(hours=1), pd.Timedelta(days=1), None, pd.Timedelta(hours=6)]
    for index in (PopularityIndex.from_behaviors(behaviors), PopularityIndex.from_history(history),
                  PopularityIndex.from_behaviors(behaviors, events="inviews")):
        dev = RecentPopularity(index, windows).counts(behaviors)
        host = RecentPopularity(index, windows, device=None).counts(behaviors)
        assert isinstance(dev.counts, torch.Tensor) and dev.counts.is_cuda and dev.counts.dtype == torch.int32
        assert isinstance(host.counts, np.ndarray) and host.counts.max() > 0
        assert np.array_equal(dev.counts.cpu().numpy(), host.counts) and np.array_equal(dev.offsets, host.offsets)
        s_dev, s_host = RecentPopularity(index, windows).predict(behaviors), RecentPopularity(index, windows, device=None).predict(behaviors)
        assert s_dev.flat.is_cuda and s_dev.flat.dtype == torch.float64 and np.array_equal(s_dev.host_flat(), s_host.flat)


def test_predict_feeds_the_device_evaluator(hip):
    from pathlib import Path

    from ebrec.evaluation import AucScore, DeviceMetricEvaluator, MetricEvaluator, MrrScore, NdcgScore, RaggedLists
    from ebrec.models import PopularityIndex, RecentPopularity

    golden = Path(__file__).resolve().parent / "golden" / "ebnerd"
    behaviors = pd.read_parquet(golden / "behaviors.parquet")
    index = PopularityIndex.from_behaviors(behaviors, events="inviews")
    scores = RecentPopularity(index, [pd.Timedelta(hours=1), pd.Timedelta(days=1), None]).predict(behaviors)
    labels = RaggedLists.from_lists([np.isin(v, c).astype(np.int64) for v, c in zip(behaviors["article_ids_inview"], behaviors["article_ids_clicked"])])
    keep = [l for l in range(len(labels)) if 0 < sum(labels.row(l)) < len(labels.row(l))]  # auc needs both classes
    assert len(keep) > 900
    y = RaggedLists.from_lists([np.asarray(labels.row(l)) for l in keep])
    p = RaggedLists.from_lists([np.asarray(scores.row(l)) for l in keep])
    metrics = [AucScore(), MrrScore(), NdcgScore(k=5), NdcgScore(k=10)]
    dev = DeviceMetricEvaluator(y, RaggedLists(torch.from_numpy(p.flat).cuda(), p.offsets), metrics).evaluate()
    host = MetricEvaluator(y.to_lists(), p.to_lists(), metrics).evaluate()
    assert dev.on_device and dev.n_host_fallback < len(keep)
    for name, v in host.evaluations.items():
        assert dev.evaluations[name] == pytest.approx(v, rel=1e-12, abs=1e-12), name
