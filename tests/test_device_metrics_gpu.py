"""Device path of the ranking metrics: ebn_rank_metrics / ebn_list_ranks through the C ABI, DeviceMetricEvaluator and
rank_predictions_by_score_ragged, against the REFERENCE's outputs (tests/golden/metrics_golden.json, ranking_golden.npz) and the
repository's host functions.

Bounds (derived, not measured).  Per-list values: rel 1e-12, the tolerance tests/test_evaluation.py uses for the host functions --
the device differs from the host by fp64 sums in another order and a device log2 / log / sqrt of a few ulps, about (k + 4) * 2^-52
per value.  Means over n lists: 1e-12 + n * 2^-53 relative (worst-case reordering of n non-negative terms).  Flags, counters, NaN
positions and ranks: exact."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import ranking_cases as rc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
G = json.loads((ROOT / "tests" / "golden" / "metrics_golden.json").read_text())
REL = 1e-12


def mean_tol(n):
    return REL + n * 2.0 ** -53


def run_kernel(labels, scores, offsets, slots=rc.SLOTS, form=0, per_list=True):
    import torch

    from ebrec.evaluation.device_metrics import rank_metrics_call
    from tests.hip_testutil import dev

    s = dev(scores, torch.float32 if scores.dtype == np.float32 else torch.float64)
    return rank_metrics_call(s, dev(labels, torch.uint8), dev(offsets, torch.int64), slots, form, per_list)


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 2.0 ** -1000)
    err[got[ok] == want[ok]] = 0.0
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: max rel err {worst:.3e} over {int(ok.sum())} values (bound {REL:.0e})")
    assert worst <= REL, what


def check_sums(sums, values, flags, what):
    """the kernel's sums against the fp64 sums of its own per-list contract: flagged lists and one-class lists left out"""
    n = values.shape[1]
    for m in range(values.shape[0]):
        use = (flags & 2) == 0
        if m in rc.RANKED_ROWS:
            use &= (flags & 1) == 0
        if m in rc.TWO_CLASS_ROWS:
            use &= ~np.isnan(values[m])
        want = float(np.sum(values[m][use]))
        if np.isnan(want):
            assert np.isnan(sums[m]), (what, m)
            continue
        err = abs(sums[m] - want) / max(abs(want), 2.0 ** -1000) if sums[m] != want else 0.0
        print(f"{what}: slot {rc.NAMES[m]} sum over {int(use.sum())} lists, rel err {err:.3e} (bound {mean_tol(n):.3e})")
        assert err <= mean_tol(n), (what, m)


# ---- 1. the evaluator against the existing golden ---------------------------------------------------------------------------
def test_evaluator_matches_the_reference_evaluator_on_the_300_golden_impressions(hip):
    from ebrec.evaluation import DeviceMetricEvaluator, RaggedLists

    before = hip.lib().ebn_launch_count()
    ev = DeviceMetricEvaluator(G["labels"], G["predictions"], rc.metrics())
    assert ev.evaluate(per_impression=True) is ev and ev.on_device
    assert hip.lib().ebn_launch_count() == before + 2, "one fused launch and its closing pass"
    assert list(ev.evaluations) == list(G["evaluations"])
    for name, want in G["evaluations"].items():
        print(f"{name}: {ev.evaluations[name]!r} vs reference {want!r}")
        assert ev.evaluations[name] == pytest.approx(want, rel=REL), name
    P, L = RaggedLists.from_lists(G["predictions"]), RaggedLists.from_lists(G["labels"])
    want_flags = rc.flags_numpy(L.flat, P.flat, L.offsets)
    assert np.array_equal(ev.flags, want_flags), "the flagged set is not the set of the definition"
    assert int((want_flags & 1).sum()) == 79 and ev.n_host_fallback == 79 and ev.n_impressions == 300
    assert ev.counters.tolist() == [0, 79, 0]
    for name in rc.NAMES:
        assert ev.sums[name] / 300 == ev.evaluations[name] and ev.per_impression[name].shape == (300,)
        assert float(np.sum(ev.per_impression[name])) / 300 == pytest.approx(G["evaluations"][name], rel=REL)
    close(ev.per_impression["auc"], G["per_row"]["roc_auc"], "per-impression auc vs reference rows")
    close(ev.per_impression["mrr"], G["per_row"]["mrr"], "per-impression mrr vs reference rows (tied rows from the host)")
    close(ev.per_impression["ndcg@10"], G["per_row"]["ndcg10"], "per-impression ndcg@10 vs reference rows")
    # without mrr / ndcg no list needs the host; the printed form is the host evaluator's
    from ebrec.evaluation import AucScore, MetricEvaluator, RootMeanSquaredError

    few = DeviceMetricEvaluator(G["labels"], G["predictions"], [AucScore(), RootMeanSquaredError()]).evaluate()
    assert few.n_host_fallback == 0 and few.evaluations["auc"] == pytest.approx(G["evaluations"]["auc"], rel=REL)
    host = MetricEvaluator(G["labels"], G["predictions"], [AucScore(), RootMeanSquaredError()]).evaluate()
    assert str(few).startswith("<MetricEvaluator class>: \n {") and str(few).count("\n") == str(host).count("\n")


# ---- 2. the kernel through the ABI ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_kernel_matches_the_reference_rows_in_both_forms(hip, kind):
    g = rc.load("main")
    labels, offsets, ref = g["labels"], g["offsets"], g["ref"]
    scores = g["scores"] if kind == "f32" else g["scores"].astype(np.float64)
    want_flags = rc.flags_numpy(labels, scores, offsets)
    plain = want_flags == 0
    out = {}
    for form in (0, 1):
        sums, flags, counters, values = run_kernel(labels, scores, offsets, form=form)
        assert np.array_equal(flags, want_flags), f"form {form}: flags"
        assert counters.tolist() == [0, int((want_flags & 1).sum()), 0], f"form {form}: counters"
        close(values[:, plain], ref[:, plain], f"{kind} form {form}: unflagged lists vs reference rows")
        rest = [m for m in range(8) if m not in rc.RANKED_ROWS]  # a tie does not touch these: every list
        close(values[rest], ref[rest], f"{kind} form {form}: auc / logloss / rmse / accuracy / f1 of every list")
        check_sums(sums, values, flags, f"{kind} form {form}")
        n_used = int(plain.sum())
        for m in range(8):  # the mean of the lists the device keeps against the reference's mean of the same lists
            use = plain if m in rc.RANKED_ROWS else np.ones_like(plain)
            want = float(np.mean(ref[m][use]))
            assert sums[m] / use.sum() == pytest.approx(want, rel=mean_tol(len(plain))), (form, m, n_used)
        out[form] = (sums, values)
    close(out[0][1], out[1][1], f"{kind}: form 0 vs form 1, every list")
    # without the per-list output the sums are the same bits
    sums_only = run_kernel(labels, scores, offsets, form=0, per_list=False)[0]
    assert np.array_equal(sums_only, out[0][0])


def test_one_class_lists_nan_positions_and_counters(hip):
    g = rc.load("one")
    n = len(g["offsets"]) - 1
    for form in (0, 1):
        sums, flags, counters, values = run_kernel(g["labels"], g["scores"], g["offsets"], form=form)
        assert counters.tolist() == [n, 0, 0] and not flags.any()
        close(values, g["ref"], f"one-class group, form {form}")
        assert np.isnan(values[list(rc.TWO_CLASS_ROWS)]).all()
        assert sums[0] == 0.0 and sums[4] == 0.0  # nothing is added to auc / logloss: the caller raises
        assert np.isnan(sums[1]) and np.isnan(sums[2])  # lists without a positive: NaN, as np.mean gives on the host
        check_sums(sums, values, flags, f"one-class group, form {form}")


def test_non_finite_scores_are_flagged_and_left_out(hip):
    g = rc.load("main")
    labels, scores, offsets = g["labels"].copy(), g["scores"].copy(), g["offsets"]
    lens = np.diff(offsets)
    hit = [int(np.flatnonzero(lens == n)[0]) for n in (2, 16, 17, 64, 65, 250, 1025, 5000)]
    for i, l in enumerate(hit):
        scores[offsets[l] + (i % lens[l])] = (np.nan, np.inf, -np.inf)[i % 3]
    want_flags = rc.flags_numpy(labels, scores, offsets)
    assert all(want_flags[l] & 2 for l in hit)
    for form in (0, 1):
        sums, flags, counters, values = run_kernel(labels, scores, offsets, form=form)
        assert np.array_equal(flags, want_flags)
        assert counters.tolist() == [0, int((want_flags & 1).sum()), len(hit)]
        check_sums(sums, values, flags, f"non-finite, form {form}")
    # the evaluator recomputes them on the host: same result as the host evaluator (rmse of a list with an inf is inf / nan there too)
    from ebrec.evaluation import AucScore, DeviceMetricEvaluator, MetricEvaluator, MrrScore, NdcgScore, RaggedLists

    fin = np.isnan(scores)
    scores[fin] = np.inf  # nan < x is False on both sides but np.argsort puts NaN last: keep to infinities for the comparison
    ms = [AucScore(), MrrScore(), NdcgScore(k=5)]
    ev = DeviceMetricEvaluator(RaggedLists(labels, offsets), RaggedLists(scores, offsets), ms).evaluate()
    host = MetricEvaluator([y.tolist() for y in rc.split(labels, offsets)], [s.astype(np.float64).tolist() for s in rc.split(scores, offsets)],
                           ms).evaluate()
    for name in ("auc", "mrr", "ndcg@5"):
        assert ev.evaluations[name] == pytest.approx(host.evaluations[name], rel=mean_tol(len(lens))), name


# ---- 3. float32 scores ------------------------------------------------------------------------------------------------------
def test_float32_scores_equal_the_host_evaluator_on_the_rounded_values(hip):
    from ebrec.evaluation import DeviceMetricEvaluator, MetricEvaluator, RaggedLists

    P32 = RaggedLists.from_lists([np.asarray(p, np.float32) for p in G["predictions"]])
    assert P32.flat.dtype == np.float32
    rounded = [np.asarray(p, np.float32).astype(np.float64).tolist() for p in G["predictions"]]
    host = MetricEvaluator(G["labels"], rounded, rc.metrics()).evaluate()
    before = P32.flat.copy()
    ev = DeviceMetricEvaluator(G["labels"], P32, rc.metrics()).evaluate()
    assert ev.on_device and np.array_equal(P32.flat, before)
    for name in rc.NAMES:
        print(f"{name}: {ev.evaluations[name]!r} vs host {host.evaluations[name]!r}")
        assert ev.evaluations[name] == pytest.approx(host.evaluations[name], rel=REL), name
    # device tensors are used in place
    import torch

    Pd = RaggedLists(torch.from_numpy(P32.flat).cuda(), P32.offsets)
    Ld = RaggedLists(torch.from_numpy(RaggedLists.from_lists(G["labels"]).flat).cuda(), P32.offsets)
    evd = DeviceMetricEvaluator(Ld, Pd, rc.metrics()).evaluate()
    assert evd.evaluations == ev.evaluations


# ---- 4. errors and routing --------------------------------------------------------------------------------------------------
def test_one_class_raises_custom_metrics_run_and_non_binary_labels_take_the_host(hip):
    from ebrec.evaluation import (AucScore, DeviceMetricEvaluator, LogLossScore, MetricEvaluator, MrrScore, RootMeanSquaredError)

    labels, preds = [[1, 0, 0], [0, 0, 0], [0, 1]], [[0.2, 0.3, 0.5], [0.1, 0.7, 0.2], [0.4, 0.6]]
    with pytest.raises(ValueError, match="Only one class present"):
        DeviceMetricEvaluator(labels, preds, [MrrScore(), AucScore()]).evaluate()
    with pytest.raises(ValueError, match="only one label"):
        DeviceMetricEvaluator(labels, preds, [LogLossScore()]).evaluate()
    ok = DeviceMetricEvaluator(labels, preds, [RootMeanSquaredError()]).evaluate()
    assert ok.on_device and ok.evaluations["rmse"] == pytest.approx(MetricEvaluator(labels, preds, [RootMeanSquaredError()]).evaluate().evaluations["rmse"], rel=REL)

    class Longest:
        name = "longest"

        def __call__(self, y_true, y_pred):
            assert isinstance(y_pred, list) and isinstance(y_pred[0], list)
            return max(len(p) for p in y_pred)

    class MyAuc(AucScore):
        def calculate(self, y_true, y_pred):
            return 42.0

    ev = DeviceMetricEvaluator(G["labels"], G["predictions"], [AucScore(), Longest(), MyAuc()]).evaluate()
    assert list(ev.evaluations) == ["auc", "longest"] and ev.evaluations["longest"] == 250
    assert ev.evaluations["auc"] == 42.0 and list(ev.sums) == ["auc"]  # same name: the later metric wins, as in the host evaluator
    # labels outside {0, 1}: the host evaluator decides
    l3, p3 = [[2, 0, 1], [1, 0]], [[0.2, 0.3, 0.5], [0.4, 0.6]]
    ms = [MrrScore(), RootMeanSquaredError()]
    ev3 = DeviceMetricEvaluator(l3, p3, ms).evaluate()
    assert not ev3.on_device and ev3.evaluations == MetricEvaluator(l3, p3, ms).evaluate().evaluations
    assert DeviceMetricEvaluator([], [], ms).evaluate().n_impressions == 0


# ---- 5. ranks ---------------------------------------------------------------------------------------------------------------
def test_list_ranks_equal_the_host_function_list_by_list(hip):
    import torch

    from ebrec.evaluation.device_metrics import list_ranks_call
    from ebrec.utils._python import rank_predictions_by_score, rank_predictions_by_score_ragged
    from tests.hip_testutil import dev

    g = rc.load("main")
    offsets = g["offsets"]
    for scores in (g["scores"], g["scores"].astype(np.float64)):
        lists = rc.split(scores, offsets)
        tied = np.array([len(np.unique(s)) < len(s) for s in lists])
        assert 0.05 < tied.mean() < 0.5
        want = [rank_predictions_by_score(s) for s in lists]
        for form in (0, 1):
            ranks, flags = list_ranks_call(dev(scores, torch.float32 if scores.dtype == np.float32 else torch.float64), dev(offsets, torch.int64), form)
            assert ranks.dtype == np.int32 and np.array_equal(flags != 0, tied), f"form {form}: exactly the tied lists are flagged"
            for l, r in enumerate(rc.split(ranks, offsets)):
                assert np.array_equal(r, want[l]) if not tied[l] else not r.any(), (form, l)
        for got in (rank_predictions_by_score_ragged(scores, offsets), rank_predictions_by_score_ragged(lists)):
            assert len(got) == len(want) and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    s = np.array([0.5, np.nan, 0.1, 0.7, 0.2], np.float32)
    ranks, flags = list_ranks_call(dev(s, torch.float32), dev(np.array([0, 3, 5]), torch.int64))
    assert flags.tolist() == [2, 0] and ranks.tolist() == [0, 0, 0, 1, 2]
    got = rank_predictions_by_score_ragged([[0.2, 0.9], [], [0.3]])
    assert [r.tolist() for r in got] == [[2, 1], [], [1]]


# ---- 6. ABI edges -----------------------------------------------------------------------------------------------------------
def test_abi_edges_empty_calls_bad_offsets_and_bad_arguments(hip):
    import torch

    from tests.hip_testutil import P, S, dev

    lib = hip.lib()
    f32 = dev(np.array([0.9, 0.1, 0.5, 0.3, 0.7, 0.2, 0.8, 0.4]), torch.float32)
    u8 = dev(np.array([1, 0, 0, 0, 1, 0, 0, 1]), torch.uint8)
    kinds, params = dev(np.array([k for k, _ in rc.SLOTS]), torch.int32), dev(np.array([p for _, p in rc.SLOTS]), torch.float64)
    sums, counters = torch.full((8,), -7.0, dtype=torch.float64, device="cuda"), torch.full((3,), -7, dtype=torch.int64, device="cuda")
    flags, ranks = torch.full((4,), 9, dtype=torch.uint8, device="cuda"), torch.full((8,), -7, dtype=torch.int32, device="cuda")
    vals = torch.full((8, 3), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")
    off = dev(np.array([0, 5, 3, 100]), torch.int64)  # list 1 runs backwards, list 2 leaves the arrays: both are empty
    assert lib.ebn_rank_metrics_workspace_bytes(0) == 0 and lib.ebn_rank_metrics_workspace_bytes(-1) == 0
    assert lib.ebn_rank_metrics_workspace_bytes(3) == 16 * 8 + 3 * 8 and lib.ebn_rank_metrics_workspace_bytes(257) == 2 * (16 * 8 + 3 * 8)
    torch.cuda.synchronize()
    before = lib.ebn_launch_count()
    assert lib.ebn_rank_metrics(P(f32), 0, P(u8), 8, P(off), 0, P(kinds), P(params), 8, 0, P(sums), P(flags), P(counters), None, P(ws), 4096, S()) == 0
    assert lib.ebn_rank_metrics(None, 1, None, 0, None, 0, None, None, 0, 0, None, None, None, None, None, 0, S()) == 0
    assert lib.ebn_list_ranks(P(f32), 0, 8, P(off), 0, 0, P(ranks), P(flags), S()) == 0
    assert lib.ebn_list_ranks(None, 0, 0, None, 0, 1, None, None, S()) == 0
    assert lib.ebn_launch_count() == before, "an empty call launched a kernel"
    torch.cuda.synchronize()
    assert sums.tolist() == [-7.0] * 8 and flags.tolist() == [9] * 4
    bad = [lambda: lib.ebn_rank_metrics(P(f32), 0, P(u8), -1, P(off), 3, P(kinds), P(params), 8, 0, P(sums), P(flags), P(counters), None, P(ws), 4096, S()),
           lambda: lib.ebn_rank_metrics(P(f32), 0, P(u8), 8, P(off), -1, P(kinds), P(params), 8, 0, P(sums), P(flags), P(counters), None, P(ws), 4096, S()),
           lambda: lib.ebn_rank_metrics(P(f32), 0, P(u8), 8, P(off), 3, P(kinds), P(params), 17, 0, P(sums), P(flags), P(counters), None, P(ws), 4096, S()),
           lambda: lib.ebn_rank_metrics(P(f32), 0, P(u8), 8, P(off), 3, P(kinds), P(params), -1, 0, P(sums), P(flags), P(counters), None, P(ws), 4096, S()),
           lambda: lib.ebn_rank_metrics(P(f32), 0, P(u8), 8, P(off), 3, P(kinds), P(params), 8, 2, P(sums), P(flags), P(counters), None, P(ws), 4096, S()),
           lambda: lib.ebn_rank_metrics(P(f32), 2, P(u8), 8, P(off), 3, P(kinds), P(params), 8, 0, P(sums), P(flags), P(counters), None, P(ws), 4096, S()),
           lambda: lib.ebn_rank_metrics(None, 0, P(u8), 8, P(off), 3, P(kinds), P(params), 8, 0, P(sums), P(flags), P(counters), None, P(ws), 4096, S()),
           lambda: lib.ebn_rank_metrics(P(f32), 0, P(u8), 8, None, 3, P(kinds), P(params), 8, 0, P(sums), P(flags), P(counters), None, P(ws), 4096, S()),
           lambda: lib.ebn_rank_metrics(P(f32), 0, P(u8), 8, P(off), 3, None, P(params), 8, 0, P(sums), P(flags), P(counters), None, P(ws), 4096, S()),
           lambda: lib.ebn_rank_metrics(P(f32), 0, P(u8), 8, P(off), 3, P(kinds), P(params), 8, 0, None, P(flags), P(counters), None, P(ws), 4096, S()),
           lambda: lib.ebn_rank_metrics(P(f32), 0, P(u8), 8, P(off), 3, P(kinds), P(params), 8, 0, P(sums), P(flags), P(counters), None, None, 4096, S()),
           lambda: lib.ebn_rank_metrics(P(f32), 0, P(u8), 8, P(off), 3, P(kinds), P(params), 8, 0, P(sums), P(flags), P(counters), None, P(ws), 151, S()),
           lambda: lib.ebn_list_ranks(P(f32), 0, -1, P(off), 3, 0, P(ranks), P(flags), S()),
           lambda: lib.ebn_list_ranks(P(f32), 0, 8, P(off), -1, 0, P(ranks), P(flags), S()),
           lambda: lib.ebn_list_ranks(P(f32), 0, 8, P(off), 3, 3, P(ranks), P(flags), S()),
           lambda: lib.ebn_list_ranks(P(f32), 5, 8, P(off), 3, 0, P(ranks), P(flags), S()),
           lambda: lib.ebn_list_ranks(P(f32), 0, 8, None, 3, 0, P(ranks), P(flags), S()),
           lambda: lib.ebn_list_ranks(P(f32), 0, 8, P(off), 3, 0, None, P(flags), S())]
    for i, call in enumerate(bad):
        assert call() == -1, i
    assert lib.ebn_launch_count() == before, "a rejected call launched a kernel"
    # untrusted offsets: the intact list is computed, the other two are empty (NaN values, one class, ranks untouched)
    for form in (0, 1):
        hip.call("ebn_rank_metrics", P(f32), 0, P(u8), 8, P(off), 3, P(kinds), P(params), 8, form, P(sums), P(flags), P(counters), P(vals), P(ws), 4096, S())
        hip.call("ebn_list_ranks", P(f32), 0, 8, P(off), 3, form, P(ranks), P(flags[1:]), S())
        torch.cuda.synchronize()
        v = vals.cpu().numpy()
        want = np.array(rc.counting_values([1, 0, 0, 0, 1], np.array([0.9, 0.1, 0.5, 0.3, 0.7], np.float32)))
        close(v[:, 0], want, f"the intact list, form {form}")
        assert np.isnan(v[:7, 1:]).all() and np.all(v[7, 1:] == 0.0)  # f1 of nothing is 0.0, everything else is undefined
        assert counters.tolist() == [2, 0, 0] and flags.tolist() == [0, 0, 0, 0]
        assert ranks.tolist() == [1, 5, 3, 4, 2, -7, -7, -7]
        assert sums[0].item() == v[0, 0] and np.isnan(sums[1].item()) and sums[7].item() == v[7, 0]
    # zero slots: flags and counters only; zero candidates under non-empty offsets
    hip.call("ebn_rank_metrics", P(f32), 0, P(u8), 8, P(off), 3, None, None, 0, 0, None, P(flags), P(counters), None, P(ws), 4096, S())
    zero = dev(np.zeros(4), torch.int64)
    hip.call("ebn_rank_metrics", None, 0, None, 0, P(zero), 3, P(kinds), P(params), 8, 0, P(sums), P(flags), P(counters), None, P(ws), 4096, S())
    torch.cuda.synchronize()
    assert counters.tolist() == [3, 0, 0]
    # a non-default stream computes the same bits
    g = rc.load("main")
    base = run_kernel(g["labels"], g["scores"], g["offsets"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = run_kernel(g["labels"], g["scores"], g["offsets"])
    side.synchronize()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(base, other))


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_a_subsample_matches_the_host(hip):
    from ebrec.evaluation import DeviceMetricEvaluator, MetricEvaluator, RaggedLists

    labels, scores, offsets = rc.synthetic(200_000, seed=7)
    scores[::13] = np.round(scores[::13], 1)  # some ties, some of them ambiguous
    runs = [run_kernel(labels, scores, offsets, per_list=False) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes(), "two runs over the same input differ in their sums"
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    assert runs[0][2][0] == 0 and 0 < runs[0][2][1] < 20_000 and np.isfinite(runs[0][0]).all()
    n = 20_000
    o = offsets[:n + 1]
    ms = [m for m in rc.metrics()]
    ev = DeviceMetricEvaluator(RaggedLists(labels[:o[-1]], o), RaggedLists(scores[:o[-1]], o), ms).evaluate()
    host = MetricEvaluator([y.tolist() for y in rc.split(labels, o)], [s.astype(np.float64).tolist() for s in rc.split(scores, o)], rc.metrics()).evaluate()
    assert 0 < ev.n_host_fallback < n // 10
    for name in rc.NAMES:
        print(f"{name}: device {ev.evaluations[name]!r} host {host.evaluations[name]!r}")
        assert ev.evaluations[name] == pytest.approx(host.evaluations[name], rel=mean_tol(n)), name


# ---- 8. the driver ----------------------------------------------------------------------------------------------------------
def test_ebnerd_nrms_driver_with_device_metrics(hip, tmp_path):
    sys.path.insert(0, str(ROOT / "tools"))
    sys.path.insert(0, str(ROOT / "examples" / "reproducibility_scripts"))
    import ebnerd_nrms
    import pandas as pd
    from make_synthetic_ebnerd import make

    from ebrec.utils._python import rank_predictions_by_score

    data = make(tmp_path / "data", split="ebnerd_demo", n_impressions=500, n_users=40, n_articles=300, seed=1)
    dump = tmp_path / "out"
    before = hip.lib().ebn_launch_count()
    hist, metrics = ebnerd_nrms.main(["--data_path", str(data), "--datasplit", "ebnerd_demo", "--epochs", "2", "--bs_train", "32",
                                      "--n_chunks_test", "3", "--tokenizer", "hash", "--vocab_size", "500", "--word_emb_dim", "64",
                                      "--learning_rate", "1e-3", "--dump_dir", str(dump), "--device_metrics"])
    assert hip.lib().ebn_launch_count() > before
    assert set(metrics) == {"auc", "mrr", "ndcg@5", "ndcg@10"} and all(0.0 <= v <= 1.0 for v in metrics.values())
    out = pd.read_parquet(next(dump.rglob("test_predictions.parquet")))
    assert len(out) > 0 and any(len(r) == 250 for r in out["ranked_scores"])
    for s, r in zip(out["scores"], out["ranked_scores"]):
        assert np.array_equal(np.asarray(r), rank_predictions_by_score(np.asarray(s))), "ranked_scores is not the rank of scores"
    assert len(list(dump.rglob("NRMSModel-123-ebnerd_demo.zip"))) == 1
