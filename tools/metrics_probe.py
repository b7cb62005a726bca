"""Times the ranking-metric kernel and the device evaluator at the me-c1 shape on one GPU.

me-c1: 1 000 000 impressions, in-view lengths 4 + geometric with mean about 11.6, 0.2 % of the lists 250
long (beyond-accuracy rows), one positive per list, float32 scores.  Reported:
  * the kernel alone (HIP events around `--reps` back-to-back ebn_rank_metrics calls after warm-up calls, inputs already on the
    device) for the four driver metrics [auc, mrr, ndcg@5, ndcg@10] and for all eight slots, and ebn_list_ranks;
  * "input bytes" = what the algorithm has to read once: 5 bytes per candidate (fp32 score, uint8 label) + 8 per list (offset),
    as bytes / kernel time, next to this box's float4-copy calibration measured in the same run (the library's gather kernel
    over the identity permutation of 4 KB rows, 1 GiB, (read + write bytes) / time);
  * DeviceMetricEvaluator end to end from RaggedLists over host arrays (upload, kernel, download, host recomputation of flagged
    lists) and from nested Python lists (flattening included), and rank_predictions_by_score_ragged from flat arrays;
  * the HOST evaluator of this package (the reference's per-impression form) in the same run on the first `--host-lists` lists.
Prints ONE JSON line; asserts only that both end-to-end device figures beat the host figure.
usage: metrics_probe.py [--lists N] [--reps K] [--warmup W] [--host-lists M]"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec import _hip  # noqa: E402
from ebrec.evaluation import (AccuracyScore, AucScore, DeviceMetricEvaluator, F1Score, LogLossScore, MetricEvaluator, MrrScore,  # noqa: E402
                              NdcgScore, RaggedLists, RootMeanSquaredError)
from ebrec.utils._python import rank_predictions_by_score, rank_predictions_by_score_ragged  # noqa: E402

DRIVER_SLOTS = [(0, 0.0), (1, 0.0), (2, 5.0), (2, 10.0)]
ALL_SLOTS = DRIVER_SLOTS + [(3, 0.0), (4, 0.0), (5, 0.5), (6, 0.5)]


def driver_metrics():
    return [AucScore(), MrrScore(), NdcgScore(k=5), NdcgScore(k=10)]


def all_metrics():
    return driver_metrics() + [LogLossScore(), RootMeanSquaredError(), AccuracyScore(threshold=0.5), F1Score(threshold=0.5)]


def make_lists(n_lists, seed=0, long_share=0.002):
    rng = np.random.default_rng(seed)
    lens = np.minimum(4 + rng.geometric(1 / 7.6, n_lists), 100)
    lens[rng.random(n_lists) < long_share] = 250
    offsets = np.zeros(n_lists + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    scores = rng.random(int(offsets[-1]), dtype=np.float32)
    labels = np.zeros(int(offsets[-1]), np.uint8)
    labels[offsets[:-1] + (rng.random(n_lists) * lens).astype(np.int64)] = 1
    return labels, scores, offsets


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def float4_copy_gbs(reps):
    n = (1 << 30) // 4
    src, dst = torch.empty(n, device="cuda").normal_(), torch.empty(n, device="cuda")
    rows = n // 1024
    ids = torch.arange(rows, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    fn = lambda: _hip.call("ebn_gather_rows_f32", _hip.ptr(ids), _hip.ptr(src), _hip.ptr(dst), rows, 1024, rows, None, -1,
                           ctypes.c_float(0.0), _hip.ptr(flag), _hip.stream_handle())
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = events_ms(fn, reps)
    return (2.0 * n * 4 + rows * 4) / ms / 1e6


def timed(fn):
    t0 = time.perf_counter()
    out = fn()  # every call ends in a device-to-host copy: synchronised
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-lists", type=int, default=20_000)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    labels, scores, offsets = make_lists(a.lists)
    n_items = int(offsets[-1])
    input_bytes = 5 * n_items + 8 * (a.lists + 1)
    S, P = _hip.stream_handle, _hip.ptr
    d_s, d_y, d_o = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(offsets).cuda()
    sums, counters = torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
    flags, ranks = torch.zeros(a.lists, dtype=torch.uint8, device="cuda"), torch.zeros(n_items, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(_hip.lib().ebn_rank_metrics_workspace_bytes(a.lists)), dtype=torch.uint8, device="cuda")
    res = {}

    def kernel(slots, form=0):
        kinds = torch.tensor([k for k, _ in slots], dtype=torch.int32, device="cuda")
        params = torch.tensor([p for _, p in slots], dtype=torch.float64, device="cuda")
        return lambda: _hip.call("ebn_rank_metrics", P(d_s), 0, P(d_y), n_items, P(d_o), a.lists, P(kinds), P(params), len(slots), form,
                                 P(sums), P(flags), P(counters), None, P(ws), ws.numel(), S())

    cases = [("kernel_driver_metrics", kernel(DRIVER_SLOTS)), ("kernel_all_eight", kernel(ALL_SLOTS)),
             ("kernel_list_ranks", lambda: _hip.call("ebn_list_ranks", P(d_s), 0, n_items, P(d_o), a.lists, 0, P(ranks), P(flags), S()))]
    for name, fn in cases:
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        rounds = [events_ms(fn, a.reps) for _ in range(3)]
        ms = sorted(rounds)[1]
        res[name] = {"ms": round(ms, 3), "rounds_ms": [round(v, 3) for v in rounds], "lists_per_s": round(a.lists / ms * 1e3),
                     "input_gbs": round(input_bytes / ms / 1e6, 1)}
    copy_gbs = float4_copy_gbs(a.reps)
    for name, _ in cases:
        res[name]["input_of_float4_copy"] = round(res[name]["input_gbs"] / copy_gbs, 4)

    # end to end, host arrays in, numbers out
    RL, RP = RaggedLists(labels, offsets), RaggedLists(scores, offsets)
    ragged = lambda: DeviceMetricEvaluator(RL, RP, driver_metrics()).evaluate()
    ragged()
    ev, t_ragged = timed(ragged)
    t0 = time.perf_counter()
    nested_l, nested_p = RL.to_lists(), RP.to_lists()
    t_build = time.perf_counter() - t0
    nested = lambda: DeviceMetricEvaluator(nested_l, nested_p, driver_metrics()).evaluate()
    ev_n, t_nested = timed(nested)
    ev_all, t_all = timed(lambda: DeviceMetricEvaluator(RL, RP, all_metrics()).evaluate())
    _, t_ranks = timed(lambda: rank_predictions_by_score_ragged(scores, offsets))
    n = min(a.host_lists, a.lists)
    host, t_host = timed(lambda: MetricEvaluator(nested_l[:n], nested_p[:n], driver_metrics()).evaluate())
    _, t_host_ranks = timed(lambda: [rank_predictions_by_score(x) for x in nested_p[:n]])
    sub = DeviceMetricEvaluator(nested_l[:n], nested_p[:n], driver_metrics()).evaluate()
    diff = max(abs(sub.evaluations[k] - host.evaluations[k]) / abs(host.evaluations[k]) for k in host.evaluations)
    assert diff <= 1e-12 + n * 2.0 ** -53, diff
    assert ev_n.evaluations == ev.evaluations
    res["end_to_end"] = {
        "ragged_driver_metrics_s": round(t_ragged, 4), "ragged_lists_per_s": round(a.lists / t_ragged),
        "nested_driver_metrics_s": round(t_nested, 4), "nested_lists_per_s": round(a.lists / t_nested),
        "ragged_all_eight_s": round(t_all, 4), "ragged_ranks_s": round(t_ranks, 4), "ranks_lists_per_s": round(a.lists / t_ranks),
        "host_fallback_lists": ev.n_host_fallback, "nested_lists_built_in_s": round(t_build, 3),
        "host_evaluator_lists_timed": n, "host_evaluator_s": round(t_host, 4), "host_evaluator_lists_per_s": round(n / t_host, 1),
        "host_evaluator_us_per_list": round(t_host / n * 1e6, 1), "host_ranks_lists_per_s": round(n / t_host_ranks, 1),
        "max_rel_diff_vs_host_on_subsample": diff}
    e = res["end_to_end"]
    assert e["ragged_lists_per_s"] > e["host_evaluator_lists_per_s"], "RaggedLists end to end is not faster than the host evaluator"
    assert e["nested_lists_per_s"] > e["host_evaluator_lists_per_s"], "nested lists end to end is not faster than the host evaluator"
    print(json.dumps({"what": "metrics_probe", "config": "me-c1", "device": torch.cuda.get_device_name(0), "lists": a.lists,
                      "candidates": n_items, "mean_length": round(n_items / a.lists, 2), "share_250_long": 0.002, "scores": "float32",
                      "reps": a.reps, "input_bytes": input_bytes, "float4_copy_gbs": round(copy_gbs, 1),
                      "host_path": "this package's MetricEvaluator (the reference's per-impression form), timed in this run on "
                                   "host_evaluator_lists_timed lists", "evaluations": ev.evaluations, **res}))


if __name__ == "__main__":
    main()
