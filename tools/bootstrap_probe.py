"""Times ebn_poisson_bootstrap_f64 (csrc/ebn_bootstrap.hip) beside an unfused route on the same GPU and beside the numpy twin, in
ONE run:

  bs-c1  1 000 000 impressions x 4 metric columns x 2000 resamples   (the me-c1 size of metrics_probe.py)
  bs-c2  13 500 000 x 4 x 2000                                        (test-set scale)

The unfused route draws its weights with torch.poisson, a block of resamples at a time (a [block, n] float64 matrix of about 1 GiB),
and multiplies with torch.matmul; it is timed on `--unfused_resamples` resamples and scaled to all of them (it is linear in them).
Kernel and unfused route are warmed up, then timed `--reps` rounds each, ALTERNATING, with device events; reported are the median
and the min / max.  The numpy twin (ebrec/evaluation/bootstrap.py) is timed on `--twin_pairs` (item, resample) pairs and scaled;
its weight sums on that block are compared with the kernel's (must be equal).

Per shape: milliseconds, (item, resample) pairs per second, value bytes read per second (every workgroup row of 512 resamples
streams the columns once: ceil(B / 512) * n * m * 8 bytes), the ratios to the unfused route and to the twin, and
`valu_slots_per_pair` = the device's VALU lane-cycles (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz) over the pair rate: what one pair
costs in full-rate vector-ALU issue slots, to hold against the instruction count of the inner loop.
Prints one JSON line per shape; `--out FILE` appends them (default profiles/bootstrap_c1.jsonl).
usage: bootstrap_probe.py [--shapes bs-c1,bs-c2] [--resamples 2000] [--cols 4] [--reps 5] [--out FILE]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec.evaluation import bootstrap as bs  # noqa: E402

SHAPES = {"bs-c1": 1_000_000, "bs-c2": 13_500_000}
VALU_LANE_HZ = 256 * 4 * 16 * 2.4e9


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def unfused(values, n_resamples, block, gen):
    """torch.poisson blocks + matmul: (sums [B, m], weights [B])"""
    m, n = values.shape
    ones = torch.ones(block, n, dtype=torch.float64, device=values.device)
    sums = torch.empty(n_resamples, m, dtype=torch.float64, device=values.device)
    weights = torch.empty(n_resamples, dtype=torch.float64, device=values.device)
    for b0 in range(0, n_resamples, block):
        nb = min(block, n_resamples - b0)
        w = torch.poisson(ones[:nb], generator=gen)
        sums[b0:b0 + nb] = w @ values.T
        weights[b0:b0 + nb] = w.sum(1)
    return sums, weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bs-c1,bs-c2")
    ap.add_argument("--resamples", type=int, default=2000)
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--unfused_resamples", type=int, default=0, help="0: about 2^29 pairs' worth")
    ap.add_argument("--twin_pairs", type=int, default=1 << 24)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bootstrap_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bootstrap_probe needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    B, m = args.resamples, args.cols
    for name in args.shapes.split(","):
        n = SHAPES[name]
        g = torch.Generator(device="cuda").manual_seed(0)
        values = torch.rand(m, n, dtype=torch.float64, device="cuda", generator=g)
        kernel = lambda: bs.bootstrap_call(values, None, 0, args.seed, 0, B)
        block = max(1, (1 << 27) // n)  # 2^27 doubles = 1 GiB of weights at a time
        ub = args.unfused_resamples or max(block, min(B, (1 << 29) // n))
        other = lambda: unfused(values, ub, block, g)
        for _ in range(2):
            kernel()
            other()
        torch.cuda.synchronize()
        t_k, t_u = [], []
        for _ in range(args.reps):
            ms, (sums, weights) = timed(kernel)
            t_k.append(ms)
            ms, _ = timed(other)
            t_u.append(ms * B / ub)
        # the twin on a block of resamples, scaled; its weights must be the kernel's
        tb = max(1, min(B, args.twin_pairs // n))
        host = values.cpu().numpy()
        keys = np.arange(n, dtype=np.uint32)
        t0 = time.perf_counter()
        t_sums, t_weights = bs._twin_sums(host, keys, args.seed, 0, tb)
        twin_ms = (time.perf_counter() - t0) * 1e3 * B / tb
        weights_equal = bool(np.array_equal(t_weights, weights[:tb].cpu().numpy()))
        sums_rel = float(np.abs(sums[:tb].cpu().numpy() - t_sums).max() / np.abs(t_sums).max())
        km, um = statistics.median(t_k), statistics.median(t_u)
        pairs = float(n) * B
        rec = {"probe": name, "n_items": n, "n_cols": m, "n_resamples": B, "reps": args.reps,
               "kernel_ms": round(km, 3), "kernel_ms_min_max": [round(min(t_k), 3), round(max(t_k), 3)],
               "pairs_per_s": round(pairs / (km * 1e-3)), "valu_slots_per_pair": round(VALU_LANE_HZ / (pairs / (km * 1e-3)), 2),
               "value_bytes_read_per_s": round(-(-B // bs.RESAMPLES) * n * m * 8 / (km * 1e-3)),
               "unfused_ms_scaled": round(um, 3), "unfused_ms_scaled_min_max": [round(min(t_u), 3), round(max(t_u), 3)],
               "unfused_resamples_timed": ub, "unfused_block": block, "unfused_over_kernel": round(um / km, 2),
               "twin_ms_scaled": round(twin_ms, 1), "twin_resamples_timed": tb, "twin_over_kernel": round(twin_ms / km, 1),
               "twin_weights_equal": weights_equal, "twin_sums_max_rel_diff": sums_rel,
               "mean_weight": round(float(weights.double().mean()) / n, 6), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del values, sums, weights
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
