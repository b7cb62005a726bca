"""Times ebn_window_counts_i32 (csrc/ebn_popularity.hip) beside the unfused torch route on the same GPU, in ONE run:

  pop-c1  125 541 article rows, 20 000 000 events (Zipf rows, times uniform over 28 days, microseconds), 1 000 000 impressions with
          the me-c1 in-view lengths (4 + geometric, mean about 11.6, 0.2 % of 250; metrics_probe.py) whose articles follow the same
          Zipf law (2 % unknown), times uniform over the last 7 days, windows 1 h / 6 h / 24 h, min_age 0

The unfused route is composite-key ``torch.searchsorted``: the events as one sorted int64 key ``row * span + (time - first time)``
(built once, outside the timing, like the kernel's event table), then per call one ``repeat_interleave`` of the impression times
over the items, and per window end -- t and t - max_age_w, four ends here -- one int64 key tensor of n_items and one searchsorted
with int64 results; the counts are the differences.  It needs rows * span < 2^63.
The impressions are run once in random time order and once sorted by time (neighbouring items then search neighbouring places).
Kernel and unfused route are warmed up, then timed `--reps` rounds each, ALTERNATING, with device events; reported are the median
and the min / max, (item, window) pairs per second, and the ratio.  The counts of the two routes are compared for equality in the
same run.  Prints one JSON line per order; `--out FILE` appends them (default profiles/popularity_c1.jsonl).
usage: popularity_probe.py [--rows N] [--events N] [--impressions N] [--reps 5] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec.models.baselines.popularity import window_counts_call  # noqa: E402

US = 1_000_000
DAY = 86_400 * US
WINDOWS = [3600 * US, 6 * 3600 * US, 24 * 3600 * US]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def zipf_rows(n, n_rows, gen, perm):
    """n row numbers with P(rank k) ~ 1 / k, the ranks scattered over the table by `perm`"""
    cdf = torch.cumsum(1.0 / torch.arange(1, n_rows + 1, dtype=torch.float64, device="cuda"), 0)
    u = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * cdf[-1]
    return perm[torch.searchsorted(cdf, u).clamp_(max=n_rows - 1)]


def unfused(comp, span, t_first, item_rows, lengths, list_times, max_ages, min_age):
    t = torch.repeat_interleave(list_times, lengths)
    known = item_rows >= 0
    base = item_rows.to(torch.int64).clamp_(min=0) * span
    end = lambda x: torch.searchsorted(comp, base + (x - t_first).clamp_(0, span - 1))
    p_hi = end(t - min_age)
    return torch.stack([((p_hi - end(t - a)).clamp_(min=0) * known).to(torch.int32) for a in max_ages])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_541)
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--impressions", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "popularity_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("popularity_probe needs a GPU: nothing is measured without one")
    if args.reps < 5:
        raise SystemExit("at least 5 rounds")
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    n_rows, span = args.rows, 28 * DAY + 1  # key offsets 0 .. span - 1
    perm = torch.randperm(n_rows, device="cuda", generator=gen)
    ev_rows = zipf_rows(args.events, n_rows, gen, perm)
    ev_t = torch.randint(0, 28 * DAY, (args.events,), device="cuda", generator=gen)
    comp = torch.sort(ev_rows * span + ev_t).values  # the unfused route's table; rows * span = 3.0e17 < 2^63
    event_times = (comp % span).contiguous()         # the kernel's table: per-row ascending times
    row_offsets = torch.zeros(n_rows + 1, dtype=torch.int64, device="cuda")
    row_offsets[1:] = torch.cumsum(torch.bincount(ev_rows, minlength=n_rows), 0)
    del ev_rows, ev_t

    from metrics_probe import make_lists

    offsets_np = make_lists(args.impressions, seed=args.seed)[2]
    n_items = int(offsets_np[-1])
    list_offsets = torch.from_numpy(offsets_np).cuda()
    lengths = list_offsets[1:] - list_offsets[:-1]
    item_rows = zipf_rows(n_items, n_rows, gen, perm).to(torch.int32)
    item_rows[torch.rand(n_items, device="cuda", generator=gen) < 0.02] = -1
    times_random = torch.randint(21 * DAY, 28 * DAY, (args.impressions,), device="cuda", generator=gen)
    longest = int((row_offsets[1:] - row_offsets[:-1]).max())
    for order, list_times in (("random", times_random), ("sorted", torch.sort(times_random).values)):
        kernel = lambda: window_counts_call(event_times, row_offsets, item_rows, list_offsets, list_times, WINDOWS, 0)
        other = lambda: unfused(comp, span, 0, item_rows, lengths, list_times, WINDOWS, 0)
        for _ in range(2):
            kernel()
            other()
        torch.cuda.synchronize()
        t_k, t_u = [], []
        for _ in range(args.reps):
            ms, got = timed(kernel)
            t_k.append(ms)
            ms, want = timed(other)
            t_u.append(ms)
        equal = bool(torch.equal(got, want))
        km, um = statistics.median(t_k), statistics.median(t_u)
        pairs = float(n_items) * len(WINDOWS)
        rec = {"probe": "pop-c1", "impression_order": order, "n_rows": n_rows, "n_events": args.events, "longest_row": longest,
               "n_impressions": args.impressions, "n_items": n_items, "windows_h": [1, 6, 24], "reps": args.reps,
               "kernel_ms": round(km, 3), "kernel_ms_min_max": [round(min(t_k), 3), round(max(t_k), 3)],
               "pairs_per_s": round(pairs / (km * 1e-3)),
               "unfused_ms": round(um, 3), "unfused_ms_min_max": [round(min(t_u), 3), round(max(t_u), 3)],
               "unfused_over_kernel": round(um / km, 2), "counts_equal": equal,
               "share_nonzero_24h": round(float((got[2] > 0).double().mean()), 4), "max_count_24h": int(got[2].max()),
               "unfused_bytes_materialised_per_item": 8 * (2 + 2 * (len(WINDOWS) + 1)), "kernel_bytes_per_item": 4 + 4 * len(WINDOWS),
               "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        if not equal:
            raise SystemExit("the counts of the two routes differ")


if __name__ == "__main__":
    main()
