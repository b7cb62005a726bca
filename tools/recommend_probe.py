"""Times ebn_topk_score_f32 (csrc/ebn_topk.hip) alone on synthetic unit-variance vectors, beside the route the library offered before
it -- ebn_gemm_f32 over user chunks whose score block is at most 1 GiB, then torch.topk -- in ONE run on one GPU:

  rec-c1   U = 200 000 users, F = 400, k = 10, M = 20 000 candidates (the whole catalogue)
  rec-c2   the same with M = 250 (the reference's candidate list)

Per shape: the two routes are warmed up, then timed `--reps` rounds each, ALTERNATING, with device events around a whole pass over
the users; reported are the median and the min / max of the rounds.  The fused kernel's lists are compared with the unfused route's on
the way (same candidates wherever the unfused scores leave no tie or near-tie at the boundary; the count of differing lists is
reported, not asserted: torch.topk breaks ties its own way and the GEMM sums in another order).
Derived figures, from shapes: FLOP = 2 U M F over the fused time as a share of the 157.3 TFLOP/s exact-fp32 MFMA peak (rec-c1);
bytes the algorithm must read, (U + M) F 4, over the fused time (rec-c2); the ratio unfused / fused.
Prints one JSON line per shape; `--out FILE` appends them.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/recommend_probe.py --reps 2`.
usage: recommend_probe.py [--users N] [--reps K] [--shapes c1,c2] [--out FILE]"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec import _hip  # noqa: E402
from ebrec.models.newsrec._recommend import topk  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
SHAPES = {"c1": dict(M=20000), "c2": dict(M=250)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200000)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recommend_probe needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    U, F, k = args.users, args.width, args.k
    g = torch.Generator(device="cuda").manual_seed(0)
    users = torch.randn(U, F, device="cuda", generator=g)
    for name in args.shapes.split(","):
        M = SHAPES[name]["M"]
        news = torch.randn(M, F, device="cuda", generator=g)
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        chunk = max(1, min(U, (1 << 30) // (4 * M)))  # users per score block of at most 1 GiB
        block = torch.empty(chunk, M, device="cuda")

        def fused():
            return topk(users, news, None, None, k, False, flags)

        def unfused():
            idx = torch.empty(U, k, dtype=torch.int64, device="cuda")
            val = torch.empty(U, k, device="cuda")
            for s in range(0, U, chunk):
                n = min(chunk, U - s)
                # scores [n, M] = users[s:s+n] . news^T
                _hip.call("ebn_gemm_f32", 0, 1, n, M, F, ctypes.c_float(1.0), ctypes.c_void_p(users.data_ptr() + s * F * 4), F,
                          _hip.ptr(news), F, ctypes.c_float(0.0), _hip.ptr(block), M, _hip.stream_handle())
                v, i = torch.topk(block[:n], k, dim=1)
                val[s:s + n], idx[s:s + n] = v, i
            return idx, val

        for _ in range(2):  # warm-up of both routes at the timed shape
            fused()
            unfused()
        torch.cuda.synchronize()
        t_f, t_u = [], []
        for _ in range(args.reps):
            ms, (pos, score) = timed(fused)
            t_f.append(ms)
            ms, (idx, val) = timed(unfused)
            t_u.append(ms)
        differing = int((pos.to(torch.int64) != idx).any(dim=1).sum())
        max_dev = float((score - val).abs().max())
        fm, um = statistics.median(t_f), statistics.median(t_u)
        rec = {"probe": f"rec-{name}", "U": U, "M": M, "F": F, "k": k, "reps": args.reps,
               "n_splits": int(_hip.lib().ebn_topk_auto_splits(U, M)),
               "fused_ms": round(fm, 3), "fused_ms_min_max": [round(min(t_f), 3), round(max(t_f), 3)],
               "unfused_ms": round(um, 3), "unfused_ms_min_max": [round(min(t_u), 3), round(max(t_u), 3)],
               "unfused_users_per_block": chunk,
               "fused_tflops": round(2.0 * U * M * F / (fm * 1e-3) / 1e12, 2),
               "fused_share_of_fp32_mfma_peak": round(2.0 * U * M * F / (fm * 1e-3) / PEAK_FP32_MFMA, 4),
               "fused_required_read_gb_per_s": round((U + M) * F * 4 / (fm * 1e-3) / 1e9, 1),
               "unfused_over_fused": round(um / fm, 3),
               "lists_differing_from_unfused": differing, "max_abs_score_difference": max_dev,
               "flags": flags.cpu().tolist(), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
