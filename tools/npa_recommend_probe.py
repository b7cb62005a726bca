"""Times ebn_npa_topk_score_f32 (csrc/ebn_npa_topk.hip) alone at the npa-c1 widths (L = 30, F = 400, A = 200, k = 10) on unit-scale
random operands over a 20 000-row catalogue, beside the route the library offered before it -- ebn_pap_indexed_f32 over (user,
candidate) pairs in score blocks of at most 1 GiB (filled by launches of at most 2^23 pairs), then torch.topk -- in ONE run on one GPU:

  nrec-c2   U = 200 000 users, M = 250 candidates (the reference's candidate list)
  nrec-c1   U = 20 000 users, M = 20 000 candidates (the whole catalogue)

Per shape: the two routes are warmed up at the timed shape, then timed `--reps` rounds each, ALTERNATING, with device events around a
whole pass; reported are the median and the min / max of the rounds.  At nrec-c1 the unfused route is timed on the first
`--unfused-users` users only and SCALED by U / that (one workgroup per pair: its time is proportional to the pairs); the line says so.
The fused lists are compared with the unfused route's on the users both cover (count of differing lists and the largest score
difference are reported, not asserted: torch.topk breaks ties its own way and the other kernel pools first and dots second).
Derived figures, from shapes: issued FLOP = 2 U M Lpad (F + A) with Lpad = 32 and useful FLOP with L = 30, each over the fused time
as a share of the 157.3 TFLOP/s exact-fp32 MFMA peak; catalogue bytes read = (user tiles of 128) x M x L x (F + A) x 4 over the
fused time, next to this run's float4-copy calibration (1 GiB through ebn_gather_rows_f32); the ratio unfused / fused.
Prints one JSON line per shape; `--out FILE` appends them.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/npa_recommend_probe.py --reps 2`.
usage: npa_recommend_probe.py [--reps K] [--shapes c2,c1] [--unfused-users N] [--out FILE]"""
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
from ebrec.models.newsrec._recommend import npa_topk  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
N_ROWS, L, F, A, K = 20000, 30, 400, 200, 10
# ebn_pap_indexed_f32 launches one 256-thread workgroup per pair; a launch is kept below 2^32 threads in all (2^23 pairs), the size
# up to which its results were checked against the fused lists in this probe
PAIRS_PER_LAUNCH = 1 << 23
SHAPES = {"c2": dict(U=200000, M=250), "c1": dict(U=20000, M=20000)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def float4_copy_gbs(reps=10):
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
    ms, _ = timed(lambda: [fn() for _ in range(reps)])
    return (2.0 * n * 4 + rows * 4) / (ms / reps) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="c2,c1")
    ap.add_argument("--unfused-users", type=int, default=1000, help="users the unfused route is timed on at nrec-c1 (then scaled)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("npa_recommend_probe needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    Ua = torch.empty(N_ROWS, L, A, device="cuda").uniform_(-1, 1, generator=g)  # tanh outputs lie in (-1, 1)
    Vd = torch.empty(N_ROWS, L, F, device="cuda").uniform_(0, 1, generator=g)   # relu outputs
    copy_gbs = float4_copy_gbs()
    for name in args.shapes.split(","):
        U, M = SHAPES[name]["U"], SHAPES[name]["M"]
        users = torch.randn(U, F, device="cuda", generator=g) / F ** 0.5
        Q = torch.empty(U, A, device="cuda").uniform_(-1, 1, generator=g)
        cand = None if M == N_ROWS else torch.randperm(N_ROWS, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
        rows = torch.arange(N_ROWS, dtype=torch.int32, device="cuda") if cand is None else cand
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        oob = torch.zeros(1, dtype=torch.int32, device="cuda")
        Uu = U if name == "c2" else min(U, args.unfused_users)  # users of the unfused pass
        chunk = max(1, min(Uu, (1 << 30) // (4 * M)))  # users per score block of at most 1 GiB
        block = torch.empty(chunk * M, device="cuda")
        row_idx = rows.repeat(chunk).contiguous()  # pair n of a block: user n // M, candidate n % M
        q_idx = torch.arange(chunk, dtype=torch.int32, device="cuda").repeat_interleave(M).contiguous()

        def fused():
            return npa_topk(users, Q, Ua, Vd, cand, None, K, False, flags)

        def unfused():
            idx = torch.empty(Uu, K, dtype=torch.int64, device="cuda")
            val = torch.empty(Uu, K, device="cuda")
            for s in range(0, Uu, chunk):
                n = min(chunk, Uu - s)
                for p0 in range(0, n * M, PAIRS_PER_LAUNCH):  # one workgroup per pair: see PAIRS_PER_LAUNCH
                    m = min(PAIRS_PER_LAUNCH, n * M - p0)
                    _hip.call("ebn_pap_indexed_f32", _hip.ptr(Ua), _hip.ptr(Vd), N_ROWS, _hip.ptr(row_idx[p0:]), _hip.ptr(Q[s:s + n]),
                              _hip.ptr(q_idx[p0:]), n, None, _hip.ptr(users[s:s + n]), _hip.ptr(block[p0:]), 0, _hip.ptr(oob), m, L, F, A,
                              _hip.stream_handle())
                v, i = torch.topk(block[:n * M].view(n, M), K, dim=1)
                val[s:s + n], idx[s:s + n] = v, i
            return idx, val

        fused()  # warm-up of both routes at the timed shape
        unfused()
        torch.cuda.synchronize()
        t_f, t_u = [], []
        for _ in range(args.reps):
            ms, (pos, score) = timed(fused)
            t_f.append(ms)
            ms, (idx, val) = timed(unfused)
            t_u.append(ms)
        differing = int((pos[:Uu].to(torch.int64) != idx).any(dim=1).sum())
        max_dev = float((score[:Uu] - val).abs().max())
        scale = U / Uu
        fm, um = statistics.median(t_f), statistics.median(t_u) * scale
        pairs = float(U) * M
        issued, useful = 2.0 * pairs * 32 * (F + A), 2.0 * pairs * L * (F + A)
        cat_bytes = float(-(-U // 128)) * M * L * (F + A) * 4
        rec = {"probe": f"nrec-{name}", "U": U, "M": M, "n_rows": N_ROWS, "L": L, "F": F, "A": A, "k": K, "reps": args.reps,
               "n_splits": int(_hip.lib().ebn_npa_topk_auto_splits(U, M, L)),
               "fused_ms": round(fm, 3), "fused_ms_min_max": [round(min(t_f), 3), round(max(t_f), 3)],
               "fused_users_per_s": round(U / (fm * 1e-3), 1), "fused_pairs_per_s": round(pairs / (fm * 1e-3), 1),
               "unfused_ms": round(um, 3), "unfused_ms_min_max": [round(min(t_u) * scale, 3), round(max(t_u) * scale, 3)],
               "unfused_timed_on_users": Uu, "unfused_pairs_per_launch": PAIRS_PER_LAUNCH, "unfused_scaled_by": round(scale, 3), "unfused_users_per_block": chunk,
               "unfused_pairs_per_s": round(pairs / (um * 1e-3), 1),
               "fused_issued_tflops": round(issued / (fm * 1e-3) / 1e12, 2),
               "fused_issued_share_of_fp32_mfma_peak": round(issued / (fm * 1e-3) / PEAK_FP32_MFMA, 4),
               "fused_useful_tflops": round(useful / (fm * 1e-3) / 1e12, 2),
               "fused_useful_share_of_fp32_mfma_peak": round(useful / (fm * 1e-3) / PEAK_FP32_MFMA, 4),
               "fused_catalogue_read_gb_per_s": round(cat_bytes / (fm * 1e-3) / 1e9, 1), "float4_copy_gb_per_s": round(copy_gbs, 1),
               "unfused_over_fused": round(um / fm, 3),
               "lists_differing_from_unfused": differing, "max_abs_score_difference": max_dev,
               "flags": flags.cpu().tolist(), "oob": int(oob.item()), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del users, Q, block, row_idx, q_idx


if __name__ == "__main__":
    main()
