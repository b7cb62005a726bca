"""Times ebn_mmr_rerank_f32 (csrc/ebn_rerank.hip) alone, beside a torch route over the same pools, in ONE run on one GPU:

  rr-c1     U = 200 000 users, P = 64, D = 768, k = 10, lam = 0.7, pool rows uniform over a 125 541 x 768 unit table (EB-NeRD's catalogue)
  rr-m250   the same over a 250-row table (the reference's shared candidate list: every row stays in cache)

The torch route: gather [n, P, D] in user chunks of at most 1 GiB, `torch.bmm` for the Gram matrices, the clip, and a greedy loop of
k torch steps (masked argmax, scatter, running minimum).  Both routes are warmed up, then timed `--reps` rounds each, ALTERNATING,
with device events around a whole pass over the users; reported are the median and the min / max of the rounds.  The picks are
compared on the way (the count of differing lists is reported, not asserted: bmm sums in another order and argmax breaks ties its
own way).  Derived figures, from shapes: Gram FLOP = 2 U P^2 D (the whole P x P matrix, as the torch route forms it) over the
kernel's time as a share of the 157.3 TFLOP/s exact-fp32 MFMA peak, and next to it the share the kernel ISSUES: it forms three of
the four 32 x 32 tiles when P > 32 (the Gram matrix is symmetric) and one when P <= 32, zero padding included; the row bytes the
algorithm needs, U P D 4 (every pool row once, caches not counted), over the kernel's time, beside this box's float4-copy calibration measured in the same run (the library's gather kernel over the identity permutation of 4 KB rows,
1 GiB, (read + write bytes) / time); the ratio torch / kernel.
Prints one JSON line per shape; `--out FILE` appends them.
usage: rerank_probe.py [--users N] [--reps K] [--shapes c1,m250] [--out FILE]"""
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
from ebrec.evaluation.rerank import mmr_select  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
SHAPES = {"c1": dict(n_rows=125_541), "m250": dict(n_rows=250)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


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
    ms = statistics.median(timed(fn)[0] for _ in range(reps))
    return (2.0 * n * 4 + rows * 4) / ms / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200000)
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="c1,m250")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rerank_probe needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    U, P, D, k, lam = args.users, args.pool, args.width, args.k, args.lam
    g = torch.Generator(device="cuda").manual_seed(0)
    copy_gbs = float4_copy_gbs(args.reps)
    rel = torch.rand(U, P, device="cuda", generator=g)
    chunk = max(1, min(U, (1 << 30) // (4 * P * D)))  # users per gathered block of at most 1 GiB
    for name in args.shapes.split(","):
        n_rows = SHAPES[name]["n_rows"]
        unit = torch.nn.functional.normalize(torch.randn(n_rows, D, device="cuda", generator=g), dim=1).contiguous()
        rows = torch.randint(0, n_rows, (U, P), device="cuda", generator=g, dtype=torch.int32)
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")

        def kernel():
            return mmr_select(unit, rows, rel, k, lam, flags)[0]

        def torch_route():
            sel = torch.full((U, k), -1, dtype=torch.int64, device="cuda")
            for s in range(0, U, chunk):
                r, x = rows[s:s + chunk], rel[s:s + chunk]
                n = r.shape[0]
                vec = unit[r.clamp(min=0).long()]                                  # [n, P, D]
                dist = (1.0 - torch.bmm(vec, vec.transpose(1, 2))).clamp_(0.0, 2.0)
                left = (r >= 0) & torch.isfinite(x)
                mind = torch.full_like(x, float("inf"))
                lines = torch.arange(n, device="cuda")
                for t in range(k):
                    obj = x if t == 0 else lam * x + (1.0 - lam) * mind
                    best = torch.where(left, obj, torch.full_like(obj, float("-inf"))).argmax(1)
                    sel[s:s + n, t] = torch.where(left.any(1), best, torch.full_like(best, -1))
                    left = left.scatter(1, best[:, None], False)
                    mind = torch.minimum(mind, dist[lines, best])
            return sel

        for _ in range(2):  # warm-up of both routes at the timed shape
            kernel()
            torch_route()
        torch.cuda.synchronize()
        t_k, t_t = [], []
        for _ in range(args.reps):
            ms, sel = timed(kernel)
            t_k.append(ms)
            ms, ref = timed(torch_route)
            t_t.append(ms)
        differing = int((sel.to(torch.int64) != ref).any(dim=1).sum())
        km, tm = statistics.median(t_k), statistics.median(t_t)
        row_gbs = U * P * D * 4.0 / (km * 1e-3) / 1e9
        issued = 2.0 * U * (3 if P > 32 else 1) * 32 * 32 * D  # FLOP of the MFMA tiles the kernel forms
        rec = {"probe": f"rr-{name}", "U": U, "P": P, "D": D, "k": k, "lam": lam, "n_rows": n_rows, "reps": args.reps,
               "kernel_ms": round(km, 3), "kernel_ms_min_max": [round(min(t_k), 3), round(max(t_k), 3)],
               "torch_ms": round(tm, 3), "torch_ms_min_max": [round(min(t_t), 3), round(max(t_t), 3)],
               "torch_users_per_block": chunk,
               "kernel_gram_tflops": round(2.0 * U * P * P * D / (km * 1e-3) / 1e12, 2),
               "kernel_share_of_fp32_mfma_peak": round(2.0 * U * P * P * D / (km * 1e-3) / PEAK_FP32_MFMA, 4),
               "kernel_issued_share_of_fp32_mfma_peak": round(issued / (km * 1e-3) / PEAK_FP32_MFMA, 4),
               "kernel_row_read_gbs": round(row_gbs, 1), "float4_copy_gbs": round(copy_gbs, 1),
               "row_read_of_float4_copy": round(row_gbs / copy_gbs, 3),
               "kernel_users_per_s": round(U / (km * 1e-3)), "torch_over_kernel": round(tm / km, 3),
               "lists_differing_from_torch": differing, "flags": flags.cpu().tolist(), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del unit, rows


if __name__ == "__main__":
    main()
