"""Times ebn_calibrated_rerank_f32 (csrc/ebn_calibrate.hip) alone, beside a torch route over the same pools, in ONE run on one GPU:

  cal-c1      U = 200 000 users, P = 64, C = 64 one-hot label rows, H = 20, k = 10, lam = 0.7, alpha = 0.01, pool and history rows
              uniform over a 125 541-row label table (EB-NeRD's catalogue)
  cal-topics  the same with C = 128 and one to three labels per article (1 / len each)

The targets come from ebn_label_target_f32 over the histories (timed on its own, reported as `target_ms`); both routes read the same
target.  The torch route: gather [n, P, C] in user chunks of at most 1 GiB, then k greedy steps, each forming q~ and the KL of every
entry on an [n, P, C] block (masked where p = 0), a masked argmax, a scatter and the update of S.  Both routes are warmed up, then
timed `--reps` rounds each, ALTERNATING, with device events around a whole pass over the users; reported are the median and the
min / max of the rounds.  The picks are compared on the way (the count of differing lists is reported, not asserted: torch.log and
the sum over the labels round in their own way and argmax breaks ties its own way).  Derived figures, from shapes: the logf
evaluations the rule asks for, U k P (labels with p > 0), over the kernel's time; the label-row bytes the algorithm needs, U P C 4
(every pool row once, caches not counted), over the kernel's time; the ratio torch / kernel.
Prints one JSON line per shape; `--out FILE` appends them.
usage: calibrated_probe.py [--users N] [--reps K] [--shapes c1,topics] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec.evaluation.rerank import calibrated_select, label_target  # noqa: E402

SHAPES = {"c1": dict(C=64, multi=False), "topics": dict(C=128, multi=True)}
N_ROWS = 125_541


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def label_table(n_rows, C, multi, g):
    W = torch.zeros(n_rows, C, device="cuda")
    n_labels = torch.randint(1, 4, (n_rows,), device="cuda", generator=g) if multi else torch.ones(n_rows, dtype=torch.int64, device="cuda")
    picks = torch.rand(n_rows, C, device="cuda", generator=g).argsort(1)[:, :3]  # three distinct labels per row
    for j in range(3 if multi else 1):
        on = n_labels > j
        W[on, picks[on, j]] = 1.0 / n_labels[on].float()
    return W.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200000)
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("--history", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="c1,topics")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("calibrated_probe needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    U, P, H, k, lam, alpha = args.users, args.pool, args.history, args.k, args.lam, args.alpha
    g = torch.Generator(device="cuda").manual_seed(0)
    rel = torch.rand(U, P, device="cuda", generator=g)
    for name in args.shapes.split(","):
        C, multi = SHAPES[name]["C"], SHAPES[name]["multi"]
        W = label_table(N_ROWS, C, multi, g)
        rows = torch.randint(0, N_ROWS, (U, P), device="cuda", generator=g, dtype=torch.int32)
        hist = torch.randint(0, N_ROWS, (U, H), device="cuda", generator=g, dtype=torch.int32)
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        chunk = max(1, min(U, (1 << 30) // (4 * P * C)))  # users per gathered block of at most 1 GiB

        def target_kernel():
            return label_target(W, hist, None, flags)

        target = target_kernel()

        def kernel():
            return calibrated_select(W, rows, rel, target, k, lam, alpha, flags)[0]

        def torch_route():
            sel = torch.full((U, k), -1, dtype=torch.int64, device="cuda")
            for s in range(0, U, chunk):
                r, x, p = rows[s:s + chunk], rel[s:s + chunk], target[s:s + chunk]
                n = r.shape[0]
                w = W[r.clamp(min=0).long()]                                       # [n, P, C]
                left = (r >= 0) & torch.isfinite(x)
                S = torch.zeros(n, 1, C, device="cuda")
                pp, pos = p[:, None, :], (p > 0)[:, None, :]
                lines = torch.arange(n, device="cuda")
                for t in range(k):
                    q = (1.0 - alpha) * (S + w) / (t + 1) + alpha * pp              # [n, P, C]
                    kl = torch.where(pos, pp * torch.log(pp / q), torch.zeros_like(q)).sum(2)
                    obj = lam * x - (1.0 - lam) * kl
                    best = torch.where(left, obj, torch.full_like(obj, float("-inf"))).argmax(1)
                    sel[s:s + n, t] = torch.where(left.any(1), best, torch.full_like(best, -1))
                    left = left.scatter(1, best[:, None], False)
                    S = S + w[lines, best][:, None, :]
            return sel

        for _ in range(2):  # warm-up of both routes at the timed shape
            kernel()
            torch_route()
        torch.cuda.synchronize()
        t_k, t_t, t_p = [], [], []
        for _ in range(args.reps):
            t_p.append(timed(target_kernel)[0])
            ms, sel = timed(kernel)
            t_k.append(ms)
            ms, ref = timed(torch_route)
            t_t.append(ms)
        differing = int((sel.to(torch.int64) != ref).any(dim=1).sum())
        km, tm = statistics.median(t_k), statistics.median(t_t)
        n_log = float(U) * k * P * float((target > 0).sum(1).float().mean())
        rec = {"probe": f"cal-{name}", "U": U, "P": P, "C": C, "H": H, "k": k, "lam": lam, "alpha": alpha, "n_rows": N_ROWS,
               "labels_per_article": "1-3" if multi else "1", "reps": args.reps,
               "kernel_ms": round(km, 3), "kernel_ms_min_max": [round(min(t_k), 3), round(max(t_k), 3)],
               "torch_ms": round(tm, 3), "torch_ms_min_max": [round(min(t_t), 3), round(max(t_t), 3)],
               "target_ms": round(statistics.median(t_p), 3), "torch_users_per_block": chunk,
               "mean_labels_with_p_gt_0": round(float((target > 0).sum(1).float().mean()), 2),
               "kernel_glogf_per_s": round(n_log / (km * 1e-3) / 1e9, 2),
               "kernel_row_read_gbs": round(U * P * C * 4.0 / (km * 1e-3) / 1e9, 1),
               "kernel_users_per_s": round(U / (km * 1e-3)), "torch_over_kernel": round(tm / km, 3),
               "lists_differing_from_torch": differing, "flags": flags.cpu().tolist(), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del W, rows, hist, target


if __name__ == "__main__":
    main()
