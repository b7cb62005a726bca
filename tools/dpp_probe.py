"""Times ebn_dpp_rerank_f32 (csrc/ebn_dpp.hip) beside the unchanged ebn_mmr_rerank_f32 (csrc/ebn_rerank.hip) over the same pools,
in ONE run on one GPU:

  dpp-c1      U = 200 000 users, P = 64, D = 768, k = 10, lam = 0.7, pool rows uniform over a 125 541 x 768 unit table (EB-NeRD's catalogue)
  dpp-c1-k64  the same at k = 64, where the Cholesky sums are 40 times as many (k (k - 1) / 2 = 2016 against 45 fma per entry)

MMR is the floor: it has the same Gram stage and a cheaper greedy stage (one LDS row read per round), in half the LDS.  Both
kernels are warmed up, then timed `--reps` rounds each, ALTERNATING, with device events around a whole pass over the users;
reported are the median and the min / max of the rounds, users per second, the ratio DPP / MMR of the medians, and the Gram FLOP
2 U P^2 D (the whole P x P matrix) over each kernel's time as a share of the 157.3 TFLOP/s exact-fp32 MFMA peak.  The lists are
compared on the way (the share of round-0 picks that agree -- both start from the most relevant entry -- is reported, not asserted).
Prints one JSON line per shape; `--out FILE` appends them (default profiles/dpp_c1.jsonl).
usage: dpp_probe.py [--users N] [--reps K] [--ks 10,64] [--out FILE]"""
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
from ebrec.evaluation.rerank import dpp_select, mmr_select  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
N_ROWS = 125_541


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
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--ks", default="10,64")
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dpp_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dpp_probe needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    U, P, D, lam = args.users, args.pool, args.width, args.lam
    g = torch.Generator(device="cuda").manual_seed(0)
    rel = torch.rand(U, P, device="cuda", generator=g)
    unit = torch.nn.functional.normalize(torch.randn(N_ROWS, D, device="cuda", generator=g), dim=1).contiguous()
    rows = torch.randint(0, N_ROWS, (U, P), device="cuda", generator=g, dtype=torch.int32)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    gram_flop = 2.0 * U * P * P * D
    for k in (int(x) for x in args.ks.split(",")):
        dpp = lambda: dpp_select(unit, rows, rel, k, lam, flags)[0]
        mmr = lambda: mmr_select(unit, rows, rel, k, lam, flags)[0]
        for _ in range(2):  # warm-up of both kernels at the timed shape
            dpp()
            mmr()
        torch.cuda.synchronize()
        t_d, t_m = [], []
        for _ in range(args.reps):
            ms, sel_d = timed(dpp)
            t_d.append(ms)
            ms, sel_m = timed(mmr)
            t_m.append(ms)
        dm, mm = statistics.median(t_d), statistics.median(t_m)
        rec = {"probe": "dpp-c1" if k == 10 else f"dpp-c1-k{k}", "U": U, "P": P, "D": D, "k": k, "lam": lam, "n_rows": N_ROWS,
               "reps": args.reps,
               "dpp_ms": round(dm, 3), "dpp_ms_min_max": [round(min(t_d), 3), round(max(t_d), 3)],
               "mmr_ms": round(mm, 3), "mmr_ms_min_max": [round(min(t_m), 3), round(max(t_m), 3)],
               "dpp_users_per_s": round(U / (dm * 1e-3)), "mmr_users_per_s": round(U / (mm * 1e-3)),
               "dpp_over_mmr": round(dm / mm, 3),
               "dpp_gram_share_of_fp32_mfma_peak": round(gram_flop / (dm * 1e-3) / PEAK_FP32_MFMA, 4),
               "mmr_gram_share_of_fp32_mfma_peak": round(gram_flop / (mm * 1e-3) / PEAK_FP32_MFMA, 4),
               "first_picks_equal": round(float((sel_d[:, 0] == sel_m[:, 0]).float().mean()), 4),
               "lists_differing_from_mmr": int((sel_d != sel_m).any(dim=1).sum()),
               "flags": flags.cpu().tolist(), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
