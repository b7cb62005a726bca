"""Times ebn_npa_target_rank_f32 (csrc/ebn_npa_target_rank.hip) beside the unchanged ebn_npa_topk_score_f32 at the npa-c1 widths
(L = 30, F = 400, A = 200) on unit-scale random operands over a 20 000-row catalogue, in ONE run on one GPU:

  nrec-c2   U = 200 000 users, M = 250 candidates (the reference's candidate list)
  nrec-c1   U = 20 000 users, M = 20 000 candidates (the whole catalogue)

  topk        ebn_npa_topk_score_f32 at k = 10: the yardstick (existing code, the same step body with the selection epilogue)
  rank_x0     the new entry without exclusion rows: target pass + walk + the adding launch
  rank_x20    the same with X = 20 exclusion rows per user (random catalogue rows): the price of the exclusion compare
  rank_w16    the same with windows of M / 16 candidates sliding over the list, users in order of lo
  tpass       the target pass on its own: the entry with EVERY window empty, so the walk has no step.  The pass runs all its steps
              (128 / 4 per workgroup) and MFMAs, but every target is then "no rank" and its operand row is catalogue row 0

All are warmed up, then timed `--reps` rounds each, ALTERNATING, with device events around a whole call, the whole loop under
`--time-limit` seconds (a shape that would pass it is cut short and says so); reported are the median and the min / max of the
rounds, the ratio to `topk` of the same run and the spread of `topk` itself.  On the way the ranks are checked at full size against
the lists: a target taken from slot u % 10 of user u's top-10 must come back with rank slot + 1 and the slot's score bits, with and
without the exclusion rows (a row that hits a target takes its rank away, one ahead of it moves it up a place); under the windows
count is the window's width and a target has a rank exactly when its position lies inside.
Prints one JSON line per shape; `--out FILE` appends them.
usage: npa_target_rank_probe.py [--reps K] [--shapes c2,c1] [--time-limit S] [--out FILE] [--note TEXT]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec import _hip  # noqa: E402
from ebrec.models.newsrec._recommend import npa_target_rank, npa_topk  # noqa: E402

N_ROWS, L, F, A, K, X = 20000, 30, 400, 200, 10, 20
SHAPES = {"c2": dict(U=200000, M=250), "c1": dict(U=20000, M=20000)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def sliding(U, M, width, device):
    """[U, 2] int32: a window of `width` candidates that slides from the start of the list to its end, users in order"""
    lo = (torch.arange(U, dtype=torch.int64, device=device) * (M - width)) // max(U - 1, 1)
    return torch.stack([lo, lo + width], 1).to(torch.int32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="c2,c1")
    ap.add_argument("--time-limit", type=float, default=240.0, help="seconds for the timed rounds of one shape")
    ap.add_argument("--out", default=None)
    ap.add_argument("--note", default=None, help="free text kept in the record (which build was timed)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("npa_target_rank_probe needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    Ua = torch.empty(N_ROWS, L, A, device="cuda").uniform_(-1, 1, generator=g)  # tanh outputs lie in (-1, 1)
    Vd = torch.empty(N_ROWS, L, F, device="cuda").uniform_(0, 1, generator=g)   # relu outputs
    for name in args.shapes.split(","):
        U, M = SHAPES[name]["U"], SHAPES[name]["M"]
        users = torch.randn(U, F, device="cuda", generator=g) / F ** 0.5
        Q = torch.empty(U, A, device="cuda").uniform_(-1, 1, generator=g)
        cand = None if M == N_ROWS else torch.randperm(N_ROWS, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
        rows = torch.arange(N_ROWS, dtype=torch.int32, device="cuda") if cand is None else cand
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        exclude = rows[torch.randint(0, M, (U, X), device="cuda", generator=g)].contiguous()  # rows of the candidate list
        width = max(1, M // 16)
        w16 = sliding(U, M, width, "cuda")
        empty = torch.zeros(U, 2, dtype=torch.int32, device="cuda")
        # targets out of the lists themselves: slot u % k of user u's top-k without exclusion
        list_pos, list_score = npa_topk(users, Q, Ua, Vd, cand, None, K, False, flags)
        slot = (torch.arange(U, device="cuda") % K).view(-1, 1)
        target = list_pos.gather(1, slot).view(-1).contiguous()
        routes = {
            "topk": lambda: npa_topk(users, Q, Ua, Vd, cand, None, K, False, flags),
            "rank_x0": lambda: npa_target_rank(users, Q, Ua, Vd, cand, target, None, None, False, flags),
            "rank_x20": lambda: npa_target_rank(users, Q, Ua, Vd, cand, target, None, exclude, False, flags),
            "rank_w16": lambda: npa_target_rank(users, Q, Ua, Vd, cand, target, w16, None, False, flags),
            "tpass": lambda: npa_target_rank(users, Q, Ua, Vd, cand, target, empty, None, False, flags),
        }
        for fn in routes.values():  # warm-up of every route at the timed shape
            fn()
        torch.cuda.synchronize()
        times, out = {r: [] for r in routes}, {}
        t0, rounds = time.monotonic(), 0
        for _ in range(args.reps):
            if time.monotonic() - t0 > args.time_limit:
                break
            for r, fn in routes.items():
                ms, out[r] = timed(fn)
                times[r].append(ms)
            rounds += 1
        want_score = list_score.gather(1, slot).view(-1)
        rank0, count0, score0 = out["rank_x0"]
        x0_ok = bool((rank0 == slot.view(-1) + 1).all() and (count0 == M).all()
                     and torch.equal(score0.view(torch.int32), want_score.view(torch.int32)))
        # with exclusion: a user's rank drops by the excluded positions ahead of the target; an excluded target has rank 0
        rank20, count20, score20 = out["rank_x20"]
        trow = rows[target.long()]
        hit = (exclude == trow.view(-1, 1)).any(1)
        ex_sorted = exclude.sort(1).values
        distinct = 1 + (ex_sorted[:, 1:] != ex_sorted[:, :-1]).sum(1)  # the candidate rows are distinct: one position each
        head = rows[list_pos.long()].unsqueeze(2) == exclude.unsqueeze(1)  # [U, k, X]
        ahead_excluded = (head.any(2) & (torch.arange(K, device="cuda").view(1, -1) < slot)).sum(1)
        x20_ok = bool((count20 == M - distinct).all() and (rank20[hit] == 0).all()
                      and (rank20[~hit] == (slot.view(-1) + 1 - ahead_excluded)[~hit]).all()
                      and torch.equal(score20[~hit].view(torch.int32), want_score[~hit].view(torch.int32)))
        rank16, count16, score16 = out["rank_w16"]
        inside = (target >= w16[:, 0]) & (target < w16[:, 1])
        w16_ok = bool((count16 == width).all() and ((rank16 > 0) == inside).all() and (rank16[inside] <= rank0[inside]).all()
                      and torch.equal(score16[inside].view(torch.int32), want_score[inside].view(torch.int32)))
        rank_e, count_e, _ = out["tpass"]
        tpass_ok = bool((rank_e == 0).all() and (count_e == 0).all())
        med = {r: statistics.median(t) for r, t in times.items()}
        spread = (max(times["topk"]) - min(times["topk"])) / med["topk"]
        pairs = float(U) * M
        issued = 2.0 * pairs * 32 * (F + A)
        rec = {"probe": f"npa-rank-{name}", **({"note": args.note} if args.note else {}), "U": U, "M": M, "n_rows": N_ROWS, "L": L, "F": F,
               "A": A, "k": K, "X": X, "reps": rounds, "reps_asked": args.reps, "n_splits": int(_hip.lib().ebn_npa_topk_auto_splits(U, M, L)),
               "ms": {r: round(m, 3) for r, m in med.items()},
               "ms_min_max": {r: [round(min(t), 3), round(max(t), 3)] for r, t in times.items()},
               "over_topk": {r: round(med[r] / med["topk"], 4) for r in routes if r != "topk"},
               "topk_spread": round(spread, 4), "x0_within_5_percent_of_topk": bool(med["rank_x0"] <= 1.05 * med["topk"]),
               "x20_over_x0": round(med["rank_x20"] / med["rank_x0"], 4),
               "tpass_share_of_rank_x0": round(med["tpass"] / med["rank_x0"], 4), "tpass_steps_over_walk_steps": round(128.0 / M, 4),
               "topk_issued_tflops": round(issued / (med["topk"] * 1e-3) / 1e12, 2),
               "rank_x0_issued_tflops": round(issued * (1 + 128.0 / M / 4) / (med["rank_x0"] * 1e-3) / 1e12, 2),
               "x0_ranks_are_the_list_slots_bitwise": x0_ok, "x20_ranks_follow_the_exclusion": x20_ok,
               "w16_ranks_inside_their_windows": w16_ok, "empty_windows_rank_nobody": tpass_ok,
               "flags": flags.cpu().tolist(), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del users, Q, exclude, w16, empty


if __name__ == "__main__":
    main()
