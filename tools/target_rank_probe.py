"""Times ebn_target_rank_f32 (csrc/ebn_target_rank.hip) beside the unchanged ebn_topk_score_f32 on synthetic unit-variance vectors,
in ONE run on one GPU, at the rec-c1 shape: U = 200 000 users, M = 20 000 candidates, F = 400.

  topk        ebn_topk_score_f32 at k = 10: the yardstick (existing code, the same MFMAs with the selection epilogue)
  rank_x0     the new kernel without exclusion rows
  rank_x20    the new kernel with X = 20 exclusion rows per user (random catalogue rows): the price of the exclusion compare
  rank_w16    the new kernel with windows of M / 16 candidates sliding over the list, users in order of lo

All four are warmed up, then timed `--reps` rounds each, ALTERNATING, with device events around a whole call; reported are the
median and the min / max of the rounds, the ratio to `topk` of the same run, and the spread of `topk` itself (max - min over its
median) -- the yardstick of the issue: rank_x0 should not exceed topk by more than that.  On the way the ranks are checked against
the lists: a target taken from slot j of a user's top-10 must come back with rank j + 1 and the slot's score bits, with and
without the exclusion rows (random rows: one that hits a target takes its rank away, one ahead of it moves it up a place).
Prints one JSON line; `--out FILE` appends it.
usage: target_rank_probe.py [--users N] [--cands M] [--reps K] [--out FILE] [--note TEXT]"""
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
from ebrec import _hip  # noqa: E402
from ebrec.models.newsrec._recommend import target_rank, topk  # noqa: E402


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
    ap.add_argument("--users", type=int, default=200000)
    ap.add_argument("--cands", type=int, default=20000)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--x", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--note", default=None, help="free text kept in the record (which build was timed)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("target_rank_probe needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    U, M, F, k, X = args.users, args.cands, args.width, args.k, args.x
    g = torch.Generator(device="cuda").manual_seed(0)
    users = torch.randn(U, F, device="cuda", generator=g)
    news = torch.randn(M, F, device="cuda", generator=g)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    exclude = torch.randint(0, M, (U, X), device="cuda", generator=g, dtype=torch.int32).contiguous()
    w16 = sliding(U, M, max(1, M // 16), "cuda")
    # targets out of the lists themselves: slot u % k of user u's top-k without exclusion
    list_pos, list_score = topk(users, news, None, None, k, False, flags)
    slot = (torch.arange(U, device="cuda") % k).view(-1, 1)
    target = list_pos.gather(1, slot).view(-1).contiguous()
    routes = {
        "topk": lambda: topk(users, news, None, None, k, False, flags),
        "rank_x0": lambda: target_rank(users, news, None, target, None, None, False, flags),
        "rank_x20": lambda: target_rank(users, news, None, target, None, exclude, False, flags),
        "rank_w16": lambda: target_rank(users, news, None, target, w16, None, False, flags),
    }
    for _ in range(2):  # warm-up of every route at the timed shape
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times, out = {name: [] for name in routes}, {}
    for _ in range(args.reps):
        for name, fn in routes.items():
            ms, out[name] = timed(fn)
            times[name].append(ms)
    want_score = list_score.gather(1, slot).view(-1)
    rank0, count0, score0 = out["rank_x0"]
    x0_ok = bool((rank0 == slot.view(-1) + 1).all() and (count0 == M).all() and torch.equal(score0.view(torch.int32), want_score.view(torch.int32)))
    # with exclusion: a user's rank drops by the excluded rows ahead of the target; an excluded target has rank 0
    rank20, count20, score20 = out["rank_x20"]
    hit = (exclude == target.view(-1, 1)).any(1)
    ex_sorted = exclude.sort(1).values
    distinct = 1 + (ex_sorted[:, 1:] != ex_sorted[:, :-1]).sum(1) if X > 1 else torch.full((U,), min(X, 1), device="cuda")
    head = list_pos[:, :k].unsqueeze(2) == exclude.unsqueeze(1)  # [U, k, X]
    ahead_excluded = (head.any(2) & (torch.arange(k, device="cuda").view(1, -1) < slot)).sum(1)
    x20_ok = bool((count20 == M - distinct).all() and (rank20[hit] == 0).all()
                  and (rank20[~hit] == (slot.view(-1) + 1 - ahead_excluded)[~hit]).all()
                  and torch.equal(score20[~hit].view(torch.int32), want_score[~hit].view(torch.int32)))
    rank16, count16, _ = out["rank_w16"]
    inside = (target >= w16[:, 0]) & (target < w16[:, 1])
    w16_ok = bool((count16 == max(1, M // 16)).all() and ((rank16 > 0) == inside).all() and (rank16[inside] <= rank0[inside]).all())
    med = {name: statistics.median(t) for name, t in times.items()}
    spread = (max(times["topk"]) - min(times["topk"])) / med["topk"]
    rec = {"probe": "rank-c1", **({"note": args.note} if args.note else {}), "U": U, "M": M, "F": F, "k": k, "X": X, "reps": args.reps, "n_splits": int(_hip.lib().ebn_topk_auto_splits(U, M)),
           "ms": {name: round(m, 3) for name, m in med.items()},
           "ms_min_max": {name: [round(min(t), 3), round(max(t), 3)] for name, t in times.items()},
           "over_topk": {name: round(med[name] / med["topk"], 4) for name in routes if name != "topk"},
           "topk_spread": round(spread, 4), "x0_within_topk_spread": bool(med["rank_x0"] <= med["topk"] * (1 + spread)),
           "x20_over_x0": round(med["rank_x20"] / med["rank_x0"], 4),
           "topk_tflops": round(2.0 * U * M * F / (med["topk"] * 1e-3) / 1e12, 2),
           "rank_x0_tflops": round(2.0 * U * M * F / (med["rank_x0"] * 1e-3) / 1e12, 2),
           "x0_ranks_are_the_list_slots_bitwise": x0_ok, "x20_ranks_follow_the_exclusion": x20_ok, "w16_ranks_inside_their_windows": w16_ok,
           "flags": flags.cpu().tolist(), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
