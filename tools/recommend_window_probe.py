"""Times ebn_topk_score_window_f32 (csrc/ebn_topk.hip, the windowed instantiation) alone beside ebn_topk_score_f32 on synthetic
unit-variance vectors, in ONE run on one GPU, at the rec-c1 shape: U = 200 000 users, M = 20 000 candidates, F = 400, k = 10.

  plain          ebn_topk_score_f32: the comparison (the unwindowed kernel is unchanged by the windowed one)
  full           the windowed entry with every window [0, M): the price of the gate
  w16            windows of M / 16 candidates sliding over the list, users in order of lo (what recommend()'s flush produces)
  w64            the same with M / 64
  w16_shuffled   the windows of w16 with the users in random order: what sorting buys

All five are warmed up, then timed `--reps` rounds each, ALTERNATING, with device events around a whole call (merge launch
included where the candidates are split); reported are the median and the min / max of the rounds, the ratio to `plain` of the
same run, and for the sliding windows the candidate tiles the workgroups visit as a share of all (computed from the windows the
way the kernel does: per 128-user tile the tiles that meet the union of its users' ranges), which is the ideal ratio.
On the way the lists are checked: `full` must equal `plain` bit for bit, `w16_shuffled` must equal `w16` after un-permuting.
Prints one JSON line; `--out FILE` appends it.
usage: recommend_window_probe.py [--users N] [--cands M] [--reps K] [--out FILE]"""
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
from ebrec.models.newsrec._recommend import topk, topk_window  # noqa: E402

TILE = 128  # users per workgroup and candidates per tile (csrc/ebn_catalogue_walk.h)


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


def visited_share(window, M):
    """candidate tiles the 128-user workgroups visit / all (user tile, candidate tile) pairs"""
    U = window.shape[0]
    pad = (-U) % TILE
    lo = torch.cat([window[:, 0], window[-1:, 0].expand(pad)]).view(-1, TILE).min(1).values.long()
    hi = torch.cat([window[:, 1], window[-1:, 1].expand(pad)]).view(-1, TILE).max(1).values.long()
    tiles = (hi + TILE - 1) // TILE - lo // TILE
    return float(tiles.sum()) / (tiles.numel() * ((M + TILE - 1) // TILE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200000)
    ap.add_argument("--cands", type=int, default=20000)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recommend_window_probe needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    U, M, F, k = args.users, args.cands, args.width, args.k
    g = torch.Generator(device="cuda").manual_seed(0)
    users = torch.randn(U, F, device="cuda", generator=g)
    news = torch.randn(M, F, device="cuda", generator=g)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    perm = torch.randperm(U, device="cuda", generator=g)
    users_shuffled = users[perm].contiguous()
    w_full = torch.tensor([[0, M]], dtype=torch.int32, device="cuda").repeat(U, 1).contiguous()
    w16, w64 = sliding(U, M, max(1, M // 16), "cuda"), sliding(U, M, max(1, M // 64), "cuda")
    w16_shuffled = w16[perm].contiguous()
    routes = {
        "plain": lambda: topk(users, news, None, None, k, False, flags),
        "full": lambda: topk_window(users, news, None, w_full, None, k, False, flags),
        "w16": lambda: topk_window(users, news, None, w16, None, k, False, flags),
        "w64": lambda: topk_window(users, news, None, w64, None, k, False, flags),
        "w16_shuffled": lambda: topk_window(users_shuffled, news, None, w16_shuffled, None, k, False, flags),
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
    same_full = bool(torch.equal(out["full"][0], out["plain"][0]) and torch.equal(out["full"][1].view(torch.int32), out["plain"][1].view(torch.int32)))
    same_shuffled = bool(torch.equal(out["w16_shuffled"][0], out["w16"][0][perm])
                         and torch.equal(out["w16_shuffled"][1].view(torch.int32), out["w16"][1][perm].view(torch.int32)))
    inside = bool(((out["w64"][0] >= w64[:, :1]) & (out["w64"][0] < w64[:, 1:])).all())
    med = {name: statistics.median(t) for name, t in times.items()}
    rec = {"probe": "recw-c1", "U": U, "M": M, "F": F, "k": k, "reps": args.reps, "n_splits": int(_hip.lib().ebn_topk_auto_splits(U, M)),
           "ms": {name: round(m, 3) for name, m in med.items()},
           "ms_min_max": {name: [round(min(t), 3), round(max(t), 3)] for name, t in times.items()},
           "over_plain": {name: round(med[name] / med["plain"], 4) for name in routes if name != "plain"},
           "visited_tile_share": {"w16": round(visited_share(w16, M), 4), "w64": round(visited_share(w64, M), 4),
                                  "w16_shuffled": round(visited_share(w16_shuffled, M), 4)},
           "window_share": {"w16": round(max(1, M // 16) / M, 4), "w64": round(max(1, M // 64) / M, 4)},
           "plain_tflops": round(2.0 * U * M * F / (med["plain"] * 1e-3) / 1e12, 2),
           "full_equals_plain_bitwise": same_full, "shuffled_equals_sorted_bitwise": same_shuffled, "w64_lists_inside_their_windows": inside,
           "flags": flags.cpu().tolist(), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
