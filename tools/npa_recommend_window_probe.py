"""Times ebn_npa_topk_score_window_f32 (csrc/ebn_npa_topk.hip, the windowed instantiations) alone beside the unchanged
ebn_npa_topk_score_f32 at the npa-c1 widths (L = 30, F = 400, A = 200, k = 10) on unit-scale random operands over a 20 000-row
catalogue, in ONE run on one GPU:

  nrec-c1   U = 20 000 users, M = 20 000 candidates (the whole catalogue)
  nrec-c2   U = 200 000 users, M = 250 candidates (the reference's candidate list)

  plain         ebn_npa_topk_score_f32: the yardstick (existing code, untouched instantiation)
  open          the windowed entry with every window [0, M): the cost of the window logic when it skips nothing
  w16_sorted    windows of M / 16 candidates sliding over the list, users in order of lo (what the host flush produces)
  w64_sorted    the same with M / 64
  w16_shuffled  the M / 16 windows with the users shuffled: every workgroup's union is about the whole list, gating buys nothing

All are warmed up, then timed `--reps` rounds each, ALTERNATING, with device events around a whole call, the whole loop under
`--time-limit` seconds (a shape that would pass it is cut short and says so); reported are the median and the min / max of the
rounds, the ratio to `plain` of the same run, every route's own (max - min) / median spread (`open_ratio_is_noise`: that of `plain`
or `open` is above 5 %, so their ratio should not be read) and, next to each windowed route, the share of the (workgroup, step)
pairs of the plain walk that its workgroups visit.  Checked in the same run: the all-open lists equal the plain
ones bit for bit, and the shuffled lists equal the sorted ones after un-permuting.
Prints one JSON line per shape; `--out FILE` appends them (default profiles/npa_recommend_window_c1.jsonl).
usage: npa_recommend_window_probe.py [--reps K] [--shapes c1,c2] [--time-limit S] [--out FILE] [--note TEXT]"""
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
from ebrec.models.newsrec._recommend import npa_topk, npa_topk_window  # noqa: E402

N_ROWS, L, F, A, K = 20000, 30, 400, 200, 10
TILE, CPS = 128, 4  # users of a workgroup, candidates of a step at L <= 32
SHAPES = {"c1": dict(U=20000, M=20000), "c2": dict(U=200000, M=250)}


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
    """the steps the 128-user workgroups walk (each the steps its users' union meets) over those of the plain walk"""
    U = window.shape[0]
    tiles = (U + TILE - 1) // TILE
    w = window.long()
    pad = tiles * TILE - U
    lo = torch.cat([w[:, 0], w[-1:, 0].expand(pad)]).view(tiles, TILE).min(1).values
    hi = torch.cat([w[:, 1], w[-1:, 1].expand(pad)]).view(tiles, TILE).max(1).values
    steps = (hi + CPS - 1) // CPS - lo // CPS
    return float(steps.sum()) / (tiles * ((M + CPS - 1) // CPS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--time-limit", type=float, default=240.0, help="seconds for the timed rounds of one shape")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "npa_recommend_window_c1.jsonl"))
    ap.add_argument("--note", default=None, help="free text kept in the record (which build was timed)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("npa_recommend_window_probe needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    Ua = torch.empty(N_ROWS, L, A, device="cuda").uniform_(-1, 1, generator=g)  # tanh outputs lie in (-1, 1)
    Vd = torch.empty(N_ROWS, L, F, device="cuda").uniform_(0, 1, generator=g)   # relu outputs
    for name in args.shapes.split(","):
        U, M = SHAPES[name]["U"], SHAPES[name]["M"]
        users = torch.randn(U, F, device="cuda", generator=g) / F ** 0.5
        Q = torch.empty(U, A, device="cuda").uniform_(-1, 1, generator=g)
        cand = None if M == N_ROWS else torch.randperm(N_ROWS, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        w_open = torch.tensor([[0, M]], dtype=torch.int32, device="cuda").repeat(U, 1).contiguous()
        w16, w64 = sliding(U, M, max(1, M // 16), "cuda"), sliding(U, M, max(1, M // 64), "cuda")
        perm = torch.randperm(U, device="cuda", generator=g)
        users_p, Q_p, w16_p = users[perm].contiguous(), Q[perm].contiguous(), w16[perm].contiguous()
        routes = {
            "plain": lambda: npa_topk(users, Q, Ua, Vd, cand, None, K, False, flags),
            "open": lambda: npa_topk_window(users, Q, Ua, Vd, cand, w_open, None, K, False, flags),
            "w16_sorted": lambda: npa_topk_window(users, Q, Ua, Vd, cand, w16, None, K, False, flags),
            "w64_sorted": lambda: npa_topk_window(users, Q, Ua, Vd, cand, w64, None, K, False, flags),
            "w16_shuffled": lambda: npa_topk_window(users_p, Q_p, Ua, Vd, cand, w16_p, None, K, False, flags),
        }
        shares = {"open": visited_share(w_open, M), "w16_sorted": visited_share(w16, M), "w64_sorted": visited_share(w64, M),
                  "w16_shuffled": visited_share(w16_p, M)}
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
        same = lambda a, b: bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
        open_ok = same(out["open"], out["plain"])
        unpermuted = tuple(torch.empty_like(t).index_copy_(0, perm, t) for t in out["w16_shuffled"])
        shuffled_ok = same(unpermuted, out["w16_sorted"])
        pos16 = out["w16_sorted"][0]
        inside_ok = bool(((pos16 >= w16[:, :1]) & (pos16 < w16[:, 1:])).all())  # M / 16 >= k here: every list is full
        med = {r: statistics.median(t) for r, t in times.items()}
        spread = {r: round((max(t) - min(t)) / med[r], 4) for r, t in times.items()}
        rec = {"probe": f"npa-recommend-window-{name}", **({"note": args.note} if args.note else {}), "U": U, "M": M, "n_rows": N_ROWS, "L": L,
               "F": F, "A": A, "k": K, "reps": rounds, "reps_asked": args.reps, "n_splits": int(_hip.lib().ebn_npa_topk_auto_splits(U, M, L)),
               "ms": {r: round(m, 3) for r, m in med.items()},
               "ms_min_max": {r: [round(min(t), 3), round(max(t), 3)] for r, t in times.items()},
               "over_plain": {r: round(med[r] / med["plain"], 4) for r in routes if r != "plain"},
               "steps_visited_share": {r: round(s, 4) for r, s in shares.items()},
               # the gated ratio is open / plain: a spread above 5 % in either makes it noise; the short routes' spreads stand beside them
               "spread": spread, "open_ratio_is_noise": bool(max(spread["plain"], spread["open"]) > 0.05),
               "open_within_5_percent_of_plain": bool(med["open"] <= 1.05 * med["plain"]),
               "sorted_windows_below_plain": bool(med["w16_sorted"] < med["plain"] and med["w64_sorted"] < med["plain"]),
               "open_lists_equal_plain_bitwise": open_ok, "shuffled_lists_equal_sorted_bitwise": shuffled_ok,
               "w16_lists_inside_their_windows": inside_ok, "flags": flags.cpu().tolist(), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del users, Q, users_p, Q_p, w_open, w16, w64, w16_p


if __name__ == "__main__":
    main()
