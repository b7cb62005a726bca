"""Times the content-similarity kernels (csrc/ebn_content.hip) beside a chunked torch route on the same GPU, in ONE run:

  cs-c1  a 125 541 x 768 table of unit rows, 200 000 users with click histories of 5 to 50 articles (exponential weights, 0.9),
         1 000 000 impressions with the me-c1 in-view lengths (4 + geometric, mean about 11.6, 0.2 % of 250; metrics_probe.py), each
         mapped to a user under the Zipf law of pop-c1 (P(rank k) ~ 1 / k); history and in-view articles follow the same law over
         the table, 2 % of both unknown (-1)

The torch route cannot run unchunked (3 KB per gathered row): it works in blocks whose gathers fit 1 GiB.
  profiles   per block of history entries: index_select of the rows, times the weights, index_add_ into the users' sums; then the norm
  centroid   per block of items: index_select of the candidate rows and of the items' profile rows, row-wise dot
  nearest    per block of lists: the (item, history entry) pairs by repeat_interleave, two index_selects, row-wise dot times the
             weight, scatter_reduce amax per item
Kernels and torch route are warmed up, then timed `--reps` rounds each, ALTERNATING, with device events: median and min / max.  The
two routes are compared in the same run: both are fp32 evaluations, each within the derived bound of tests/content_cases.py of the
exact value, so they agree within TWICE that bound (centroid: 2 (H + D + 8) u (sum_k a_k |T[c, k]| / ||p|| + |score|); nearest:
2 (D + 8) u max w, and max w = 1 here).  Gather bandwidth = the table rows a kernel must read (4 D bytes each) over its time.
Prints one JSON line per timed thing; `--out FILE` appends them (default profiles/content_c1.jsonl).
usage: content_probe.py [--rows N] [--dim D] [--users N] [--impressions N] [--reps 5] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec import _hip  # noqa: E402
from ebrec.models.baselines.content import history_weight_values  # noqa: E402
from popularity_probe import timed, zipf_rows  # noqa: E402

U = 2.0 ** -24
GIB = 1 << 30


class Problem:
    def __init__(self, args):
        gen = torch.Generator(device="cuda").manual_seed(args.seed)
        rng = np.random.default_rng(args.seed)
        self.D, self.n_rows = args.dim, args.rows
        t = torch.randn((args.rows, args.dim), device="cuda", generator=gen)
        self.table = (t / t.norm(dim=1, keepdim=True)).contiguous()
        perm = torch.randperm(args.rows, device="cuda", generator=gen)
        h_len = rng.integers(5, 51, args.users)
        self.h_off_np = np.zeros(args.users + 1, np.int64)
        np.cumsum(h_len, out=self.h_off_np[1:])
        self.n_hist_items = int(self.h_off_np[-1])
        self.h_rows = zipf_rows(self.n_hist_items, args.rows, gen, perm).to(torch.int32)
        self.h_rows[torch.rand(self.n_hist_items, device="cuda", generator=gen) < 0.02] = -1
        self.h_w = torch.from_numpy(history_weight_values("exponential", self.h_off_np, 0.9).astype(np.float32)).cuda()
        self.h_off = torch.from_numpy(self.h_off_np).cuda()
        from metrics_probe import make_lists

        self.c_off_np = make_lists(args.impressions, seed=args.seed)[2]
        self.n_items = int(self.c_off_np[-1])
        self.c_off = torch.from_numpy(self.c_off_np).cuda()
        self.c_rows = zipf_rows(self.n_items, args.rows, gen, perm).to(torch.int32)
        self.c_rows[torch.rand(self.n_items, device="cuda", generator=gen) < 0.02] = -1
        uperm = torch.randperm(args.users, device="cuda", generator=gen)
        self.list_hist = zipf_rows(args.impressions, args.users, gen, uperm).to(torch.int32)
        self.n_users, self.n_lists = args.users, args.impressions
        self.item_list = torch.repeat_interleave(torch.arange(self.n_lists, device="cuda"), self.c_off[1:] - self.c_off[:-1])
        # blocks of lists whose (item, entry) pairs fit the torch route's 1 GiB (two gathers of pairs x D floats)
        lh = self.list_hist.cpu().numpy().astype(np.int64)
        pairs = np.diff(self.c_off_np) * h_len[lh]
        self.n_pairs = int(pairs.sum())
        budget = GIB // (2 * 4 * args.dim)
        ends, cut, acc = np.cumsum(pairs), [0], 0
        while cut[-1] < self.n_lists:
            nxt = int(np.searchsorted(ends, acc + budget, side="right"))
            nxt = max(nxt, cut[-1] + 1)
            cut.append(min(nxt, self.n_lists))
            acc = int(ends[cut[-1] - 1])
        self.list_blocks = cut

    # ---- the kernels
    def k_profiles(self):
        out = torch.empty((self.n_users, self.D), dtype=torch.float32, device="cuda")
        _hip.call("ebn_cs_profiles_f32", _hip.ptr(self.table), self.n_rows, self.D, self.D, _hip.ptr(self.h_rows), _hip.ptr(self.h_w),
                  _hip.ptr(self.h_off), self.n_users, self.n_hist_items, _hip.ptr(out), self.D, _hip.stream_handle())
        return out

    def k_centroid(self, prof):
        out = torch.empty(self.n_items, dtype=torch.float32, device="cuda")
        _hip.call("ebn_cs_centroid_scores_f32", _hip.ptr(self.table), self.n_rows, self.D, self.D, _hip.ptr(prof), self.n_users, self.D,
                  _hip.ptr(self.list_hist), _hip.ptr(self.c_rows), _hip.ptr(self.c_off), self.n_lists, self.n_items, _hip.ptr(out),
                  _hip.stream_handle())
        return out

    def k_nearest(self):
        out = torch.empty(self.n_items, dtype=torch.float32, device="cuda")
        _hip.call("ebn_cs_nearest_scores_f32", _hip.ptr(self.table), self.n_rows, self.D, self.D, _hip.ptr(self.h_rows), _hip.ptr(self.h_w),
                  _hip.ptr(self.h_off), self.n_users, self.n_hist_items, _hip.ptr(self.list_hist), _hip.ptr(self.c_rows), _hip.ptr(self.c_off),
                  self.n_lists, self.n_items, _hip.ptr(out), _hip.stream_handle())
        return out

    # ---- the chunked torch route
    def t_sums(self, absolute=False):
        """per user sum_j w_j T[h_j] (or of the absolute values: the a_k of the bound)"""
        p = torch.zeros((self.n_users, self.D), dtype=torch.float32, device="cuda")
        owner = torch.repeat_interleave(torch.arange(self.n_users, device="cuda"), self.h_off[1:] - self.h_off[:-1])
        step = GIB // (4 * self.D)
        for a in range(0, self.n_hist_items, step):
            r = self.h_rows[a:a + step]
            g = self.table.index_select(0, r.clamp(min=0).long())
            g = (g.abs() if absolute else g) * (self.h_w[a:a + step] * (r >= 0))[:, None]
            p.index_add_(0, owner[a:a + step], g)
        return p

    def t_profiles(self):
        p = self.t_sums()
        n = p.norm(dim=1, keepdim=True)
        return torch.where(n > 0, p / n.clamp(min=1e-30), torch.zeros_like(p))

    def t_centroid(self, prof, table=None):
        table = self.table if table is None else table
        out = torch.empty(self.n_items, dtype=torch.float32, device="cuda")
        step = GIB // (2 * 4 * self.D)
        for a in range(0, self.n_items, step):
            r = self.c_rows[a:a + step]
            u = self.list_hist[self.item_list[a:a + step]].long()
            out[a:a + step] = (table.index_select(0, r.clamp(min=0).long()) * prof.index_select(0, u)).sum(1) * (r >= 0)
        return out

    def t_nearest(self):
        out = torch.zeros(self.n_items, dtype=torch.float32, device="cuda")
        lh = self.list_hist.long()
        for b0, b1 in zip(self.list_blocks[:-1], self.list_blocks[1:]):
            i0, i1 = int(self.c_off_np[b0]), int(self.c_off_np[b1])
            if i0 == i1:
                continue
            u = lh[self.item_list[i0:i1]]
            first, count = self.h_off[u], self.h_off[u + 1] - self.h_off[u]
            item = torch.repeat_interleave(torch.arange(i1 - i0, device="cuda"), count)
            start = torch.cumsum(count, 0) - count
            entry = torch.arange(item.numel(), device="cuda") - start[item] + first[item]
            hr, cr = self.h_rows[entry], self.c_rows[i0:i1][item]
            dots = (self.table.index_select(0, hr.clamp(min=0).long()) * self.table.index_select(0, cr.clamp(min=0).long())).sum(1)
            val = torch.where((hr >= 0) & (cr >= 0), dots * self.h_w[entry], torch.full_like(dots, float("-inf")))
            best = torch.full((i1 - i0,), float("-inf"), device="cuda").scatter_reduce_(0, item, val, "amax")
            out[i0:i1] = torch.where(torch.isinf(best), torch.zeros_like(best), best)
        return out


def alternate(kernel, other, reps):
    for _ in range(2):
        kernel()
        other()
    torch.cuda.synchronize()
    t_k, t_o = [], []
    for _ in range(reps):
        ms, got = timed(kernel)
        t_k.append(ms)
        ms, want = timed(other)
        t_o.append(ms)
    return t_k, t_o, got, want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_541)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--impressions", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "content_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("content_probe needs a GPU: nothing is measured without one")
    if args.reps < 5:
        raise SystemExit("at least 5 rounds")
    torch.cuda.set_device(0)
    P = Problem(args)
    D, row_bytes = P.D, 4 * P.D
    present_h = int((P.h_rows >= 0).sum())
    present_c = int((P.c_rows >= 0).sum())
    prof = P.k_profiles()
    # the bounds of tests/content_cases.py, evaluated in fp32 on the device (H <= 50)
    p_norm = P.t_sums().norm(dim=1)
    a = P.t_sums(absolute=True)
    s_ref = P.t_centroid(P.t_profiles())
    amp = P.t_centroid(a / p_norm.clamp(min=1e-30)[:, None], table=P.table.abs())
    bound_c = 2 * (50 + D + 8) * U * (amp + s_ref.abs())
    bound_n = 2 * (D + 8) * U * float(P.h_w.max())
    del a, amp
    base = {"probe": "cs-c1", "n_rows": P.n_rows, "D": D, "n_users": P.n_users, "n_hist_items": P.n_hist_items, "n_impressions": P.n_lists,
            "n_items": P.n_items, "n_pairs": P.n_pairs, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    jobs = [
        ("profiles kernel", P.k_profiles, P.t_profiles, present_h * row_bytes, None),
        ("centroid scores kernel", lambda: P.k_centroid(prof), lambda: P.t_centroid(prof), present_c * row_bytes + P.n_lists * row_bytes, bound_c),
        ("centroid end to end", lambda: P.k_centroid(P.k_profiles()), lambda: P.t_centroid(P.t_profiles()),
         (present_h + present_c + P.n_lists) * row_bytes, bound_c),
        ("nearest kernel = end to end", P.k_nearest, P.t_nearest, None, bound_n),
    ]
    # rows the nearest kernel reads: per list its candidates once and its history once per tile of 16 candidates
    lens = np.diff(P.c_off_np)
    h_len = np.diff(P.h_off_np)[P.list_hist.cpu().numpy().astype(np.int64)]
    nearest_rows = int((lens + -(-lens // 16) * h_len).sum())
    failed = False
    for what, kernel, other, gather_bytes, bound in jobs:
        t_k, t_o, got, want = alternate(kernel, other, args.reps)
        km, om = statistics.median(t_k), statistics.median(t_o)
        if gather_bytes is None:
            gather_bytes = nearest_rows * row_bytes
        diff = (got - want).abs()
        if bound is None:  # profiles: per element 2 (H + D + 8) u (a_k + |p_k|) / ||p||, twice for two fp32 routes
            bound = 2 * (50 + D + 8) * U * (P.t_sums(absolute=True) + P.t_sums().abs()) / p_norm.clamp(min=1e-30)[:, None]
        agree = bool((diff <= 2 * bound).all())
        rec = dict(base, what=what, kernel_ms=round(km, 3), kernel_ms_min_max=[round(min(t_k), 3), round(max(t_k), 3)],
                   torch_ms=round(om, 3), torch_ms_min_max=[round(min(t_o), 3), round(max(t_o), 3)], torch_over_kernel=round(om / km, 2),
                   gather_gb=round(gather_bytes / 1e9, 2), gather_gb_per_s=round(gather_bytes / 1e9 / (km * 1e-3), 1),
                   largest_difference=float(diff.max()), largest_twice_bound=float((2 * bound).max()) if torch.is_tensor(bound) else 2 * bound,
                   routes_agree_within_twice_the_bound=agree)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        failed |= not agree
        del got, want, diff
    if failed:
        raise SystemExit("the two routes differ by more than twice the bound")


if __name__ == "__main__":
    main()
