"""Times the implicit-ALS baseline (csrc/ebn_als.hip + ebn_gemm_f32_ws + ebn_cs_centroid_scores_f32, as ebrec/models/baselines/als.py
calls them) beside an unfused torch route on the same GPU, in ONE run:

  als-c1  cv-c1's operands (covisit_probe.py): 125 541 items, 200 000 user sequences of 5 to 50 articles under the Zipf law of pop-c1
          (2 % unknown, dropped), duplicates combined, a = 40 * count; 1 000 000 impressions with the me-c1 in-view lengths, each
          mapped to a user under the same law; F = 64, and one more run at F = 128 (``--factors 64 128``)

  a. one user half-sweep: Gram of the item factors + ebn_als_solve_f32 over the 200 000 user rows
  b. one item half-sweep: Gram of the user factors + ebn_als_partials_f32 over the parts of the rows longer than split_len +
     ebn_als_solve_f32 over the 125 541 item rows (Zipf: a few rows hold a large share of the entries)
  c. fold-in + scores: the 200 000 histories solved against the item factors, ebn_cs_centroid_scores_f32 over the impressions
  torch: the same three without the kernels -- rows sorted by length and cut into blocks whose padded gather [rows, longest, F] and
     matrices [rows, F, F] fit 1 GiB, ``bmm`` for the sums, ``torch.linalg.cholesky`` + ``torch.cholesky_solve``; scores by a gather
     of both operands and a row-wise sum in blocks of 1 GiB

All are warmed up, then timed `--reps` rounds, ALTERNATING inside every round, with device events: median and min / max.  Per
phase the probe prints the gathered bytes and the flops it needed and what share of the card's peaks (8 TB/s, 157 TFLOP/s fp32
vector) that is: a phase far below both is bound by neither -- by latency, LDS traffic and barriers.
Prints one JSON line per timed thing; `--out FILE` appends them (default profiles/als_c1.jsonl).
usage: als_probe.py [--items N] [--users N] [--impressions N] [--factors 64 128] [--reps 5] [--out FILE]"""
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
from ebrec.models.baselines import als  # noqa: E402
from popularity_probe import timed, zipf_rows  # noqa: E402

GIB = 1 << 30
ALPHA, REG = 40.0, 0.01
PEAK_BYTES, PEAK_FLOPS = 8.0e12, 157.3e12


class Problem:
    def __init__(self, args, F):
        gen = torch.Generator(device="cuda").manual_seed(args.seed)
        rng = np.random.default_rng(args.seed)
        self.F, self.n_items, self.n_users = F, args.items, args.users
        perm = torch.randperm(args.items, device="cuda", generator=gen)
        h_len = rng.integers(5, 51, args.users)
        rows = zipf_rows(int(h_len.sum()), args.items, gen, perm).to(torch.int32)
        rows[torch.rand(rows.numel(), device="cuda", generator=gen) < 0.02] = -1
        rows = rows.cpu().numpy()
        owner = np.repeat(np.arange(args.users, dtype=np.int64), h_len)
        ok = rows >= 0
        csr = als._combine_device(owner[ok], rows[ok], np.ones(int(ok.sum())), args.users, args.items, ALPHA, torch.device("cuda"))
        self.users = als._Side(*csr, args.split_len)
        self.items = als._Side(*als._transpose_device(*csr, args.items), args.split_len)
        self.Y = torch.from_numpy((rng.standard_normal((args.items, F)) * 0.1).astype(np.float32)).cuda()
        self.X = als.solve_call(self.Y, als.gram_call(self.Y), self.users, REG)
        from metrics_probe import make_lists

        c_off = make_lists(args.impressions, seed=args.seed)[2]
        self.n_lists, self.n_cand = args.impressions, int(c_off[-1])
        self.c_off = torch.from_numpy(c_off).cuda()
        self.c_rows = zipf_rows(self.n_cand, args.items, gen, perm).to(torch.int32)
        self.c_rows[torch.rand(self.n_cand, device="cuda", generator=gen) < 0.02] = -1
        uperm = torch.randperm(args.users, device="cuda", generator=gen)
        self.list_hist = zipf_rows(args.impressions, args.users, gen, uperm).to(torch.int32)
        self.item_list = torch.repeat_interleave(torch.arange(self.n_lists, device="cuda"), self.c_off[1:] - self.c_off[:-1])
        self.blocks = {id(s): self._blocks(s) for s in (self.users, self.items)}

    def _blocks(self, side):
        """rows sorted by length, cut where the padded gather and the matrices of a block would pass 1 GiB -> (order, cuts)"""
        length = (side.indptr[1:] - side.indptr[:-1]).cpu().numpy()
        order = np.argsort(length, kind="stable")
        F, cuts = self.F, [0]
        cost = lambda a, b: (b - a) * (int(length[order[b - 1]]) * F * 8 + F * F * 8)  # the gather and its weighted copy, A and L
        while cuts[-1] < order.size:
            a, lo, hi = cuts[-1], cuts[-1] + 1, order.size
            while lo < hi:  # the cost ascends with b: the longest block within the budget (a single row past it stands alone)
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if cost(a, mid) <= GIB else (lo, mid - 1)
            cuts.append(lo)
        return torch.from_numpy(order).cuda(), cuts, length

    # ---- the kernels
    def k_half(self, fixed, side):
        return als.solve_call(fixed, als.gram_call(fixed), side, REG)

    def k_scores(self, rows):
        scores = torch.empty(self.n_cand, dtype=torch.float32, device="cuda")
        _hip.call("ebn_cs_centroid_scores_f32", _hip.ptr(self.Y), self.n_items, self.F, self.F, _hip.ptr(rows), self.n_users, self.F,
                  _hip.ptr(self.list_hist), _hip.ptr(self.c_rows), _hip.ptr(self.c_off), self.n_lists, self.n_cand, _hip.ptr(scores), _hip.stream_handle())
        return scores

    def k_fold(self):
        return self.k_scores(self.k_half(self.Y, self.users))

    # ---- the unfused torch route
    def t_half(self, fixed, side):
        F = self.F
        order, cuts, length = self.blocks[id(side)]
        base = fixed.T @ fixed + REG * torch.eye(F, device="cuda")
        out = torch.zeros((side.indptr.numel() - 1, F), dtype=torch.float32, device="cuda")
        for a, b in zip(cuts[:-1], cuts[1:]):
            rows = order[a:b]
            longest = int(length[order[b - 1].item()]) if b > a else 0
            if longest == 0:
                continue
            first, count = side.indptr[rows], side.indptr[rows + 1] - side.indptr[rows]
            slot = torch.arange(longest, device="cuda")[None, :]
            live = slot < count[:, None]
            entry = (first[:, None] + slot).clamp_(max=side.cols.numel() - 1)
            y = fixed[side.cols[entry].long()] * live[:, :, None]
            w = side.conf[entry] * live
            A = base + torch.bmm((y * w[:, :, None]).transpose(1, 2), y)
            rhs = ((1.0 + w)[:, :, None] * y).sum(dim=1)
            x = torch.cholesky_solve(rhs[:, :, None], torch.linalg.cholesky(A))[:, :, 0]
            out[rows] = torch.where(count[:, None] > 0, x, torch.zeros((), device="cuda"))
        return out

    def t_scores(self, rows):
        out = torch.empty(self.n_cand, dtype=torch.float32, device="cuda")
        step = GIB // (self.F * 8)
        lh = self.list_hist.long()
        for a in range(0, self.n_cand, step):
            c = self.c_rows[a:a + step].long()
            u = lh[self.item_list[a:a + step]]
            out[a:a + step] = torch.where(c >= 0, (self.Y[c.clamp(min=0)] * rows[u]).sum(dim=1), torch.zeros((), device="cuda"))
        return out

    def t_fold(self):
        return self.t_scores(self.t_half(self.Y, self.users))


def bound_of(bytes_, flops, ms):
    b, f = bytes_ / (ms * 1e-3) / PEAK_BYTES, flops / (ms * 1e-3) / PEAK_FLOPS
    what = "memory bandwidth" if b >= 0.5 else "fp32 throughput" if f >= 0.5 else "neither peak: latency, LDS traffic and barriers"
    return dict(gathered_gb=round(bytes_ / 1e9, 3), gflop=round(flops / 1e9, 1), share_of_peak_bandwidth=round(b, 3),
                share_of_peak_fp32=round(f, 3), bound_by=what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=125_541)
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--impressions", type=int, default=1_000_000)
    ap.add_argument("--factors", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--split-len", type=int, default=als.SPLIT_LEN)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "als_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("als_probe needs a GPU: nothing is measured without one")
    if args.reps < 5:
        raise SystemExit("at least 5 rounds")
    torch.cuda.set_device(0)
    for F in args.factors:
        P = Problem(args, F)
        jobs = {"users kernel": lambda: timed(lambda: P.k_half(P.Y, P.users)), "users torch": lambda: timed(lambda: P.t_half(P.Y, P.users)),
                "items kernel": lambda: timed(lambda: P.k_half(P.X, P.items)), "items torch": lambda: timed(lambda: P.t_half(P.X, P.items)),
                "fold kernel": lambda: timed(P.k_fold), "fold torch": lambda: timed(P.t_fold)}
        for fn in jobs.values():  # warm-up
            fn()
        ms, last = {k: [] for k in jobs}, {}
        for _ in range(args.reps):  # alternating: every round times each thing once
            for k, fn in jobs.items():
                t, out = fn()
                ms[k].append(t)
                last[k] = out
        stat = lambda k: dict(ms=round(statistics.median(ms[k]), 3), ms_min_max=[round(min(ms[k]), 3), round(max(ms[k]), 3)])
        nnz = int(P.users.cols.numel())
        ilen = (P.items.indptr[1:] - P.items.indptr[:-1])
        n_parts = 0 if P.items.row_parts is None else int(P.items.part_begin.numel())
        base = {"probe": "als-c1", "F": F, "n_items": P.n_items, "n_users": P.n_users, "nnz": nnz, "alpha": ALPHA, "reg": REG,
                "split_len": args.split_len, "longest_item_row": int(ilen.max()), "item_rows_split": int((ilen > args.split_len).sum()),
                "item_parts": n_parts, "n_impressions": P.n_lists, "n_candidates": P.n_cand, "reps": args.reps,
                "device": torch.cuda.get_device_name(0)}
        work = lambda n_rows: (nnz * F * 4.0, n_rows * (F ** 3 / 3.0 + 2.0 * F * F) * 2.0 + nnz * F * (F + 1.0))  # gathered bytes, flops
        for name, n_rows, what in (("users", P.n_users, "one user half-sweep (Gram + solve)"),
                                   ("items", P.n_items, "one item half-sweep (Gram + partials + solve)"),
                                   ("fold", P.n_users, "fold-in of the histories + scores of the impressions")):
            got, want = last[f"{name} kernel"], last[f"{name} torch"]
            rel = float((got - want).norm() / want.norm())
            ratios = [o / k for k, o in zip(ms[f"{name} kernel"], ms[f"{name} torch"])]
            bytes_, flops = work(n_rows)
            if name == "fold":
                bytes_, flops = bytes_ + P.n_cand * F * 4.0, flops + P.n_cand * F * 2.0
            rec = dict(base, what=what, kernel=stat(f"{name} kernel"), torch=stat(f"{name} torch"), torch_over_kernel=round(statistics.median(ratios), 2),
                       torch_over_kernel_min_max=[round(min(ratios), 2), round(max(ratios), 2)], relative_difference_of_the_routes=rel,
                       **bound_of(bytes_, flops, statistics.median(ms[f"{name} kernel"])))
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        del P
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
