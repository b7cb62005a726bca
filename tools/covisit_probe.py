"""Times the co-visitation baseline (csrc/ebn_covisit.hip + the torch plumbing of ebrec/models/baselines/covisit.py) beside an
unfused torch route on the same GPU, in ONE run:

  cv-c1  cs-c1's operands (content_probe.py): 125 541 matrix rows, 200 000 user sequences of 5 to 50 articles under the Zipf law of
         pop-c1 (2 % unknown), max_gap 3, both directions, cosine values; 1 000 000 impressions with the me-c1 in-view lengths, each
         mapped to a user under the same law; the users' sequences are their histories (exponential weights, 0.9)

  a. the matrix build: ``covisit_matrix_device`` (upload of the rows, ebn_cv_pair_keys_i64, torch.sort, unique_consecutive,
     searchsorted) + the cosine values; the pair-key kernel alone is timed beside it
  b. ebn_cv_scores_f32 in both modes against the unfused route: per block of lists whose (item, history entry) pairs fit 1 GiB
     (40 bytes per pair: two int64 indices, the composite key, the position, the value) the pairs by repeat_interleave, one
     searchsorted of ``candidate * n_rows + history row`` over the matrix's composite keys, a gather of the values, times the
     weight, ``index_add_`` (sum) or ``scatter_reduce amax`` (max) per item

All are warmed up, then timed `--reps` rounds, ALTERNATING inside every round, with device events (the build, which has host work
in it, with a synchronised wall clock): median and min / max.  The two score routes are fp32 evaluations of the same sums, each
within n u / (1 - n u) sum |w S| of the exact value (n <= 50 present entries; the values and weights are positive, so sum |w S| is
the score itself), so they agree within TWICE that; in max mode both round the same products: twice u |score|.
Prints one JSON line per timed thing; `--out FILE` appends them (default profiles/covisit_c1.jsonl).
usage: covisit_probe.py [--rows N] [--users N] [--impressions N] [--reps 5] [--out FILE]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec.models.baselines import covisit as cv  # noqa: E402
from ebrec.models.baselines.content import history_weight_values  # noqa: E402
from popularity_probe import timed, zipf_rows  # noqa: E402

U = 2.0 ** -24
GIB = 1 << 30
PAIR_BYTES = 40
MAX_GAP, SYMMETRIC, SIMILARITY = 3, True, "cosine"


class Problem:
    def __init__(self, args):
        gen = torch.Generator(device="cuda").manual_seed(args.seed)
        rng = np.random.default_rng(args.seed)
        self.n_rows = args.rows
        perm = torch.randperm(args.rows, device="cuda", generator=gen)
        self.perm = perm  # rank -> row: knn_probe.py draws its query histories under the SAME popularity of rows
        h_len = rng.integers(5, 51, args.users)
        self.h_off_np = np.zeros(args.users + 1, np.int64)
        np.cumsum(h_len, out=self.h_off_np[1:])
        self.n_hist_items = int(self.h_off_np[-1])
        self.h_rows = zipf_rows(self.n_hist_items, args.rows, gen, perm).to(torch.int32)
        self.h_rows[torch.rand(self.n_hist_items, device="cuda", generator=gen) < 0.02] = -1
        self.h_rows_np = self.h_rows.cpu().numpy()
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
        lh = self.list_hist.cpu().numpy().astype(np.int64)
        pairs = np.diff(self.c_off_np) * h_len[lh]
        self.n_pairs = int(pairs.sum())
        budget = GIB // PAIR_BYTES
        ends, cut, acc = np.cumsum(pairs), [0], 0
        while cut[-1] < self.n_lists:
            nxt = max(int(np.searchsorted(ends, acc + budget, side="right")), cut[-1] + 1)
            cut.append(min(nxt, self.n_lists))
            acc = int(ends[cut[-1] - 1])
        self.list_blocks = cut
        self.indptr = self.cols = self.vals = self.comp = None

    # ---- a. the build
    def build(self):
        indptr, cols, counts = cv.covisit_matrix_device(self.h_rows_np, self.h_off_np, self.n_rows, MAX_GAP, SYMMETRIC, 2 ** 27, "cuda")
        return indptr, cols, counts, cv.covisit_values_device(indptr, cols, counts, SIMILARITY)

    def k_pair_keys(self):
        return cv.pair_keys_call(self.h_rows, self.h_off, self.n_rows, MAX_GAP, SYMMETRIC)

    def set_matrix(self, indptr, cols, vals):
        self.indptr, self.cols, self.vals = indptr, cols, vals
        row_of = torch.repeat_interleave(torch.arange(self.n_rows, device="cuda"), indptr[1:] - indptr[:-1])
        self.comp = row_of * self.n_rows + cols.long()

    # ---- b. the scores
    def k_scores(self, mode):
        return cv.scores_call(self.indptr, self.cols, self.vals, self.h_rows, self.h_w, self.h_off, self.list_hist, self.c_rows, self.c_off, mode)

    def t_scores(self, mode):
        out = torch.zeros(self.n_items, dtype=torch.float32, device="cuda")
        lh = self.list_hist.long()
        nnz = self.comp.numel()
        for b0, b1 in zip(self.list_blocks[:-1], self.list_blocks[1:]):
            i0, i1 = int(self.c_off_np[b0]), int(self.c_off_np[b1])
            if i0 == i1:
                continue
            u = lh[self.item_list[i0:i1]]
            first, count = self.h_off[u], self.h_off[u + 1] - self.h_off[u]
            item = torch.repeat_interleave(torch.arange(i1 - i0, device="cuda"), count)
            start = torch.cumsum(count, 0) - count
            entry = torch.arange(item.numel(), device="cuda") - start[item] + first[item]
            hr, cr = self.h_rows[entry].long(), self.c_rows[i0:i1][item].long()
            present = (hr >= 0) & (cr >= 0)
            key = cr.clamp(min=0) * self.n_rows + hr.clamp(min=0)
            pos = torch.searchsorted(self.comp, key).clamp_(max=nnz - 1)
            s = torch.where(present & (self.comp[pos] == key), self.vals[pos], torch.zeros((), device="cuda")) * self.h_w[entry]
            if mode == 0:
                out[i0:i1].index_add_(0, item, s)
            else:
                best = torch.full((i1 - i0,), float("-inf"), device="cuda").scatter_reduce_(
                    0, item, torch.where(present, s, torch.full_like(s, float("-inf"))), "amax")
                out[i0:i1] = torch.where(torch.isinf(best), torch.zeros_like(best), best)
        return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_541)
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--impressions", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "covisit_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("covisit_probe needs a GPU: nothing is measured without one")
    if args.reps < 5:
        raise SystemExit("at least 5 rounds")
    torch.cuda.set_device(0)
    P = Problem(args)
    indptr, cols, counts, vals = P.build()
    P.set_matrix(indptr, cols, vals)
    row_len = (indptr[1:] - indptr[:-1]).float()
    jobs = {"matrix build": lambda: wall(P.build), "pair-key kernel": lambda: timed(P.k_pair_keys),
            "sum kernel": lambda: timed(lambda: P.k_scores(0)), "sum torch": lambda: timed(lambda: P.t_scores(0)),
            "max kernel": lambda: timed(lambda: P.k_scores(1)), "max torch": lambda: timed(lambda: P.t_scores(1))}
    for _ in range(2):  # warm-up
        for fn in jobs.values():
            fn()
    ms = {k: [] for k in jobs}
    last = {}
    for _ in range(args.reps):  # alternating: every round times each thing once
        for k, fn in jobs.items():
            t, out = fn()
            ms[k].append(t)
            last[k] = out
    stat = lambda k: dict(ms=round(statistics.median(ms[k]), 3), ms_min_max=[round(min(ms[k]), 3), round(max(ms[k]), 3)])
    base = {"probe": "cv-c1", "n_rows": P.n_rows, "n_users": P.n_users, "n_entries": P.n_hist_items, "max_gap": MAX_GAP, "symmetric": SYMMETRIC,
            "similarity": SIMILARITY, "n_keys": P.n_hist_items * 2 * MAX_GAP, "nnz": int(cols.numel()), "mean_row_length": round(float(row_len.mean()), 1),
            "longest_row": int(row_len.max()), "n_impressions": P.n_lists, "n_items": P.n_items, "n_pairs": P.n_pairs, "reps": args.reps,
            "device": torch.cuda.get_device_name(0)}
    records = [dict(base, what="matrix build (upload, pair keys, sort, runs, indptr, cosine values)", **stat("matrix build")),
               dict(base, what="pair-key kernel alone", **stat("pair-key kernel"),
                    keys_gb_per_s=round(P.n_hist_items * 2 * MAX_GAP * 8 / 1e9 / (statistics.median(ms["pair-key kernel"]) * 1e-3), 1))]
    failed = False
    for mode, name in ((0, "sum"), (1, "max")):
        got, want = last[f"{name} kernel"], last[f"{name} torch"]
        diff = (got - want).abs()
        bound = 2 * (50 * U / (1 - 50 * U)) * want.abs() if mode == 0 else 2 * U * want.abs()
        agree = bool((diff <= bound).all())
        ratios = [o / k for k, o in zip(ms[f"{name} kernel"], ms[f"{name} torch"])]
        km = statistics.median(ms[f"{name} kernel"])
        records.append(dict(base, what=f"ebn_cv_scores_f32 mode {mode} ({name}) against the unfused torch route", kernel=stat(f"{name} kernel"),
                            torch=stat(f"{name} torch"), torch_over_kernel=round(statistics.median(ratios), 2),
                            torch_over_kernel_min_max=[round(min(ratios), 2), round(max(ratios), 2)],
                            pairs_per_ns=round(P.n_pairs / (km * 1e6), 2), nonzero_scores=int((want != 0).sum()),
                            largest_difference=float(diff.max()), largest_twice_bound=float(bound.max()), routes_agree_within_twice_the_bound=agree))
        failed |= not agree
    for rec in records:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if failed:
        raise SystemExit("the two routes differ by more than twice the bound")


if __name__ == "__main__":
    main()
