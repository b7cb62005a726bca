"""Times the co-visitation top-N kernels (csrc/ebn_covisit_topk.hip) beside the two other ways to the same lists on the same GPU, in
ONE run, at cv-c1 (covisit_probe.py: 125 541 matrix rows, 200 000 user sequences of 5 to 50 articles under a Zipf law, max_gap 3,
both directions, cosine values, exponential history weights): a batch of `--batch` users drawn under the impressions' law, every
catalogue row a candidate, k = 10, no exclusion.

  topk / rank     ebn_cv_topk_f32 and ebn_cv_target_rank_f32 (targets: each user's own 5th slot) for n_splits = 0 (automatic) and
                  every alternative of `--splits`
  scores route    the one existing way to these scores: ebn_cv_scores_f32 over the same users with every catalogue row as a
                  candidate of every user (the score matrix is written out; no selection is timed with it)
  cand_pos        both kernels again with a row -> position map (a random permutation), as candidate_ids= and window= calls pass one
  torch route     unfused: the users' weights as a dense [n_rows, batch] matrix (index_put_ with accumulate), torch.sparse.mm of the
                  CSR matrix with it, torch.topk over the rows

All are warmed up, then timed `--reps` rounds, ALTERNATING inside every round, with device events: median and min / max.  The
kernel's and the torch route's k-th scores are fp32 evaluations of the same sums of positive terms in different orders: each within
n u / (1 - n u) of the exact value (n <= 50), so they agree within twice that, relative.  The record names the tile size R
(ebn_cv_topk_range()), the automatic n_splits and every alternative.  Prints one JSON line per timed thing; `--out FILE` appends
them (default profiles/covisit_topn_c1.jsonl).
usage: covisit_topn_probe.py [--rows N] [--users N] [--batch 1024] [--splits 1,2,4,8] [--reps 5] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec import _hip  # noqa: E402
from ebrec.models.baselines import covisit as cv  # noqa: E402
from covisit_probe import Problem  # noqa: E402
from popularity_probe import timed, zipf_rows  # noqa: E402

U32 = 2.0 ** -24
K = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_541)
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--impressions", type=int, default=1000)  # the in-view lists of covisit_probe's Problem: not used here
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--splits", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "covisit_topn_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("covisit_topn_probe needs a GPU: nothing is measured without one")
    if args.reps < 5:
        raise SystemExit("at least 5 rounds")
    torch.cuda.set_device(0)
    P = Problem(args)
    indptr, cols, counts, vals = P.build()
    n_rows, B = P.n_rows, args.batch
    t = cv.covisit_transpose_device(indptr, cols, vals)
    gen = torch.Generator(device="cuda").manual_seed(args.seed + 1)
    user_hist = zipf_rows(B, args.users, gen, torch.randperm(args.users, device="cuda", generator=gen)).to(torch.int32)
    lib = _hip.lib()
    R, auto = int(lib.ebn_cv_topk_range()), int(lib.ebn_cv_topk_auto_splits(B, n_rows))
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    hist = (P.h_rows, P.h_w, P.h_off)
    topk = lambda s: cv.topk_call(*t, *hist, user_hist, B, None, n_rows, None, None, K, 0, flags, s)
    target = topk(0)[0][:, 4].contiguous()
    rank = lambda s: cv.target_rank_call(*t, *hist, user_hist, B, None, n_rows, target, None, None, 0, flags, s)
    # the same with a row -> position map, as every candidate_ids= and window= call has one: a random permutation of the rows
    cand_pos = torch.randperm(n_rows, device="cuda", generator=gen).to(torch.int32)
    topk_perm = lambda: cv.topk_call(*t, *hist, user_hist, B, cand_pos, n_rows, None, None, K, 0, flags, 0)
    target_perm = topk_perm()[0][:, 4].contiguous()
    rank_perm = lambda: cv.target_rank_call(*t, *hist, user_hist, B, cand_pos, n_rows, target_perm, None, None, 0, flags, 0)

    # the scores route: every catalogue row a candidate of every user of the batch
    all_rows = torch.arange(n_rows, dtype=torch.int32, device="cuda").repeat(B)
    all_off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * n_rows
    scores_route = lambda: cv.scores_call(indptr, cols, vals, *hist, user_hist, all_rows, all_off, 0)

    # the torch route
    S = torch.sparse_csr_tensor(indptr, cols.long(), vals, size=(n_rows, n_rows))
    try:
        torch.sparse.mm(S, torch.zeros((n_rows, 1), device="cuda"))
    except RuntimeError:  # no CSR product in this build: the COO form of the same matrix
        S = S.to_sparse_coo().coalesce()
    uh = user_hist.long()
    first, count = P.h_off[uh], P.h_off[uh + 1] - P.h_off[uh]
    owner = torch.repeat_interleave(torch.arange(B, device="cuda"), count)
    entry = torch.arange(owner.numel(), device="cuda") - (torch.cumsum(count, 0) - count)[owner] + first[owner]
    e_rows, e_w = P.h_rows[entry].long(), P.h_w[entry]
    known = e_rows >= 0

    def torch_route():
        W = torch.zeros((n_rows, B), dtype=torch.float32, device="cuda")
        W.index_put_((e_rows[known], owner[known]), e_w[known], accumulate=True)
        return torch.topk(torch.sparse.mm(S, W), K, dim=0)

    alternatives = sorted({int(s) for s in args.splits.split(",") if s})
    jobs = {"topk auto": lambda: timed(lambda: topk(0)), "rank auto": lambda: timed(lambda: rank(0)),
            "scores route": lambda: timed(scores_route), "torch route": lambda: timed(torch_route),
            "topk cand_pos": lambda: timed(topk_perm), "rank cand_pos": lambda: timed(rank_perm)}
    for s in alternatives:
        jobs[f"topk n_splits={s}"] = (lambda s=s: timed(lambda: topk(s)))
        jobs[f"rank n_splits={s}"] = (lambda s=s: timed(lambda: rank(s)))
    for _ in range(2):  # warm-up
        for fn in jobs.values():
            fn()
    ms, last = {k: [] for k in jobs}, {}
    for _ in range(args.reps):  # alternating: every round times each thing once
        for k, fn in jobs.items():
            dt, out = fn()
            ms[k].append(dt)
            last[k] = out
    stat = lambda k: dict(ms=round(statistics.median(ms[k]), 3), ms_min_max=[round(min(ms[k]), 3), round(max(ms[k]), 3)])
    over = lambda a, b: round(statistics.median([x / y for x, y in zip(ms[a], ms[b])]), 2)
    row_len = (t[0][1:] - t[0][:-1]).float()
    base = {"probe": "cv-c1 top-N", "n_rows": n_rows, "nnz": int(cols.numel()), "longest_row": int(row_len.max()), "batch_users": B,
            "history_entries_of_the_batch": int(count.sum()), "stored_values_walked": int(row_len[e_rows[known]].sum()), "k": K, "R": R,
            "ranges": -(-n_rows // R), "auto_n_splits": auto, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    kernel_kth, torch_kth = last["topk auto"][1][:, K - 1], last["torch route"].values[K - 1]
    full = torch.isfinite(kernel_kth) & (torch_kth > 0)
    rel = ((kernel_kth - torch_kth).abs() / torch_kth.abs())[full]
    bound = 2 * 50 * U32 / (1 - 50 * U32)
    records = [dict(base, what="ebn_cv_topk_f32, automatic n_splits", **stat("topk auto"), torch_route=stat("torch route"),
                    scores_route=stat("scores route"), torch_over_kernel=over("torch route", "topk auto"),
                    scores_route_over_kernel=over("scores route", "topk auto"), users_compared=int(full.sum()),
                    largest_relative_difference_of_the_kth_score=float(rel.max()) if rel.numel() else 0.0, twice_the_bound=bound,
                    flags=flags.cpu().tolist()),
               dict(base, what="ebn_cv_target_rank_f32, automatic n_splits", **stat("rank auto"),
                    scores_route_over_kernel=over("scores route", "rank auto"), ranks_equal_5=int((last["rank auto"][0] == 5).sum()))]
    records.append(dict(base, what="both kernels with a cand_pos (a random permutation of the rows), automatic n_splits",
                        topk=stat("topk cand_pos"), rank=stat("rank cand_pos"), ranks_equal_5=int((last["rank cand_pos"][0] == 5).sum())))
    for s in alternatives:
        same = bool(torch.equal(last[f"topk n_splits={s}"][0], last["topk auto"][0]) and
                    torch.equal(last[f"topk n_splits={s}"][1].view(torch.int32), last["topk auto"][1].view(torch.int32)))
        records.append(dict(base, what=f"alternative: n_splits = {s}", n_splits=s, topk=stat(f"topk n_splits={s}"), rank=stat(f"rank n_splits={s}"),
                            same_bits_as_auto=same))
    for rec in records:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if rel.numel() and float(rel.max()) > bound:
        raise SystemExit("the kernel and the torch route differ by more than twice the bound")
    if int((last["rank auto"][0] == 5).sum()) != int((target >= 0).sum()):
        raise SystemExit("a target taken from slot 5 of a list does not rank 5th")


if __name__ == "__main__":
    main()
