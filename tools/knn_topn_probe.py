"""Times the history-kNN top-N kernels (csrc/ebn_knn_topk.hip) beside the two other ways to the same lists on the same GPU, in ONE
run, at knn-c1 (knn_probe.py: 125 541 rows, 200 000 training sequences, query histories of the same law, k = 100 of the 1000 most
recent, cosine, linear weights): the first `--batch` query histories, their neighbours from ONE ebn_knn_neighbours_f32 launch, every
catalogue row a candidate, top_n = 10, exclusion on (each history's own rows).

  topk / rank     ebn_knn_topk_f32 and ebn_knn_target_rank_f32 (targets: each user's own 5th slot) for n_splits = 0 (automatic) and
                  every alternative of `--splits`
  scores route    (i) the one existing way to these scores: ebn_knn_scores_f32 with every catalogue row as every user's candidate,
                  in blocks of `--score-block` users, the excluded rows set to -inf, torch.topk per block
  torch route     (ii) unfused: the neighbours' sims as a dense [n_seqs, batch] matrix (index_put_ with accumulate), torch.sparse.mm
                  of the postings CSR (row -> the sequences that hold it) with it, the excluded rows set to -inf, torch.topk

All are warmed up, then timed `--reps` rounds, ALTERNATING inside every round, with device events: median and min / max.  The three
k-th scores are fp32 sums of the same positive sims in different orders: each within the bound of tests/knn_cases.py of the exact
value -- (gamma_k + 2 u) |score| with the sims positive -- so two routes agree within twice that; the probe FAILS beyond it.
`--kernels-only` times the two kernels alone: the run for a library built with another range or form (EBNERD_HIP_LIB selects it;
csrc/ebn_knn_tile.h: -DEBN_KNT_R=2048 / 4096 / 8192, -DEBN_KNT_SHARED), `--label` names it in the record; the lists' checksum must
equal the default library's (all forms give the same bits).  Prints one JSON line per timed thing; `--out FILE` appends them
(default profiles/knn_topn_c1.jsonl).
usage: knn_topn_probe.py [--rows N] [--users N] [--batch 1024] [--splits 1,2,4] [--reps 5] [--kernels-only] [--label NAME] [--out FILE]"""
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
from ebrec.models.baselines import knn  # noqa: E402
from knn_probe import K as K_NBR, SAMPLE, KnnProblem  # noqa: E402
from popularity_probe import timed  # noqa: E402

U32 = 2.0 ** -24
TOP_N = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_541)
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--impressions", type=int, default=1000)  # the in-view lists of the underlying Problem: not used here
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--score-block", type=int, default=512)
    ap.add_argument("--splits", default="1,2,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--label", default="default build")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "knn_topn_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_topn_probe needs a GPU: nothing is measured without one")
    if args.reps < 5:
        raise SystemExit("at least 5 rounds")
    torch.cuda.set_device(0)
    P = KnnProblem(args)
    (p_indptr, p_seqs, s_indptr, s_items), scale = P.build()
    n_rows, n_seqs, B = P.n_rows, P.n_seqs, args.batch
    n_b = int(P.q_off_np[B])
    q_rows, q_off = P.q_rows[:n_b], P.q_off[:B + 1]
    seq, sim = knn.neighbours_call(p_indptr, p_seqs, n_seqs, scale, q_rows, P.q_w[:n_b], q_off, P.q_self[:B], SAMPLE, K_NBR)
    lens = q_off[1:] - q_off[:-1]
    owner = torch.repeat_interleave(torch.arange(B, device="cuda"), lens)
    exclude = torch.full((B, int(lens.max())), -1, dtype=torch.int32, device="cuda")
    exclude[owner, torch.arange(n_b, device="cuda") - q_off[owner]] = q_rows
    ex_known = q_rows >= 0
    ex_rows, ex_owner = q_rows[ex_known].long(), owner[ex_known]

    lib = _hip.lib()
    R, auto = int(lib.ebn_knn_topk_range()), int(lib.ebn_knn_topk_auto_splits(B, n_rows))
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    sets = (s_indptr, s_items, n_rows, None)
    topk = lambda s: knn.topk_call(*sets, seq, sim, None, B, None, n_rows, None, exclude, TOP_N, flags, s)
    target = topk(0)[0][:, 4].contiguous()
    rank = lambda s: knn.target_rank_call(*sets, seq, sim, None, B, None, n_rows, target, None, exclude, flags, s)

    # (i) the scores route: every catalogue row a candidate of every user of a block
    blk = min(args.score_block, B)
    all_rows = torch.arange(n_rows, dtype=torch.int32, device="cuda").repeat(blk)
    all_off = torch.arange(blk + 1, dtype=torch.int64, device="cuda") * n_rows

    def scores_route():
        vals = []
        for b0 in range(0, B, blk):
            b1 = min(b0 + blk, B)
            n = b1 - b0
            list_hist = torch.arange(b0, b1, dtype=torch.int32, device="cuda")
            s = knn.scores_call(s_indptr, s_items, n_rows, None, seq, sim, list_hist, all_rows[:n * n_rows], all_off[:n + 1]).view(n, n_rows)
            mine = (ex_owner >= b0) & (ex_owner < b1)
            s[ex_owner[mine] - b0, ex_rows[mine]] = float("-inf")
            vals.append(torch.topk(s, TOP_N, dim=1).values)
        return torch.cat(vals)

    # (ii) the torch route: the postings are the transposed sets, a CSR of [n_rows, n_seqs]
    def make_sparse():
        S = torch.sparse_csr_tensor(p_indptr, p_seqs.long(), torch.ones(p_seqs.numel(), device="cuda"), size=(n_rows, n_seqs))
        try:
            torch.sparse.mm(S, torch.zeros((n_seqs, 1), device="cuda"))
        except RuntimeError:  # no CSR product in this build: the COO form of the same matrix
            S = S.to_sparse_coo().coalesce()
        return S

    present = seq >= 0
    n_owner = torch.arange(B, device="cuda")[:, None].expand_as(seq)[present]
    n_seq, n_sim = seq[present].long(), sim[present]

    def torch_route():
        W = torch.zeros((n_seqs, B), dtype=torch.float32, device="cuda")
        W.index_put_((n_seq, n_owner), n_sim, accumulate=True)
        D = torch.sparse.mm(S, W)
        D[ex_rows, ex_owner] = float("-inf")
        return torch.topk(D, TOP_N, dim=0).values.t()

    alternatives = sorted({int(s) for s in args.splits.split(",") if s})
    jobs = {"topk auto": lambda: timed(lambda: topk(0)), "rank auto": lambda: timed(lambda: rank(0))}
    if not args.kernels_only:
        S = make_sparse()
        jobs["scores route"] = lambda: timed(scores_route)
        jobs["torch route"] = lambda: timed(torch_route)
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
    set_len = (s_indptr[1:] - s_indptr[:-1]).float()
    pos, score = last["topk auto"]
    checksum = int((pos.long() * 1000003 + score.view(torch.int32).long()).sum().item())
    base = {"probe": "knn-c1 top-N", "build": args.label, "n_rows": n_rows, "n_seqs": n_seqs, "nnz_sets": int(s_items.numel()),
            "mean_set": round(float(set_len.mean()), 2), "batch_users": B, "k_nbr": K_NBR, "sample_size": SAMPLE,
            "neighbours_of_the_batch": int(present.sum()), "set_rows_walked": int(set_len[n_seq].sum()), "top_n": TOP_N,
            "exclude_width": int(exclude.shape[1]), "R": R, "ranges": -(-n_rows // R), "auto_n_splits": auto, "reps": args.reps,
            "device": torch.cuda.get_device_name(0), "checksum_of_the_lists": checksum}
    records, failed = [], False
    first = dict(base, what="ebn_knn_topk_f32, automatic n_splits", **stat("topk auto"), flags=flags.cpu().tolist())
    if not args.kernels_only:
        kth = score[:, TOP_N - 1]
        gk = K_NBR * U32 / (1 - K_NBR * U32)
        agree = {}
        for name in ("scores route", "torch route"):
            other = last[name][:, TOP_N - 1]
            full = torch.isfinite(kth) & (other > 0)
            diff, bound = (kth - other).abs()[full], (2 * (gk + 2 * U32) * other.abs())[full]
            agree[name] = dict(users_compared=int(full.sum()), largest_difference_of_the_kth_score=float(diff.max()) if diff.numel() else 0.0,
                               largest_twice_the_bound=float(bound.max()) if bound.numel() else 0.0, within=bool((diff <= bound).all()))
            failed |= not agree[name]["within"]
        first.update(scores_route=stat("scores route"), torch_route=stat("torch route"), scores_route_over_kernel=over("scores route", "topk auto"),
                     torch_over_kernel=over("torch route", "topk auto"), agreement=agree)
    records.append(first)
    second = dict(base, what="ebn_knn_target_rank_f32, automatic n_splits", **stat("rank auto"), ranks_equal_5=int((last["rank auto"][0] == 5).sum()))
    if not args.kernels_only:
        second.update(scores_route_over_kernel=over("scores route", "rank auto"), torch_over_kernel=over("torch route", "rank auto"))
    records.append(second)
    for s in alternatives:
        same = bool(torch.equal(last[f"topk n_splits={s}"][0], pos) and torch.equal(last[f"topk n_splits={s}"][1].view(torch.int32), score.view(torch.int32)))
        records.append(dict(base, what=f"alternative: n_splits = {s}", n_splits=s, topk=stat(f"topk n_splits={s}"), rank=stat(f"rank n_splits={s}"),
                            same_bits_as_auto=same))
        failed |= not same
    for rec in records:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if failed:
        raise SystemExit("the routes' k-th scores differ by more than twice the bound, or a split count changed the bits")
    if int((last["rank auto"][0] == 5).sum()) != int((target >= 0).sum()):
        raise SystemExit("a target taken from slot 5 of a list does not rank 5th")


if __name__ == "__main__":
    main()
