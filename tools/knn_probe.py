"""Times the history-kNN baseline (csrc/ebn_knn.hip + the torch plumbing of ebrec/models/baselines/knn.py) beside an unfused torch
route on the same GPU, in ONE run:

  knn-c1  cv-c1's operands (covisit_probe.py): 125 541 rows, 200 000 training sequences of 5 to 50 rows under the Zipf law of pop-c1
          (2 % unknown); 200 000 query histories of the same law OVER THE SAME ROWS (the rank-to-row permutation of the training
          sequences: what is popular in the index is popular in the queries; linear weights; history u never uses sequence u); the
          me-c1 lists: 1 000 000 impressions, 12 069 397 items, each impression mapped to a query history under the same law;
          k = 100, sample_size = 1000, cosine

  a. the index build: ``knn_index_device`` (upload, composite keys, torch.sort, unique_consecutive, searchsorted) + the cosine scale
  b. ebn_knn_neighbours_f32 against the unfused route: the last occurrence of every (history, row) by a stable sort; per block of
     histories whose (item, posting-tail entry) pairs fit 1 GiB (48 bytes per pair: the tail position, the composite key, the sort's
     keys and indices, the run index, the weight) the pairs by repeat_interleave, a sort of ``history * n_seqs + sequence``,
     unique_consecutive and an ``index_add_`` of the weights per run (the segment sums), hist_self dropped, the last sample_size
     runs of every history scattered into a dense [histories, sample_size] matrix by recency rank, a stable descending sort of its
     rows (stable: ties keep the more recent first), the first k
  c. ebn_knn_scores_f32 against the unfused route over the SAME neighbours (the kernel's): per block of items whose (item,
     neighbour) pairs fit 1 GiB (32 bytes per pair) one searchsorted of ``sequence * n_rows + row`` over the composite keys of the
     sets, a masked sum over the neighbours, times the item scale (none here)

All are warmed up, then timed ``--reps`` rounds, ALTERNATING inside every round, with device events (the build, which has host work in
it, with a synchronised wall clock): median and min / max.  The float4-copy rate of the same run is the calibration the bytes of
the neighbour launch are set against.
AGREEMENT.  The torch route adds a candidate's weights in the order ``index_add_`` happens to take, the kernel in history order: the
sims agree within 2 gamma_50 |sim| slot by slot (sorted lists of perturbed values stay within the perturbation), and the ids are
equal except where two candidates' sims lie within that tolerance of each other (the routes may rank them the other way round) or
at a list's last slot (the cut) -- the probe ASSERTS both: a slot with another id must have a neighbouring slot within twice the
tolerance or be the last, and reports how many slots hold equal ids.  The scores agree within twice the bound of tests/knn_cases.py.
Prints one JSON line per timed thing; ``--out FILE`` appends them (default profiles/knn_c1.jsonl).
usage: knn_probe.py [--rows N] [--users N] [--impressions N] [--reps 5] [--out FILE]"""
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
from covisit_probe import Problem, wall  # noqa: E402
from ebrec.models.baselines import knn  # noqa: E402
from ebrec.models.baselines.content import history_weight_values  # noqa: E402
from metrics_probe import float4_copy_gbs  # noqa: E402
from popularity_probe import timed, zipf_rows  # noqa: E402

U = 2.0 ** -24
GIB = 1 << 30
K, SAMPLE = 100, 1000
NBR_PAIR_BYTES, SCORE_PAIR_BYTES = 48, 32


class KnnProblem:
    def __init__(self, args):
        self.cv = Problem(args)  # the training sequences (its histories), the lists and their history indices
        c = self.cv
        self.n_rows, self.n_seqs = c.n_rows, c.n_users
        gen = torch.Generator(device="cuda").manual_seed(args.seed + 1)
        rng = np.random.default_rng(args.seed + 1)
        q_len = rng.integers(5, 51, args.users)
        self.q_off_np = np.zeros(args.users + 1, np.int64)
        np.cumsum(q_len, out=self.q_off_np[1:])
        n = int(self.q_off_np[-1])
        self.q_rows = zipf_rows(n, args.rows, gen, c.perm).to(torch.int32)  # the training sequences' permutation: the same rows are popular
        self.q_rows[torch.rand(n, device="cuda", generator=gen) < 0.02] = -1
        self.q_w = torch.from_numpy(history_weight_values("linear", self.q_off_np).astype(np.float32)).cuda()
        self.q_off = torch.from_numpy(self.q_off_np).cuda()
        self.q_self = torch.arange(args.users, dtype=torch.int32, device="cuda")
        self.n_hists, self.n_hist_items = args.users, n
        self.index = self.scale = self.comp = self.nbr = None

    # ---- a. the build
    def build(self):
        c = self.cv
        ix = knn.knn_index_device(c.h_rows_np, c.h_off_np, self.n_rows, 2 ** 27, "cuda")
        return ix, torch.from_numpy(knn.knn_seq_scale_host(ix[2].cpu().numpy())).cuda()

    def set_index(self, ix, scale):
        self.index, self.scale = ix, scale
        p_indptr, p_seqs, s_indptr, s_items = ix
        self.comp = torch.repeat_interleave(torch.arange(self.n_seqs, device="cuda"), s_indptr[1:] - s_indptr[:-1]) * self.n_rows + s_items.long()
        # the query items of the torch route's blocks: counted once, on the host, for the block cuts
        q, row, w = self._items()
        tail = torch.minimum(p_indptr[row + 1] - p_indptr[row], torch.tensor(SAMPLE + 1, device="cuda"))
        per_hist = torch.zeros(self.n_hists, dtype=torch.int64, device="cuda").index_add_(0, q, tail).cpu().numpy()
        self.n_pairs = int(per_hist.sum())
        self.hist_blocks = _cuts(per_hist, GIB // NBR_PAIR_BYTES)
        self.item_blocks = _cuts(np.full(self.cv.n_items, K, np.int64), GIB // SCORE_PAIR_BYTES)

    # ---- b. the neighbours
    def k_neighbours(self):
        p_indptr, p_seqs = self.index[:2]
        return knn.neighbours_call(p_indptr, p_seqs, self.n_seqs, self.scale, self.q_rows, self.q_w, self.q_off, self.q_self, SAMPLE, K)

    def _items(self):
        """(history, row, weight) of every query item: the LAST occurrence of a present row, by a stable sort of history * n_rows + row"""
        q = torch.repeat_interleave(torch.arange(self.n_hists, device="cuda"), self.q_off[1:] - self.q_off[:-1])
        ok = self.q_rows >= 0
        key, order = torch.sort((q * self.n_rows + self.q_rows.long())[ok], stable=True)
        last = torch.ones_like(key, dtype=torch.bool)
        last[:-1] = key[1:] != key[:-1]
        key, at = key[last], torch.nonzero(ok).squeeze(1)[order[last]]
        return torch.div(key, self.n_rows, rounding_mode="floor"), key % self.n_rows, self.q_w[at]

    def t_neighbours(self):
        p_indptr, p_seqs = self.index[:2]
        q, row, w = self._items()
        tb = p_indptr[row + 1]
        ta = torch.maximum(p_indptr[row], tb - (SAMPLE + 1))
        first = torch.searchsorted(q, torch.arange(self.n_hists + 1, device="cuda"))  # the items of history u: [first[u], first[u + 1])
        out_seq = torch.full((self.n_hists, K), -1, dtype=torch.int32, device="cuda")
        out_sim = torch.full((self.n_hists, K), float("-inf"), dtype=torch.float32, device="cuda")
        for b0, b1 in zip(self.hist_blocks[:-1], self.hist_blocks[1:]):
            i0, i1 = int(first[b0]), int(first[b1])
            if i0 == i1:
                continue
            count = (tb - ta)[i0:i1]
            item = torch.repeat_interleave(torch.arange(i1 - i0, device="cuda"), count)
            start = torch.cumsum(count, 0) - count
            seq = p_seqs[torch.arange(item.numel(), device="cuda") - start[item] + ta[i0:i1][item]].long()
            key, order = torch.sort((q[i0:i1][item] - b0) * self.n_seqs + seq)
            runs, inverse = torch.unique_consecutive(key, return_inverse=True)
            dot = torch.zeros(runs.numel(), dtype=torch.float32, device="cuda").index_add_(0, inverse, w[i0:i1][item][order])
            u, s = torch.div(runs, self.n_seqs, rounding_mode="floor"), runs % self.n_seqs
            keep = s != self.q_self[b0:b1].long()[u]
            u, s, dot = u[keep], s[keep], dot[keep]
            end = torch.searchsorted(u, torch.arange(b1 - b0 + 1, device="cuda"))  # ascending ids inside every history
            rank = end[u + 1] - 1 - torch.arange(u.numel(), device="cuda")  # 0: the most recent
            near = rank < SAMPLE
            dense = torch.full((b1 - b0, SAMPLE), float("-inf"), dtype=torch.float32, device="cuda")
            ids = torch.full((b1 - b0, SAMPLE), -1, dtype=torch.int32, device="cuda")
            dense[u[near], rank[near]] = dot[near] * self.scale[s[near]]
            ids[u[near], rank[near]] = s[near].to(torch.int32)
            best, col = torch.sort(dense, dim=1, descending=True, stable=True)
            out_sim[b0:b1] = best[:, :K]
            out_seq[b0:b1] = torch.gather(ids, 1, col[:, :K])
        return out_seq, out_sim

    # ---- c. the scores
    def k_scores(self):
        c = self.cv
        return knn.scores_call(self.index[2], self.index[3], self.n_rows, None, self.nbr[0], self.nbr[1], c.list_hist, c.c_rows, c.c_off)

    def t_scores(self):
        c = self.cv
        seq, sim = self.nbr
        out = torch.zeros(c.n_items, dtype=torch.float32, device="cuda")
        lh, nnz = c.list_hist.long(), self.comp.numel()
        for i0, i1 in zip(self.item_blocks[:-1], self.item_blocks[1:]):
            u, row = lh[c.item_list[i0:i1]], c.c_rows[i0:i1].long()
            s = seq[u].long()
            key = s.clamp(min=0) * self.n_rows + row.clamp(min=0)[:, None]
            pos = torch.searchsorted(self.comp, key).clamp_(max=nnz - 1)
            hit = (s >= 0) & (row >= 0)[:, None] & (self.comp[pos] == key)
            out[i0:i1] = torch.where(hit, sim[u], torch.zeros((), device="cuda")).sum(1)
        return out


def _cuts(work, budget):
    """block boundaries over ``work`` (per element) so that a block's work stays within ``budget`` (at least one element a block)"""
    ends, cut, acc = np.cumsum(work), [0], 0
    while cut[-1] < work.size:
        nxt = max(int(np.searchsorted(ends, acc + budget, side="right")), cut[-1] + 1)
        cut.append(min(nxt, work.size))
        acc = int(ends[cut[-1] - 1])
    return cut


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_541)
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--impressions", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "knn_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_probe needs a GPU: nothing is measured without one")
    if args.reps < 5:
        raise SystemExit("at least 5 rounds")
    torch.cuda.set_device(0)
    P = KnnProblem(args)
    P.set_index(*P.build())
    P.nbr = P.k_neighbours()
    copy_gbs = float4_copy_gbs(10)
    jobs = {"index build": lambda: wall(P.build), "neighbour kernel": lambda: timed(P.k_neighbours), "neighbour torch": lambda: timed(P.t_neighbours),
            "score kernel": lambda: timed(P.k_scores), "score torch": lambda: timed(P.t_scores)}
    for fn in jobs.values():  # warm-up
        fn()
    ms, last = {k: [] for k in jobs}, {}
    for _ in range(args.reps):  # alternating: every round times each thing once
        for k, fn in jobs.items():
            t, out = fn()
            ms[k].append(t)
            last[k] = out
    stat = lambda k: dict(ms=round(statistics.median(ms[k]), 3), ms_min_max=[round(min(ms[k]), 3), round(max(ms[k]), 3)])
    p_indptr, p_seqs, s_indptr, s_items = P.index
    post_len = (p_indptr[1:] - p_indptr[:-1]).float()
    base = {"probe": "knn-c1", "n_rows": P.n_rows, "n_seqs": P.n_seqs, "n_entries": P.cv.n_hist_items, "nnz_postings": int(p_seqs.numel()),
            "longest_posting": int(post_len.max()), "n_hists": P.n_hists, "n_hist_items": P.n_hist_items, "k": K, "sample_size": SAMPLE,
            "similarity": "cosine", "n_tail_pairs": P.n_pairs, "n_impressions": P.cv.n_lists, "n_items": P.cv.n_items, "reps": args.reps,
            "float4_copy_gbs": round(copy_gbs, 1), "device": torch.cuda.get_device_name(0)}
    records = [dict(base, what="index build (upload, composite keys, sort, unique_consecutive, searchsorted, cosine scale)", **stat("index build"))]
    failed = False

    def versus(name, pairs, **more):
        ratios = [o / k for k, o in zip(ms[f"{name} kernel"], ms[f"{name} torch"])]
        km = statistics.median(ms[f"{name} kernel"])
        return dict(base, kernel=stat(f"{name} kernel"), torch=stat(f"{name} torch"), torch_over_kernel=round(statistics.median(ratios), 2),
                    torch_over_kernel_min_max=[round(min(ratios), 2), round(max(ratios), 2)], pairs_per_ns=round(pairs / (km * 1e6), 2), **more)

    (k_seq, k_sim), (t_seq, t_sim) = last["neighbour kernel"], last["neighbour torch"]
    gamma = 50 * U / (1 - 50 * U)
    finite = torch.isfinite(t_sim)
    tol = 2 * gamma * t_sim.abs()
    sims_agree = bool(torch.equal(finite, torch.isfinite(k_sim)) and ((k_sim - t_sim).abs()[finite] <= tol[finite]).all())
    # NEIGHBOURS EQUAL, up to what the two orders of addition can do: a slot whose ids differ must hold a sim within the tolerance
    # of the slot before or behind it (two candidates the routes rank the other way round), or be the list's last slot (the cut)
    differ = k_seq != t_seq
    gap = torch.full_like(k_sim, float("inf"))
    step = (k_sim[:, 1:] - k_sim[:, :-1]).abs()
    gap[:, 1:] = torch.minimum(gap[:, 1:], step)
    gap[:, :-1] = torch.minimum(gap[:, :-1], step)
    excused = gap <= 2 * tol
    excused[:, -1] = True
    ids_agree = bool((~differ | (excused & finite & torch.isfinite(k_sim))).all())
    tail_bytes = 4 * P.n_pairs + 8 * P.n_hists * K + 12 * P.n_hist_items
    rate = tail_bytes / 1e9 / (statistics.median(ms["neighbour kernel"]) * 1e-3)
    records.append(versus("neighbour", P.n_pairs, what="ebn_knn_neighbours_f32 against the unfused torch route", bytes_it_must_read_and_write=tail_bytes,
                          gb_per_s=round(rate, 1), share_of_float4_copy=round(rate / copy_gbs, 4), neighbours_found=int((k_seq >= 0).sum()),
                          slots_with_equal_ids=round(float((~differ).float().mean()), 6), slots_with_other_ids=int(differ.sum()),
                          other_ids_only_between_sims_within_tolerance_or_at_the_cut=ids_agree, sims_agree_within_twice_gamma_50=sims_agree))
    failed |= not (sims_agree and ids_agree)
    got, want = last["score kernel"], last["score torch"]
    gk = K * U / (1 - K * U)
    bound = 2 * (gk + 2 * U) * want.abs()  # the bound of tests/knn_cases.py with sum |sim| = the score itself: the sims are positive
    scores_agree = bool(((got - want).abs() <= bound).all())
    records.append(versus("score", P.cv.n_items * K, what="ebn_knn_scores_f32 against the unfused torch route (the kernel's neighbours)",
                          nonzero_scores=int((want != 0).sum()), largest_difference=float((got - want).abs().max()),
                          largest_twice_bound=float(bound.max()), routes_agree_within_twice_the_bound=scores_agree))
    failed |= not scores_agree
    for rec in records:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if failed:
        raise SystemExit("the two routes differ by more than they may")


if __name__ == "__main__":
    main()
