"""Times the EASE top-N kernels (csrc/ebn_ease_topk.hip) beside an unfused torch route on the same GPU, in ONE run, at ease-c1's
operands (ease_probe.py: 200 000 user sequences of 5 to 50 Zipf rows restricted to the 8192, then the 16384 most-clicked rows, B
fitted by the library's own entries at reg 500): every user's own sequence is its history, every kept row a candidate, k = 10, the
history's rows excluded, n_splits automatic.

  topk / rank     ebn_ease_topk_f32 and ebn_ease_target_rank_f32 (targets: each user's own 5th slot) over all users in one launch
  torch route     unfused: per block of users (score blocks of at most 1 GiB) a dense X [block, n] from the histories (index_put_ with
                  accumulate), X @ B, the excluded entries masked to -inf, then torch.topk -- or, for the ranks, a gather of the
                  target's score and a comparison count
  alternatives    n_splits in `--splits`; and, for every `--variant NAME=PATH` (a build of the library with csrc/ebn_ease_topk.hip
                  under other flags, tools/build_variant.sh: -DEBN_EZK_V=2 / 4 the range width, -DEBN_EZK_EX_DIRECT the exclusion as
                  compares, -DEBN_EZK_SPLIT_X the split as the fast grid dimension), both entries of that build on `--variant-users`
                  users next to the in-tree build on the same users

All are warmed up, then timed `--reps` rounds, ALTERNATING inside every round, with device events: median and min / max.  The two
routes' scores are two fp32 evaluations of the same sum of m <= 50 products; each is within (m + 2) u / (1 - (m + 2) u) sum |p_j| of
the exact value, so where both list a (user, article) pair their scores differ by at most 2 (m + 2) 2^-24 sum_j |B[h_j, c]| (the
bound of tests/test_ease_topn_cpu.py).  The probe ASSERTS that the ids of the two routes are equal in every slot where the scores of
the two routes differ by more than that bound.  The row reads the kernel must make, entries x n x 4 bytes, over its time are
reported as a share of the float4-copy rate measured in the same run (1 GiB through ebn_gather_rows_f32).
Prints one JSON line per leg; `--out FILE` appends them (default profiles/ease_topn_c1.jsonl).
usage: ease_topn_probe.py [--items 8192 16384] [--users N] [--splits 1,2,4] [--variant NAME=PATH ...] [--reps 5] [--out FILE]"""
import argparse
import ctypes
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
from ebrec.models.baselines import ease as ez  # noqa: E402
from ease_probe import REG, Problem, events  # noqa: E402
from npa_recommend_probe import float4_copy_gbs  # noqa: E402

U32, K, SCORE_BLOCK = 2.0 ** -24, 10, 1 << 28  # floats of one score block: 1 GiB


def load_variant(path):
    handle = ctypes.CDLL(str(path))
    for name, (res, argt) in _hip.declared_functions().items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, argt
    return handle


def exclusion_lists(h_rows, h_off, n_users):
    """[U, X] int32: every history's distinct known rows, padded with -1 (the histories hold at most 50 entries)"""
    count = (h_off[1:] - h_off[:-1])[:n_users]
    X = int(count.max())
    owner = torch.repeat_interleave(torch.arange(n_users, device="cuda"), count)
    slot = torch.arange(owner.numel(), device="cuda") - (torch.cumsum(count, 0) - count)[owner]
    ex = torch.full((n_users, X), -1, dtype=torch.int32, device="cuda")
    ex[owner, slot] = h_rows[:owner.numel()]
    return ex.contiguous(), owner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_541)
    ap.add_argument("--items", type=int, nargs="+", default=[8192, 16384])
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--impressions", type=int, default=1000)  # the in-view lists of ease_probe's Problem: not used here
    ap.add_argument("--splits", default="1,2,4")
    ap.add_argument("--variant", action="append", default=[])
    ap.add_argument("--variant-users", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ease_topn_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ease_topn_probe needs a GPU: nothing is measured without one")
    if args.reps < 5:
        raise SystemExit("at least 5 rounds")
    torch.cuda.set_device(0)
    torch.backends.cuda.matmul.allow_tf32 = False
    lib = _hip.lib()
    variants = {v.rsplit("=", 1)[0]: load_variant(v.rsplit("=", 1)[1]) for v in args.variant}
    copy_gbs = float4_copy_gbs()
    for n in args.items:
        P = Problem(args, n)
        P.k_gram()
        P.k_system()
        P.A.copy_(P.A0)
        P.k_invert(int(lib.ebn_ease_block()))
        B = P.k_weights()
        torch.cuda.synchronize()
        assert [int(v) for v in P.status.cpu()] == [0, 0]
        U = P.n_users
        ex, owner = exclusion_lists(P.h_rows, P.h_off, U)
        X = ex.shape[1]
        e_rows = P.h_rows[:owner.numel()].long()
        known = e_rows >= 0
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        hist = (P.h_rows, None, P.h_off)
        topk = lambda s=0, users=U: ez.topk_call(B, *hist, None, users, None, n, None, ex[:users], K, flags, s)
        target = topk()[0][:, 4].contiguous()
        rank = lambda s=0, users=U: ez.rank_call(B, *hist, None, users, None, n, target[:users], None, ex[:users], flags, s)

        block = max(1, SCORE_BLOCK // n)
        first_entry = P.h_off[:U + 1]

        def scores_of(a, b):
            """the masked score block of the users [a, b)"""
            lo, hi = int(first_entry[a]), int(first_entry[b])
            Xd = torch.zeros((b - a, n), dtype=torch.float32, device="cuda")
            sel = known[lo:hi]
            Xd.index_put_((owner[lo:hi][sel] - a, e_rows[lo:hi][sel]), torch.ones((), device="cuda"), accumulate=True)
            S = Xd @ B
            S[owner[lo:hi][sel] - a, e_rows[lo:hi][sel]] = float("-inf")
            return S

        def torch_topk():
            out = [torch.topk(scores_of(a, min(a + block, U)), K, dim=1) for a in range(0, U, block)]
            return torch.cat([o.indices for o in out]), torch.cat([o.values for o in out])

        def torch_rank():
            ranks = []
            for a in range(0, U, block):
                b = min(a + block, U)
                S, t = scores_of(a, b), target[a:b].long()
                ts = S.gather(1, t.clamp(min=0)[:, None])
                col = torch.arange(n, device="cuda")[None, :]
                ahead = ((S > ts) | ((S == ts) & (col < t[:, None]))).sum(1)
                ranks.append(torch.where(t >= 0, ahead + 1, torch.zeros_like(ahead)))
            return torch.cat(ranks)

        alternatives = sorted({int(s) for s in args.splits.split(",") if s})
        jobs = {"topk": lambda: events(topk), "rank": lambda: events(rank), "torch topk": lambda: events(torch_topk),
                "torch rank": lambda: events(torch_rank)}
        for s in alternatives:
            jobs[f"topk n_splits={s}"] = (lambda s=s: events(lambda: topk(s)))
            jobs[f"rank n_splits={s}"] = (lambda s=s: events(lambda: rank(s)))
        Uv = min(args.variant_users, U)
        if variants:
            jobs["topk in-tree, variant users"] = lambda: events(lambda: topk(0, Uv))
            jobs["rank in-tree, variant users"] = lambda: events(lambda: rank(0, Uv))
        v_out = {name: (torch.empty(Uv, K, dtype=torch.int32, device="cuda"), torch.empty(Uv, K, dtype=torch.float32, device="cuda"),
                        torch.empty(Uv, dtype=torch.int32, device="cuda"), torch.empty(Uv, dtype=torch.int32, device="cuda"),
                        torch.empty(Uv, dtype=torch.float32, device="cuda")) for name in variants}
        ws = torch.empty(1 << 26, dtype=torch.uint8, device="cuda")
        head = (_hip.ptr(B), n, B.stride(0), _hip.ptr(P.h_rows), None, _hip.ptr(P.h_off), int(P.h_off.numel() - 1), int(P.h_rows.numel()), None,
                None, n)
        for name, h in variants.items():
            o = v_out[name]

            def v_topk(h=h, o=o):
                rc = h.ebn_ease_topk_f32(*head, None, _hip.ptr(ex), X, K, 0, _hip.ptr(o[0]), _hip.ptr(o[1]), _hip.ptr(flags), _hip.ptr(ws),
                                         ws.numel(), Uv, _hip.stream_handle())
                assert rc == 0, rc
                return o[0], o[1]

            def v_rank(h=h, o=o):
                rc = h.ebn_ease_target_rank_f32(*head, _hip.ptr(target), None, _hip.ptr(ex), X, 0, _hip.ptr(o[2]), _hip.ptr(o[3]), _hip.ptr(o[4]),
                                                _hip.ptr(flags), _hip.ptr(ws), ws.numel(), Uv, _hip.stream_handle())
                assert rc == 0, rc
                return o[2], o[3], o[4]

            jobs[f"topk variant {name}"] = (lambda f=v_topk: events(f))
            jobs[f"rank variant {name}"] = (lambda f=v_rank: events(f))
        ms, last = {k: [] for k in jobs}, {}
        for rnd in range(args.reps + 1):  # round 0 warms up; then alternating: every round times each thing once
            for k, fn in jobs.items():
                t, out = fn()
                if rnd:
                    ms[k].append(t)
                last[k] = tuple(x.clone() for x in out) if isinstance(out, tuple) else out.clone()
        stat = lambda k: dict(ms=round(statistics.median(ms[k]), 3), ms_min_max=[round(min(ms[k]), 3), round(max(ms[k]), 3)])
        over = lambda a, b: round(statistics.median([x / y for x, y in zip(ms[a], ms[b])]), 2)

        # ---- the two routes against each other: ids equal wherever the scores differ by more than the bound
        k_pos, k_score = last["topk"]
        t_pos, t_score = last["torch topk"]
        m_present = torch.zeros(U, dtype=torch.int64, device="cuda").index_add_(0, owner[known], torch.ones_like(owner[known]))
        absB = B.abs()
        bound = torch.zeros((U, K), dtype=torch.float64, device="cuda")
        for pos in (k_pos.long(), t_pos):  # sum_j |B[h_j, c]| for the listed columns of either route: the larger of the two bounds
            col = pos.clamp(min=0)
            sums = torch.zeros((U, K), dtype=torch.float64, device="cuda")
            sums.index_put_((owner[known][:, None].expand(-1, K), torch.arange(K, device="cuda")[None, :].expand(int(known.sum()), -1)),
                            absB[e_rows[known][:, None], col[owner[known]]].double(), accumulate=True)
            bound = torch.maximum(bound, 2.0 * (m_present[:, None] + 2).double() * U32 * sums)
        full = k_pos[:, K - 1] >= 0
        diff = (k_score.double() - t_score.double()).abs()
        apart = (diff > bound) & full[:, None]
        ids_differ = (k_pos.long() != t_pos) & full[:, None]
        unexplained = int((apart & ids_differ).sum())
        r_kernel, r_torch = last["rank"][0].long(), last["torch rank"]
        bytes_rows = float(known.sum()) * n * 4
        base = {"probe": "ease-c1 top-N", "n_items": n, "n_users": U, "history_entries": int(owner.numel()), "present_entries": int(known.sum()),
                "k": K, "X": X, "R": int(lib.ebn_ease_topk_range()), "auto_n_splits": int(lib.ebn_ease_topk_auto_splits(U, n)), "reg": REG,
                "reps": args.reps, "device": torch.cuda.get_device_name(0), "float4_copy_gbs": round(copy_gbs, 1)}
        rec = dict(base, what="ebn_ease_topk_f32 / ebn_ease_target_rank_f32, automatic n_splits, beside the unfused torch route",
                   topk=dict(stat("topk"), torch=stat("torch topk"), torch_over_kernel=over("torch topk", "topk"),
                             row_read_gbs=round(bytes_rows / statistics.median(ms["topk"]) / 1e6, 1),
                             row_reads_share_of_float4_copy=round(bytes_rows / statistics.median(ms["topk"]) / 1e6 / copy_gbs, 3)),
                   rank=dict(stat("rank"), torch=stat("torch rank"), torch_over_kernel=over("torch rank", "rank"),
                             row_read_gbs=round(bytes_rows / statistics.median(ms["rank"]) / 1e6, 1),
                             row_reads_share_of_float4_copy=round(bytes_rows / statistics.median(ms["rank"]) / 1e6 / copy_gbs, 3)),
                   users_with_full_lists=int(full.sum()), slots_with_other_ids=int(ids_differ.sum()),
                   slots_with_scores_apart_by_more_than_the_bound=int(apart.sum()), slots_with_other_ids_and_scores_apart=unexplained,
                   ranks_equal_5=int((r_kernel == 5).sum()), ranks_equal_between_the_routes=int((r_kernel == r_torch).sum()),
                   flags=flags.cpu().tolist())
        records = [rec]
        for s in alternatives:
            same = bool(torch.equal(last[f"topk n_splits={s}"][0], k_pos) and torch.equal(last[f"topk n_splits={s}"][1].view(torch.int32), k_score.view(torch.int32)))
            records.append(dict(base, what=f"alternative: n_splits = {s}", n_splits=s, topk=stat(f"topk n_splits={s}"), rank=stat(f"rank n_splits={s}"),
                                same_bits_as_auto=same))
        for name in variants:
            vp, vs = last[f"topk variant {name}"]
            same = bool(torch.equal(vp, k_pos[:Uv]) and torch.equal(vs.view(torch.int32), k_score[:Uv].view(torch.int32)) and
                        torch.equal(last[f"rank variant {name}"][0], last["rank"][0][:Uv]))
            records.append(dict(base, what=f"alternative build: {name}", users=Uv, R_of_the_build=int(variants[name].ebn_ease_topk_range()),
                                topk=stat(f"topk variant {name}"), rank=stat(f"rank variant {name}"),
                                in_tree_topk=stat("topk in-tree, variant users"), in_tree_rank=stat("rank in-tree, variant users"),
                                variant_over_in_tree_topk=over(f"topk variant {name}", "topk in-tree, variant users"),
                                variant_over_in_tree_rank=over(f"rank variant {name}", "rank in-tree, variant users"), same_bits_as_in_tree=same))
        for r in records:
            line = json.dumps(r)
            print(line, flush=True)
            if args.out:
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        if unexplained:
            raise SystemExit(f"{unexplained} slots hold other ids although their scores differ by more than the bound")
        if int((r_kernel == 5).sum()) != int((target >= 0).sum()):
            raise SystemExit("a target taken from slot 5 of a list does not rank 5th")
        del P, B, last, absB
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
