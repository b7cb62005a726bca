"""Times the EASE baseline's entries (csrc/ebn_ease.hip, as ebrec/models/baselines/ease.py calls them) beside an unfused torch route
on the same GPU, in ONE run:

  ease-c1  cv-c1's sequences (covisit_probe.py): 200 000 user sequences of 5 to 50 articles under the Zipf law of pop-c1 over
           125 541 rows, restricted to the ``--items`` most-clicked rows (8192, then 16384), duplicates combined; 1 000 000
           impressions with the me-c1 in-view lengths over the kept rows (2 % unknown), each mapped to a user under the same law,
           scored against that user's training sequence; reg = 500

  kernel: ebn_ease_gram_i32, ebn_ease_system_f32, ebn_ease_invert_nb_f32 at NB = 32 / 64 / 128, ebn_ease_weights_f32 (in place),
          ebn_ease_scores_f32 -- each timed on its own
  torch:  the Gram matrix as a dense X (``index_put_``) and ``X.T @ X``, ``torch.linalg.cholesky`` + ``torch.cholesky_inverse``, the
          weights as a broadcast division, the scores by a gather of B[h, c] over the (item, history entry) pairs in blocks of
          2^25 pairs and an ``index_add_``

All are warmed up, then timed `--reps` rounds, ALTERNATING inside every round, with device events: median and min / max.  The
invert's share of the exact-fp32 MFMA peak (157.3 TFLOP/s) counts n^3 useful FLOP: n^3 / 3 each for the Cholesky factor, the
triangular inverse and the symmetric product.  The errors of both routes' inverses against each other and their residuals
max |A P - I| (fp64 product on the device) are reported next to kappa's stand-in, (trace(G) + reg) / reg.
Prints one JSON line per leg; `--out FILE` appends it (default profiles/ease_c1.jsonl).
usage: ease_probe.py [--items 8192 16384] [--users N] [--impressions N] [--reps 5] [--out FILE]"""
import argparse
import ctypes
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
from popularity_probe import zipf_rows  # noqa: E402

REG, PEAK_FLOPS, PAIR_BLOCK = 500.0, 157.3e12, 1 << 25
NBS = (32, 64, 128)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


class Problem:
    def __init__(self, args, n):
        gen = torch.Generator(device="cuda").manual_seed(args.seed)
        rng = np.random.default_rng(args.seed)
        self.n, self.n_users = n, args.users
        perm = torch.randperm(args.rows, device="cuda", generator=gen)
        h_len = rng.integers(5, 51, args.users)
        rows = zipf_rows(int(h_len.sum()), args.rows, gen, perm)
        owner = torch.repeat_interleave(torch.arange(args.users, device="cuda"), torch.from_numpy(h_len).cuda())
        pairs = torch.unique(owner * args.rows + rows)  # duplicates count once
        counts = torch.bincount(pairs % args.rows, minlength=args.rows)
        keep = torch.sort(torch.argsort(counts, descending=True, stable=True)[:n]).values
        new = torch.full((args.rows,), -1, dtype=torch.int64, device="cuda")
        new[keep] = torch.arange(n, device="cuda")
        r = new[rows]
        self.h_rows = r.to(torch.int32)  # the sequences as histories: -1 for a row that was cut
        self.h_off = torch.from_numpy(np.concatenate([[0], np.cumsum(h_len)]).astype(np.int64)).cuda()
        ok = (r >= 0).cpu().numpy()
        self.indptr, self.cols, _ = als._combine_device(owner.cpu().numpy()[ok], r.cpu().numpy()[ok], np.ones(int(ok.sum())), args.users, n, 1.0,
                                                        torch.device("cuda"))
        self.nnz = int(self.cols.numel())
        from metrics_probe import make_lists

        c_off = make_lists(args.impressions, seed=args.seed)[2]
        self.n_lists, self.n_cand = args.impressions, int(c_off[-1])
        self.c_off = torch.from_numpy(c_off).cuda()
        self.c_rows = zipf_rows(self.n_cand, n, gen, torch.randperm(n, device="cuda", generator=gen)).to(torch.int32)
        self.c_rows[torch.rand(self.n_cand, device="cuda", generator=gen) < 0.02] = -1
        self.list_hist = zipf_rows(args.impressions, args.users, gen, torch.randperm(args.users, device="cuda", generator=gen)).to(torch.int32)
        self.item_list = torch.repeat_interleave(torch.arange(self.n_lists, device="cuda"), self.c_off[1:] - self.c_off[:-1])
        # buffers of the kernel route
        self.G = torch.empty((n, n), dtype=torch.int32, device="cuda")
        self.A0 = torch.empty((n, n), dtype=torch.float32, device="cuda")
        self.A = torch.empty_like(self.A0)
        self.status = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.floats = int(_hip.lib().ebn_ease_workspace_floats(n))
        self.work = torch.empty(self.floats, dtype=torch.float32, device="cuda")
        self.scores = torch.empty(self.n_cand, dtype=torch.float32, device="cuda")

    # ---- the kernels
    def k_gram(self):
        _hip.call("ebn_ease_gram_i32", _hip.ptr(self.indptr), _hip.ptr(self.cols), self.n_users, self.nnz, self.n, _hip.ptr(self.G), self.n,
                  _hip.stream_handle())
        return self.G

    def k_system(self):
        _hip.call("ebn_ease_system_f32", _hip.ptr(self.G), self.n, self.n, ctypes.c_float(REG), _hip.ptr(self.A0), self.n, _hip.ptr(self.status),
                  _hip.stream_handle())
        return self.A0

    def k_invert(self, nb):
        _hip.call("ebn_ease_invert_nb_f32", _hip.ptr(self.A), self.n, self.n, _hip.ptr(self.work), self.floats,
                  ctypes.c_void_p(self.status.data_ptr() + 4), nb, _hip.stream_handle())
        return self.A

    def k_weights(self):
        _hip.call("ebn_ease_weights_f32", _hip.ptr(self.A), self.n, self.n, _hip.ptr(self.A), self.n, _hip.stream_handle())
        return self.A

    def k_scores(self, B):
        _hip.call("ebn_ease_scores_f32", _hip.ptr(B), self.n, self.n, _hip.ptr(self.h_rows), None, _hip.ptr(self.h_off), self.n_users,
                  int(self.h_rows.numel()), _hip.ptr(self.list_hist), _hip.ptr(self.c_rows), _hip.ptr(self.c_off), self.n_lists, self.n_cand,
                  _hip.ptr(self.scores), _hip.stream_handle())
        return self.scores

    # ---- the unfused torch route
    def t_gram(self):
        X = torch.zeros((self.n_users, self.n), dtype=torch.float32, device="cuda")
        owner = torch.repeat_interleave(torch.arange(self.n_users, device="cuda"), self.indptr[1:] - self.indptr[:-1])
        X.index_put_((owner, self.cols.long()), torch.ones((), device="cuda"))
        return X.T @ X

    def t_invert(self, A):
        return torch.cholesky_inverse(torch.linalg.cholesky(A))

    def t_weights(self, P):
        B = -P / P.diagonal()[None, :]
        B.fill_diagonal_(0.0)
        return B

    def t_scores(self, B):
        out = torch.zeros(self.n_cand, dtype=torch.float32, device="cuda")
        u = self.list_hist.long()[self.item_list]
        first, count = self.h_off[u], self.h_off[u + 1] - self.h_off[u]
        ends = torch.cumsum(count, 0)
        a = 0
        while a < self.n_cand:
            done = int(ends[a - 1]) if a else 0
            b = max(a + 1, int(torch.searchsorted(ends, torch.tensor(done + PAIR_BLOCK, device="cuda"), right=True)))
            c = count[a:b]
            item = torch.repeat_interleave(torch.arange(a, b, device="cuda"), c)
            entry = torch.arange(int(c.sum()), device="cuda") - torch.repeat_interleave(ends[a:b] - c - done, c) + first[item]
            h, cand = self.h_rows[entry].long(), self.c_rows[item].long()
            ok = (h >= 0) & (cand >= 0)
            out.index_add_(0, item[ok], B[h[ok], cand[ok]])
            a = b
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_541)
    ap.add_argument("--items", type=int, nargs="+", default=[8192, 16384])
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--impressions", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ease_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ease_probe needs a GPU: nothing is measured without one")
    if args.reps < 5:
        raise SystemExit("at least 5 rounds")
    torch.cuda.set_device(0)
    torch.backends.cuda.matmul.allow_tf32 = False
    for n in args.items:
        P = Problem(args, n)
        state = {}

        def invert(nb):
            P.A.copy_(P.A0)  # outside the timed region
            torch.cuda.synchronize()
            return events(lambda: P.k_invert(nb))

        def t_invert():
            A = P.A0.clone()
            torch.cuda.synchronize()
            return events(lambda: P.t_invert(A))

        def weights():
            invert(ease_nb)
            return events(P.k_weights)

        ease_nb = int(_hip.lib().ebn_ease_block())
        jobs = {"gram kernel": lambda: events(P.k_gram), "gram torch": lambda: events(P.t_gram), "system kernel": lambda: events(P.k_system)}
        jobs.update({f"invert kernel nb{nb}": (lambda nb=nb: invert(nb)) for nb in NBS})
        jobs.update({"invert torch": t_invert, "weights kernel": weights, "weights torch": lambda: events(lambda: P.t_weights(state["P_torch"])),
                     "scores kernel": lambda: events(lambda: P.k_scores(P.A)), "scores torch": lambda: events(lambda: P.t_scores(P.A))})
        ms, last = {k: [] for k in jobs}, {}
        for rnd in range(args.reps + 1):  # round 0 warms up; then alternating: every round times each thing once
            for k, fn in jobs.items():
                t, out = fn()
                if k == "invert torch":
                    state["P_torch"] = out
                if k.startswith("invert kernel"):
                    out = out.clone()
                if k in ("scores kernel", "scores torch"):
                    out = out.clone()
                if rnd:
                    ms[k].append(t)
                last[k] = out
        flag, info = (int(v) for v in P.status.cpu().numpy())
        stat = lambda k: dict(ms=round(statistics.median(ms[k]), 3), ms_min_max=[round(min(ms[k]), 3), round(max(ms[k]), 3)])
        ratio = lambda k, t: round(statistics.median([o / x for x, o in zip(ms[k], ms[t])]), 3)
        # ---- errors: the two routes against each other and their residuals in fp64
        A64 = P.A0.double()
        eye = torch.eye(n, dtype=torch.float64, device="cuda")
        Pt = state["P_torch"].double()
        trace = float(P.G.diagonal().double().sum())
        errors = {"kappa_upper_bound": (trace + REG) / REG, "torch_residual": float((A64 @ Pt - eye).abs().max())}
        for nb in NBS:
            Pk = last[f"invert kernel nb{nb}"].double()
            errors[f"nb{nb}"] = dict(residual=float((A64 @ Pk - eye).abs().max()), max_abs_difference_to_torch=float((Pk - Pt).abs().max()),
                                     symmetric_bit_for_bit=bool(torch.equal(last[f"invert kernel nb{nb}"], last[f"invert kernel nb{nb}"].T)))
        errors["max_abs_P"] = float(Pt.abs().max())
        gram_equal = bool(torch.equal(torch.tril(last["gram kernel"]).float(), torch.tril(last["gram torch"])))
        s_rel = float((last["scores kernel"] - last["scores torch"]).norm() / last["scores torch"].norm())
        rec = {"probe": "ease-c1", "n_items": n, "n_users": P.n_users, "nnz": P.nnz, "pairs": int(((P.indptr[1:] - P.indptr[:-1]) * (P.indptr[1:] - P.indptr[:-1] + 1) // 2).sum()),
               "reg": REG, "n_impressions": P.n_lists, "n_candidates": P.n_cand, "reps": args.reps, "device": torch.cuda.get_device_name(0),
               "count_flag": flag, "info": info, "block_of_the_library": ease_nb,
               "gram": dict(kernel=stat("gram kernel"), torch=stat("gram torch"), torch_over_kernel=ratio("gram kernel", "gram torch"),
                            lower_triangles_equal=gram_equal),
               "system": dict(kernel=stat("system kernel")),
               "invert": dict({f"kernel_nb{nb}": dict(stat(f"invert kernel nb{nb}"),
                                                      share_of_fp32_mfma_peak=round(n ** 3 / (statistics.median(ms[f"invert kernel nb{nb}"]) * 1e-3)
                                                                                    / PEAK_FLOPS, 4),
                                                      torch_over_kernel=ratio(f"invert kernel nb{nb}", "invert torch")) for nb in NBS},
                              torch=stat("invert torch"), useful_gflop=round(n ** 3 / 1e9, 1)),
               "weights": dict(kernel=stat("weights kernel"), torch=stat("weights torch"), torch_over_kernel=ratio("weights kernel", "weights torch")),
               "scores": dict(kernel=stat("scores kernel"), torch=stat("scores torch"), torch_over_kernel=ratio("scores kernel", "scores torch"),
                              relative_difference_of_the_routes=s_rel),
               "errors": errors}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del P, state, last, A64, Pt, eye
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
