"""Times the score-blending kernels (csrc/ebn_blend.hip, as ebrec/models/ensemble.py calls them) beside unfused torch routes on the
same GPU, in ONE run:

  bl-c1  the me-c1 lists (metrics_probe.make_lists: 1 000 000 impressions, in-view mean 11.6, 0.2 % of 250), M = 6 float32 score
         columns with kinds raw, zscore, zscore, minmax, rank, rrf; one positive per list

  a. features   ebn_blend_features_f32: the [6, n] float32 features
  b. sums       one ebn_blend_sums_f64 launch (+ its closing launch) at the fitted weights
  c. combine    ebn_blend_combine_f64: transforms + weighted sum in one pass
  d. fit        ScoreBlend.fit from stacked device columns: features, then the Newton iteration's sums launches and M x M solves
  torch, two routes for each of a-d, the faster one is the yardstick:
     padded   lists sorted by length and cut into blocks whose [lists, Lmax] (for the ranks [lists, Lmax, Lmax]) tensors fit 1 GiB
     segment  flat segment operations: index_add_ / scatter_reduce_ over the item -> list map, ranks from two stable sorts

All are warmed up, then timed `--reps` rounds, ALTERNATING inside every round, with device events: median and min / max.  The sums
launch must read (4 M + 1) bytes per item plus the offsets; the probe reports that as a share of a float4 copy calibrated in the
same run.  Prints one JSON line per timed thing; `--out FILE` appends them (default profiles/blend_c1.jsonl).
With --no-torch only the kernels are timed (a quick A/B of two builds of the library through EBNERD_HIP_LIB).
usage: blend_probe.py [--lists N] [--reps 5] [--no-torch] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec.evaluation import RaggedLists  # noqa: E402
from ebrec.models import ensemble as en  # noqa: E402
from metrics_probe import float4_copy_gbs, make_lists  # noqa: E402
from popularity_probe import timed  # noqa: E402

GIB = 1 << 30
NAMES = ["raw", "zscore", "zscore", "minmax", "rank", "rrf"]
KINDS = [en.KINDS[k] for k in NAMES]
RRF_K, L2 = 60.0, 1e-3


class Problem:
    def __init__(self, n_lists, seed):
        labels, base, offsets = make_lists(n_lists, seed=seed)
        rng = np.random.default_rng(seed + 1)
        self.M, self.n, self.n_lists, self.offsets_host = len(KINDS), int(offsets[-1]), n_lists, offsets
        noise = rng.standard_normal((self.M, self.n)).astype(np.float32)
        scores = noise + (0.3 * np.arange(1, self.M + 1, dtype=np.float32))[:, None] * labels[None, :]  # every column knows a little
        scores[4] = np.round(scores[4] * 2)  # the ranked column has ties
        self.scores = torch.from_numpy(scores).cuda()
        self.labels = torch.from_numpy(labels).cuda()
        self.offsets = torch.from_numpy(offsets).cuda()
        self.params = [RRF_K if k == "rrf" else 0.0 for k in NAMES]
        self.length = self.offsets[1:] - self.offsets[:-1]
        self.lid = torch.repeat_interleave(torch.arange(n_lists, device="cuda"), self.length)
        self.start = self.offsets[:-1][self.lid]
        self.features, _ = en.blend_features_call(self.scores, self.offsets, KINDS, self.params)
        self.sums = en.BlendSums(self.features, self.labels, self.offsets)
        self.blend = self.k_fit()
        self.w = torch.from_numpy(self.blend.weights).cuda()
        # padded route: lists sorted by length, cut where [rows, L, L] floats would pass 1 GiB
        length = self.length.cpu().numpy()
        order = np.argsort(length, kind="stable")
        cuts = [0]
        while cuts[-1] < n_lists:
            a, lo, hi = cuts[-1], cuts[-1] + 1, n_lists
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if (mid - a) * int(length[order[mid - 1]]) ** 2 * 4 <= GIB else (lo, mid - 1)
            cuts.append(lo)
        self.order, self.cuts, self.len_host = torch.from_numpy(order).cuda(), cuts, length

    # ---- the kernels
    def k_features(self):
        return en.blend_features_call(self.scores, self.offsets, KINDS, self.params)[0]

    def k_sums(self):
        self.sums.launch(self.blend.weights)
        return self.sums.sums

    def k_combine(self):
        return en.blend_combine_call(self.scores, self.offsets, KINDS, self.params, self.blend.weights)[0]

    def k_fit(self):
        cols = [RaggedLists(self.scores[m], self.offsets_host) for m in range(self.M)]
        return en.ScoreBlend(transforms=NAMES, l2=L2, rrf_k=RRF_K).fit(RaggedLists(self.labels, self.offsets_host), cols)

    # ---- torch, segment operations
    def _seg_sum(self, v):
        return torch.zeros(self.n_lists, dtype=v.dtype, device="cuda").index_add_(0, self.lid, v)

    def _seg_ext(self, v, how):
        init = float("-inf") if how == "amax" else float("inf")
        return torch.full((self.n_lists,), init, dtype=v.dtype, device="cuda").scatter_reduce_(0, self.lid, v, how)

    def s_features(self):
        n_f, out = self.length.double(), torch.empty((self.M, self.n), dtype=torch.float32, device="cuda")
        for m, kind in enumerate(NAMES):
            s = self.scores[m].double()
            if kind == "raw":
                out[m] = self.scores[m]
            elif kind == "zscore":
                mean = self._seg_sum(s) / n_f
                d = s - mean[self.lid]
                sd = torch.sqrt(self._seg_sum(d * d) / n_f)
                out[m] = torch.where(sd[self.lid] == 0, torch.zeros((), dtype=torch.float64, device="cuda"), d / sd[self.lid])
            elif kind == "minmax":
                mn, mx = self._seg_ext(s, "amin"), self._seg_ext(s, "amax")
                span = (mx - mn)[self.lid]
                out[m] = torch.where(span == 0, torch.zeros((), dtype=torch.float64, device="cuda"), (s - mn[self.lid]) / span)
            else:
                by_score = torch.argsort(s, descending=True, stable=True)
                order = by_score[torch.argsort(self.lid[by_score], stable=True)]  # by list, then descending score
                ls, ll = s[order], self.lid[order]
                new = torch.ones(self.n, dtype=torch.bool, device="cuda")
                new[1:] = (ls[1:] != ls[:-1]) | (ll[1:] != ll[:-1])
                first = torch.nonzero(new)[:, 0]
                count = torch.diff(first, append=torch.tensor([self.n], device="cuda"))
                r_group = 1.0 + (first - self.offsets[:-1][ll[first]]).double() + 0.5 * (count - 1).double()
                r = torch.empty(self.n, dtype=torch.float64, device="cuda")
                r[order] = torch.repeat_interleave(r_group, count)
                nn = n_f[self.lid]
                out[m] = torch.where(nn == 1, torch.zeros((), dtype=torch.float64, device="cuda"), (nn - r) / (nn - 1)) if kind == "rank" else 1.0 / (RRF_K + r)
        return out

    def s_sums(self, features=None, w=None):
        F = (self.features if features is None else features).double()
        w = self.w if w is None else w
        y = self.labels.double()
        n_pos = self._seg_sum(y)
        used = (n_pos > 0) & (n_pos < self.length)
        keep = used[self.lid].double()
        z = w @ F
        zc = z - self._seg_ext(z, "amax")[self.lid]
        e = torch.exp(zc)
        S = self._seg_sum(e)
        p = e / S[self.lid] * keep
        t = y / n_pos.clamp(min=1)[self.lid] * keep
        loss = -(t * (zc - torch.log(S)[self.lid])).sum()
        u = torch.stack([self._seg_sum(p * F[m]) for m in range(self.M)])
        C = F - u[:, self.lid]
        H = (C * p) @ C.T
        g = F @ (p - t)
        return torch.cat([loss[None], g, H[torch.triu_indices(self.M, self.M).unbind()]]), int(used.sum())

    def s_combine(self):
        return self.w @ self.s_features().double()

    def _torch_fit(self, features_fn, sums_fn):
        """the Newton iteration of ScoreBlend._newton over a torch route"""
        F = features_fn()
        blend = en.ScoreBlend(transforms=NAMES, l2=L2, rrf_k=RRF_K)

        def fn(w):
            sums, n = sums_fn(F, torch.from_numpy(np.asarray(w, np.float64)).cuda())
            return sums.cpu().numpy(), np.array([n, 0, 0])
        return blend._newton(fn, self.M)[0]

    def s_fit(self):
        return self._torch_fit(self.s_features, self.s_sums)

    # ---- torch, padded blocks
    def _blocks(self):
        for a, b in zip(self.cuts[:-1], self.cuts[1:]):
            L = int(self.len_host[self.order[b - 1].item()])
            if L == 0:
                continue
            rows = self.order[a:b]
            slot = torch.arange(L, device="cuda")[None, :]
            live = slot < self.length[rows][:, None]
            item = (self.offsets[:-1][rows][:, None] + slot).clamp_(max=self.n - 1)
            yield rows, live, item

    def p_features(self):
        out = torch.empty((self.M, self.n), dtype=torch.float32, device="cuda")
        zero = torch.zeros((), dtype=torch.float64, device="cuda")
        for rows, live, item in self._blocks():
            n_f = live.sum(1, keepdim=True).double()
            for m, kind in enumerate(NAMES):
                s = self.scores[m][item].double()
                if kind == "raw":
                    f = s
                elif kind == "zscore":
                    d = (s - (s * live).sum(1, keepdim=True) / n_f) * live
                    sd = torch.sqrt((d * d).sum(1, keepdim=True) / n_f)
                    f = torch.where(sd == 0, zero, d / sd)
                elif kind == "minmax":
                    mn = torch.where(live, s, torch.full_like(s, float("inf"))).amin(1, keepdim=True)
                    mx = torch.where(live, s, torch.full_like(s, float("-inf"))).amax(1, keepdim=True)
                    f = torch.where(mx == mn, zero, (s - mn) / (mx - mn))
                else:
                    s32 = self.scores[m][item]
                    gt = ((s32[:, None, :] > s32[:, :, None]) & live[:, None, :]).sum(2)
                    eq = ((s32[:, None, :] == s32[:, :, None]) & live[:, None, :]).sum(2)
                    r = 1.0 + gt.double() + 0.5 * (eq - 1).double()
                    f = torch.where(n_f == 1, zero, (n_f - r) / (n_f - 1)) if kind == "rank" else 1.0 / (RRF_K + r)
                out[m][item[live]] = f[live].float()
        return out

    def p_sums(self, features=None, w=None):
        Fall = self.features if features is None else features
        w = self.w if w is None else w
        total, n_used = torch.zeros(en.n_entries(self.M), dtype=torch.float64, device="cuda"), 0
        iu = torch.triu_indices(self.M, self.M).unbind()
        for rows, live, item in self._blocks():
            F = Fall[:, item].double() * live  # [M, R, L]
            y = self.labels[item].double() * live
            n_pos = y.sum(1, keepdim=True)
            used = ((n_pos > 0) & (n_pos < live.sum(1, keepdim=True)))
            z = torch.einsum("m,mrl->rl", w, F).masked_fill(~live, float("-inf"))
            zc = z - z.amax(1, keepdim=True)
            e = torch.exp(zc)
            S = e.sum(1, keepdim=True)
            keep = used.double()
            p = e / S * keep
            t = y / n_pos.clamp(min=1) * keep
            loss = -(t * torch.where(live, zc - torch.log(S), torch.zeros_like(zc))).sum()
            u = torch.einsum("rl,mrl->mr", p, F)
            C = (F - u[:, :, None]) * live
            H = torch.einsum("rl,arl,brl->ab", p, C, C)
            g = torch.einsum("rl,mrl->m", p - t, F)
            total += torch.cat([loss[None], g, H[iu]])
            n_used += int(used.sum())
        return total, n_used

    def p_combine(self):
        return self.w @ self.p_features().double()

    def p_fit(self):
        return self._torch_fit(self.p_features, self.p_sums)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-torch", action="store_true", help="time the kernels only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "blend_c1.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blend_probe needs a GPU: nothing is measured without one")
    if args.reps < 5:
        raise SystemExit("at least 5 rounds")
    torch.cuda.set_device(0)
    copy_gbs = float4_copy_gbs(10)
    P = Problem(args.lists, args.seed)
    things = ("features", "sums", "combine", "fit")
    jobs = {}
    for name in things:
        for route, prefix in (("kernel", "k_"),) if args.no_torch else (("kernel", "k_"), ("segment", "s_"), ("padded", "p_")):
            jobs[f"{name} {route}"] = (lambda fn: (lambda: timed(fn)))(getattr(P, prefix + name))
    for fn in jobs.values():  # warm-up
        fn()
    ms, last = {k: [] for k in jobs}, {}
    for _ in range(args.reps):  # alternating: every round times each thing once
        for k, fn in jobs.items():
            t, out = fn()
            ms[k].append(t)
            last[k] = out
    stat = lambda k: dict(ms=round(statistics.median(ms[k]), 3), ms_min_max=[round(min(ms[k]), 3), round(max(ms[k]), 3)])
    value = {"features": lambda o: o.double(), "sums": lambda o: (o[0] if isinstance(o, tuple) else o).double(), "combine": lambda o: o,
             "fit": lambda o: torch.as_tensor(o.weights if hasattr(o, "weights") else o).double()}
    base = {"probe": "bl-c1", "n_lists": P.n_lists, "n_items": P.n, "M": P.M, "kinds": NAMES, "l2": L2, "reps": args.reps,
            "float4_copy_gbs": round(copy_gbs, 1), "fit_iterations": len(P.blend.losses) - 1, "fit_converged": bool(P.blend.converged),
            "fit_weights": [round(float(w), 6) for w in P.blend.weights], "device": torch.cuda.get_device_name(0)}
    for name in things:
        k = f"{name} kernel"
        if args.no_torch:
            print(json.dumps(dict(base, what=name, kernel=stat(k), library=os.environ.get("EBNERD_HIP_LIB", "in-tree"))), flush=True)
            continue
        routes = {r: statistics.median(ms[f"{name} {r}"]) for r in ("segment", "padded")}
        best = min(routes, key=routes.get)
        ratios = [o / kk for kk, o in zip(ms[k], ms[f"{name} {best}"])]
        got, want = value[name](last[k]).cpu(), value[name](last[f"{name} {best}"]).cpu()
        ok = torch.isfinite(want) & torch.isfinite(got)
        rec = dict(base, what=name, kernel=stat(k), torch_segment=stat(f"{name} segment"), torch_padded=stat(f"{name} padded"), torch_route=best,
                   torch_over_kernel=round(statistics.median(ratios), 2), torch_over_kernel_min_max=[round(min(ratios), 2), round(max(ratios), 2)],
                   largest_difference_of_the_routes=float((got[ok] - want[ok]).abs().max()), largest_value=float(want[ok].abs().max()))
        if name == "sums":
            need = (4 * P.M + 1) * P.n + 8 * (P.n_lists + 1)
            rate = need / (statistics.median(ms[k]) * 1e-3) / 1e9
            rec.update(bytes_it_must_read=need, read_gbs=round(rate, 1), share_of_float4_copy=round(rate / copy_gbs, 4))
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
