"""Generates tests/golden/ranking_golden.npz by running the REFERENCE's own metric wrappers (src/ebrec/evaluation of
ebanalyse/ebnerd-benchmark, importable without TF / polars), one impression at a time, on seeded ragged impressions:

    python tests/golden/make_ranking_golden.py <path to the reference's src directory>

The reference never travels; the inputs and the per-row expected values do.  Two groups:
  main : a few thousand lists with both classes, mostly EB-NeRD-shaped (in-view mean about 11.6), plus the lengths at which the
         forms of csrc/ebn_rankmetrics.hip hand over (2, 15 / 16 / 17, 63 / 64 / 65, 250, 255 / 256 / 257, 1023 / 1024 / 1025) and
         one list past the LDS form (5000).  Scores are float32-representable, some are exactly 0 or 1 (the logloss clip), some
         lists have ties: between negatives only, between positives only, and between a positive and a negative (those are
         "tie-ambiguous": the reference's value then depends on its sort; at most 10 % of the group, asserted below);
  one  : lists with one class only (length 1 included): auc / logloss raise there (stored as NaN), mrr / ndcg of a list without
         a positive are NaN.
ref[m, l] = metric m (METRICS order) of list l, from `<Wrapper>.calculate([labels_l], [scores_l])` on list inputs."""
import sys
import warnings
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, sys.argv[1])
from ebrec.evaluation import (AccuracyScore, AucScore, F1Score, LogLossScore, MrrScore, NdcgScore,  # noqa: E402
                              RootMeanSquaredError)

METRICS = [AucScore(), MrrScore(), NdcgScore(k=5), NdcgScore(k=10), LogLossScore(), RootMeanSquaredError(),
           AccuracyScore(threshold=0.5), F1Score(threshold=0.5)]
EDGES = [2, 15, 16, 17, 63, 64, 65, 250, 255, 256, 257, 1023, 1024, 1025, 5000]
rng = np.random.default_rng(20261017)


def scores_of(n, mode):
    p = rng.random(n).astype(np.float32)
    if mode == "round2":
        p = np.round(p, 2).astype(np.float32)
    elif mode == "round1":
        p = np.round(p, 1).astype(np.float32)
    if n >= 4 and rng.random() < 0.15:
        p[rng.integers(0, n)] = 0.0
    if n >= 4 and rng.random() < 0.15:
        p[rng.integers(0, n)] = 1.0
    return p


def main_group():
    lens = [int(min(2 + rng.geometric(1 / 9.6), 120)) for _ in range(3000)]  # mean about 11.6
    lens += [n for n in EDGES for _ in range(3)][:-2]  # every edge three times, the 5000-long list once
    rng.shuffle(lens)
    L, P = [], []
    for i, n in enumerate(lens):
        mode = "round2" if i % 8 == 0 else ("round1" if i % 16 == 1 else ("pos_tie" if i % 16 == 2 else "plain"))
        p = scores_of(n, mode)
        y = np.zeros(n, np.uint8)
        n_pos = 1 if (i % 4 and mode != "pos_tie") else int(rng.integers(1 if mode != "pos_tie" else 2, max(2, min(n - 1, 1 + n // 3)) + 1))
        n_pos = min(n_pos, n - 1)
        y[rng.choice(n, size=n_pos, replace=False)] = 1
        if mode == "pos_tie" and n_pos >= 2:  # two positives share a score no negative has
            a, b = np.flatnonzero(y)[:2]
            p[b] = p[a]
        L.append(y)
        P.append(p)
    return L, P


def one_class_group():
    L, P = [], []
    for n in [1, 1, 2, 2, 3, 11, 16, 17, 40, 64, 65, 70, 300] * 3:
        L.append(np.full(n, len(L) % 2, np.uint8))
        P.append(scores_of(n, "round1" if len(L) % 5 == 0 else "plain"))
    return L, P


def reference_values(L, P):
    ref = np.full((len(METRICS), len(L)), np.nan)
    for l, (y, p) in enumerate(zip(L, P)):
        y, p = [int(v) for v in y], [float(v) for v in p]
        for m, metric in enumerate(METRICS):
            try:
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore")
                    ref[m, l] = metric.calculate([list(y)], [list(p)])
            except ValueError:
                pass  # one class: auc / logloss are undefined
    return ref


def ambiguous(y, p):
    eq = p[:, None] == p[None, :]
    return bool(np.any(eq & (y[:, None] != y[None, :])))


def pack(L, P):
    off = np.zeros(len(L) + 1, np.int64)
    np.cumsum([len(y) for y in L], out=off[1:])
    return np.concatenate(L).astype(np.uint8), np.concatenate(P).astype(np.float32), off


Lm, Pm = main_group()
Lo, Po = one_class_group()
share = np.mean([ambiguous(y, p) for y, p in zip(Lm, Pm)])
assert share <= 0.10, share
tied = np.mean([len(np.unique(p)) < len(p) for p in Pm])
out = {}
for name, (L, P) in (("main", (Lm, Pm)), ("one", (Lo, Po))):
    out[f"{name}_labels"], out[f"{name}_scores"], out[f"{name}_offsets"] = pack(L, P)
    out[f"{name}_ref"] = reference_values(L, P)
assert not np.isnan(out["main_ref"]).any()
out["metric_names"] = np.array([m.name for m in METRICS])
np.savez_compressed(Path(__file__).with_name("ranking_golden.npz"), **out)
print(f"main: {len(Lm)} lists, {out['main_scores'].size} candidates, mean length {np.mean([len(y) for y in Lm]):.2f}, "
      f"{tied:.1%} with ties, {share:.1%} tie-ambiguous; one-class: {len(Lo)} lists")
