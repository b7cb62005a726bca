"""Shared by the ranking-metric tests: the reference-generated fixture tests/golden/ranking_golden.npz (made by
tests/golden/make_ranking_golden.py), the eight metrics in its row order, and numpy restatements used as the tests' yardsticks."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).parent / "golden" / "ranking_golden.npz"
NAMES = ["auc", "mrr", "ndcg@5", "ndcg@10", "logloss", "rmse", "accuracy", "f1"]
SLOTS = [(0, 0.0), (1, 0.0), (2, 5.0), (2, 10.0), (3, 0.0), (4, 0.0), (5, 0.5), (6, 0.5)]  # (EBN_RM_* kind, param) per row
RANKED_ROWS = (1, 2, 3)  # mrr, ndcg@5, ndcg@10: the rows that depend on the order inside a tie group
TWO_CLASS_ROWS = (0, 4)  # auc, logloss: undefined on a one-class list


def metrics():
    from ebrec.evaluation import (AccuracyScore, AucScore, F1Score, LogLossScore, MrrScore, NdcgScore, RootMeanSquaredError)

    return [AucScore(), MrrScore(), NdcgScore(k=5), NdcgScore(k=10), LogLossScore(), RootMeanSquaredError(),
            AccuracyScore(threshold=0.5), F1Score(threshold=0.5)]


def load(group):
    """{labels uint8 [n_items], scores float32 [n_items], offsets int64 [n_lists + 1], ref float64 [8, n_lists]}"""
    g = np.load(GOLDEN)
    assert list(g["metric_names"]) == NAMES
    return {k: g[f"{group}_{k}"] for k in ("labels", "scores", "offsets", "ref")}


def split(flat, offsets):
    return [flat[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


def flags_numpy(labels, scores, offsets):
    """bit 0: two equal scores of the list carry different labels; bit 1: a non-finite score -- the definitions, list by list"""
    from ebrec.evaluation.device_metrics import tie_ambiguous_and_nonfinite

    out = np.zeros(len(offsets) - 1, np.uint8)
    for l, (y, s) in enumerate(zip(split(labels, offsets), split(scores, offsets))):
        tie, bad = tie_ambiguous_and_nonfinite(y, s)
        out[l] = (1 if tie else 0) | (2 if bad else 0)
    return out


def host_values(labels, scores, offsets):
    """[8, n_lists] from the repository's host wrappers on list inputs, one impression at a time; NaN where they raise"""
    import warnings

    ms = metrics()
    out = np.full((len(ms), len(offsets) - 1), np.nan)
    for l, (y, s) in enumerate(zip(split(labels, offsets), split(scores, offsets))):
        y, s = [int(v) for v in y], [float(v) for v in s]
        for m, metric in enumerate(ms):
            try:
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore")
                    out[m, l] = metric.calculate([list(y)], [list(s)])
            except ValueError:
                pass
    return out


def counting_values(y, s):
    """The eight values of one list the way csrc/ebn_rankmetrics.hip takes them: ranks by counting (ties in index order), auc from
    integer pair counts, everything in float64."""
    y, s = np.asarray(y).astype(np.int64), np.asarray(s)
    n, n_pos = len(y), int(y.sum())
    gt = (s[None, :] > s[:, None]).sum(1)
    eq = s[None, :] == s[:, None]
    rank = 1 + gt + np.tril(eq, -1).sum(1)
    nan = float("nan")
    s64 = s.astype(np.float64)
    out = []
    neg = y == 0
    w2 = sum(2 * int((neg & (s < s[i])).sum()) + int((neg & (s == s[i])).sum()) for i in np.flatnonzero(y))
    two = 0 < n_pos < n
    out.append(w2 / (2.0 * n_pos * (n - n_pos)) if two else nan)
    out.append(float(np.sum(1.0 / rank[y == 1])) / n_pos if n_pos else nan)
    for k in (5, 10):
        dcg = float(np.sum(1.0 / np.log2(rank[(y == 1) & (rank <= min(k, n))] + 1.0)))
        ideal = float(np.sum(1.0 / np.log2(np.arange(1, min(k, n, n_pos) + 1) + 1.0)))
        out.append(dcg / ideal if ideal else nan)
    p = np.maximum(np.minimum(s64, 1.0 - 10e-12), 10e-12)
    out.append(-float(np.sum(np.where(y == 1, np.log(p), np.log(1.0 - p)))) / n if two else nan)
    out.append(float(np.sqrt(np.sum((y - s64) ** 2) / n)) if n else nan)
    pred = s64 >= 0.5
    out.append(float(np.sum(pred == (y == 1))) / n if n else nan)
    tp, wrong = float(np.sum(pred & (y == 1))), float(np.sum(pred != (y == 1)))
    out.append(0.0 if 2 * tp + wrong == 0 else 2 * tp / (2 * tp + wrong))
    return out


def synthetic(n_lists, seed, long_share=0.002):
    """EB-NeRD-shaped synthetic impressions: lengths 5 + geometric (mean about 11.6), a share of 250-long lists, one positive per
    list, float32 scores.  Returns (labels uint8, scores float32, offsets int64)."""
    rng = np.random.default_rng(seed)
    lens = np.minimum(4 + rng.geometric(1 / 7.6, n_lists), 100)
    lens[rng.random(n_lists) < long_share] = 250
    offsets = np.zeros(n_lists + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    scores = rng.random(int(offsets[-1]), dtype=np.float32)
    labels = np.zeros(int(offsets[-1]), np.uint8)
    labels[offsets[:-1] + (rng.random(n_lists) * lens).astype(np.int64)] = 1
    return labels, scores, offsets
