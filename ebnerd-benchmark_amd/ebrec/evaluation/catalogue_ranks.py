"""Accuracy over the whole candidate list: hit-rate@k, MRR and nDCG@k from the ranks ``model.rank_targets`` gives each
(impression, clicked article) pair -- the unsampled measures (Krichene and Rendle, KDD 2020, "On Sampled Metrics for Item
Recommendation"), where ``MetricEvaluator`` scores an impression's dozen in-view articles only.

    ranks = model.rank_targets(loader, candidate_ids=candidates, window=fresh)
    rank_metrics(ranks.rank, ks=(5, 10), counts=ranks.count)

Plain numpy; no device."""
import numpy as np


def rank_metrics(ranks, ks=(5, 10), counts=None) -> dict:
    """``ranks``: 1-based rank of each pair's target among its candidates, 0 = not ranked (the target is no candidate, or was
    excluded).  -> {"hit_rate@k", "ndcg@k" for every k of ``ks``, "mrr", "unranked" and, with ``counts`` (the number of candidates
    each pair was ranked among), "mean_percentile"}.
    ndcg@k is for one relevant item, 1 / log2(1 + rank) when rank <= k, else 0 (the ideal DCG is 1); mean_percentile is the mean
    of (rank - 1) / max(count - 1, 1): 0 = always first, 1 = always last.  ``unranked`` is the share of pairs with rank 0; every
    mean runs over the RANKED pairs.  No pairs, or none ranked: NaN."""
    r = np.asarray(ranks).reshape(-1).astype(np.int64)
    if (r < 0).any():
        raise ValueError("ranks are 1-based, 0 for a pair that was not ranked: negative values are not ranks")
    ranked = r > 0
    n = int(ranked.sum())
    rr = r[ranked].astype(np.float64)
    mean = lambda v: float(np.sum(v) / n) if n else float("nan")
    out = {}
    for k in ks:
        k = int(k)
        if k < 1:
            raise ValueError(f"every k must be at least 1, got {k}")
        out[f"hit_rate@{k}"] = mean(rr <= k)
        out[f"ndcg@{k}"] = mean(np.where(rr <= k, 1.0 / np.log2(1.0 + rr), 0.0))
    out["mrr"] = mean(1.0 / rr)
    out["unranked"] = float(1.0 - n / len(r)) if len(r) else float("nan")
    if counts is not None:
        c = np.asarray(counts).reshape(-1).astype(np.float64)
        if c.shape != r.shape:
            raise ValueError(f"counts must have one entry per rank: {c.shape} against {r.shape}")
        out["mean_percentile"] = mean((rr - 1.0) / np.maximum(c[ranked] - 1.0, 1.0))
    return out
