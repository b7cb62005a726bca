"""Accuracy over the whole candidate list: hit-rate@k, MRR and nDCG@k from the ranks ``model.rank_targets`` gives each
(impression, clicked article) pair -- the unsampled measures (Krichene and Rendle, KDD 2020, "On Sampled Metrics for Item
Recommendation"), where ``MetricEvaluator`` scores an impression's dozen in-view articles only.

    ranks = model.rank_targets(loader, candidate_ids=candidates, window=fresh)
    rank_metrics(ranks.rank, ks=(5, 10), counts=ranks.count)

``rank_values`` gives the per-pair columns behind those means and ``bootstrap_rank_metrics`` their confidence intervals
(evaluation/bootstrap.py).  ``rank_metrics`` and ``rank_values`` are plain numpy; no device."""
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


def rank_values(ranks, ks=(5, 10), counts=None) -> dict:
    """The per-pair columns behind ``rank_metrics``: {"hit_rate@k", "ndcg@k" for every k, "mrr", with ``counts``
    "mean_percentile", then "unranked" and "ranked"}, each [n_pairs] float64.  A pair that was not ranked holds 0 in every metric
    column and in the "ranked" indicator, so sum(column) / sum(ranked) is the mean over the ranked pairs ``rank_metrics`` reports,
    and mean("unranked") its share of unranked pairs -- the form ``bootstrap_means`` resamples (a ratio of two weighted sums)."""
    r = np.asarray(ranks).reshape(-1).astype(np.int64)
    if (r < 0).any():
        raise ValueError("ranks are 1-based, 0 for a pair that was not ranked: negative values are not ranks")
    ranked = r > 0
    rr = np.where(ranked, r, 1).astype(np.float64)
    out = {}
    for k in ks:
        k = int(k)
        if k < 1:
            raise ValueError(f"every k must be at least 1, got {k}")
        out[f"hit_rate@{k}"] = (ranked & (r <= k)).astype(np.float64)
        out[f"ndcg@{k}"] = np.where(ranked & (r <= k), 1.0 / np.log2(1.0 + rr), 0.0)
    out["mrr"] = np.where(ranked, 1.0 / rr, 0.0)
    if counts is not None:
        c = np.asarray(counts).reshape(-1).astype(np.float64)
        if c.shape != r.shape:
            raise ValueError(f"counts must have one entry per rank: {c.shape} against {r.shape}")
        out["mean_percentile"] = np.where(ranked, (rr - 1.0) / np.maximum(c - 1.0, 1.0), 0.0)
    out["unranked"] = (~ranked).astype(np.float64)
    out["ranked"] = ranked.astype(np.float64)
    return out


def bootstrap_rank_metrics(ranks, ks=(5, 10), counts=None, n_resamples: int = 2000, seed: int = 0, clusters=None, device="cuda", **kw):
    """``rank_metrics`` with a bootstrap behind every number: a ``BootstrapResult`` (evaluation/bootstrap.py) whose estimates are
    those of ``rank_metrics`` -- means over the ranked pairs, through the "ranked" denominator; "unranked" over all pairs.
    ``clusters``: one id per pair (its user), so that whole users are resampled."""
    from .bootstrap import bootstrap_means

    cols = rank_values(ranks, ks, counts)
    denominators = {k: "ranked" for k in cols if k not in ("ranked", "unranked")}
    return bootstrap_means(cols, denominators, n_resamples=n_resamples, seed=seed, clusters=clusters, device=device, **kw)
