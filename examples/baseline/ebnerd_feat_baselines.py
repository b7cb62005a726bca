"""Popularity baselines on an EB-NeRD split (the job of the reference's examples/baseline/ebnerd_feat_baselines.py):

    python examples/baseline/ebnerd_feat_baselines.py --data_path ~/ebnerd_data --datasplit ebnerd_small --device_metrics

Scores the split's validation impressions with every baseline the data has the columns for, prints AUC / MRR / nDCG@5 / nDCG@10 per
baseline and writes one zipped submission file per baseline into --dump_dir:

  * total_pageviews / total_inviews / total_read_time of articles.parquet (``ArticleFeatureBaseline``) and the in-view frequency of
    the evaluated frame (``InviewEstimateBaseline``): the reference script's four lookups, totals over the whole dataset;
  * recent_popularity: clicks in the 1 h / 6 h / 24 h before each impression (``RecentPopularity``), counted over the train
    behaviours, the train history when it carries its times, and -- with --index_validation_clicks -- the evaluated impressions'
    own clicks (the window ends before the impression's own time, so an impression never sees its own click);
  * covisit (with --covisit): item-to-item co-visitation (``CoVisitation``: max gap 3, both directions, cosine, summed over the
    user's history), counted over train/history.parquet and scored against each user's validation/history.parquet;
  * als (with --als): implicit-feedback ALS (``ImplicitALS``: 64 factors, regularization 0.01, alpha 40, 15 sweeps), fitted on
    train/history.parquet; each user's validation/history.parquet is folded into the factor space and scored by dot products;
  * knn (with --knn): sequence-neighbourhood collaborative filtering (``HistoryKNN``: the 100 nearest of the 1000 most recent train
    histories that share an article with the user's validation history, cosine, linear history weights, the user's own train
    history excluded), fitted on train/history.parquet;
  * ease (with --ease): the item-to-item ridge regression EASE^R (``EASE``: regularization --ease_reg, 500 by default, the 16384
    most-clicked articles), fitted on train/history.parquet and scored against each user's validation/history.parquet.

--topn K adds, for each of covisit, als, knn and ease that is selected, the full-catalogue view (``recommend`` / ``rank_targets``): where the
clicked article stands among ALL fitted articles under the user's validation history (hit-rate@K, MRR, nDCG@K,
``ebrec.evaluation.rank_metrics``) and what the K-lists look like beyond accuracy: coverage of the fitted catalogue and novelty
(mean -log2 of an article's share of the train-history clicks, relative to the most clicked one).

--blend adds one more row, blend_prediction_scores: a ``ScoreBlend`` over every baseline the run computed (--blend_transform: the per-list
transform of every column, zscore by default), cross-fitted in 5 folds by ``user_id`` so that no impression is judged with weights
fitted on it or on another impression of its user; the mean fold weights per source are printed next to its metrics.

With --device_metrics the counts, the ranking and the metrics run on the GPU; without it everything runs on the host."""
from __future__ import annotations

import argparse
import datetime as dt
import sys
from pathlib import Path

import numpy as np
import pandas as pd

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "ebnerd-benchmark_amd"))

from ebrec.evaluation import (AucScore, Coverage, DeviceMetricEvaluator, MetricEvaluator, MrrScore, NdcgScore, Novelty,  # noqa: E402
                              RaggedLists, rank_metrics)
from ebrec.models import (EASE, ArticleFeatureBaseline, CoVisitation, HistoryKNN, ImplicitALS, InviewEstimateBaseline,  # noqa: E402
                          PopularityIndex, RecentPopularity, ScoreBlend)
from ebrec.utils._constants import (DEFAULT_CLICKED_ARTICLES_COL, DEFAULT_HISTORY_ARTICLE_ID_COL,  # noqa: E402
                                    DEFAULT_HISTORY_IMPRESSION_TIMESTAMP_COL, DEFAULT_IMPRESSION_ID_COL, DEFAULT_IMPRESSION_TIMESTAMP_COL,
                                    DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_TOTAL_INVIEWS_COL, DEFAULT_TOTAL_PAGEVIEWS_COL,
                                    DEFAULT_TOTAL_READ_TIME_COL, DEFAULT_USER_COL)
from ebrec.utils._python import rank_predictions_by_score_ragged, write_submission_file  # noqa: E402

WINDOWS = [dt.timedelta(hours=1), dt.timedelta(hours=6), dt.timedelta(hours=24)]
FEATURES = {"clicked_prediction_scores": DEFAULT_TOTAL_PAGEVIEWS_COL, "inview_prediction_scores": DEFAULT_TOTAL_INVIEWS_COL,
            "readtime_prediction_scores": DEFAULT_TOTAL_READ_TIME_COL}


def get_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data_path", default="~/ebnerd_data")
    ap.add_argument("--datasplit", default="ebnerd_demo")
    ap.add_argument("--dump_dir", default="ebnerd_predictions/baselines")
    ap.add_argument("--device_metrics", action="store_true", help="counts, ranks and metrics on the GPU")
    ap.add_argument("--index_validation_clicks", action="store_true", help="count the evaluated impressions' earlier clicks too")
    ap.add_argument("--covisit", action="store_true", help="add the co-visitation baseline (fit on the train history)")
    ap.add_argument("--als", action="store_true", help="add the implicit-ALS baseline (fit on the train history)")
    ap.add_argument("--knn", action="store_true", help="add the history-kNN baseline (fit on the train history)")
    ap.add_argument("--ease", action="store_true", help="add the EASE baseline (fit on the train history)")
    ap.add_argument("--ease_reg", type=float, default=500.0, metavar="R", help="EASE's ridge regularization")
    ap.add_argument("--topn", type=int, default=0, metavar="K", help="also rank the clicked articles among ALL fitted articles and judge the "
                    "top-K lists (covisit / als / knn / ease), 1 to 64")
    ap.add_argument("--blend", action="store_true", help="add a cross-fitted blend of every baseline of the run (5 folds by user)")
    ap.add_argument("--blend_transform", default="zscore", choices=["raw", "zscore", "minmax", "rank", "rrf"],
                    help="per-list transform of every column before the blend")
    return ap.parse_args(argv)


def topn_report(name, model, catalogue, df, df_val_history, df_history, k):
    """hit-rate@k / MRR / nDCG@k of the clicked articles over the whole fitted catalogue, coverage and novelty of the k-lists"""
    ranks = model.rank_targets(df, history=df_val_history)
    out = {m: v for m, v in rank_metrics(ranks.rank, ks=(k,), counts=ranks.count).items()}
    lists = model.recommend(df, history=df_val_history, top_n=k)
    out["coverage"] = Coverage()([row[row >= 0] for row in lists], catalogue)[1]
    ids, clicks = np.unique(np.concatenate([np.asarray(x).ravel() for x in df_history[DEFAULT_HISTORY_ARTICLE_ID_COL]]), return_counts=True)
    popularity = {int(a): {"popularity": float(c) / float(clicks.max())} for a, c in zip(ids, clicks)}
    novelty = Novelty()([row[row >= 0] for row in lists if (row >= 0).any()], popularity, "popularity")
    out["novelty"] = float(np.mean(novelty)) if len(novelty) else float("nan")
    print(f"{name} top-{k} over {len(catalogue)} articles: " + "  ".join(f"{m} {v:.4f}" for m, v in out.items()))
    return out


def labels_of(df) -> RaggedLists:
    """1 where an in-view article was clicked, aligned with the in-view lists"""
    inview = RaggedLists.from_lists([np.asarray(x) for x in df[DEFAULT_INVIEW_ARTICLES_COL]], dtype=np.int64)
    clicked = RaggedLists.from_lists([np.asarray(x) for x in df[DEFAULT_CLICKED_ARTICLES_COL]], dtype=np.int64)
    ids, codes = np.unique(np.concatenate([inview.flat, clicked.flat]), return_inverse=True)
    of_list = lambda r: np.repeat(np.arange(len(r), dtype=np.int64), r.lengths) * len(ids)  # (list, article) as one integer
    n = len(inview.flat)
    labels = np.isin(of_list(inview) + codes[:n], of_list(clicked) + codes[n:])
    return RaggedLists(labels.astype(np.int64), inview.offsets)


def main(argv=None):
    args = get_args(argv)
    device = "cuda" if args.device_metrics else None
    PATH = Path(args.data_path).expanduser()
    df_articles = pd.read_parquet(PATH / "articles.parquet")
    df_train = pd.read_parquet(PATH / args.datasplit / "train" / "behaviors.parquet")
    df_history = pd.read_parquet(PATH / args.datasplit / "train" / "history.parquet")
    df = pd.read_parquet(PATH / args.datasplit / "validation" / "behaviors.parquet")

    baselines, skipped, topn = {}, {}, {}
    if args.topn and not 1 <= args.topn <= 64:
        raise SystemExit("--topn takes 1 to 64")
    for name, column in FEATURES.items():
        if column in df_articles.columns:
            baselines[name] = ArticleFeatureBaseline(df_articles, column).predict
        else:
            skipped[name] = f"articles.parquet has no column '{column}'"
    baselines["inview_estimate_prediction_scores"] = InviewEstimateBaseline().predict
    if DEFAULT_IMPRESSION_TIMESTAMP_COL in df_train.columns and DEFAULT_IMPRESSION_TIMESTAMP_COL in df.columns:
        parts = [PopularityIndex.from_behaviors(df_train, events="clicks")]
        if {DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_HISTORY_IMPRESSION_TIMESTAMP_COL} <= set(df_history.columns):
            parts.append(PopularityIndex.from_history(df_history))
        else:
            print(f"recent_popularity: history.parquet has no column '{DEFAULT_HISTORY_IMPRESSION_TIMESTAMP_COL}', counting the behaviours only")
        if args.index_validation_clicks:
            parts.append(PopularityIndex.from_behaviors(df, events="clicks"))
        index = PopularityIndex.concat(*parts)
        print(f"recent_popularity: {index.n_events} click events of {len(index)} articles, windows 1 h / 6 h / 24 h")
        baselines["recent_popularity_prediction_scores"] = RecentPopularity(index, WINDOWS, device=device).predict
    else:
        skipped["recent_popularity_prediction_scores"] = f"behaviors.parquet has no column '{DEFAULT_IMPRESSION_TIMESTAMP_COL}'"
    if args.covisit:
        if DEFAULT_HISTORY_ARTICLE_ID_COL in df_history.columns:
            cv = CoVisitation(max_gap=3, symmetric=True, similarity="cosine", mode="sum", device=device).fit(df_history)
            df_val_history = pd.read_parquet(PATH / args.datasplit / "validation" / "history.parquet")
            print(f"covisit: {cv.matrix.nnz} pairs of {cv.matrix.n_rows} articles, max gap 3, cosine, sum")
            baselines["covisit_prediction_scores"] = lambda frame: cv.predict(frame, history=df_val_history)
            topn["covisit"] = (cv, cv.matrix.article_ids, df_val_history)
        else:
            skipped["covisit_prediction_scores"] = f"history.parquet has no column '{DEFAULT_HISTORY_ARTICLE_ID_COL}'"
    if args.als:
        if DEFAULT_HISTORY_ARTICLE_ID_COL in df_history.columns:
            als = ImplicitALS(factors=64, regularization=0.01, alpha=40.0, iterations=15, device=device).fit(df_history)
            df_als_history = pd.read_parquet(PATH / args.datasplit / "validation" / "history.parquet")
            print(f"als: {als.factors} factors of {len(als.article_ids)} articles and {len(df_history)} users, regularization 0.01, alpha 40, 15 sweeps")
            baselines["als_prediction_scores"] = lambda frame: als.predict(frame, history=df_als_history)
            topn["als"] = (als, als.article_ids, df_als_history)
        else:
            skipped["als_prediction_scores"] = f"history.parquet has no column '{DEFAULT_HISTORY_ARTICLE_ID_COL}'"
    if args.knn:
        if DEFAULT_HISTORY_ARTICLE_ID_COL in df_history.columns:
            knn = HistoryKNN(k=100, sample_size=1000, similarity="cosine", history_weights="linear", device=device).fit(df_history)
            df_knn_history = pd.read_parquet(PATH / args.datasplit / "validation" / "history.parquet")
            print(f"knn: {knn.index.n_seqs} sequences of {knn.index.n_rows} articles, k 100 of the 1000 most recent, cosine, linear weights")
            baselines["knn_prediction_scores"] = lambda frame: knn.predict(frame, history=df_knn_history)
            topn["knn"] = (knn, knn.index.article_ids, df_knn_history)
        else:
            skipped["knn_prediction_scores"] = f"history.parquet has no column '{DEFAULT_HISTORY_ARTICLE_ID_COL}'"
    if args.ease:
        if DEFAULT_HISTORY_ARTICLE_ID_COL in df_history.columns:
            ease = EASE(regularization=args.ease_reg, device=device).fit(df_history)
            df_ease_history = pd.read_parquet(PATH / args.datasplit / "validation" / "history.parquet")
            print(f"ease: {len(df_history)} sequences of {ease.article_ids.size} articles, regularization {args.ease_reg:g}")
            baselines["ease_prediction_scores"] = lambda frame: ease.predict(frame, history=df_ease_history)
            topn["ease"] = (ease, ease.article_ids, df_ease_history)
        else:
            skipped["ease_prediction_scores"] = f"history.parquet has no column '{DEFAULT_HISTORY_ARTICLE_ID_COL}'"
    for name, why in skipped.items():
        print(f"skipped {name}: {why}")

    labels = labels_of(df)
    metrics = [AucScore(), MrrScore(), NdcgScore(k=5), NdcgScore(k=10)]
    dump = Path(args.dump_dir)
    dump.mkdir(parents=True, exist_ok=True)
    results, columns = {}, {}
    BLEND = "blend_prediction_scores"

    def blend_predict(frame):
        blend = ScoreBlend(transforms=args.blend_transform, device=device)
        groups = frame[DEFAULT_USER_COL] if DEFAULT_USER_COL in frame.columns else None
        scores, fold_weights = blend.cross_fit_predict(labels, list(columns.values()), folds=5, groups=groups)
        print(f"blend: {len(columns)} sources, transform {args.blend_transform}, 5 folds by " + ("user" if groups is not None else "list") +
              "; mean fold weights: " + "  ".join(f"{n} {w:.4f}" for n, w in zip(columns, fold_weights.mean(axis=0))))
        return scores

    if args.blend:
        baselines[BLEND] = blend_predict
    for name, predict in baselines.items():
        scores = predict(df)
        if args.blend and name != BLEND:
            columns[name] = scores
        if args.device_metrics:
            ev = DeviceMetricEvaluator(labels, scores, metrics, device=device).evaluate()
        else:
            ev = MetricEvaluator(labels.to_lists(), scores.to_lists(), metrics).evaluate()
        results[name] = ev.evaluations
        print(f"{name}: " + "  ".join(f"{k} {v:.4f}" for k, v in ev.evaluations.items()))
        print("Writing submission file for:", name)
        write_submission_file(impression_ids=df[DEFAULT_IMPRESSION_ID_COL].tolist(),
                              prediction_scores=rank_predictions_by_score_ragged(scores, device=device),
                              path=dump / "predictions.txt", filename_zip=f"{name}.zip")
    if args.topn:
        for name, (model, catalogue, val_history) in topn.items():
            results[f"{name}_top{args.topn}"] = topn_report(name, model, catalogue, df, val_history, df_history, args.topn)
    return results, skipped


if __name__ == "__main__":
    main()
