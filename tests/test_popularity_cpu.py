"""The popularity baselines on the host (ebrec/models/baselines): the numpy twin of ebn_window_counts_i32 against the brute force of
tests/popularity_cases.py, the index builders on the fixture frames, the half-open window, lexicographic_scores, the reference
script's lookups, the time-kind errors and the example script."""
import datetime as dt
import re
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from ebrec import _hip
from ebrec.evaluation import RaggedLists
from ebrec.models import (ArticleFeatureBaseline, InviewEstimateBaseline, PopularityIndex, RecentPopularity, lexicographic_scores,
                          window_counts_host)
from ebrec.models.baselines import popularity as pop
from ebrec.utils import _constants as C
from ebrec.utils._python import rank_predictions_by_score, read_submission_file
from tests import popularity_cases as pc

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "ebnerd"
DAY = dt.timedelta(days=1)


def _twin(c):
    return window_counts_host(c["event_times"], c["row_offsets"], c["item_rows"], c["list_offsets"], c["list_times"], c["max_ages"], c["min_age"])


def test_header_python_and_reference_constants_agree():
    text = _hip.header_path().read_text()
    assert int(re.search(r"#define\s+EBN_WC_MAX_WINDOWS\s+(\d+)", text).group(1)) == pop.MAX_WINDOWS == 8
    assert re.search(r"#define\s+EBN_WC_UNBOUNDED\s+INT64_MAX\b", text) and pop.UNBOUNDED == pc.UNBOUNDED == 2 ** 63 - 1
    res, argt = _hip.declared_functions()["ebn_window_counts_i32"]
    assert len(argt) == 21
    assert (C.DEFAULT_TOTAL_PAGEVIEWS_COL, C.DEFAULT_TOTAL_INVIEWS_COL, C.DEFAULT_TOTAL_READ_TIME_COL) == \
        ("total_pageviews", "total_inviews", "total_read_time")


def test_brute_force_on_the_hand_written_window_ends():
    """an event exactly at t - max_age is counted, one exactly at t - min_age is not"""
    assert np.array_equal(pc.case("hand_written_window_ends")[1], pc.HAND_WANT)


@pytest.mark.parametrize("name", pc.NAMES)
def test_twin_equals_brute_force(name):
    c, want = pc.case(name)
    got = _twin(c)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} counts differ"
    zero_by_design = name.startswith(("items_0", "zero_ages")) or name == "near_int64_min_min_age_saturates"
    assert zero_by_design or want.max() > 0, "a vacuous case"


def _brute_for(index, rows, offsets, times, max_ages, min_age=0):
    return pc.brute_force(dict(event_times=index.event_times, row_offsets=index.row_offsets, item_rows=rows, list_offsets=offsets,
                               list_times=times, max_ages=max_ages, min_age=min_age))


@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


def _fixture_counts(index, behaviors):
    c = RecentPopularity(index, [DAY], device=None).counts(behaviors)
    flat, offsets = pop._explode(behaviors[C.DEFAULT_INVIEW_ARTICLES_COL])
    t = behaviors[C.DEFAULT_IMPRESSION_TIMESTAMP_COL].to_numpy().astype("datetime64[us]").view(np.int64)
    want = _brute_for(index, index.rows_of(flat), offsets, t, [int(DAY.total_seconds()) * 10 ** 6])
    assert isinstance(c.counts, np.ndarray) and np.array_equal(c.offsets, offsets)
    return c.counts, want


def test_clicks_from_behaviours_on_the_fixture_frames(frames):
    behaviors, _ = frames
    index = PopularityIndex.from_behaviors(behaviors, events="clicks")
    assert index.kind == "datetime" and index.n_events == int(behaviors[C.DEFAULT_CLICKED_ARTICLES_COL].map(len).sum())
    assert np.all(np.diff(index.ids) > 0) and index.row_offsets[-1] == index.n_events
    for r in range(len(index)):
        assert np.all(np.diff(index.event_times[index.row_offsets[r]:index.row_offsets[r + 1]]) >= 0)
    got, want = _fixture_counts(index, behaviors)
    assert np.array_equal(got, want)
    # the comparison is not vacuous: 10 848 items, 35 % of them with a click in the day before, at most 9
    assert got.shape == (1, 10848) and got.max() == 9 and round(100 * float((got > 0).mean())) == 35


def test_history_and_inviews_on_the_fixture_frames(frames):
    behaviors, history = frames
    for index in (PopularityIndex.from_history(history), PopularityIndex.from_behaviors(behaviors, events="inviews")):
        assert index.kind == "datetime" and index.n_events > 0
        got, want = _fixture_counts(index, behaviors)
        assert np.array_equal(got, want) and got.max() > 0
    assert PopularityIndex.from_behaviors(behaviors, events="inviews").n_events == 10848
    both = PopularityIndex.concat(PopularityIndex.from_history(history), PopularityIndex.from_behaviors(behaviors))
    assert both.n_events == PopularityIndex.from_history(history).n_events + PopularityIndex.from_behaviors(behaviors).n_events
    got, want = _fixture_counts(both, behaviors)
    assert np.array_equal(got, want)


def test_an_impressions_own_click_is_not_counted():
    t0 = dt.datetime(2023, 5, 18, 12)
    df = pd.DataFrame({C.DEFAULT_IMPRESSION_TIMESTAMP_COL: [t0, t0 + dt.timedelta(minutes=5)],
                       C.DEFAULT_INVIEW_ARTICLES_COL: [[7, 8], [7, 8]], C.DEFAULT_CLICKED_ARTICLES_COL: [[7], [8]]})
    index = PopularityIndex.from_behaviors(df)
    rp = RecentPopularity(index, [dt.timedelta(hours=1)], device=None)
    assert rp.counts(df).counts.tolist() == [[0, 0, 1, 0]]  # neither impression sees its own click, the second sees the first's
    later = df.assign(**{C.DEFAULT_IMPRESSION_TIMESTAMP_COL: df[C.DEFAULT_IMPRESSION_TIMESTAMP_COL] + dt.timedelta(microseconds=1)})
    assert rp.counts(later).counts.tolist() == [[1, 0, 1, 1]]  # one microsecond later the own click is in the window
    assert rp.counts([[7, 8], [8, 99]], [t0 + dt.timedelta(hours=1), t0 + dt.timedelta(hours=1, minutes=5)]).counts.tolist() == [[1, 1, 1, 0]]
    assert RecentPopularity(index, [None], min_age=dt.timedelta(minutes=5), device=None).counts(later).counts.tolist() == [[0, 0, 1, 0]]
    scores = RecentPopularity(index, [dt.timedelta(minutes=1), None], device=None).predict(later)
    assert isinstance(scores, RaggedLists) and scores.flat.dtype == np.float64 and scores.to_lists() == [[3.0, 0.0], [1.0, 3.0]]


def test_lexicographic_scores_order_exactness_and_limit():
    rng = np.random.default_rng(3)
    counts = np.stack([rng.integers(0, 4, 500), rng.integers(0, 1000, 500), rng.integers(0, 3, 500)]).astype(np.int32)
    s = lexicographic_scores(counts)
    assert s.dtype == np.float64
    want = np.lexsort((counts[2], counts[1], counts[0]))  # stable; primary key counts[0]
    order = np.argsort(s, kind="stable")
    assert np.array_equal(counts[:, order], counts[:, want])
    m = counts.max(1).astype(object) + 1
    exact = (counts[0].astype(object) * m[1] + counts[1].astype(object)) * m[2] + counts[2].astype(object)
    assert [int(v) for v in s] == list(exact)
    assert np.array_equal(lexicographic_scores(counts[:1]), counts[0].astype(np.float64))
    assert lexicographic_scores(np.zeros((3, 0), np.int32)).shape == (0,)
    big = np.array([[2 ** 31 - 1, 0], [2 ** 22 - 1, 0]], np.int32)  # 2^31 * 2^22 = 2^53
    with pytest.raises(ValueError, match="2\\^53"):
        lexicographic_scores(big)
    big[1, 0] -= 1  # (2^22 - 1) 2^31 < 2^53: the largest score is exact
    assert int(lexicographic_scores(big)[0]) == (2 ** 31 - 1) * (2 ** 22 - 1) + 2 ** 22 - 2
    with pytest.raises(ValueError):
        lexicographic_scores(np.array([[1, -1]]))
    with pytest.raises(TypeError):
        lexicographic_scores(np.array([[0.5, 1.0]]))


def test_article_feature_and_inview_estimate_baselines():
    articles = pd.DataFrame({C.DEFAULT_ARTICLE_ID_COL: [30, 10, 20, 40], C.DEFAULT_TOTAL_PAGEVIEWS_COL: [5.0, 100.0, None, 7.0],
                             C.DEFAULT_TOTAL_INVIEWS_COL: [1, 2, 3, 4]})
    df = pd.DataFrame({C.DEFAULT_INVIEW_ARTICLES_COL: [[10, 20, 30], [99, 40, 30, 10], []]})
    base = ArticleFeatureBaseline(articles, C.DEFAULT_TOTAL_PAGEVIEWS_COL)
    assert base.rows_of([10, 99, 40]).tolist() == [0, -1, 3]
    scores = base.predict(df)
    assert isinstance(scores, RaggedLists) and scores.to_lists() == [[100.0, 0.0, 5.0], [0.0, 7.0, 5.0, 100.0], []]  # null and unknown: 0
    for got, values in zip(scores.to_lists()[:2], ([100.0, 0.0, 5.0], [0.0, 7.0, 5.0, 100.0])):
        assert np.array_equal(rank_predictions_by_score(got), rank_predictions_by_score(values))
    assert rank_predictions_by_score(scores.to_lists()[1]).tolist() == [4, 2, 3, 1]
    assert ArticleFeatureBaseline(articles, C.DEFAULT_TOTAL_INVIEWS_COL).predict([[40, 10]]).to_lists() == [[4.0, 2.0]]
    with pytest.raises(ValueError, match="total_read_time"):
        ArticleFeatureBaseline(articles, C.DEFAULT_TOTAL_READ_TIME_COL)
    est = InviewEstimateBaseline().predict(df)
    assert est.to_lists() == [[2.0, 1.0, 2.0], [1.0, 1.0, 2.0, 2.0], []] and np.array_equal(est.offsets, scores.offsets)


def test_time_kind_errors():
    t0 = dt.datetime(2023, 5, 18)
    index = PopularityIndex([1, 2], [t0, t0 + DAY])
    with pytest.raises(TypeError, match="do not mix"):
        RecentPopularity(index, [DAY], device=None).counts([[1]], [5])
    with pytest.raises(TypeError):
        RecentPopularity(index, [3600], device=None)  # a plain number against datetimes
    numbers = PopularityIndex([1, 2, 1], [10, 20, 30])
    assert numbers.kind == "number" and numbers.event_times.tolist() == [10, 30, 20]
    with pytest.raises(TypeError):
        RecentPopularity(numbers, [DAY], device=None)
    with pytest.raises(TypeError, match="scale the times to an integer unit"):
        PopularityIndex([1, 2], [0.5, 1.0])
    with pytest.raises(TypeError, match="scale the times to an integer unit"):
        RecentPopularity(numbers, [10], device=None).counts([[1]], [30.5])
    with pytest.raises(TypeError, match="integer unit"):
        RecentPopularity(numbers, [2.5], device=None)
    assert RecentPopularity(numbers, [20.0], device=None).counts([[1, 2]], [30.0]).counts.tolist() == [[1, 1]]
    with pytest.raises(ValueError, match="no time"):
        PopularityIndex([1, 2], [t0, None])
    with pytest.raises(ValueError, match="no time"):
        RecentPopularity(index, [DAY], device=None).counts([[1], [2]], [t0, pd.NaT])
    with pytest.raises(ValueError):
        RecentPopularity(index, [-DAY], device=None)
    with pytest.raises(ValueError):
        RecentPopularity(index, [DAY] * 9, device=None)
    with pytest.raises(ValueError):
        RecentPopularity(index, [], device=None)
    big = PopularityIndex([1], [2 ** 62 + 1])  # exact past 2^53
    assert big.event_times.tolist() == [2 ** 62 + 1]
    assert RecentPopularity(big, [1], device=None).counts([[1]], [2 ** 62 + 2]).counts.tolist() == [[1]]


def test_example_script_end_to_end_on_the_host(tmp_path, capsys):
    sys.path.insert(0, str(ROOT / "tools"))
    sys.path.insert(0, str(ROOT / "examples" / "baseline"))
    import ebnerd_feat_baselines
    from make_synthetic_ebnerd import make

    data = make(tmp_path / "data", split="ebnerd_demo", n_impressions=120, n_users=20, n_articles=60, seed=2)
    arts = pd.read_parquet(data / "articles.parquet")
    arts[C.DEFAULT_TOTAL_PAGEVIEWS_COL] = np.arange(len(arts), dtype=np.float64)
    arts.to_parquet(data / "articles.parquet")  # total_inviews / total_read_time stay missing: those baselines are skipped
    results, skipped = ebnerd_feat_baselines.main(["--data_path", str(data), "--datasplit", "ebnerd_demo", "--dump_dir", str(tmp_path / "out"),
                                                   "--index_validation_clicks"])
    out = capsys.readouterr().out
    assert set(results) == {"clicked_prediction_scores", "inview_estimate_prediction_scores", "recent_popularity_prediction_scores"}
    assert set(skipped) == {"inview_prediction_scores", "readtime_prediction_scores"}
    assert "skipped inview_prediction_scores: articles.parquet has no column 'total_inviews'" in out
    for name, res in results.items():
        assert set(res) == {"auc", "mrr", "ndcg@5", "ndcg@10"} and all(0.0 <= v <= 1.0 for v in res.values()), name
        assert re.search(rf"^{name}: auc \d\.\d{{4}}  mrr ", out, flags=re.M)
    import zipfile

    val = pd.read_parquet(data / "ebnerd_demo" / "validation" / "behaviors.parquet")
    for name in results:
        with zipfile.ZipFile(tmp_path / "out" / f"{name}.zip") as z:
            z.extractall(tmp_path / "read" / name)
        ids, ranks = read_submission_file(tmp_path / "read" / name / "predictions.txt")
        assert ids == val[C.DEFAULT_IMPRESSION_ID_COL].tolist()
        assert all(sorted(r) == list(range(1, len(v) + 1)) for r, v in zip(ranks, val[C.DEFAULT_INVIEW_ARTICLES_COL]))
