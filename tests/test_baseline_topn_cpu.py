"""``recommend`` / ``rank_targets`` of the baselines on the host path (ebrec/models/baselines/_topn.py): CoVisitation through the float32
twins of the co-visitation kernels, ImplicitALS and ContentSimilarity (centroid) through the float64 twins of the dense launches,
on the golden frames of tests/golden/ebnerd.  No GPU."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from ebrec.evaluation import RaggedLists, rank_metrics
from ebrec.evaluation.freshness import Freshness
from ebrec.models import ContentSimilarity, CoVisitation, ImplicitALS, dense_target_rank_host, dense_topk_host

GOLDEN = Path(__file__).resolve().parent / "golden" / "ebnerd"
KINDS = ("covisit", "als", "content")


def build(kind, history, device=None, **kw):
    """the three fitted models of these tests (also imported by the GPU test); content: seeded random document vectors"""
    if kind == "covisit":
        return CoVisitation(max_gap=3, similarity=kw.get("similarity", "count"), history_weights=kw.get("weights"), device=device).fit(history)
    if kind == "als":
        return ImplicitALS(factors=kw.get("factors", 13), iterations=3, regularization=0.1, alpha=10.0, history_weights=kw.get("weights"),
                           device=device).fit(history)  # well-conditioned systems: this file is not about the solver
    ids = np.unique(np.concatenate([np.asarray(x) for x in history["article_id_fixed"]]))
    rng = np.random.default_rng(3)
    table = {int(a): {"v": rng.standard_normal(kw.get("factors", 10)).astype(np.float32)} for a in ids}
    return ContentSimilarity(table, "v", mode=kw.get("mode", "centroid"), history_weights=kw.get("weights"), device=device)


@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet").iloc[:60].reset_index(drop=True), pd.read_parquet(GOLDEN / "history.parquet")


@pytest.fixture(scope="module", params=KINDS)
def model(request, frames):
    return build(request.param, frames[1])


def _histories(behaviors, history):
    by_user = {u: list(h) for u, h in zip(history["user_id"], history["article_id_fixed"])}
    return [by_user.get(u, []) for u in behaviors["user_id"]]


def test_the_three_call_forms_agree(model, frames):
    behaviors, history = frames
    lists = _histories(behaviors, history)
    assert sum(1 for l in lists if l) > 40
    a = model.recommend(behaviors, history=history, top_n=7, return_scores=True)
    b = model.recommend(behaviors.assign(article_id_fixed=lists), top_n=7, return_scores=True)
    c = model.recommend(lists, top_n=7, return_scores=True)
    d = model.recommend(RaggedLists.from_lists([np.asarray(l, np.int64) for l in lists]), top_n=7, return_scores=True)
    assert a[0].shape == (len(behaviors), 7) and a[1].dtype == np.float32 and (a[0] >= 0).sum() > 200
    for other in (b, c, d):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1].view(np.int32), other[1].view(np.int32))
    assert np.array_equal(model.recommend(behaviors, history=history, top_n=7, batch_users=7), a[0])
    targets = [t[:1] for t in behaviors["article_ids_clicked"]]
    ra = model.rank_targets(behaviors, history=history)
    rb = model.rank_targets(lists, targets=[list(t) for t in behaviors["article_ids_clicked"]], batch_users=11)
    assert len(ra) == sum(len(t) for t in behaviors["article_ids_clicked"]) >= len(targets)
    for f in ("impression", "target_id", "rank", "count"):
        assert np.array_equal(getattr(ra, f), getattr(rb, f)), f
    assert np.array_equal(ra.score.view(np.int32), rb.score.view(np.int32))
    m = rank_metrics(ra.rank, ks=(5, 10), counts=ra.count)
    assert set(m) >= {"hit_rate@5", "hit_rate@10", "ndcg@10", "mrr", "unranked"}


def test_rank_is_the_index_in_the_list_plus_one(model, frames):
    behaviors, history = frames
    for kw in (dict(), dict(exclude_history=False)):
        ids, scores = model.recommend(behaviors, history=history, top_n=20, return_scores=True, **kw)
        for slot in (0, 3, 19):
            listed = ids[:, slot] >= 0
            ranks = model.rank_targets(behaviors, history=history, targets=[[a] if a >= 0 else [] for a in ids[:, slot]], **kw)
            assert len(ranks) == int(listed.sum()) and np.array_equal(ranks.impression, np.flatnonzero(listed))
            assert np.array_equal(ranks.rank, np.full(len(ranks), slot + 1))
            assert np.array_equal(ranks.score.view(np.int32), scores[listed, slot].view(np.int32))
    # the clicked articles: wherever the rank is within the list, the list has the article there
    ids = model.recommend(behaviors, history=history, top_n=64)
    ranks = model.rank_targets(behaviors, history=history)
    inside = (ranks.rank >= 1) & (ranks.rank <= 64)
    assert np.array_equal(ids[ranks.impression[inside], ranks.rank[inside] - 1], ranks.target_id[inside])
    never = ~np.array([t in ids[i] for i, t in zip(ranks.impression, ranks.target_id)])
    assert np.array_equal(never, ~inside)


def test_candidate_order_decides_ties(frames):
    behaviors, history = frames
    cv = build("covisit", history)  # "count" without weights: small integer scores, ties everywhere
    cand = cv.matrix.article_ids[::3]
    for order in (cand, cand[::-1], np.random.default_rng(0).permutation(cand)):
        place = {a: i for i, a in enumerate(order.tolist())}
        ids, scores = cv.recommend(behaviors, history=history, candidate_ids=order, top_n=30, return_scores=True)
        ties = 0
        for row, s in zip(ids, scores):
            n = int((row >= 0).sum())
            assert all(a in place for a in row[:n].tolist())
            key = [(-float(v), place[a]) for a, v in zip(row[:n].tolist(), s[:n])]
            assert key == sorted(key)
            ties += sum(1 for x, y in zip(key, key[1:]) if x[0] == y[0])
        assert ties > 100


def test_lists_under_a_freshness_window_equal_a_brute_force_over_publish_times(model, frames):
    behaviors, history = frames
    ids_all = np.asarray(model._topn_ids())
    rng = np.random.default_rng(1)
    published = {int(a): float(t) for a, t in zip(ids_all, rng.integers(0, 50, ids_all.size))}  # repeated times: ties in the sort
    times = rng.integers(10, 60, len(behaviors)).astype(np.float64)
    fresh = Freshness(published, max_age=20.0, min_age=2.0)
    lists = _histories(behaviors, history)
    got = model.recommend(lists, top_n=10, window=fresh, impression_times=times, return_scores=True)
    ranks = model.rank_targets(lists, targets=[list(t) for t in behaviors["article_ids_clicked"]], window=fresh, impression_times=times)
    for i in range(0, len(behaviors), 7):
        inside = [int(a) for a in ids_all if times[i] - 20.0 <= published[int(a)] <= times[i] - 2.0]
        inside.sort(key=lambda a: published[a])  # stable: the older article first, then the order of candidate_ids
        want = model.recommend([lists[i]], candidate_ids=inside, top_n=10, return_scores=True) if inside else None
        if want is None:
            assert (got[0][i] == -1).all()
            continue
        assert np.array_equal(got[0][i], want[0][0]) and np.array_equal(got[1][i].view(np.int32), want[1][0].view(np.int32))
        for j in np.flatnonzero(ranks.impression == i):
            alone = model.rank_targets([lists[i]], targets=[[ranks.target_id[j]]], candidate_ids=inside) if ranks.target_id[j] in inside else None
            assert ranks.rank[j] == (alone.rank[0] if alone is not None else 0)
    assert (got[0] >= 0).sum() > 100
    # the frame's own column serves as well
    dated = {int(a): behaviors["impression_time"].min() - pd.Timedelta(hours=int(h)) for a, h in zip(ids_all, rng.integers(0, 200, ids_all.size))}
    by_time = model.recommend(behaviors, history=history, top_n=5, window=Freshness(dated, max_age=pd.Timedelta(hours=150)))
    assert by_time.shape == (len(behaviors), 5) and (by_time >= 0).any()


def test_exclude_history_fill_id_and_users_without_a_score(model, frames):
    behaviors, history = frames
    lists = _histories(behaviors, history)
    on = model.recommend(lists, top_n=64)
    off = model.recommend(lists, top_n=64, exclude_history=False)
    read = 0
    for l, a, b in zip(lists, on, off):
        known = set(list(dict.fromkeys(reversed(l)))[:256])  # the history's last 256 distinct articles
        assert not known & set(a[a >= 0].tolist())
        read += len(known & set(b[b >= 0].tolist()))
        kept = [x for x in b.tolist() if x >= 0 and x not in known]
        assert a[:len(kept)].tolist() == kept  # the same order without the history's own articles
    assert read > 50
    unknown = int(np.asarray(model._topn_ids()).max()) + 1
    ids, scores = model.recommend([[], [unknown], lists[0]], top_n=4, fill_id=-7, return_scores=True)
    assert (ids[:2] == -7).all() and np.isneginf(scores[:2]).all() and (ids[2] != -7).all()
    r = model.rank_targets([[], [unknown], lists[0]], targets=[ids[2, 0], [ids[2, 1]], [ids[2, 2], unknown]])
    assert r.rank.tolist() == [0, 0, 3, 0] and r.count[:2].tolist() == [0, 0] and np.isneginf(r.score[[0, 1, 3]]).all()


def test_argument_errors(frames):
    behaviors, history = frames
    cv = build("covisit", history)
    lists = _histories(behaviors, history)
    ids = cv.matrix.article_ids
    for top_n in (0, 65, True, 2.5):
        with pytest.raises(ValueError, match="top_n"):
            cv.recommend(lists, top_n=top_n)
    with pytest.raises(ValueError, match="not among the fitted"):
        cv.recommend(lists, candidate_ids=[int(ids[0]), int(ids.max()) + 5])
    with pytest.raises(ValueError, match="twice"):
        cv.recommend(lists, candidate_ids=[int(ids[0]), int(ids[1]), int(ids[0])])
    with pytest.raises(ValueError, match="Freshness"):
        cv.recommend(lists, window=(0, 5))
    fresh = Freshness({int(a): 1.0 for a in ids})
    with pytest.raises(ValueError, match="impression times"):
        cv.recommend(lists, window=fresh)
    with pytest.raises(ValueError, match="impression times"):
        cv.recommend(lists, window=fresh, impression_times=np.ones(3))
    with pytest.raises(ValueError, match="impression_times= goes with"):
        cv.recommend(lists, impression_times=np.ones(len(lists)))
    with pytest.raises(ValueError, match="without a publish time"):
        cv.recommend(lists, window=Freshness({int(ids[0]): 1.0}), impression_times=np.ones(len(lists)))
    for batch in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="batch_users"):
            cv.recommend(lists, batch_users=batch)
    with pytest.raises(ValueError, match="history= goes with"):
        cv.recommend(lists, history=history)
    with pytest.raises(ValueError, match="pass history="):
        cv.recommend(behaviors)
    with pytest.raises(ValueError, match="lacks the column"):
        cv.recommend(behaviors, history=history.drop(columns=["user_id"]))
    with pytest.raises(ValueError, match="targets=None"):
        cv.rank_targets(lists)
    with pytest.raises(ValueError, match="one list of ids per impression"):
        cv.rank_targets(lists, targets=[[1]])
    with pytest.raises(RuntimeError, match="fit"):
        CoVisitation(device=None).recommend(lists)
    with pytest.raises(RuntimeError, match="fit"):
        ImplicitALS(device=None).rank_targets(lists, targets=[[]] * len(lists))
    with pytest.raises(NotImplementedError, match="nearest"):
        build("content", history, mode="nearest").recommend(lists)
    with pytest.raises(NotImplementedError, match="nearest"):
        build("content", history, mode="nearest").rank_targets(lists, targets=[[]] * len(lists))


def test_dense_twins_on_a_tiny_case():
    users = np.array([[1, 0], [0, 1], [1, 1], [0, 0]], np.float32)
    cat = np.array([[2, 0], [0, 2], [1, 1], [np.nan, 0], [3, 3]], np.float32)
    flags = np.zeros(2, np.int32)
    pos, score = dense_topk_host(users, cat, np.array([4, 2, 1, 0]), None, None, 3, flags)
    assert pos.tolist() == [[0, 3, 1], [0, 2, 1], [0, 1, 2], [0, 1, 2]] and score[0].tolist() == [3.0, 2.0, 1.0] and not flags.any()
    pos, _ = dense_topk_host(users, cat, np.array([4, 2, 1, 0]), np.array([[1, 9], [0, 0], [2, 1], [-3, 2]]), np.array([[1], [1], [1], [4]]), 3, flags)
    assert pos.tolist() == [[3, 1, -1], [-1, -1, -1], [-1, -1, -1], [1, -1, -1]] and not flags.any()
    rank, count, t = dense_target_rank_host(users, cat, np.array([4, 2, 1, 0]), np.array([1, 1, -1, 9]), None, None, flags)
    assert (rank.tolist(), count.tolist(), flags.tolist()) == ([3, 3, 0, 0], [4, 4, 4, 4], [1, 0]) and t[:2].tolist() == [1.0, 1.0]
    flags[:] = 0
    dense_topk_host(users, cat, np.array([3, 7]), None, None, 1, flags)  # a NaN score, a row outside the table
    assert flags.tolist() == [1, 1]


def test_example_script_with_topn_on_the_host(tmp_path, capsys):
    import re
    import sys

    root = Path(__file__).resolve().parents[1]
    sys.path.insert(0, str(root / "tools"))
    sys.path.insert(0, str(root / "examples" / "baseline"))
    import ebnerd_feat_baselines
    from make_synthetic_ebnerd import make

    data = make(tmp_path / "data", split="ebnerd_demo", n_impressions=120, n_users=20, n_articles=60, seed=2)
    argv = ["--data_path", str(data), "--datasplit", "ebnerd_demo", "--dump_dir", str(tmp_path / "out"), "--covisit", "--als"]
    without, _ = ebnerd_feat_baselines.main(argv)
    results, _ = ebnerd_feat_baselines.main(argv + ["--topn", "5"])
    out = capsys.readouterr().out
    assert set(results) == set(without) | {"covisit_top5", "als_top5"} and all(results[k] == without[k] for k in without)
    for name in ("covisit", "als"):
        res = results[f"{name}_top5"]
        assert {"hit_rate@5", "ndcg@5", "mrr", "unranked", "coverage", "novelty"} <= set(res)
        assert 0.0 <= res["hit_rate@5"] <= 1.0 and 0.0 < res["coverage"] <= 1.0 and res["novelty"] >= 0.0
        assert re.search(rf"^{name} top-5 over \d+ articles: hit_rate@5 ", out, flags=re.M)
    # the numbers are the class's own
    val = pd.read_parquet(data / "ebnerd_demo" / "validation" / "behaviors.parquet")
    val_h = pd.read_parquet(data / "ebnerd_demo" / "validation" / "history.parquet")
    train_h = pd.read_parquet(data / "ebnerd_demo" / "train" / "history.parquet")
    cv = CoVisitation(max_gap=3, symmetric=True, similarity="cosine", mode="sum", device=None).fit(train_h)
    ranks = cv.rank_targets(val, history=val_h)
    assert results["covisit_top5"]["hit_rate@5"] == rank_metrics(ranks.rank, ks=(5,), counts=ranks.count)["hit_rate@5"]
    with pytest.raises(SystemExit):
        ebnerd_feat_baselines.main(argv + ["--topn", "65"])
