"""EASE on the host: the numpy twins of csrc/ebn_ease.hip against the plain-Python / float64 brute force of tests/ease_cases.py, the
host layer ``ebrec.models.EASE`` (duplicates, the max_items cut, fill, the call forms, from_weights, similar_items), its scores in
``DeviceMetricEvaluator``'s host path and ``ScoreBlend``, and the example script with --ease."""
import re
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from ebrec import _hip
from ebrec.evaluation import AucScore, DeviceMetricEvaluator, MrrScore, NdcgScore, RaggedLists
from ebrec.models import EASE, ScoreBlend, ease_gram_host, ease_invert_host, ease_scores_host, ease_system_host, ease_weights_host
from ebrec.models.baselines import ease as ease_mod
from ebrec.utils import _constants as C
from tests import ease_cases as ec

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "ebnerd"


@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


def test_header_kernel_and_module_constants_agree():
    text = _hip.header_path().read_text()
    assert int(re.search(r"#define\s+EBN_EASE_MAX_ITEMS\s+(\d+)", text).group(1)) == ease_mod.MAX_ITEMS == 32768
    lib = _hip.lib()  # pure host queries: no GPU
    nb = int(lib.ebn_ease_block())
    src = (ROOT / "ebnerd-benchmark_amd" / "csrc" / "ebn_ease.hip").read_text()
    assert nb in (32, 64, 128) and int(re.search(r"#define\s+EASE_NB\s+(\d+)", src).group(1)) == nb
    assert "atomicAdd(&G[" in src and not re.search(r"atomic\w*\((?!&G\[)", src)  # the one atomic of the file is the integer one
    decl = _hip.declared_functions()
    names = ("ebn_ease_gram_i32", "ebn_ease_system_f32", "ebn_ease_invert_f32", "ebn_ease_invert_nb_f32", "ebn_ease_weights_f32",
             "ebn_ease_scores_f32", "ebn_ease_workspace_floats", "ebn_ease_block")
    assert [len(decl[n][1]) for n in names] == [8, 8, 7, 8, 6, 15, 1, 0]
    ws = lib.ebn_ease_workspace_floats
    assert ws(-1) == 0 and ws(32769) == 0 and ws(0) == 0 and ws(1) >= 1 + 128 * 128 + 128 * 4
    for n in (5, 300, 8192, 32768):
        assert n * n < ws(n) <= n * n + 300 * n + 128 * 128 * 2


def test_gram_twin_against_the_brute_force():
    for n in (1, 5, 300):
        indptr, cols, rows = ec.gram_case(n)
        G = ease_gram_host(indptr, cols, n)
        assert G.dtype == np.int32 and G.shape == (n, n) and not np.triu(G, 1).any()
        distinct = [r for r in rows if len(set(r)) == len(r)]
        # rows of distinct entries: the brute force's sets; the row of 60 repeats: x (x + 1) / 2 on the diagonal, x_a x_b off it
        want = np.tril(ec.brute_gram(distinct, n))
        for r in rows:
            if len(set(r)) != len(r):
                x = np.bincount([c for c in r if 0 <= c < n], minlength=n)
                want += np.tril(np.outer(x, x), -1) + np.diag(x * (x + 1) // 2)
        assert np.array_equal(G, want)
    assert ease_gram_host(np.zeros(1, np.int64), np.zeros(0, np.int32), 4).tolist() == np.zeros((4, 4), int).tolist()
    # clamped extents: an indptr that runs past the entries
    assert np.array_equal(ease_gram_host(np.array([0, 9]), np.array([1, 2], np.int32), 3), [[0, 0, 0], [0, 1, 0], [0, 1, 1]])


def test_system_invert_and_weights_twins_against_the_brute_force():
    seqs = ec.click_sequences(40, 300, seed=3)
    G = ec.brute_gram(seqs, 40)
    A64 = ec.system(G, 7.5)
    low = np.tril(G).astype(np.int32)
    low[0, 5] = 12345  # the upper triangle is never read
    A = ease_system_host(low, 7.5)
    assert A.dtype == np.float32 and np.array_equal(A.astype(np.float64), A64)
    with pytest.raises(OverflowError):
        ease_system_host(np.array([[(1 << 24) + 1]]), 1.0)
    assert ease_system_host(np.array([[1 << 24]]), 1.0)[0, 0] == np.float32((1 << 24) + 1.0)
    garbage = A.copy()
    garbage[np.triu_indices(40, 1)] = np.nan  # only the lower triangle is read
    P, info = ease_invert_host(garbage)
    P_ref = np.linalg.inv(A64)
    assert info == 0 and P.dtype == np.float32 and np.array_equal(P, P.T)
    assert np.abs(P - P_ref).max() <= 2 * ec.EPS32 * np.abs(P_ref).max()  # one rounding of the float64 inverse
    B = ease_weights_host(P)
    want = ec.brute_weights(G, 7.5)
    assert B.dtype == np.float32 and not B[np.diag_indices(40)].view(np.int32).any()
    assert np.abs(B - want).max() <= 8 * ec.EPS32 * np.abs(want).max()
    assert not np.allclose(B, B.T)  # x^T B, not B x
    for bad, k in ((np.array([[1, 2], [2, 1]], np.float32), 2), (np.array([[0.0]], np.float32), 1),
                   (np.array([[4, 0, 0], [0, np.nan, 0], [0, 0, 1]], np.float32), 2)):
        P, info = ease_invert_host(bad)
        assert info == k and np.isnan(P).all()
    assert ease_invert_host(np.zeros((0, 0), np.float32))[0].shape == (0, 0)


@pytest.mark.parametrize("name", ec.SCORE_CASES)
def test_score_twin_against_the_brute_force(name):
    c, want, bound, length = ec.score_case(name)
    got = ease_scores_host(c["B"], c["hist_rows"], c["hist_weights"], c["hist_offsets"], c["list_hist"], c["cand_rows"], c["cand_offsets"])
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12
    assert sorted(set(length.tolist())) == [0, 1, 63, 64, 200] and (got[length == 0] == 0.0).all()  # 65 entries, two of them unknown
    assert np.count_nonzero(want) > 15 and (bound[length > 0] > 0).all()


def test_duplicates_count_once_and_the_model_equals_the_brute_force():
    seqs = ec.click_sequences(30, 200, seed=11)
    assert any(len(set(s)) < len(s) for s in seqs)
    ids = 1000 + 7 * np.arange(30)  # article ids, not rows
    model = EASE(regularization=3.0, device=None).fit([[int(ids[i]) for i in s] for s in seqs])
    G = ec.brute_gram(seqs, 30)
    present = np.flatnonzero(np.diag(G))
    assert np.array_equal(model.article_ids, ids[present]) and np.array_equal(model.item_counts, np.diag(G)[present])
    want = ec.brute_weights(G[np.ix_(present, present)], 3.0)
    assert isinstance(model.weights, np.ndarray) and model.weights.dtype == np.float32
    assert np.abs(model.weights - want).max() <= 8 * ec.EPS32 * np.abs(want).max()
    once = EASE(regularization=3.0, device=None).fit([sorted({int(ids[i]) for i in s}) for s in seqs])
    assert np.array_equal(once.weights, model.weights)
    # history_size cuts the training sequences too
    cut = EASE(regularization=3.0, device=None, history_size=4).fit([[int(ids[i]) for i in s] for s in seqs])
    G4 = ec.brute_gram([s[-4:] for s in seqs], 30)
    assert np.array_equal(cut.item_counts, np.diag(G4)[np.flatnonzero(np.diag(G4))])
    # the forms of fit: lists of lists, RaggedLists, a frame
    lists = [[int(ids[i]) for i in s] for s in seqs]
    frame = pd.DataFrame({C.DEFAULT_USER_COL: np.arange(len(lists)), C.DEFAULT_HISTORY_ARTICLE_ID_COL: lists})
    for other in (EASE(regularization=3.0, device=None).fit(RaggedLists.from_lists([np.asarray(s) for s in lists])),
                  EASE(regularization=3.0, device=None).fit(frame)):
        assert np.array_equal(other.weights, model.weights) and np.array_equal(other.article_ids, model.article_ids)


def test_max_items_keeps_the_most_clicked_with_ties_to_the_smaller_id():
    # counts: 10 -> 3 users, 20 -> 2, 30 -> 2, 40 -> 1, 50 -> 1 (the repeat in the first sequence counts once)
    seqs = [[10, 10, 20, 40], [10, 30], [10, 20, 30, 50]]
    full = EASE(regularization=1.0, device=None).fit(seqs)
    assert full.article_ids.tolist() == [10, 20, 30, 40, 50] and full.item_counts.tolist() == [3, 2, 2, 1, 1]
    for k, ids in ((4, [10, 20, 30, 40]), (2, [10, 20]), (1, [10])):
        m = EASE(regularization=1.0, max_items=k, device=None).fit(seqs)
        assert m.article_ids.tolist() == ids and m.weights.shape == (k, k)
        rows = {a: i for i, a in enumerate(ids)}
        want = ec.brute_weights(ec.brute_gram([[rows[a] for a in s if a in rows] for s in seqs], k), 1.0)
        assert np.abs(m.weights - want).max() <= 8 * ec.EPS32 * max(np.abs(want).max(), 1.0)
    m = EASE(regularization=1.0, max_items=2, device=None, fill=-9.0).fit(seqs)
    s = m.predict([[10, 20, 30], [20]], [[10, 30], [40]])  # 30 was cut: an unknown article; the second history holds nothing known
    assert s.flat[2] == -9.0 and s.flat[3] == -9.0 and s.flat[0] == 0.0 and s.flat[1] == float(m.weights[0, 1])


def test_fill_placement_and_the_three_call_forms(frames):
    behaviors, history = frames
    model = EASE(regularization=20.0, device=None, fill=-2.5, history_size=30, history_weights="exponential").fit(history.iloc[:40])
    from ebrec.models import CoVisitation

    cut = [list(h)[-30:] for h in history.iloc[:40][C.DEFAULT_HISTORY_ARTICLE_ID_COL]]  # EASE's history_size cuts its training sequences too
    other = CoVisitation(device=None, fill=-2.5, history_size=30, history_weights="exponential").fit(cut)
    late = history.iloc[5:]
    got, ref = model.predict(behaviors, history=late), other.predict(behaviors, history=late)
    assert isinstance(got, RaggedLists) and got.flat.dtype == np.float64 and np.array_equal(got.offsets, ref.offsets)
    assert np.array_equal(model.article_ids, other._fitted().article_ids)
    assert np.array_equal(got.flat == -2.5, ref.flat == -2.5) and 500 < (got.flat == -2.5).sum() < got.flat.size  # where the others put it
    # form 2: the behaviours frame's own histories; form 3: ids with and without list_hist
    hist_of = dict(zip(late[C.DEFAULT_USER_COL], late[C.DEFAULT_HISTORY_ARTICLE_ID_COL]))
    users = behaviors[C.DEFAULT_USER_COL].tolist()
    known = [i for i, u in enumerate(users) if u in hist_of][:50]
    sub = behaviors.iloc[known].copy()
    sub[C.DEFAULT_HISTORY_ARTICLE_ID_COL] = [hist_of[users[i]] for i in known]
    form2 = model.predict(sub)
    cands, hists = list(sub[C.DEFAULT_INVIEW_ARTICLES_COL]), list(sub[C.DEFAULT_HISTORY_ARTICLE_ID_COL])
    form3 = model.predict(cands, hists)
    form3b = model.predict(cands, hists[::-1], list_hist=np.arange(len(hists))[::-1])
    want = np.concatenate([got.flat[got.offsets[i]:got.offsets[i + 1]] for i in known])
    for f in (form2, form3, form3b):
        assert np.array_equal(f.flat, want)
    with pytest.raises(ValueError):
        model.predict(cands, hists[:-1])
    with pytest.raises(ValueError):
        model.predict(cands)
    with pytest.raises(RuntimeError):
        EASE(device=None).predict(cands, hists)
    # the scores are the brute force's
    plain = EASE(regularization=20.0, device=None).fit(history)
    s = plain.predict(cands, hists)
    off = np.zeros(len(cands) + 1, np.int64)
    np.cumsum([len(x) for x in cands], out=off[1:])
    hoff = np.zeros(len(cands) + 1, np.int64)
    np.cumsum([len(x) for x in hists], out=hoff[1:])
    want5, _, _ = ec.brute_scores(plain.weights.astype(np.float64), plain.rows_of(np.concatenate(hists)), None, hoff, None,
                                  plain.rows_of(np.concatenate(cands)), off)
    assert np.abs(s.flat - want5).max() <= 1e-12 and np.count_nonzero(want5) > 10


def test_from_weights_round_trip_and_similar_items_tie_order():
    seqs = ec.click_sequences(12, 80, seed=2)
    model = EASE(regularization=2.0, device=None).fit(seqs)
    perm = np.random.default_rng(0).permutation(model.article_ids.size)
    back = EASE.from_weights(model.article_ids[perm], model.weights[np.ix_(perm, perm)], device=None, fill=1.5)
    assert np.array_equal(back.article_ids, model.article_ids) and np.array_equal(back.weights, model.weights) and back.item_counts is None
    cands, hists = [[0, 1, 2, 99], [3, 4]], [[5, 6, 5], [99]]
    a, b = model.predict(cands, hists).flat, back.predict(cands, hists).flat
    assert np.array_equal(a[:3], b[:3]) and b[3:].tolist() == [1.5, 1.5, 1.5] and a[3:].tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        EASE.from_weights([1, 1], np.zeros((2, 2)))
    with pytest.raises(ValueError):
        EASE.from_weights([1, 2], np.zeros((2, 3)))
    B = np.array([[0, .5, .25, .5], [.1, 0, .1, .1], [9, 9, 0, 9], [1, 2, 3, 0]], np.float32)
    m = EASE.from_weights([40, 10, 30, 20], B, device=None)  # rows and columns in the order of the given ids
    ids, w = m.similar_items(40, n=3)
    assert ids.tolist() == [10, 20, 30] and w.tolist() == [0.5, 0.5, 0.25]  # the tie goes to the smaller id
    assert m.similar_items(30, n=10)[0].tolist() == [10, 20, 40] and m.similar_items(20, n=1)[0].tolist() == [30]
    assert m.similar_items(10, n=0)[0].size == 0
    with pytest.raises(KeyError):
        m.similar_items(77)


def test_errors_and_the_empty_fit():
    for kw in (dict(regularization=0.0), dict(regularization=-1.0), dict(regularization=float("nan")), dict(regularization=float("inf")),
               dict(max_items=0), dict(max_items=32769), dict(max_items=2.5), dict(history_weights="cubic"), dict(history_size=0)):
        with pytest.raises(ValueError):
            EASE(device=None, **kw)
    with pytest.raises(TypeError):
        EASE(device=None).fit([[1.5, 2.5]])
    with pytest.raises(ValueError):
        EASE(device=None).fit(pd.DataFrame({"x": [1]}))
    empty = EASE(device=None, fill=-1.0).fit([[], []])
    assert empty.article_ids.size == 0 and empty.weights.shape == (0, 0)
    assert (empty.predict([[1, 2], []], [[1], [2]]).flat == -1.0).all()


def test_class_on_the_fixture_frames_feeds_the_evaluator_and_the_blend(frames):
    behaviors, history = frames
    scores = EASE(regularization=50.0, device=None).fit(history).predict(behaviors, history=history)
    assert isinstance(scores, RaggedLists) and isinstance(scores.flat, np.ndarray) and scores.flat.dtype == np.float64
    assert scores.lengths.tolist() == [len(x) for x in behaviors[C.DEFAULT_INVIEW_ARTICLES_COL]]
    labels = RaggedLists.from_lists([np.isin(v, c).astype(np.int64) for v, c in zip(behaviors[C.DEFAULT_INVIEW_ARTICLES_COL],
                                                                                   behaviors[C.DEFAULT_CLICKED_ARTICLES_COL])])
    keep = [l for l in range(len(labels)) if 0 < sum(labels.row(l)) < len(labels.row(l))]
    y = RaggedLists.from_lists([np.asarray(labels.row(l)) for l in keep])
    p = RaggedLists.from_lists([scores.flat[scores.offsets[l]:scores.offsets[l + 1]] for l in keep])
    ev = DeviceMetricEvaluator(y, p, [AucScore(), MrrScore(), NdcgScore(k=5), NdcgScore(k=10)], device=None).evaluate()
    assert set(ev.evaluations) == {"auc", "mrr", "ndcg@5", "ndcg@10"} and all(0.0 <= v <= 1.0 for v in ev.evaluations.values())
    assert len(keep) > 900 and np.count_nonzero(scores.flat) > 500
    from ebrec.models import CoVisitation

    cv = CoVisitation(device=None).fit(history).predict(behaviors, history=history)
    q = RaggedLists.from_lists([cv.flat[cv.offsets[l]:cv.offsets[l + 1]] for l in keep])
    blend = ScoreBlend(device=None).fit(y, [p, q], names=["ease", "covisit"])
    out = blend.predict([p, q])
    assert isinstance(out, RaggedLists) and np.array_equal(out.offsets, p.offsets) and np.isfinite(out.flat).all()
    assert len(blend.weights) == 2 and np.isfinite(blend.weights).all()


def test_example_script_with_ease_on_the_host(tmp_path, capsys):
    sys.path.insert(0, str(ROOT / "tools"))
    sys.path.insert(0, str(ROOT / "examples" / "baseline"))
    import ebnerd_feat_baselines
    from make_synthetic_ebnerd import make

    data = make(tmp_path / "data", split="ebnerd_demo", n_impressions=120, n_users=20, n_articles=60, seed=2)
    argv = ["--data_path", str(data), "--datasplit", "ebnerd_demo", "--dump_dir", str(tmp_path / "out")]
    without, _ = ebnerd_feat_baselines.main(argv)
    results, _ = ebnerd_feat_baselines.main(argv + ["--ease", "--ease_reg", "10"])
    out = capsys.readouterr().out
    assert set(results) == set(without) | {"ease_prediction_scores"} and "ease_prediction_scores" not in without
    assert all(results[k] == without[k] for k in without)
    res = results["ease_prediction_scores"]
    assert set(res) == {"auc", "mrr", "ndcg@5", "ndcg@10"} and all(0.0 <= v <= 1.0 for v in res.values())
    assert re.search(r"^ease: \d+ sequences of \d+ articles, regularization 10$", out, flags=re.M)
    assert (tmp_path / "out" / "ease_prediction_scores.zip").exists()
    blended, _ = ebnerd_feat_baselines.main(argv + ["--ease", "--blend"])
    assert re.search(rf"^blend: {len(without) + 1} sources", capsys.readouterr().out, flags=re.M) and "blend_prediction_scores" in blended
