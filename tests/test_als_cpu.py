"""The numpy twins of the implicit-ALS kernels against the float64 brute force and the derived bound of tests/als_cases.py, the loss
against an explicit all-pairs double loop, and ImplicitALS on the host path (device=None) on the fixture frames."""
import re
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import als_cases as ac

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "ebnerd"


@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


@pytest.mark.parametrize("F", ac.FS)
def test_the_brute_force_is_a_hundred_times_closer_than_the_bound(F):
    ac.check_reference(F)


@pytest.mark.parametrize("F", ac.FS)
def test_solve_twin_against_the_brute_force(F):
    from ebrec.models.baselines.als import als_solve_host

    c, refs = ac.solve_case(F), ac.reference(F)
    out = als_solve_host(c["fixed"], c["gram"], c["indptr"], c["cols"], c["conf"], c["reg"])
    ac.check_rows(out, refs, f"twin F={F}")
    assert refs[0]["n"] == 0 and refs[c["all_absent"]]["n"] == 0  # the exact +0 rows were among them
    assert refs[c["long_row"]]["n"] == 3 * ac.SPLIT_SMALL + 7 - 3


@pytest.mark.parametrize("F", ac.FS)
def test_partials_route_meets_the_same_bound(F):
    from ebrec.models.baselines.als import als_partials_host, als_solve_host

    c, refs = ac.solve_case(F), ac.reference(F)
    parts = als_partials_host(c["fixed"], c["cols"], c["conf"], c["part_begin"], c["part_end"])
    assert parts.dtype == np.float32 and parts.shape == (4, F * (F + 1))
    S = parts[:, :F * F].reshape(4, F, F)
    assert np.array_equal(S, S.transpose(0, 2, 1))  # the full symmetric matrix
    direct = als_solve_host(c["fixed"], c["gram"], c["indptr"], c["cols"], c["conf"], c["reg"])
    split = als_solve_host(c["fixed"], c["gram"], c["indptr"], c["cols"], c["conf"], c["reg"], c["row_parts"], parts)
    ac.check_rows(split, refs, f"twin, partials route F={F}", n_of=ac.parts_n(c))
    other = np.arange(len(refs)) != c["long_row"]
    assert np.array_equal(split[other].view(np.int32), direct[other].view(np.int32))  # the other rows walk their entries


def test_breakdown_row_is_nan():
    from ebrec.models.baselines.als import als_solve_host

    c = ac.breakdown_case()
    out = als_solve_host(c["fixed"], c["gram"], c["indptr"], c["cols"], c["conf"], c["reg"])
    assert out.shape == (1, 2) and np.isnan(out).all()
    with pytest.raises(ValueError):
        als_solve_host(c["fixed"], c["gram"], c["indptr"], c["cols"], c["conf"], 0.0)


def test_loss_against_an_explicit_all_pairs_loop():
    from ebrec.models.baselines.als import als_loss_host

    X, Y, indptr, cols, conf = ac.random_problem(3)
    reg = 0.3
    a = {(u, int(cols[k])): float(conf[k]) for u in range(7) for k in range(int(indptr[u]), int(indptr[u + 1]))}
    want = 0.0
    for u in range(7):
        for i in range(9):
            s = float(np.dot(X[u].astype(np.float64), Y[i].astype(np.float64)))
            want += (1.0 + a[(u, i)]) * (1.0 - s) ** 2 if (u, i) in a else s * s
    want += float(np.float32(reg)) * (float((X.astype(np.float64) ** 2).sum()) + float((Y.astype(np.float64) ** 2).sum()))
    assert len(a) > 10 and als_loss_host(X, Y, indptr, cols, conf, reg) == pytest.approx(want, rel=1e-12)


def _sweep_models(history, **kw):
    from ebrec.models import ImplicitALS

    return [ImplicitALS(iterations=k, compute_loss=True, **kw).fit(history) for k in (1, 2, 3)]


def test_fit_on_the_host_never_increases_the_loss(frames):
    _, history = frames
    models = _sweep_models(history, device=None, **ac.FIT_KW)
    m = models[-1]
    assert isinstance(m.item_factors, np.ndarray) and m.item_factors.dtype == np.float32 and m.item_factors.shape == (len(m.article_ids), 32)
    assert m.user_factors.dtype == np.float32 and m.user_factors.shape == (len(history), 32)
    ac.check_monotone(models)


def test_split_len_does_not_change_what_fit_computes(frames):
    from ebrec.models import ImplicitALS

    _, history = frames
    kw = dict(factors=8, iterations=1, device=None, regularization=0.1)
    a, b = ImplicitALS(**kw).fit(history), ImplicitALS(split_len=16, **kw).fit(history)
    assert b._sides[0].row_parts is not None and b._sides[1].row_parts is not None and a._sides[0].row_parts is None
    assert np.allclose(a.item_factors, b.item_factors, rtol=1e-4, atol=1e-6) and np.allclose(a.user_factors, b.user_factors, rtol=1e-4, atol=1e-6)


@pytest.fixture(scope="module")
def given(frames):
    """a model from given item factors over the articles of the fixture history and of every second in-view list"""
    behaviors, history = frames
    ids = np.unique(np.concatenate(list(history["article_id_fixed"]) + list(behaviors["article_ids_inview"])[::2]))
    rng = np.random.default_rng(11)
    Y = (rng.standard_normal((ids.size, 12)) * 0.3).astype(np.float32)
    perm = rng.permutation(ids.size)  # from_factors sorts
    return ids, Y, perm


def _model(given, **kw):
    from ebrec.models import ImplicitALS

    ids, Y, perm = given
    return ImplicitALS.from_factors(ids[perm], Y[perm], regularization=1.0, device=None, **kw)


def test_from_factors_predict_call_forms_agree_and_fill(frames, given):
    from ebrec.evaluation import RaggedLists
    from ebrec.models.baselines.content import ContentSimilarity

    behaviors, history = frames
    m = _model(given)
    assert np.array_equal(m.article_ids, given[0]) and np.array_equal(m.item_factors, given[1]) and m.user_factors is None
    joined = m.predict(behaviors, history=history)
    at = {u: k for k, u in enumerate(history["user_id"].tolist())}
    per_row = behaviors.assign(article_id_fixed=[history["article_id_fixed"].iloc[at[u]] for u in behaviors["user_id"]])
    own = m.predict(per_row)
    lists = m.predict(list(behaviors["article_ids_inview"]), list(history["article_id_fixed"]),
                      list_hist=np.array([at[u] for u in behaviors["user_id"]]))
    ragged = m.predict(RaggedLists.from_lists(list(behaviors["article_ids_inview"])), RaggedLists.from_lists(list(per_row["article_id_fixed"])))
    assert isinstance(joined.flat, np.ndarray) and joined.flat.dtype == np.float64 and np.count_nonzero(joined.flat) > 1000
    for other in (own, lists, ragged):
        assert np.array_equal(other.offsets, joined.offsets) and np.array_equal(other.flat, joined.flat)
    # fill: exactly ContentSimilarity._unscorable -- unknown candidates, users without a known history article
    filled = _model(given, fill=-7.0).predict(behaviors, history=history.iloc[5:])
    cand, hist, lh = ContentSimilarity._frames(None, behaviors, history.iloc[5:])
    want = ContentSimilarity._unscorable(m.rows_of(cand[0]), cand[1], m.rows_of(hist[0]), hist[1], lh)
    assert np.array_equal(filled.flat == -7.0, want) and 100 < want.sum() < want.size
    with pytest.raises(ValueError):
        m.predict(list(behaviors["article_ids_inview"]), list(history["article_id_fixed"]))  # 1046 lists, 44 histories
    with pytest.raises(RuntimeError):
        from ebrec.models import ImplicitALS
        ImplicitALS(device=None).predict(behaviors, history=history)


def test_scores_are_the_fold_in_rows_dotted_with_the_candidates(given):
    from ebrec.models.baselines.als import als_solve_host

    ids, Y, _ = given
    m = _model(given, alpha=3.0)
    hist = [[ids[5], ids[9], ids[5], -12345, ids[2]], [], [-1]]
    cands = [[ids[2], ids[7], -5], [ids[1]], [ids[3]]]
    got = m.predict(cands, hist)
    gram = (Y.astype(np.float64).T @ Y.astype(np.float64)).astype(np.float32)
    x = als_solve_host(Y, gram, [0, 3], [2, 5, 9], np.array([3.0, 6.0, 3.0], np.float32), 1.0)  # the duplicate: one entry, summed weight
    want = [float(x[0].astype(np.float64) @ Y[r].astype(np.float64)) for r in (2, 7)]
    assert np.allclose(got.flat[:2], want, rtol=1e-12, atol=0) and np.array_equal(got.flat[2:], np.zeros(3))
    assert np.array_equal(m.fold_in(hist)[0], x[0]) and not m.fold_in(hist)[1:].any()


def test_history_size_and_decay_weights_are_applied(given):
    from ebrec.models.baselines.als import als_solve_host
    from ebrec.utils._decay import exponential_decay_weights

    ids, Y, _ = given
    m = _model(given, alpha=2.0, history_size=3, history_weights="exponential", lambda_factor=0.5)
    hist = [[ids[40], ids[4], ids[8], ids[4]]]  # the last three, weights 0.25, 0.5, 1 oldest first; ids[4] twice: 0.25 + 1
    w = np.asarray(exponential_decay_weights(3, 0.5, ascending=True), np.float64)
    assert np.allclose(w, [0.25, 0.5, 1.0])
    gram = (Y.astype(np.float64).T @ Y.astype(np.float64)).astype(np.float32)
    x = als_solve_host(Y, gram, [0, 2], [4, 8], np.array([2.0 * 1.25, 2.0 * 0.5], np.float32), 1.0)
    assert np.array_equal(m.fold_in(hist), x)
    assert not np.array_equal(_model(given, alpha=2.0).fold_in(hist), x)


def test_similar_items_ordering_and_key_error(given):
    from ebrec.models import ImplicitALS

    ids = np.array([50, 10, 40, 20, 30])
    Y = np.array([[1, 0], [2, 0], [0, 1], [1, 1], [3, 0]], np.float32)  # 10, 30, 50 are parallel: cosine 1, ties by the smaller id
    m = ImplicitALS.from_factors(ids, Y, device=None)
    got_ids, cos = m.similar_items(10, n=3)
    assert got_ids.tolist() == [30, 50, 20] and np.allclose(cos, [1.0, 1.0, np.sqrt(0.5)])
    assert m.similar_items(40, n=10)[0].tolist() == [20, 10, 30, 50] and m.similar_items(40, n=0)[0].size == 0
    with pytest.raises(KeyError):
        m.similar_items(99)


def test_constructor_validation():
    from ebrec.models import ImplicitALS

    for kw in (dict(factors=0), dict(factors=129), dict(factors=2.5), dict(factors=True), dict(regularization=0.0), dict(regularization=-1.0),
               dict(regularization=float("nan")), dict(regularization=float("inf")), dict(regularization=1e-50), dict(alpha=-1.0),
               dict(alpha=float("nan")), dict(iterations=-1), dict(iterations=1.5), dict(split_len=0), dict(history_weights="cubic"),
               dict(history_size=0), dict(history_size=True)):
        with pytest.raises(ValueError):
            ImplicitALS(device=None, **kw)
    ImplicitALS(factors=128, regularization=1e-30, iterations=0, device=None)
    with pytest.raises(ValueError):
        ImplicitALS.from_factors([1, 1], np.ones((2, 2), np.float32), device=None)
    with pytest.raises(ValueError):
        ImplicitALS(device=None).fit(pd.DataFrame({"user_id": [1]}))


def test_a_degenerate_problem_raises_and_names_regularization():
    """two items with the factors (1, 1), one user who read both, alpha = 1: A = 4 [[1, 1], [1, 1]] + 1e-30 I, the second pivot is
    exactly 0 in float32 and in float64"""
    from ebrec.models import ImplicitALS

    m = ImplicitALS(factors=2, regularization=1e-30, alpha=1.0, iterations=1, device=None)
    with pytest.raises(FloatingPointError, match="regularization"):
        m.fit([[7, 9]], init_item_factors=np.ones((2, 2), np.float32))
    ImplicitALS(factors=2, regularization=0.5, alpha=1.0, iterations=1, device=None).fit([[7, 9]], init_item_factors=np.ones((2, 2), np.float32))


def test_example_script_with_als_on_the_host(tmp_path, capsys):
    sys.path.insert(0, str(ROOT / "tools"))
    sys.path.insert(0, str(ROOT / "examples" / "baseline"))
    import ebnerd_feat_baselines
    from make_synthetic_ebnerd import make

    data = make(tmp_path / "data", split="ebnerd_demo", n_impressions=120, n_users=20, n_articles=60, seed=2)
    argv = ["--data_path", str(data), "--datasplit", "ebnerd_demo", "--dump_dir", str(tmp_path / "out")]
    without, _ = ebnerd_feat_baselines.main(argv)
    results, _ = ebnerd_feat_baselines.main(argv + ["--als"])
    out = capsys.readouterr().out
    assert set(results) == set(without) | {"als_prediction_scores"} and all(results[k] == without[k] for k in without)
    res = results["als_prediction_scores"]
    assert set(res) == {"auc", "mrr", "ndcg@5", "ndcg@10"} and all(0.0 <= v <= 1.0 for v in res.values())
    assert re.search(r"^als: 64 factors of \d+ articles and \d+ users, regularization 0.01, alpha 40, 15 sweeps$", out, flags=re.M)
    assert (tmp_path / "out" / "als_prediction_scores.zip").exists()
