"""Score blending on the host (ebrec/models/ensemble.py with device=None): the numpy twins against the plain-Python brute force of
tests/blend_cases.py, the derivatives against central differences, the Newton fit, the skipped lists, RankFusion,
cross_fit_predict, the errors and the driver's --blend row."""
import re
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from ebrec.evaluation import RaggedLists
from ebrec.models import RankFusion, ScoreBlend, blend_combine_host, blend_features_host, blend_sums_host
from ebrec.models import ensemble as en
from tests import blend_cases as bc

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "ebnerd"


def _within(got, want, bound, what):
    """|got - want| <= bound element-wise, written so that a NaN fails unless both are NaN; prints the largest error and its bound"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    both_nan = np.isnan(got) & np.isnan(want)
    err = np.where(both_nan, 0.0, np.abs(got - want))
    bad = ~(err <= bound)
    if err.size:
        k = int(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), err)))
        print(f"{what}: largest error {np.nanmax(err):.3e}; closest to its bound: {err.ravel()[k]:.3e} of {np.asarray(bound).ravel()[k]:.3e}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {err.size} outside the bound"


def _sources(idx, kind_of_scores=1):
    c = bc.case()
    return [RaggedLists(bc.scores(kind_of_scores)[m].copy(), c["offsets"]) for m in idx]


def _labels():
    c = bc.case()
    return RaggedLists(c["labels"].astype(np.int64), c["offsets"])


# ---- transforms ------------------------------------------------------------------------------------------------------------------
def test_transform_known_answers():
    s = np.array([[3.0, 1.0, 3.0, 2.0, 5.0, 5.0, 5.0, 7.0]] * 5)
    off = np.array([0, 4, 4, 7, 8], np.int64)  # [3 1 3 2], an empty list, a constant list, one item
    f, flags = blend_features_host(s, off, [bc.RAW, bc.ZSCORE, bc.MINMAX, bc.RANK, bc.RRF], [0, 0, 0, 0, 60.0])
    assert f.dtype == np.float32 and f.shape == (5, 8) and flags.tolist() == [0, 0, 0, 0]
    r = np.array([1.5, 4.0, 1.5, 3.0])  # mid-ranks of [3, 1, 3, 2]
    assert np.array_equal(f[0], s[0].astype(np.float32))
    mean, sd = 2.25, np.sqrt(np.mean((s[0, :4] - 2.25) ** 2))
    assert np.array_equal(f[1, :4], ((s[0, :4] - mean) / sd).astype(np.float32))
    assert np.array_equal(f[2, :4], np.array([1.0, 0.0, 1.0, 0.5], np.float32))
    assert np.array_equal(f[3, :4], ((4 - r) / 3).astype(np.float32))
    assert np.array_equal(f[4, :4], (1.0 / (60.0 + r)).astype(np.float32))
    # a constant list: 0 for zscore and minmax, every item at the middle rank 2; one item: 0, 0, 0 and rank 1
    assert f[1, 4:7].tolist() == [0, 0, 0] and f[2, 4:7].tolist() == [0, 0, 0] and f[3, 4:7].tolist() == [0.5, 0.5, 0.5]
    assert np.array_equal(f[4, 4:7], np.full(3, 1.0 / 62.0, np.float32))
    assert f[1:4, 7].tolist() == [0, 0, 0] and f[4, 7] == np.float32(1.0 / 61.0)
    # non-finite: the list is flagged, the source's row is NaN there, raw copies through, an unknown kind is NaN everywhere
    s2 = np.array([[1.0, np.inf, 2.0, 3.0]] * 3)
    f2, flags2 = blend_features_host(s2, np.array([0, 2, 4]), [bc.RAW, bc.RANK, 9], [0, 0, 0])
    assert flags2.tolist() == [2, 0] and f2[0].tolist() == [1.0, np.inf, 2.0, 3.0]
    assert np.isnan(f2[1, :2]).all() and f2[1, 2:].tolist() == [0.0, 1.0] and np.isnan(f2[2]).all()
    # malformed offsets: treated as empty, nothing written
    f3, flags3 = blend_features_host(s2[:1], np.array([0, 2, 1, 9]), [bc.RAW], [0])
    assert flags3.tolist() == [2, 0, 0] and f3[0].tolist() == [1.0, np.inf, 0.0, 0.0]  # list 0 holds the inf


@pytest.mark.parametrize("kind_of_scores", [0, 1])
def test_feature_twin_equals_the_brute_force(kind_of_scores):
    c = bc.case()
    for kind in range(5):
        src = list(range(bc.N_SOURCES))
        want, bound, flags = bc.features_reference(src, [kind] * len(src), kind_of_scores)
        got, got_flags = blend_features_host(bc.scores(kind_of_scores), c["offsets_bad"], [kind] * len(src), [bc.RRF_K] * len(src))
        assert np.array_equal(got_flags, flags) and flags.sum() == 2 * 3
        if kind == bc.RAW:
            assert np.array_equal(got, want.astype(np.float32), equal_nan=True)
        else:
            _within(got, want, bound, f"{bc.KIND_NAMES[kind]} of {('float32', 'float64')[kind_of_scores]} scores")


def test_combine_twin_equals_the_brute_force():
    c = bc.case()
    w = np.array([0.7, -1.3, 0.2, 2.0, 31.0, 0.5])
    want, bound, flags = bc.features_reference(bc.FIT_SOURCES, bc.FIT_KINDS, 1)
    got, got_flags = blend_combine_host(bc.scores(1)[bc.FIT_SOURCES], c["offsets_bad"], bc.FIT_KINDS, [bc.RRF_K] * 6, w)
    f32 = want.astype(np.float32).astype(np.float64)
    ref = np.where(np.repeat(flags[:-1] != 0, c["lengths"]), np.nan, sum(w[m] * f32[m] for m in range(6)))
    _within(got, ref, np.abs(w) @ bound + 2.0 ** -50 * (np.abs(w) @ np.abs(np.nan_to_num(f32))), "combine")
    assert np.array_equal(got_flags, flags) and np.array_equal(np.isnan(got), np.repeat(flags[:-1] != 0, c["lengths"]))


# ---- sums ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_case():
    c = bc.case()
    features, flags = bc.fit_features(1)
    blend = ScoreBlend(transforms=[bc.KIND_NAMES[k] for k in bc.FIT_KINDS], l2=bc.FIT_L2, rrf_k=bc.RRF_K, device=None)
    blend.fit(_labels(), _sources(bc.FIT_SOURCES))
    return dict(features=features, flags=flags, blend=blend, labels=c["labels"], offsets=c["offsets"])


@pytest.mark.parametrize("which", ["zero", "optimum", "saturated"])
def test_sums_twin_equals_the_brute_force(fit_case, which):
    c = bc.case()
    w = {"zero": np.zeros(6), "optimum": fit_case["blend"].weights, "saturated": np.array([30.0, -30.0, 30.0, 30.0, -30.0, 30.0])}[which]
    want, counters, absum = bc.brute_sums(fit_case["features"], c["labels"], c["offsets_bad"], w)
    got, got_counters, got_abs = blend_sums_host(fit_case["features"], c["labels"], c["offsets_bad"], w, return_abs=True)
    assert np.array_equal(got_counters, counters) and counters.sum() == c["n_lists"] + 1 and counters[2] == 2
    _within(got, want, 1e-10 * absum, f"sums at the {which} weights")
    _within(got_abs, absum, 1e-10 * absum, "sums of the absolute terms")
    assert np.isfinite(got).all()


def test_gradient_and_hessian_against_central_differences(fit_case):
    f, y, off = fit_case["features"], fit_case["labels"], fit_case["offsets"]
    rng = np.random.default_rng(3)
    # away from the optimum: there the gradient of the summed loss is about -l2 n w, three orders below the loss whose rounding
    # (eps |loss| / step, about 1e-7 absolute) is the floor of a central difference, and an error RELATIVE to it says nothing
    for w in (np.zeros(6), rng.normal(size=6)):
        sums, _ = blend_sums_host(f, y, off, w)
        _, g, H = en.unpack_sums(sums, 6)
        h = 1e-6
        fd_g, fd_H = np.zeros(6), np.zeros((6, 6))
        for a in range(6):
            e = np.zeros(6)
            e[a] = h
            sp, sm = blend_sums_host(f, y, off, w + e)[0], blend_sums_host(f, y, off, w - e)[0]
            fd_g[a] = (sp[0] - sm[0]) / (2 * h)
            fd_H[a] = (sp[1:7] - sm[1:7]) / (2 * h)
        eg, eh = np.abs(fd_g - g).max() / np.abs(g).max(), np.abs(fd_H - H).max() / np.abs(H).max()
        print(f"gradient {eg:.2e}, Hessian {eh:.2e} relative to central differences")
        assert eg <= 1e-7 and eh <= 1e-7


def test_hessian_is_positive_semidefinite_with_the_1e6_raw_source():
    c = bc.case()
    f, _ = blend_features_host(bc.scores(1)[[0, 1, 4]], c["offsets"], [bc.RAW, bc.ZSCORE, bc.RANK], [0, 0, 0])
    assert np.nanmax(np.abs(f[0])) > 1e6
    for w in (np.zeros(3), np.array([1e-6, 0.5, -0.3]), np.array([3e-6, -2.0, 4.0])):
        sums, counters = blend_sums_host(f, c["labels"], c["offsets"], w)
        _, _, H = en.unpack_sums(sums, 3)
        lam = np.linalg.eigvalsh(H)
        print(f"eigenvalues {lam}, trace {np.trace(H):.3e}")
        assert counters[0] > 190 and lam.min() >= -1e-12 * np.trace(H) and H[0, 0] > 1e12


# ---- the fit ---------------------------------------------------------------------------------------------------------------------
def test_fit_converges_to_the_minimum(fit_case):
    blend, c = fit_case["blend"], bc.case()
    assert blend.converged and len(blend.losses) - 1 <= 20 and np.all(np.diff(blend.losses) <= 0)
    assert blend.names == [f"source_{m}" for m in range(6)] and blend.weights.shape == (6,)
    sums, counters, _ = bc.brute_sums(fit_case["features"], c["labels"], c["offsets"], blend.weights)
    J, grad = bc.objective(sums, counters, blend.weights)
    print(f"{len(blend.losses) - 1} iterations, J {J:.6f}, max |grad J| {np.abs(grad).max():.2e}, weights {blend.weights}")
    assert np.abs(grad).max() <= 1e-9 + 1e-12 and abs(J - blend.losses[-1]) <= 1e-12
    assert blend.weights[0] > 0.5  # the raw source carries the largest share of the latent score
    rng = np.random.default_rng(5)
    for _ in range(20):
        w = blend.weights + rng.normal(size=6) * 10.0 ** rng.uniform(-3, 0)
        s, k = blend_sums_host(fit_case["features"], c["labels"], c["offsets"], w)
        assert bc.objective(s, k, w)[0] >= J


def test_skipped_lists_and_nan_predictions(fit_case):
    blend, c = fit_case["blend"], bc.case()
    _, counters, _ = bc.brute_sums(fit_case["features"], c["labels"], c["offsets"], np.zeros(6))
    assert (blend.n_lists_used, blend.n_one_class, blend.n_nonfinite) == tuple(int(v) for v in counters)
    assert blend.n_nonfinite == 2 and blend.n_one_class >= 6 and blend.n_lists_used + blend.n_one_class + blend.n_nonfinite == c["n_lists"]
    pred = blend.predict(_sources(bc.FIT_SOURCES))
    assert isinstance(pred.flat, np.ndarray) and pred.flat.dtype == np.float64 and np.array_equal(pred.offsets, c["offsets"])
    flagged = np.repeat(fit_case["flags"] != 0, c["lengths"])
    assert flagged.sum() > 2 and np.array_equal(np.isnan(pred.flat), flagged)
    f64 = fit_case["features"].astype(np.float64)
    want = sum(blend.weights[m] * f64[m] for m in range(6))
    assert np.allclose(pred.flat[~flagged], want[~flagged], rtol=0, atol=1e-12 * np.abs(want[~flagged]).max())


def test_float32_sources_stay_float32_and_mixed_ones_go_to_float64():
    blend = ScoreBlend(device=None)
    a32 = RaggedLists(np.array([1, 2, 3], np.float32), [0, 3])
    a64 = RaggedLists(np.array([1, 2, 3], np.float64), [0, 3])
    assert blend._stack([a32, a32])[0].dtype == np.float32 and blend._stack([a32, a64])[0].dtype == np.float64
    assert blend._stack([[[1, 2, 3]], a32])[0].dtype == np.float64


def test_rank_fusion_equals_a_hand_computed_fusion():
    a, b = [[0.9, 0.1, 0.5], [2.0, 2.0]], [[1.0, 3.0, 2.0], [5.0, 1.0]]
    got = RankFusion(k=60.0, device=None).predict([a, b])
    # ranks of a: [1, 3, 2] and [1.5, 1.5]; of b: [3, 1, 2] and [1, 2]
    want = np.array([1 / 61 + 1 / 63, 1 / 63 + 1 / 61, 1 / 62 + 1 / 62, 1 / 61.5 + 1 / 61, 1 / 61.5 + 1 / 62])
    assert got.offsets.tolist() == [0, 3, 5] and np.allclose(got.flat, want, rtol=2e-7, atol=0)
    same = ScoreBlend.from_weights(["rrf", "rrf"], [1.0, 1.0], rrf_k=60.0, device=None).predict([a, b])
    assert np.array_equal(same.flat, got.flat)
    assert np.allclose(RankFusion(k=1.0, device=None).predict([a]).flat, [1 / 2, 1 / 4, 1 / 3, 1 / 2.5, 1 / 2.5], rtol=2e-7)


# ---- cross-fitting ---------------------------------------------------------------------------------------------------------------
def test_cross_fit_predict_never_sees_the_labels_it_judges():
    c = bc.case()
    blend = ScoreBlend(transforms=[bc.KIND_NAMES[k] for k in bc.FIT_KINDS], l2=bc.FIT_L2, device=None)
    src, folds = _sources(bc.FIT_SOURCES), 4
    oof, fw = blend.cross_fit_predict(_labels(), src, folds=folds)
    assert fw.shape == (folds, 6) and oof.flat.dtype == np.float64 and np.array_equal(oof.offsets, c["offsets"]) and blend.weights is None
    fold_item = np.repeat(np.arange(c["n_lists"]) % folds, c["lengths"])
    y = c["labels"].astype(np.int64).copy()
    y[fold_item == 1] = 1 - y[fold_item == 1]  # flip the labels of fold 1
    oof2, fw2 = blend.cross_fit_predict(RaggedLists(y, c["offsets"]), src, folds=folds)
    a, b = oof.flat, oof2.flat
    assert np.array_equal(fw[1], fw2[1]) and np.array_equal(a[fold_item == 1], b[fold_item == 1], equal_nan=True)
    for f in (0, 2, 3):
        assert not np.array_equal(fw[f], fw2[f]) and not np.array_equal(a[fold_item == f], b[fold_item == f], equal_nan=True)
    # every fold's rows are the combine of that fold's weights
    for f in range(folds):
        one = ScoreBlend.from_weights([bc.KIND_NAMES[k] for k in bc.FIT_KINDS], fw[f], device=None).predict(src).flat
        assert np.array_equal(one[fold_item == f], a[fold_item == f], equal_nan=True)


def test_cross_fit_folds_by_group_keep_a_group_together():
    groups = np.array(["u3", "u1", "u3", "u7", "u1", "u9", "u7", "u2", "u3"])
    fold = en.fold_of_lists(len(groups), 3, groups)
    assert fold.tolist() == [0, 1, 0, 2, 1, 0, 2, 1, 0]  # u3 u1 u7 u9 u2 in order of first appearance -> 0 1 2 0 1
    assert en.fold_of_lists(5, 2).tolist() == [0, 1, 0, 1, 0]
    c = bc.case()
    users = pd.Series(np.arange(c["n_lists"]) // 3)  # three consecutive lists per user
    blend = ScoreBlend(transforms="zscore", device=None)
    src = _sources([3, 4, 5])
    oof, fw = blend.cross_fit_predict(_labels(), src, folds=3, groups=users)
    fold_item = np.repeat((np.arange(c["n_lists"]) // 3) % 3, c["lengths"])
    for f in range(3):
        one = ScoreBlend.from_weights("zscore", fw[f], device=None).predict(src).flat
        assert np.array_equal(one[fold_item == f], oof.flat[fold_item == f], equal_nan=True)
    with pytest.raises(ValueError):
        blend.cross_fit_predict(_labels(), src, folds=3, groups=users.iloc[:-1])


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_every_value_error():
    lab, a, b = [[0, 1, 0], [1, 0]], [[0.1, 0.9, 0.3], [0.5, 0.2]], [[1.0, 2.0, 3.0], [2.0, 1.0]]
    blend = ScoreBlend(device=None)
    with pytest.raises(ValueError, match="offsets"):
        blend.fit(lab, [a, [[1.0, 2.0], [2.0, 1.0, 0.0]]])
    with pytest.raises(ValueError, match="offsets"):
        blend.fit([[0, 1], [1, 0, 0]], [a, b])
    with pytest.raises(ValueError, match="sources"):
        blend.fit(lab, [])
    with pytest.raises(ValueError, match="sources"):
        blend.fit(lab, [a] * 17)
    with pytest.raises(ValueError, match="sources"):
        RankFusion(device=None).predict([a] * 17)
    with pytest.raises(ValueError, match="transform"):
        ScoreBlend(transforms="softmax", device=None)
    with pytest.raises(ValueError, match="transform"):
        ScoreBlend(transforms=["zscore", "nope"], device=None)
    with pytest.raises(ValueError, match="transforms"):
        ScoreBlend(transforms=["zscore"], device=None).fit(lab, [a, b])
    with pytest.raises(ValueError, match="0 or 1"):
        blend.fit([[0, 2, 0], [1, 0]], [a, b])
    with pytest.raises(ValueError, match="no usable list"):
        blend.fit([[0, 0, 0], [1, 1]], [a, b])
    with pytest.raises(ValueError, match="no usable list"):
        blend.fit(lab, [[[0.1, np.nan, 0.3], [np.inf, 0.2]], b])
    with pytest.raises(ValueError, match="weights"):
        ScoreBlend.from_weights("zscore", [1.0, 2.0], device=None).predict([a])
    with pytest.raises(ValueError):
        ScoreBlend(device=None).predict([a])  # not fitted
    with pytest.raises(ValueError):
        ScoreBlend.from_weights("zscore", np.ones(17))
    ok = blend.fit(pd.Series(lab), [pd.Series(a, name="first"), b], names=None)
    assert ok.names == ["first", "source_1"] and ok.weights.shape == (2,) and ok.n_lists_used == 2


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_example_script_with_blend_on_the_fixture_frames(tmp_path, capsys):
    sys.path.insert(0, str(ROOT / "examples" / "baseline"))
    import ebnerd_feat_baselines

    behaviors, history = pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")
    data = tmp_path / "data"
    for part in ("train", "validation"):
        (data / "fixture" / part).mkdir(parents=True)
        behaviors.to_parquet(data / "fixture" / part / "behaviors.parquet")
        history.to_parquet(data / "fixture" / part / "history.parquet")
    ids = np.unique(np.concatenate([np.concatenate(behaviors["article_ids_inview"].to_list()), np.concatenate(history["article_id_fixed"].to_list())]))
    pd.DataFrame({"article_id": ids}).to_parquet(data / "articles.parquet")
    argv = ["--data_path", str(data), "--datasplit", "fixture", "--dump_dir", str(tmp_path / "out"), "--covisit"]
    without, _ = ebnerd_feat_baselines.main(argv)
    results, _ = ebnerd_feat_baselines.main(argv + ["--blend"])
    out = capsys.readouterr().out
    assert set(results) == set(without) | {"blend_prediction_scores"} and all(results[k] == without[k] for k in without)
    res = results["blend_prediction_scores"]
    assert set(res) == {"auc", "mrr", "ndcg@5", "ndcg@10"} and all(0.0 <= v <= 1.0 for v in res.values())
    assert re.search(r"^blend_prediction_scores: auc \d\.\d{4}  mrr \d\.\d{4}  ndcg@5 \d\.\d{4}  ndcg@10 \d\.\d{4}$", out, flags=re.M)
    line = re.search(r"^blend: (\d+) sources, transform zscore, 5 folds by user; mean fold weights: (.*)$", out, flags=re.M)
    assert line and int(line.group(1)) == len(without) and all(name in line.group(2) for name in without)
    assert (tmp_path / "out" / "blend_prediction_scores.zip").exists()
    ranked, _ = ebnerd_feat_baselines.main(argv + ["--blend", "--blend_transform", "rank"])
    assert ranked["blend_prediction_scores"] != res
