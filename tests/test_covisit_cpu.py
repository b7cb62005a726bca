"""The co-visitation baseline on the host (ebrec/models/baselines/covisit.py): the numpy twins of the ebn_cv_* kernels against the
plain-Python brute force of tests/covisit_cases.py (keys, CSR and similarities exactly, scores to 1e-12), the blocked matrix build
against the unblocked one, CoVisitation(device=None) on the fixture frames -- alignment, fill, history_size, the weights, the three
call forms, the errors -- ``neighbours``, and the example script with --covisit."""
import re
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from ebrec import _hip
from ebrec.evaluation import RaggedLists
from ebrec.models import CoVisitation, ContentSimilarity, covisit_matrix_host, covisit_pair_keys_host, covisit_scores_host, covisit_values_host
from ebrec.models.baselines import covisit as cv_mod
from ebrec.utils import _constants as C
from ebrec.utils._decay import exponential_decay_weights
from tests import covisit_cases as cc

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "ebnerd"


def test_header_kernel_and_case_constants_agree():
    text = _hip.header_path().read_text()
    assert int(re.search(r"#define\s+EBN_CV_MAX_GAP\s+(\d+)", text).group(1)) == cv_mod.MAX_GAP == cc.MAX_GAP
    assert re.search(r"#define\s+EBN_CV_NO_PAIR\s+INT64_MAX", text) and cv_mod.NO_PAIR == cc.NO_PAIR == 2 ** 63 - 1
    src = (ROOT / "ebnerd-benchmark_amd" / "csrc" / "ebn_covisit.hip").read_text()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1))
    assert (define("CV_T"), define("CV_GW")) == (cc.TILE, cc.GROUP)
    decl = _hip.declared_functions()
    assert [len(decl[n][1]) for n in ("ebn_cv_pair_keys_i64", "ebn_cv_scores_f32")] == [9, 18]


def test_brute_force_by_hand():
    rows, off = [0, 1, 2, 1, 2, 3, 3, 9], [0, 4, 4, 7]  # sequences (0 1 2 1), (), (2 3 3); a trailing entry; n_rows 4
    keys = cc.brute_keys(rows, off, 4, 2, False).reshape(8, 2).tolist()
    N = cc.NO_PAIR
    assert keys == [[4, 8], [9, N], [6, N], [N, N], [14, 14], [N, N], [N, N], [N, N]]
    assert cc.brute_counts(rows, off, 4, 2, False) == {1: {0: 1, 2: 1}, 2: {0: 1, 1: 1}, 3: {2: 2}}
    sym = cc.brute_counts(rows, off, 4, 2, True)
    assert sym == {0: {1: 1, 2: 1}, 1: {0: 1, 2: 2}, 2: {0: 1, 1: 2, 3: 2}, 3: {2: 2}}
    assert cc.brute_values(sym, 4, "conditional").tolist() == np.array([1 / 3, 1 / 5, 1 / 2, 2 / 5, 1 / 2, 2 / 3, 1, 2 / 5], np.float32).tolist()
    assert cc.brute_values(sym, 4, "cosine")[0] == np.float32(1 / np.sqrt(2 * 3))


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("G", [1, 3, cc.MAX_GAP])
def test_pair_keys_twin_equals_brute_force(G, symmetric):
    rows, off, n_rows = cc.pair_case(G)
    want = cc.pair_reference(G, symmetric)
    got = covisit_pair_keys_host(rows, off, n_rows, G, symmetric)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert want[want != cc.NO_PAIR].max() > 2 ** 32 and (want != cc.NO_PAIR).sum() > 100
    tail = want.reshape(rows.size, -1)[int(off[-1]):]
    assert tail.shape[0] == 9 and (tail == cc.NO_PAIR).all()  # entries past the last sequence
    lengths = np.diff(off)
    assert {0, 1, 2, G, G + 1} <= set(lengths.tolist()) and (lengths == 0).sum() > cc.TILE


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("G", [1, 4])
def test_matrix_and_similarities_equal_brute_force(G, symmetric):
    rows, off = cc.random_sequences(10 + G)
    n_rows = 30
    counts = cc.brute_counts(rows, off, n_rows, G, symmetric)
    want = cc.brute_csr(counts, n_rows)
    got = covisit_matrix_host(rows, off, n_rows, G, symmetric)
    assert [a.dtype for a in got] == [np.int64, np.int32, np.int32]
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and want[2].max() >= 3 and want[1].size > 100
    for similarity in ("count", "cosine", "conditional"):
        v = covisit_values_host(*got, similarity)
        assert v.dtype == np.float32 and np.array_equal(v, cc.brute_values(counts, n_rows, similarity)), similarity
    with pytest.raises(ValueError):
        covisit_values_host(*got, "jaccard")


def test_blocked_build_equals_the_unblocked_one():
    rows, off = cc.random_sequences(3, n_seqs=60)
    whole = covisit_matrix_host(rows, off, 30, 3, True)
    longest_keys = int(np.diff(off).max()) * 6
    for max_keys in (6 * int(off[-1]) // 3, longest_keys + 6, longest_keys - 1, 1):
        cut = cv_mod.sequence_blocks(off, 6, max_keys)
        assert cut[0] == 0 and cut[-1] == off.size - 1 and all(b > a for a, b in zip(cut[:-1], cut[1:]))
        assert len(cut) - 1 >= 3
        for a, b in zip(cut[:-1], cut[1:]):  # within the budget, or a single sequence
            assert (off[b] - off[a]) * 6 <= max_keys or b == a + 1
        blocked = covisit_matrix_host(rows, off, 30, 3, True, max_keys=max_keys)
        assert all(np.array_equal(a, b) for a, b in zip(whole, blocked)), max_keys
    assert cv_mod.sequence_blocks(off, 6, None) == [0, off.size - 1]
    with pytest.raises(ValueError):
        cv_mod.sequence_blocks(off, 6, 0)


@pytest.mark.parametrize("name", cc.SCORE_NAMES)
def test_scores_twin_equals_brute_force(name):
    c, ref = cc.score_case(name)
    for mode in (0, 1):
        got = covisit_scores_host(c["indptr"], c["cols"], c["vals"], c["hist_rows"], c["hist_weights"], c["hist_offsets"], c["list_hist"],
                                  c["cand_rows"], c["cand_offsets"], mode)
        want = ref[mode][0]
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), 1.0)), (name, mode)
        assert np.count_nonzero(want) > 40, "a vacuous case"
    assert np.array_equal(covisit_scores_host(c["indptr"], c["cols"], c["vals"], c["hist_rows"], c["hist_weights"], c["hist_offsets"],
                                              c["list_hist"], c["cand_rows"], c["cand_offsets"], "max"), got)
    with pytest.raises(ValueError):
        covisit_scores_host(c["indptr"], c["cols"], c["vals"], c["hist_rows"], None, c["hist_offsets"], c["list_hist"], c["cand_rows"],
                            c["cand_offsets"], 2)


def test_the_score_cases_cover_the_listed_edges():
    c, ref = cc.score_case("weighted")
    indptr, cols, n_rows = c["indptr"], c["cols"], c["indptr"].size - 1
    assert np.diff(indptr)[:7].tolist() == cc.ROW_COLUMNS
    assert set(cc.HIST_LENGTHS) <= set(np.diff(c["hist_offsets"]).tolist())
    assert c["cand_rows"].size > cc.TILE and (np.diff(c["cand_offsets"]) == 0).sum() >= 3
    lh, n_hists = c["list_hist"], c["hist_offsets"].size - 1
    assert -1 in lh and n_hists in lh and np.bincount(lh[lh >= 0]).max() >= 6
    assert -1 in c["cand_rows"] and n_rows in c["cand_rows"] and -1 in c["hist_rows"] and n_rows in c["hist_rows"]
    w, v = c["hist_weights"], c["vals"]
    assert 2.0 ** -10 <= min(w.min(), v.min()) and max(w.max(), v.max()) <= 2.0 ** 10
    for u in (2, 3, 4, 5):  # the histories of 63, 64, 65 and 130 entries
        h = c["hist_rows"][c["hist_offsets"][u]:c["hist_offsets"][u + 1]]
        assert np.unique(h).size < h.size, "no duplicate entry"
        for r in range(1, 7):
            cr = cols[indptr[r]:indptr[r + 1]]
            assert cr[0] in h and cr[-1] in h and (h[(h >= 0) & (h < n_rows)] < cr[0]).any() and (h[h < n_rows] > cr[-1]).any()
            if cr.size > 1:
                assert ((h > cr[0]) & (h < cr[-1]) & ~np.isin(h, cr)).any(), "no miss between two columns"
    assert cc.score_case("unweighted")[0]["hist_weights"] is None and cc.score_case("identity")[0]["list_hist"] is None
    e, eref = cc.score_case("exact")
    assert e["exact"] and eref[0][0].max() < 2 ** 24 and np.array_equal(eref[0][0], np.round(eref[0][0])) and not eref[0][1].any()
    assert ref[0][1].max() < 1e-4 * np.abs(ref[0][0]).max()


@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


@pytest.mark.parametrize("mode", ["sum", "max"])
def test_class_on_the_fixture_frames(frames, mode):
    behaviors, history = frames
    fit_on = history.iloc[:30]  # some validation articles are unknown to the matrix
    kw = dict(max_gap=3, symmetric=True, similarity="cosine", mode=mode, history_weights="exponential", lambda_factor=0.9, history_size=25,
              device=None)
    cv = CoVisitation(**kw)
    assert cv.fit(fit_on) is cv
    m = cv.matrix
    ids = np.unique(np.concatenate(list(fit_on[C.DEFAULT_HISTORY_ARTICLE_ID_COL])))
    assert np.array_equal(m.article_ids, ids) and m.n_rows == ids.size and m.nnz == m.cols.size == m.counts.size == m.vals.size > 1000
    assert m.vals.dtype == np.float32 and m.indptr.dtype == np.int64 and not m.on_device
    seqs = [np.asarray(h) for h in fit_on[C.DEFAULT_HISTORY_ARTICLE_ID_COL]]
    rows = cv.rows_of(np.concatenate(seqs))
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    counts = cc.brute_counts(rows, off, ids.size, 3, True)
    assert all(np.array_equal(a, b) for a, b in zip((m.indptr, m.cols, m.counts), cc.brute_csr(counts, ids.size)))
    assert np.array_equal(m.vals, cc.brute_values(counts, ids.size, "cosine"))
    # predict: aligned with the in-view lists, equal to the brute force over operands assembled by hand
    scores = cv.predict(behaviors, history=history)
    assert isinstance(scores, RaggedLists) and isinstance(scores.flat, np.ndarray) and scores.flat.dtype == np.float64
    assert scores.lengths.tolist() == [len(x) for x in behaviors[C.DEFAULT_INVIEW_ARTICLES_COL]]
    case = cc.frames_case(cv, behaviors, history, lambda n: exponential_decay_weights(n, 0.9, ascending=True))
    want, _, present = cc.brute_scores(case, cv_mod.MODES.index(mode))
    assert np.all(np.abs(scores.flat - want) <= 1e-12 * np.maximum(np.abs(want), 1.0)) and np.count_nonzero(want) > 100
    assert present.max() == 25  # history_size is honoured
    # without the weights and the cut the scores differ
    plain = CoVisitation(**dict(kw, history_weights=None, history_size=None)).fit(fit_on)
    want_plain, _, _ = cc.brute_scores(cc.frames_case(plain, behaviors, history), cv_mod.MODES.index(mode))
    got_plain = plain.predict(behaviors, history=history).flat
    assert np.all(np.abs(got_plain - want_plain) <= 1e-12 * np.maximum(np.abs(want_plain), 1.0)) and not np.allclose(got_plain, scores.flat)
    # fill: exactly where ContentSimilarity._unscorable says
    filled = CoVisitation(**dict(kw, fill=-3.0)).fit(fit_on).predict(behaviors, history=history.iloc[5:])
    case5 = cc.frames_case(cv, behaviors, history.iloc[5:])
    at = ContentSimilarity._unscorable(case5["cand_rows"], case5["cand_offsets"], case5["hist_rows"], case5["hist_offsets"], case5["list_hist"])
    assert np.array_equal(filled.flat == -3.0, at) and 500 < at.sum() < at.size
    # the three call forms agree
    per_impression = behaviors.assign(**{C.DEFAULT_HISTORY_ARTICLE_ID_COL: [
        list(history[C.DEFAULT_HISTORY_ARTICLE_ID_COL].iloc[k]) if k >= 0 else [] for k in case["list_hist"]]})
    assert np.array_equal(cv.predict(per_impression).flat, scores.flat)
    lists = cv.predict(list(behaviors[C.DEFAULT_INVIEW_ARTICLES_COL]), list(history[C.DEFAULT_HISTORY_ARTICLE_ID_COL]), case["list_hist"])
    assert np.array_equal(lists.flat, scores.flat) and np.array_equal(lists.offsets, scores.offsets)
    ragged = cv.predict(RaggedLists.from_lists([np.asarray(x) for x in behaviors[C.DEFAULT_INVIEW_ARTICLES_COL]], dtype=np.int64),
                        RaggedLists.from_lists([np.asarray(x) for x in history[C.DEFAULT_HISTORY_ARTICLE_ID_COL]], dtype=np.int64), case["list_hist"])
    assert np.array_equal(ragged.flat, scores.flat)
    # fit on lists of lists gives the same matrix
    again = CoVisitation(**kw).fit([list(s) for s in seqs]).matrix
    assert all(np.array_equal(a, b) for a, b in zip(again.host(), m.host())) and np.array_equal(again.article_ids, m.article_ids)


def test_errors_and_the_empty_fit(frames):
    behaviors, history = frames
    for bad in (dict(max_gap=0), dict(max_gap=65), dict(max_gap=2.5), dict(similarity="jaccard"), dict(mode="mean"), dict(history_weights="cubic"),
                dict(history_size=0), dict(max_keys=0)):
        with pytest.raises(ValueError):
            CoVisitation(device=None, **bad)
    cv = CoVisitation(device=None)
    with pytest.raises(RuntimeError):
        cv.predict(behaviors, history=history)
    with pytest.raises(RuntimeError):
        cv.neighbours(1)
    cv.fit(history)
    with pytest.raises(ValueError):
        cv.predict(behaviors, [[1]], history=history)  # histories and history=
    with pytest.raises(ValueError):
        cv.predict([[1, 2]], [[1], [2]])  # 1 list, 2 histories, no list_hist
    with pytest.raises(ValueError):
        cv.predict([[1, 2]])  # no frame, no histories
    with pytest.raises(ValueError):
        cv.predict(behaviors.drop(columns=[C.DEFAULT_USER_COL]), history=history)
    with pytest.raises(ValueError):
        cv.fit(history.drop(columns=[C.DEFAULT_HISTORY_ARTICLE_ID_COL]))
    with pytest.raises(ValueError):
        cv.predict([[1, 2]], [[1]], list_hist=[0, 0])
    empty = CoVisitation(device=None, fill=-1.5).fit([])
    assert empty.matrix.n_rows == 0 and empty.matrix.nnz == 0 and empty.matrix.indptr.tolist() == [0]
    s = empty.predict(behaviors, history=history)
    assert s.flat.size == sum(len(x) for x in behaviors[C.DEFAULT_INVIEW_ARTICLES_COL]) and (s.flat == -1.5).all()
    assert (CoVisitation(device=None).fit([[], []]).predict([[1, 2], []], [[1], [2]]).flat == 0.0).all()


def test_neighbours_order_and_tie_rule():
    # after 10: 30 twice, 20 twice, 40 once; counts as values
    cv = CoVisitation(max_gap=1, symmetric=False, similarity="count", device=None).fit([[30, 10], [20, 10], [30, 10], [20, 10], [40, 10], [10, 50]])
    ids, vals = cv.neighbours(10, n=10)
    assert ids.tolist() == [20, 30, 40] and vals.tolist() == [2.0, 2.0, 1.0] and vals.dtype == np.float32
    assert [a.tolist() for a in cv.neighbours(10, n=1)] == [[20], [2.0]]
    assert cv.neighbours(50)[0].tolist() == [10] and cv.neighbours(30)[0].size == 0 and cv.neighbours(10, n=0)[0].size == 0
    with pytest.raises(KeyError):
        cv.neighbours(99)
    sym = CoVisitation(max_gap=2, symmetric=True, similarity="conditional", device=None).fit([[1, 2, 3], [1, 3]])
    ids, vals = sym.neighbours(3, n=5)
    # C[3, 1] = 2, C[3, 2] = 1; d_col[1] = C[2, 1] + C[3, 1] = 3, d_col[2] = C[1, 2] + C[3, 2] = 2
    assert dict(zip(ids.tolist(), vals.tolist())) == {1: float(np.float32(2 / 3)), 2: float(np.float32(1 / 2))} and ids.tolist() == [1, 2]


def test_example_script_with_covisit_on_the_host(tmp_path, capsys):
    sys.path.insert(0, str(ROOT / "tools"))
    sys.path.insert(0, str(ROOT / "examples" / "baseline"))
    import ebnerd_feat_baselines
    from make_synthetic_ebnerd import make

    data = make(tmp_path / "data", split="ebnerd_demo", n_impressions=120, n_users=20, n_articles=60, seed=2)
    argv = ["--data_path", str(data), "--datasplit", "ebnerd_demo", "--dump_dir", str(tmp_path / "out")]
    without, _ = ebnerd_feat_baselines.main(argv)
    results, _ = ebnerd_feat_baselines.main(argv + ["--covisit"])
    out = capsys.readouterr().out
    assert set(results) == set(without) | {"covisit_prediction_scores"} and "covisit_prediction_scores" not in without
    assert all(results[k] == without[k] for k in without)
    res = results["covisit_prediction_scores"]
    assert set(res) == {"auc", "mrr", "ndcg@5", "ndcg@10"} and all(0.0 <= v <= 1.0 for v in res.values())
    assert re.search(r"^covisit: \d+ pairs of \d+ articles, max gap 3, cosine, sum$", out, flags=re.M)
    assert (tmp_path / "out" / "covisit_prediction_scores.zip").exists()
    # the same scores as the class gives on the same frames
    train_h = pd.read_parquet(data / "ebnerd_demo" / "train" / "history.parquet")
    val_h = pd.read_parquet(data / "ebnerd_demo" / "validation" / "history.parquet")
    val = pd.read_parquet(data / "ebnerd_demo" / "validation" / "behaviors.parquet")
    scores = CoVisitation(device=None).fit(train_h).predict(val, history=val_h)
    assert scores.lengths.tolist() == [len(x) for x in val[C.DEFAULT_INVIEW_ARTICLES_COL]] and np.count_nonzero(scores.flat) > 0
