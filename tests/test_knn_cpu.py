"""The history-kNN baseline on the host (ebrec/models/baselines/knn.py): the numpy twins of the ebn_knn_* kernels against the
plain-Python brute force of tests/knn_cases.py (neighbours exactly, scores to 1e-12), the tail argument (a twin that reads only
the last sample_size + 1 entries of every posting row equals one that reads whole rows), the index build and its blocks, the recency
order and ``sequence_of``, ``exclude_self``, ``idf``, ``fill``, every constructor / ``predict`` error, HistoryKNN(device=None) on the
fixture frames with its scores in ``DeviceMetricEvaluator``, and the example script with --knn."""
import re
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from ebrec import _hip
from ebrec.evaluation import AucScore, DeviceMetricEvaluator, MrrScore, NdcgScore, RaggedLists
from ebrec.models import ContentSimilarity, HistoryKNN, knn_index_host, knn_neighbours_host, knn_scores_host
from ebrec.models.baselines import knn as knn_mod
from ebrec.utils import _constants as C
from tests import knn_cases as kc

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "ebnerd"
PAIRS = [(S, k) for S in kc.SAMPLES for k in kc.KS if k <= S]


@pytest.fixture(scope="module")
def R():
    return int(_hip.lib().ebn_knn_range())  # a pure host query: no GPU


@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


def test_header_kernel_and_module_constants_agree(R):
    text = _hip.header_path().read_text()
    define = lambda name, src: int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1))
    assert (define("EBN_KNN_MAX_K", text), define("EBN_KNN_MAX_SAMPLE", text)) == (knn_mod.MAX_K, knn_mod.MAX_SAMPLE) == (512, 4096)
    src = (ROOT / "ebnerd-benchmark_amd" / "csrc" / "ebn_knn.hip").read_text()
    assert define("KNN_R", src) == R and R >= 64
    decl = _hip.declared_functions()
    assert [len(decl[n][1]) for n in ("ebn_knn_neighbours_f32", "ebn_knn_scores_f32", "ebn_knn_range")] == [17, 17, 0]
    assert max(kc.SAMPLES) == knn_mod.MAX_SAMPLE and max(kc.KS) == knn_mod.MAX_K


def test_brute_force_by_hand():
    # postings: row 0 -> {0, 2, 3}, row 1 -> {1, 2}, row 2 -> {3}; history (1, 0, 1) with weights (4, 2, 1): items 0 (w 2) then 1 (w 1)
    c = dict(p_indptr=np.array([0, 3, 5, 6]), p_seqs=np.array([0, 2, 3, 1, 2, 3]), seq_scale=None, hist_rows=np.array([1, 0, 1, 7]),
             hist_weights=np.array([4.0, 2.0, 1.0, 9.0], np.float32), hist_offsets=np.array([0, 4]), hist_self=None)
    assert kc.query_items([1, 0, 1, 7], c["hist_weights"], 3) == [(0, 2.0), (1, 1.0)]
    dots = kc.brute_dots(c)
    assert dots == [{0: 2.0, 2: 3.0, 3: 2.0, 1: 1.0}]
    seq, sim = kc.brute_neighbours(c, dots, 4, 4)
    assert seq.tolist() == [[2, 3, 0, 1]] and sim.tolist() == [[3.0, 2.0, 2.0, 1.0]]  # the tie: the more recent id first
    seq, sim = kc.brute_neighbours(c, dots, 2, 2)  # the two most recent of the union are 3 and 2
    assert seq.tolist() == [[2, 3]]
    c["hist_self"] = np.array([2])
    seq, sim = kc.brute_neighbours(c, kc.brute_dots(c), 2, 2)
    assert seq.tolist() == [[3, 1]] and sim.tolist() == [[2.0, 1.0]]
    seq, sim = kc.brute_neighbours(c, kc.brute_dots(c), 9, 5)
    assert seq.tolist() == [[3, 0, 1, -1, -1]] and sim[0, 3] == -np.inf


@pytest.mark.parametrize("variant", list(kc.VARIANTS))
def test_neighbour_twin_equals_the_brute_force_with_and_without_tails(R, variant):
    c, _ = kc.neighbour_case(R, variant)
    for S, k in PAIRS:
        want_seq, want_sim = kc.neighbour_reference(R, variant, S, k)
        args = (c["p_indptr"], c["p_seqs"], c["n_seqs"], c["seq_scale"], c["hist_rows"], c["hist_weights"], c["hist_offsets"], c["hist_self"], S, k)
        seq, sim = knn_neighbours_host(*args)
        assert seq.dtype == np.int32 and sim.dtype == np.float32
        assert np.array_equal(seq, want_seq) and np.array_equal(sim.view(np.int32), want_sim.view(np.int32)), (variant, S, k)
        whole_seq, whole_sim = knn_neighbours_host(*args, tails=False)
        assert np.array_equal(whole_seq, seq) and np.array_equal(whole_sim.view(np.int32), sim.view(np.int32)), (variant, S, k)
    # the case does what its docstring says: with sample_size 300 the single-item history's last candidate sits at entry 301 from the end
    seq, _ = kc.neighbour_reference(R, "integer", 300, 300)
    row2 = c["p_seqs"][c["p_indptr"][2]:c["p_indptr"][3]]
    assert seq[2].tolist() == row2[-301:-1][::-1].tolist()


@pytest.mark.parametrize("name", list(kc.SCORE_CASES))
def test_score_twin_against_the_brute_force(name):
    c, want, _ = kc.score_case(name)
    got = knn_scores_host(c["s_indptr"], c["s_items"], c["n_rows"], c["item_scale"], c["nbr_seq"], c["nbr_sim"], c["list_hist"], c["cand_rows"],
                          c["cand_offsets"])
    assert got.dtype == np.float64 and np.all(np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), 1.0))
    assert np.array_equal(got == 0.0, want == 0.0)


def test_index_build_blocks_and_brute_force():
    seqs = kc.random_sequences(3)
    flat = np.array([a for s in seqs for a in s])
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    ids = np.unique(flat)
    rows = np.searchsorted(ids, flat)
    rows[::17] = -1  # unknown rows are skipped
    whole = knn_index_host(rows, off, ids.size)
    for max_keys in (2, 7, 64, 10 ** 6):
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(knn_index_host(rows, off, ids.size, max_keys), whole)), max_keys
    p_indptr, p_seqs, s_indptr, s_items = whole
    sets = [sorted({int(r) for r in rows[off[s]:off[s + 1]] if r >= 0}) for s in range(len(seqs))]
    assert [s_items[s_indptr[s]:s_indptr[s + 1]].tolist() for s in range(len(seqs))] == sets
    assert [p_seqs[p_indptr[r]:p_indptr[r + 1]].tolist() for r in range(ids.size)] == [[s for s in range(len(seqs)) if r in sets[s]] for r in range(ids.size)]
    assert p_indptr.dtype == s_indptr.dtype == np.int64 and p_seqs.dtype == s_items.dtype == np.int32


def test_recency_order_and_sequence_of():
    seqs = [[1, 2], [2, 3], [3, 4], [4, 5]]
    knn = HistoryKNN(k=2, sample_size=3, device=None, history_weights=None, similarity="dot")
    ix = knn.fit(seqs).index  # input order
    assert ix.sequence_of.tolist() == [0, 1, 2, 3] and ix.keys is None and ix.article_ids.tolist() == [1, 2, 3, 4, 5]
    ix = knn.fit(seqs, keys=["a", "b", "c", "d"], recency=[5, 1, 5, 0]).index  # ties keep the input order: 3, 1, 0, 2
    assert ix.sequence_of.tolist() == [3, 1, 0, 2] and ix.keys.tolist() == ["d", "b", "a", "c"]
    assert [ix.s_items[ix.s_indptr[s]:ix.s_indptr[s + 1]].tolist() for s in range(4)] == [[3, 4], [1, 2], [0, 1], [2, 3]]
    rows, sims = knn.neighbours([[3]])  # article 3: input rows 1 and 2, equal sims: the more recent (input row 2) first
    assert rows.tolist() == [[2, 1]] and sims.tolist() == [[1.0, 1.0]] and rows.dtype == np.int64 and sims.dtype == np.float32
    assert knn.neighbours([[9], []])[0].tolist() == [[-1, -1], [-1, -1]]
    t = lambda *days: [np.datetime64("2023-05-01") + np.timedelta64(d, "D") for d in days]
    frame = pd.DataFrame({C.DEFAULT_USER_COL: [10, 11, 12], C.DEFAULT_HISTORY_ARTICLE_ID_COL: [[1, 2], [2, 3], [3]],
                          C.DEFAULT_HISTORY_IMPRESSION_TIMESTAMP_COL: [t(1, 9), t(2, 3), t(5)]})
    ix = knn.fit(frame).index  # the last times: day 9, 3, 5
    assert ix.sequence_of.tolist() == [1, 2, 0] and ix.keys.tolist() == [11, 12, 10]
    ix = knn.fit(frame.drop(columns=[C.DEFAULT_HISTORY_IMPRESSION_TIMESTAMP_COL])).index  # without the times: row order
    assert ix.sequence_of.tolist() == [0, 1, 2] and ix.keys.tolist() == [10, 11, 12]
    with pytest.raises(ValueError):
        knn.fit(seqs, recency=[1, 2])
    with pytest.raises(ValueError):
        knn.fit(seqs, keys=[1])


def test_exclude_self_idf_and_fill(frames):
    behaviors, history = frames
    kw = dict(k=20, sample_size=50, similarity="cosine", history_weights="linear", history_size=30, device=None)
    knn = HistoryKNN(**kw).fit(history)
    ix = knn.index
    assert not ix.on_device and ix.n_seqs == len(history) and np.array_equal(np.sort(ix.keys), np.sort(history[C.DEFAULT_USER_COL].to_numpy()))
    hists = list(history[C.DEFAULT_HISTORY_ARTICLE_ID_COL])
    users = history[C.DEFAULT_USER_COL].to_numpy()
    rows, sims = knn.neighbours(hists, history_keys=users)
    assert not (rows == np.arange(len(hists))[:, None]).any() and (rows[:, 0] >= 0).all()  # never the user's own sequence
    with_self, sims_self = HistoryKNN(**dict(kw, exclude_self=False)).fit(history).neighbours(hists, history_keys=users)
    assert (with_self[:, 0] == np.arange(len(hists))).mean() > 0.9  # which would otherwise be the best neighbour nearly always
    no_keys, _ = knn.neighbours(hists)
    assert np.array_equal(no_keys, with_self)
    with pytest.raises(ValueError):
        knn.neighbours(hists, history_keys=users[:3])
    # the frame form joins on user_id: the same scores as the list form with the keys, other scores without the exclusion
    scores = knn.predict(behaviors, history=history)
    at = {u: i for i, u in enumerate(np.unique(users).tolist())}
    first = {u: i for i, u in reversed(list(enumerate(users.tolist())))}
    uniq_hists = [hists[first[u]] for u in np.unique(users).tolist()]
    list_hist = np.array([at.get(u, -1) for u in behaviors[C.DEFAULT_USER_COL]], np.int32)
    lists = knn.predict(list(behaviors[C.DEFAULT_INVIEW_ARTICLES_COL]), uniq_hists, list_hist, history_keys=np.unique(users))
    assert np.array_equal(lists.flat, scores.flat) and np.array_equal(lists.offsets, scores.offsets) and np.count_nonzero(scores.flat) > 100
    assert not np.array_equal(HistoryKNN(**dict(kw, exclude_self=False)).fit(history).predict(behaviors, history=history).flat, scores.flat)
    per_impression = behaviors.assign(**{C.DEFAULT_HISTORY_ARTICLE_ID_COL: [list(uniq_hists[k]) if k >= 0 else [] for k in list_hist]})
    assert np.array_equal(knn.predict(per_impression).flat, scores.flat)  # keyed by the behaviours' user_id
    # the scores are the brute force's over operands assembled by hand
    h_rows, h_off, w = knn._histories(RaggedLists.from_lists([np.asarray(h) for h in uniq_hists], dtype=np.int64))
    p_indptr, p_seqs, s_indptr, s_items, seq_scale, _ = ix.host()
    case = dict(p_indptr=p_indptr, p_seqs=p_seqs, seq_scale=seq_scale, hist_rows=h_rows, hist_weights=w, hist_offsets=h_off,
                hist_self=knn._self_of(np.unique(users), len(uniq_hists)))
    assert np.diff(h_off).max() == 30  # history_size is honoured
    nbr_seq, nbr_sim = kc.brute_neighbours(case, kc.brute_dots(case), 50, 20)
    c_rows = knn.rows_of(np.concatenate(list(behaviors[C.DEFAULT_INVIEW_ARTICLES_COL])))
    sc = dict(s_indptr=s_indptr, s_items=s_items, n_rows=ix.n_rows, nbr_seq=nbr_seq, nbr_sim=nbr_sim, item_scale=None, cand_rows=c_rows,
              cand_offsets=scores.offsets, list_hist=list_hist)
    want, _, _ = kc.brute_scores(sc)
    assert np.all(np.abs(scores.flat - want) <= 1e-12 * np.maximum(np.abs(want), 1.0))
    # idf: log(n_seqs / df), float64 rounded once
    idf = HistoryKNN(**dict(kw, idf=True)).fit(history)
    df = np.diff(p_indptr).astype(np.float64)
    assert np.array_equal(idf.index.item_scale, np.log(len(history) / df).astype(np.float32)) and knn.index.item_scale is None
    want_idf, _, _ = kc.brute_scores(dict(sc, item_scale=idf.index.item_scale))
    got_idf = idf.predict(behaviors, history=history).flat
    assert np.all(np.abs(got_idf - want_idf) <= 1e-12 * np.maximum(np.abs(want_idf), 1.0)) and not np.allclose(got_idf, scores.flat)
    # fill: exactly where ContentSimilarity._unscorable says
    filled = HistoryKNN(**dict(kw, fill=-3.0)).fit(history.iloc[:30]).predict(behaviors, history=history.iloc[5:])
    k5 = HistoryKNN(**kw).fit(history.iloc[:30])
    u5 = np.unique(users[5:])
    h5 = k5._histories([hists[5:][first5] for first5 in [list(users[5:]).index(u) for u in u5.tolist()]])
    lh5 = np.array([{u: i for i, u in enumerate(u5.tolist())}.get(u, -1) for u in behaviors[C.DEFAULT_USER_COL]], np.int32)
    where = ContentSimilarity._unscorable(k5.rows_of(np.concatenate(list(behaviors[C.DEFAULT_INVIEW_ARTICLES_COL]))), scores.offsets, h5[0], h5[1], lh5)
    assert np.array_equal(filled.flat == -3.0, where) and 500 < where.sum() < where.size


def test_errors_and_the_empty_fit(frames):
    behaviors, history = frames
    for bad in (dict(k=0), dict(k=513, sample_size=4096), dict(sample_size=0), dict(sample_size=4097), dict(k=11, sample_size=10),
                dict(similarity="jaccard"), dict(history_weights="cubic"), dict(history_size=0), dict(max_keys=1)):
        with pytest.raises(ValueError):
            HistoryKNN(device=None, **bad)
    for bad in (dict(k=2.5), dict(k=True), dict(sample_size="many"), dict(idf=1), dict(exclude_self="yes")):
        with pytest.raises(TypeError):
            HistoryKNN(device=None, **bad)
    knn = HistoryKNN(device=None)
    with pytest.raises(RuntimeError):
        knn.predict(behaviors, history=history)
    with pytest.raises(RuntimeError):
        knn.neighbours([[1]])
    knn.fit(history)
    with pytest.raises(ValueError):
        knn.predict(behaviors, [[1]], history=history)  # histories and history=
    with pytest.raises(ValueError):
        knn.predict([[1, 2]], [[1], [2]])  # 1 list, 2 histories, no list_hist
    with pytest.raises(ValueError):
        knn.predict([[1, 2]])  # no frame, no histories
    with pytest.raises(ValueError):
        knn.predict(behaviors.drop(columns=[C.DEFAULT_USER_COL]), history=history)
    with pytest.raises(ValueError):
        knn.predict(behaviors, history=history, history_keys=[1])  # the frames are joined on user_id
    with pytest.raises(ValueError):
        knn.fit(history.drop(columns=[C.DEFAULT_HISTORY_ARTICLE_ID_COL]))
    with pytest.raises(ValueError):
        knn.predict([[1, 2]], [[1]], list_hist=[0, 0])
    with pytest.raises(ValueError):
        knn.predict([[1, 2]], [[1]], history_keys=[1, 2])
    with pytest.raises(TypeError):
        knn.fit([[1.5, 2.5]])
    with pytest.raises(ValueError):  # weights are finite by contract
        HistoryKNN(device=None, history_weights=lambda n: np.full(n, np.inf)).fit(history).predict(behaviors, history=history)
    empty = HistoryKNN(device=None, fill=-1.5).fit([])
    assert empty.index.n_rows == 0 and empty.index.n_seqs == 0 and empty.index.p_indptr.tolist() == [0] and empty.index.s_indptr.tolist() == [0]
    s = empty.predict(behaviors, history=history)
    assert s.flat.size == sum(len(x) for x in behaviors[C.DEFAULT_INVIEW_ARTICLES_COL]) and (s.flat == -1.5).all()
    assert (HistoryKNN(device=None).fit([[], []]).predict([[1, 2], []], [[1], [2]]).flat == 0.0).all()


def test_class_on_the_fixture_frames_feeds_the_evaluator(frames):
    behaviors, history = frames
    scores = HistoryKNN(device=None).fit(history).predict(behaviors, history=history)
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


def test_example_script_with_knn_on_the_host(tmp_path, capsys):
    sys.path.insert(0, str(ROOT / "tools"))
    sys.path.insert(0, str(ROOT / "examples" / "baseline"))
    import ebnerd_feat_baselines
    from make_synthetic_ebnerd import make

    data = make(tmp_path / "data", split="ebnerd_demo", n_impressions=120, n_users=20, n_articles=60, seed=2)
    argv = ["--data_path", str(data), "--datasplit", "ebnerd_demo", "--dump_dir", str(tmp_path / "out")]
    without, _ = ebnerd_feat_baselines.main(argv)
    results, _ = ebnerd_feat_baselines.main(argv + ["--knn"])
    out = capsys.readouterr().out
    assert set(results) == set(without) | {"knn_prediction_scores"} and "knn_prediction_scores" not in without
    assert all(results[k] == without[k] for k in without)
    res = results["knn_prediction_scores"]
    assert set(res) == {"auc", "mrr", "ndcg@5", "ndcg@10"} and all(0.0 <= v <= 1.0 for v in res.values())
    assert re.search(r"^knn: \d+ sequences of \d+ articles, k 100 of the 1000 most recent, cosine, linear weights$", out, flags=re.M)
    assert (tmp_path / "out" / "knn_prediction_scores.zip").exists()
    blended, _ = ebnerd_feat_baselines.main(argv + ["--knn", "--blend"])
    assert re.search(rf"^blend: {len(without) + 1} sources", capsys.readouterr().out, flags=re.M) and "blend_prediction_scores" in blended
