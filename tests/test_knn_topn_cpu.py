"""History-kNN top-N on the host: the float32 twins ``knn_topk_host`` / ``knn_target_rank_host`` against the plain-Python brute force of
tests/knn_topn_cases.py -- lists, scores (as bits), ranks, counts and flags EXACTLY -- and ``HistoryKNN(device=None).recommend`` /
``.rank_targets``: the call forms, ``exclude_self`` on frames and with ``history_keys=``, ``idf``, windows, exclusion, the rank /
list identity, ``return_scores`` against ``predict`` within the bound of tests/knn_cases.py, the errors, the example.  No GPU."""
import re
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from ebrec import _hip
from ebrec.evaluation import RaggedLists, rank_metrics
from ebrec.evaluation.freshness import Freshness
from ebrec.models import CoVisitation, HistoryKNN, knn_target_rank_host, knn_topk_host
from ebrec.models.baselines import knn as knn_mod
from ebrec.models.baselines._topn import TopN
from ebrec.utils import _constants as C
from tests import knn_cases as kc
from tests import knn_topn_cases as tc

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "ebnerd"


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def R():
    return int(_hip.lib().ebn_knn_topk_range())  # a pure host query: no GPU


def test_header_source_and_module_constants_agree(R):
    lib = _hip.lib()
    assert R % 1024 == 0 and R >= 1024
    decl = _hip.declared_functions()
    names = ("ebn_knn_topk_range", "ebn_knn_topk_auto_splits", "ebn_knn_topk_workspace_bytes", "ebn_knn_target_rank_workspace_bytes",
             "ebn_knn_topk_f32", "ebn_knn_target_rank_f32")
    assert [len(decl[n][1]) for n in names] == [0, 2, 3, 3, 25, 26]
    assert (knn_mod.MAX_TOP_K, knn_mod.MAX_EXCLUDE) == (tc.MAX_K, tc.MAX_X) == (64, 256)
    assert int(re.search(r"#define\s+EBN_ABI_VERSION\s+(\d+)", _hip.header_path().read_text()).group(1)) == 1
    assert lib.ebn_knn_topk_auto_splits(1, 3 * R) == 3 and lib.ebn_knn_topk_auto_splits(10 ** 6, 3 * R) == 1
    assert lib.ebn_knn_topk_auto_splits(512, 9 * R) == 4 and lib.ebn_knn_topk_auto_splits(0, 0) == 1 and lib.ebn_knn_topk_auto_splits(-1, 5) == 1
    assert lib.ebn_knn_topk_auto_splits(1, 100 * R) == 64 and lib.ebn_knn_topk_auto_splits(2048, 9 * R) == 1 and lib.ebn_knn_topk_auto_splits(2047, 9 * R) == 2
    assert lib.ebn_knn_topk_workspace_bytes(7, 5, 3) == lib.ebn_topk_workspace_bytes(7, 5, 3) == 7 * 5 * 3 * 8 + 16
    assert lib.ebn_knn_topk_workspace_bytes(7, 65, 3) == 0 and lib.ebn_knn_topk_workspace_bytes(-1, 5, 3) == 0
    q = lib.ebn_knn_target_rank_workspace_bytes
    assert q(7, 3, 0) == (2 * 3 * 7 + 7) * 4 + 16 and q(7, 1, 0) == 16 and q(7, 3, 11) == (2 * 3 * 7 + 7 + 11) * 4 + 16 and q(7, 1, 11) == 60
    assert q(7, 0, 0) == 0 and q(2 ** 31, 2, 0) == 0 and q(7, 2, -1) == 0 and q(7, 2, 2 ** 31) == 0
    # the chain is built from single roundings, one definition for both kernels, and the object is compiled without the unsafe-atomics flag
    csrc = ROOT / "ebnerd-benchmark_amd" / "csrc"
    tile, src = (csrc / "ebn_knn_tile.h").read_text(), (csrc / "ebn_knn_topk.hip").read_text()
    assert "__fadd_rn" in tile and "__fmul_rn" in tile and not re.search(r"\bfmaf?\(|atomicAdd", tile + src)
    assert "knt_step(" in src and "__fadd_rn" not in src  # the rank kernel folds with the tile's step
    mk = (csrc / "Makefile").read_text()
    assert "ebn_knn_topk.hip" in mk and re.search(r"ebn_knn_topk\.o asan/ebn_knn_topk\.o: CXXFLAGS := \$\(filter-out -munsafe-fp-atomics", mk)


CASES = [("1", 65, "random", True), ("3", 65, "random", True), ("R-1", 65, "random", False), ("R", 64, "integer", True), ("R+1", 65, "random", True),
         ("R+1", 1, "random", True), ("R+1", 65, "nan", False), ("R+1", 512, "nan", True), ("2R+37", 512, "random", True)]


@pytest.mark.parametrize("rows,k_nbr,sims,scaled", CASES)
def test_twins_equal_the_brute_force(R, rows, k_nbr, sims, scaled):
    n_rows = {"1": 1, "3": 3, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+37": 2 * R + 37}[rows]
    c = tc.kernel_case(n_rows, R, k_nbr, sims, scaled)
    U = c["n_users"]
    chains = tc.brute_chains(c)
    seen = dict(flag0=set(), flag1=set(), listed=0, ties=0, nonpositive=0)
    for pos_kind in (None, "perm", "oob"):
        cand_pos, M = tc.positions(n_rows, pos_kind)
        p_special = c["special_col"] if cand_pos is None else int(cand_pos[c["special_col"]])
        for X in (0, 1, 256):
            exclude = tc.exclusions(c, X)
            variants = [tc.windows(U, M)] + ([None] if X == 0 else []) + ([tc.windows(U, M, avoid=p_special)] if sims == "nan" and X == 0 else [])
            for window in variants:
                what = (pos_kind, X, window is None)
                w_pos, w_score, w_flags = tc.brute_topk(c, chains, cand_pos, M, window, exclude, 64)
                for k in (64, 5, 1):
                    pos, score, flags = knn_topk_host(*tc.twin_args(c), cand_pos, M, window, exclude, k)
                    assert pos.dtype == np.int32 and score.dtype == np.float32
                    assert np.array_equal(pos, w_pos[:, :k]) and np.array_equal(_bits(score), _bits(w_score[:, :k])), (what, k)
                    assert np.array_equal(flags, w_flags), (what, k)
                target = tc.targets(w_pos, M, U)
                got = knn_target_rank_host(*tc.twin_args(c), cand_pos, M, target, window, exclude)
                want = tc.brute_rank(c, chains, cand_pos, M, target, window, exclude)
                for g, w, name in zip(got, want, ("rank", "count", "score", "flags")):
                    assert np.array_equal(_bits(g) if name == "score" else g, _bits(w) if name == "score" else w), (what, name)
                seen["flag0"].add(int(w_flags[0]))
                seen["flag1"].add(int(w_flags[1]))
                seen["listed"] += int((w_pos >= 0).sum())
                seen["nonpositive"] += int((w_score[w_pos >= 0] <= 0).sum())
                live = w_pos[:, :2].min(1) >= 0
                seen["ties"] += int((w_score[live, 0] == w_score[live, 1]).sum())
    assert seen["listed"] > 0 and seen["flag0"] == ({0, 1} if n_rows > 3 else {0})  # up to 3 rows: "oob" moves no position to M or above
    assert seen["flag1"] == ({0, 1} if sims == "nan" else {0})  # the NaN inside a window; excluded, no candidate or outside every window
    if sims == "integer":
        assert seen["ties"] > 0  # the position decides
    if k_nbr == 1 and scaled:
        assert seen["nonpositive"] > 0  # a touched row with a score of 0 or below is listed


def test_the_chain_runs_in_list_order(R):
    c, forward = tc.order_case(R + 1, R)  # folded in reversed order the special row's sum has other bits (asserted there)
    only = np.tile(np.array([c["special_col"], c["special_col"] + 1], np.int32), (c["n_users"], 1))  # a window of the special row alone
    pos, score, _ = knn_topk_host(*tc.twin_args(c), None, R + 1, only, None, 64)
    assert pos[1, 0] == c["special_col"] and pos[1, 1] == -1 and _bits(score[1, 0]) == _bits(forward)
    rank, count, t, _ = knn_target_rank_host(*tc.twin_args(c), None, R + 1, np.full(c["n_users"], c["special_col"]), None, None)
    assert rank[1] >= 1 and count[1] > 64 and _bits(t[1]) == _bits(forward)


def test_by_hand():
    # sets: 0 = {1, 2}, 1 = {2, 3}, 2 = {}; one neighbour row [0, 1, 0, 7, -1] with sims 1.5, -0.5, 2, 9, -inf: a repeated id counts twice
    sets = (np.array([0, 2, 4, 4]), np.array([1, 2, 2, 3]), 5, None)
    seq, sim = np.array([[0, 1, 0, 7, -1]]), np.array([[1.5, -0.5, 2.0, 9.0, -np.inf]], np.float32)
    pos, score, flags = knn_topk_host(*sets, seq, sim, None, 1, None, 5, None, None, 4)
    assert pos.tolist() == [[1, 2, 3, -1]] and score[0, :3].tolist() == [3.5, 3.0, -0.5] and np.isneginf(score[0, 3]) and not flags.any()
    scale = np.array([1, 0, -1, 2, 1], np.float32)  # a zero score and a negative one are listed, the untouched rows 0 and 4 are not
    pos, score, _ = knn_topk_host(*sets[:3], scale, seq, sim, None, 1, None, 5, None, None, 4)
    assert pos.tolist() == [[1, 3, 2, -1]] and score[0, :3].tolist() == [0.0, -1.0, -3.0]
    rank, count, t, _ = knn_target_rank_host(*sets[:3], scale, seq, sim, np.zeros(3, np.int32), 3, None, 5, np.array([3, 0, 2]), None, np.array([[1], [-1], [2]]))
    assert (rank.tolist(), count.tolist()) == ([1, 0, 0], [2, 3, 2]) and t[0] == -1.0 and np.isneginf(t[1:]).all()
    # a history without neighbours, and one whose only neighbour has an empty set: empty lists, rank 0
    for s in ([[-1, -1]], [[2, -1]]):
        pos, score, _ = knn_topk_host(*sets, np.array(s), np.array([[1.0, -np.inf]], np.float32), None, 1, None, 5, None, None, 3)
        assert (pos == -1).all() and np.isneginf(score).all()
    with pytest.raises(ValueError, match="k must lie"):
        knn_topk_host(*sets, seq, sim, None, 1, None, 5, None, None, 65)
    with pytest.raises(ValueError, match="cand_pos"):
        knn_topk_host(*sets, seq, sim, None, 1, None, 4, None, None, 3)
    with pytest.raises(ValueError, match="nbr_seq"):
        knn_topk_host(*sets, seq, sim[:, :3], None, 1, None, 5, None, None, 3)


# ---- the class on the fixture frames -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


KW = dict(k=20, sample_size=50, similarity="cosine", history_weights="linear", history_size=30, device=None)


@pytest.fixture(scope="module")
def fitted(frames):
    return HistoryKNN(**KW).fit(frames[1])


def _published(knn, frames):
    t0 = frames[0][C.DEFAULT_IMPRESSION_TIMESTAMP_COL].min()
    rng = np.random.default_rng(3)
    ids = knn.index.article_ids
    return {int(a): t0 - pd.Timedelta(hours=int(h)) for a, h in zip(ids, rng.integers(1, 14 * 24, ids.size))}


def test_history_knn_is_a_topn_baseline(fitted):
    assert isinstance(fitted, TopN) and np.array_equal(fitted._topn_ids(), fitted.index.article_ids)
    s = fitted._topn_session(RaggedLists(fitted.index.article_ids[:3], np.array([0, 3])))
    assert isinstance(s, knn_mod.KnnSession) and not s.on_device and s.seq.shape == (1, 20)


def test_the_three_call_forms_agree_and_exclude_self_holds(fitted, frames):
    df, hist = frames
    df = df.head(40)
    ids, scores = fitted.recommend(df, history=hist, top_n=7, return_scores=True)
    assert ids.shape == (40, 7) and scores.shape == (40, 7) and scores.dtype == np.float32
    by_user = dict(zip(hist[C.DEFAULT_USER_COL].tolist(), hist[C.DEFAULT_HISTORY_ARTICLE_ID_COL].tolist()))
    users = df[C.DEFAULT_USER_COL].tolist()
    lists = [list(by_user.get(u, [])) for u in users]
    own = df.assign(**{C.DEFAULT_HISTORY_ARTICLE_ID_COL: lists})
    ids2, scores2 = fitted.recommend(own, top_n=7, return_scores=True)  # keyed by the behaviours' user_id
    ids3, scores3 = fitted.recommend(lists, top_n=7, return_scores=True, history_keys=users)
    for i, s in ((ids2, scores2), (ids3, scores3)):
        assert np.array_equal(i, ids) and np.array_equal(_bits(s), _bits(scores))
    assert (ids >= 0).any() and np.all(np.diff(scores, axis=1)[np.isfinite(scores[:, 1:])] <= 0)
    # without the keys the user's own fitted sequence is its best neighbour: other lists; the same as exclude_self=False
    no_keys = fitted.recommend(lists, top_n=7)
    with_self = HistoryKNN(**dict(KW, exclude_self=False)).fit(hist)
    assert not np.array_equal(no_keys, ids) and np.array_equal(no_keys, with_self.recommend(df, history=hist, top_n=7))
    assert np.array_equal(no_keys, with_self.recommend(lists, top_n=7, history_keys=users))
    # exclusion: no listed article is among the history's last 256 distinct ones (TopN's rule); without it some are
    recent = [list(dict.fromkeys(h[::-1]))[:256] for h in lists]
    assert not any(set(row[row >= 0].tolist()) & set(h) for row, h in zip(ids, recent))
    free = fitted.recommend(lists, top_n=7, exclude_history=False, history_keys=users)
    assert any(set(row[row >= 0].tolist()) & set(h) for row, h in zip(free, lists))
    assert np.array_equal(fitted.recommend(lists, top_n=7, batch_users=7, history_keys=users), ids)
    targets = ids[:, 2].tolist()
    r1 = fitted.rank_targets(df, targets=targets, history=hist)
    r2 = fitted.rank_targets(own, targets=targets)
    r3 = fitted.rank_targets(lists, targets=targets, history_keys=users)
    for r in (r2, r3):
        assert np.array_equal(r.rank, r1.rank) and np.array_equal(r.count, r1.count) and np.array_equal(_bits(r.score), _bits(r1.score))
    assert np.array_equal(r1.rank, np.where(ids[:, 2] >= 0, 3, 0)) and (r1.rank == 3).any()
    clicked = fitted.rank_targets(df, history=hist)  # the clicked articles of the frame
    assert clicked.impression.size >= 40 and clicked.rank.shape == clicked.count.shape
    # a history without neighbours: an empty list padded with fill_id, rank 0, count 0
    unknown = fitted.recommend([[-5, -6], []], top_n=3, fill_id=-9)
    assert unknown.tolist() == [[-9] * 3] * 2
    r = fitted.rank_targets([[-5]], targets=[int(fitted.index.article_ids[0])])
    assert r.rank.tolist() == [0] and r.count.tolist() == [0] and np.isneginf(r.score[0])


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("exclude_history", [True, False])
def test_rank_is_the_index_in_the_list_plus_one(fitted, frames, exclude_history, windowed):
    df, hist = frames
    df = df.head(60)
    kw = dict(history=hist, exclude_history=exclude_history)
    if windowed:
        kw["window"] = Freshness(_published(fitted, frames), max_age=pd.Timedelta(days=9), min_age=pd.Timedelta(hours=2))
    k = 10
    ids, scores = fitted.recommend(df, top_n=k, return_scores=True, **kw)
    art = fitted.index.article_ids
    n = art.size  # per impression: two of its own slots and two fitted articles from anywhere
    targets = [[int(ids[i, i % k]), int(ids[i, k - 1]), int(art[(37 * i) % n]), int(art[(101 * i + 5) % n])] for i in range(len(df))]
    ranks = fitted.rank_targets(df, targets=targets, **kw)
    checked = 0
    for i, a, r, s in zip(ranks.impression, ranks.target_id, ranks.rank, ranks.score):
        at = np.flatnonzero(ids[i] == a)
        if 1 <= r <= k:
            assert at.tolist() == [r - 1] and _bits(scores[i, r - 1]) == _bits(s)
            checked += 1
        else:
            assert at.size == 0 or a == -1
    assert checked > len(df) and (ranks.rank > k).any()
    if windowed:
        assert not np.array_equal(fitted.recommend(df, top_n=k, history=hist, exclude_history=exclude_history), ids)


@pytest.mark.parametrize("idf", [False, True])
def test_return_scores_agree_with_predict_within_the_bound_of_the_scores_kernel(frames, idf):
    _, hist = frames
    knn = HistoryKNN(**dict(KW, idf=idf)).fit(hist)
    assert (knn.index.item_scale is not None) == idf
    lists, keys = list(hist[C.DEFAULT_HISTORY_ARTICLE_ID_COL])[:60], hist[C.DEFAULT_USER_COL].to_numpy()[:60]
    ids, scores = knn.recommend(lists, top_n=12, exclude_history=False, return_scores=True, history_keys=keys)
    cand = [row[row >= 0].tolist() for row in ids]
    pred = knn.predict(cand, lists, history_keys=keys)  # sums in another fixed order
    h_rows, h_off, w = knn._histories(lists)
    seq, sim = knn._neighbours(h_rows, h_off, w, knn._self_of(keys, len(lists)))
    _, _, s_indptr, s_items, _, item_scale = knn.index.host()
    c = dict(s_indptr=s_indptr, s_items=s_items, n_rows=knn.index.n_rows, nbr_seq=seq, nbr_sim=sim, item_scale=item_scale,
             cand_rows=knn.rows_of(np.concatenate([np.asarray(r, np.int64) for r in cand])), cand_offsets=np.asarray(pred.offsets), list_hist=None)
    want, absum, total = kc.brute_scores(c)
    bound = kc.score_bound(c, want, absum, total)  # the bound of the scores kernel: imported, not invented
    got = np.concatenate([s[r >= 0] for s, r in zip(scores, ids)]).astype(np.float64)
    assert got.size == want.size > 300 and np.all(np.abs(got - np.asarray(pred.flat, np.float64)) <= bound) and np.all(np.abs(got - want) <= bound)
    if idf:  # log(n_seqs / df) weighs the lists: other lists than without
        assert not np.array_equal(ids, HistoryKNN(**KW).fit(hist).recommend(lists, top_n=12, exclude_history=False, history_keys=keys))


def test_candidate_ids_exclusion_fill_and_ties_by_hand():
    # four fitted sequences; the query [10, 20] (key "q") shares articles with all of them
    seqs = [[10, 30, 40], [20, 30, 50], [10, 20, 60], [10, 20]]
    knn = HistoryKNN(k=3, sample_size=4, similarity="dot", history_weights=None, device=None).fit(seqs, keys=["a", "b", "c", "q"])
    got, scores = knn.recommend([[10, 20]], top_n=4, return_scores=True, history_keys=["q"])
    # neighbours: c (dot 2), then b and a (dot 1; the more recent first); 10 and 20 are excluded as the history's own
    assert got.tolist() == [[30, 60, 40, 50]] and scores[0].tolist() == [2.0, 2.0, 1.0, 1.0]
    with_own = knn.recommend([[10, 20]], top_n=3)  # without the key the user's own sequence "q" is a neighbour: q, c, b
    assert with_own.tolist() == [[60, 30, 50]]
    got = knn.recommend([[10, 20]], candidate_ids=[60, 50, 10, 70 - 30], top_n=4, fill_id=-7, history_keys=["q"])
    assert got.tolist() == [[60, 50, 40, -7]]  # ties by position in candidate_ids; 10 is excluded
    got = knn.recommend([[10, 20]], candidate_ids=[60, 50, 10], top_n=3, exclude_history=False, history_keys=["q"])
    assert got.tolist() == [[10, 60, 50]]  # 10: c + a = 3
    r = knn.rank_targets([[10, 20], [10, 20], [99]], targets=[40, [10, 30], 30], history_keys=["q", "q", "x"])
    assert r.rank.tolist() == [3, 0, 1, 0] and r.count.tolist() == [4, 4, 4, 0] and r.target_id.tolist() == [40, 10, 30, 30]


def test_errors(fitted, frames):
    df, hist = frames
    art = fitted.index.article_ids
    lists = [[int(art[0])]]
    with pytest.raises(ValueError, match="not among the fitted"):
        fitted.recommend(lists, candidate_ids=[int(art.max()) + 1])
    with pytest.raises(ValueError, match="twice"):
        fitted.recommend(lists, candidate_ids=[int(art[0])] * 2)
    for top_n in (0, 65, True, 2.5):
        with pytest.raises(ValueError, match="top_n"):
            fitted.recommend(lists, top_n=top_n)
    for call in (lambda m: m.recommend(lists), lambda m: m.rank_targets(lists, targets=[1])):
        with pytest.raises(RuntimeError, match="fit has not been called"):
            call(HistoryKNN(device=None))
    with pytest.raises(ValueError, match="window must be"):
        fitted.recommend(lists, window=3)
    with pytest.raises(ValueError, match="batch_users"):
        fitted.recommend(lists, batch_users=0)
    with pytest.raises(ValueError, match="history keys"):
        fitted.recommend(lists, history_keys=[1, 2])
    with pytest.raises(ValueError, match="joined on user_id"):
        fitted.recommend(df.head(3), history=hist, history_keys=[1, 2, 3])
    with pytest.raises(ValueError, match="joined on user_id"):
        fitted.rank_targets(df.head(3), history=hist, history_keys=[1, 2, 3])
    with pytest.raises(ValueError, match="targets must hold"):
        fitted.rank_targets(lists, targets=[1, 2])
    with pytest.raises(ValueError, match="impression_times"):
        fitted.recommend(lists, impression_times=[0])
    # a class whose session takes no keys refuses them, and is called as before
    cv = CoVisitation(device=None).fit([[1, 2, 3], [2, 3]])
    with pytest.raises(ValueError, match="no use for history_keys"):
        cv.recommend([[1]], history_keys=[0])
    assert cv.recommend([[1]], top_n=2).tolist() == [[2, 3]]


def test_class_on_the_fixture_frames_feeds_rank_metrics(frames):
    df, hist = frames
    knn = HistoryKNN(device=None).fit(hist)
    half = len(hist) // 2
    seen = HistoryKNN(device=None).fit(hist.iloc[:half])
    # the fixture's clicked articles are newer than its histories; each user's last history article stands in as the target
    rest = hist.iloc[half:]
    lists = [list(h[:-1]) for h in rest[C.DEFAULT_HISTORY_ARTICLE_ID_COL]]
    targets = [int(h[-1]) for h in rest[C.DEFAULT_HISTORY_ARTICLE_ID_COL]]
    ranks = seen.rank_targets(lists, targets=targets)
    m = rank_metrics(ranks.rank, ks=(5, 10), counts=ranks.count)
    assert all(0.0 <= v <= 1.0 for v in m.values()) and any(k.startswith("hit") for k in m) and (ranks.rank > 0).any()
    ids = knn.recommend(df.head(30), history=hist, top_n=5)
    assert ids.shape == (30, 5) and (ids >= 0).any()


def test_example_script_with_knn_and_topn_on_the_host(tmp_path, capsys):
    sys.path.insert(0, str(ROOT / "tools"))
    sys.path.insert(0, str(ROOT / "examples" / "baseline"))
    import ebnerd_feat_baselines
    from make_synthetic_ebnerd import make

    data = make(tmp_path / "data", split="ebnerd_demo", n_impressions=120, n_users=20, n_articles=60, seed=2)
    argv = ["--data_path", str(data), "--datasplit", "ebnerd_demo", "--dump_dir", str(tmp_path / "out"), "--knn"]
    plain, _ = ebnerd_feat_baselines.main(argv)
    results, _ = ebnerd_feat_baselines.main(argv + ["--topn", "5"])
    out = capsys.readouterr().out
    assert set(results) == set(plain) | {"knn_top5"} and all(results[k] == plain[k] for k in plain)
    row = results["knn_top5"]
    assert {"coverage", "novelty"} <= set(row) and any(k.startswith("hit") for k in row) and 0.0 < row["coverage"] <= 1.0
    assert re.search(r"^knn top-5 over \d+ articles: ", out, flags=re.M)
