"""EASE top-N on the host: the float32 twins ``ease_topk_host`` / ``ease_target_rank_host`` against the plain-Python brute force of
tests/ease_topn_cases.py -- lists, scores (as bits), ranks, counts and flags EXACTLY, on every case of up to R + 1 catalogue rows --
and ``EASE(device=None).recommend`` / ``.rank_targets`` on the fixture frames: the call forms, windows, exclusion, the rank / list
identity, ``return_scores`` against ``predict`` within the bound of two fp32 summation orders, the errors, ``from_weights``.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from ebrec import _hip
from ebrec.evaluation import RaggedLists
from ebrec.evaluation.freshness import Freshness
from ebrec.models import EASE, ease_target_rank_host, ease_topk_host
from ebrec.models.baselines import ease as ease_mod
from ebrec.models.baselines._topn import TopN
from ebrec.utils import _constants as C
from tests import ease_topn_cases as tc

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "ebnerd"
U32 = 2.0 ** -24


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _hist(c):
    return c["hist_rows"], c["hist_weights"], c["hist_offsets"], c["user_hist"], c["n_users"]


def test_header_source_and_module_constants_agree():
    lib = _hip.lib()  # pure host queries: no GPU
    assert int(lib.ebn_ease_topk_range()) == tc.R and tc.R % 1024 == 0
    decl = _hip.declared_functions()
    names = ("ebn_ease_topk_range", "ebn_ease_topk_auto_splits", "ebn_ease_topk_workspace_bytes", "ebn_ease_target_rank_workspace_bytes",
             "ebn_ease_topk_f32", "ebn_ease_target_rank_f32")
    assert [len(decl[n][1]) for n in names] == [0, 2, 3, 3, 23, 24]
    assert (ease_mod.MAX_TOP_K, ease_mod.MAX_EXCLUDE) == (tc.MAX_K, tc.MAX_X) == (64, 256)
    R = tc.R
    assert lib.ebn_ease_topk_auto_splits(1, 3 * R) == 3 and lib.ebn_ease_topk_auto_splits(10 ** 6, 3 * R) == 1
    assert lib.ebn_ease_topk_auto_splits(4096, 9 * R) == 4 and lib.ebn_ease_topk_auto_splits(0, 0) == 1 and lib.ebn_ease_topk_auto_splits(-1, 5) == 1
    assert lib.ebn_ease_topk_workspace_bytes(7, 5, 3) == lib.ebn_topk_workspace_bytes(7, 5, 3) == 7 * 5 * 3 * 8 + 16
    assert lib.ebn_ease_topk_workspace_bytes(7, 65, 3) == 0 and lib.ebn_ease_topk_workspace_bytes(-1, 5, 3) == 0
    q = lib.ebn_ease_target_rank_workspace_bytes
    assert q(7, 3, 0) == (2 * 3 * 7 + 7) * 4 + 16 and q(7, 1, 0) == 16 and q(7, 3, 11) == (2 * 3 * 7 + 7 + 11) * 4 + 16 and q(7, 1, 11) == 60
    assert q(7, 0, 0) == 0 and q(2 ** 31, 2, 0) == 0 and q(7, 2, -1) == 0 and q(7, 2, 2 ** 31) == 0
    # the chain is built from single roundings and the object is compiled without the unsafe-atomics flag
    src = (ROOT / "ebnerd-benchmark_amd" / "csrc" / "ebn_ease_topk.hip").read_text()
    assert "__fmul_rn" in src and "__fadd_rn" in src and not re.search(r"\bfmaf?\(|atomicAdd", src)
    mk = (ROOT / "ebnerd-benchmark_amd" / "csrc" / "Makefile").read_text()
    assert "ebn_ease_topk.hip" in mk and re.search(r"ebn_ease_topk\.o asan/ebn_ease_topk\.o: CXXFLAGS := \$\(filter-out -munsafe-fp-atomics", mk)


CASES = [(rows, values, weights) for rows in ("1", "3", "R-1", "R", "R+1") for values in tc.VALUES for weights in tc.WEIGHTS[values]]


@pytest.mark.parametrize("rows,values,weights", CASES)
def test_twins_equal_the_brute_force(rows, values, weights):
    n_rows = tc.ROWS[rows]
    c = tc.kernel_case(n_rows, values, weights)
    B, U = c["B"], c["n_users"]
    padded = np.full((n_rows, n_rows + 4), np.nan, np.float32)  # B at another row stride: the twins read the columns < n_rows only
    padded[:, :n_rows] = B
    chains = tc.brute_chains(c)
    seen = dict(flag0=set(), flag1=set(), listed=0, ties=0)
    for pos_kind in (None, "perm", "oob"):
        cand_pos, M = tc.positions(n_rows, pos_kind)
        p_special = c["special_col"] if cand_pos is None else int(cand_pos[c["special_col"]])
        for X in (0, 1, 256):
            exclude = tc.exclusions(c, X)
            variants = [tc.windows(U, M)] + ([None] if X == 0 else []) + ([tc.windows(U, M, avoid=p_special)] if values == "nan" and X == 0 else [])
            for window in variants:
                what = (pos_kind, X, window is None)
                w_pos, w_score, w_flags = tc.brute_topk(c, chains, cand_pos, M, window, exclude, 64)
                for k, mat in ((64, B), (5, padded[:, :n_rows]), (1, B)):
                    pos, score, flags = ease_topk_host(mat, *_hist(c), cand_pos, M, window, exclude, k)
                    assert pos.dtype == np.int32 and score.dtype == np.float32
                    assert np.array_equal(pos, w_pos[:, :k]) and np.array_equal(_bits(score), _bits(w_score[:, :k])), (what, k)
                    assert np.array_equal(flags, w_flags), (what, k)
                target = tc.targets(w_pos, M, U)
                got = ease_target_rank_host(B, *_hist(c), cand_pos, M, target, window, exclude)
                want = tc.brute_rank(c, chains, cand_pos, M, target, window, exclude)
                for g, w, name in zip(got, want, ("rank", "count", "score", "flags")):
                    assert np.array_equal(_bits(g) if name == "score" else g, _bits(w) if name == "score" else w), (what, name)
                seen["flag0"].add(int(w_flags[0]))
                seen["flag1"].add(int(w_flags[1]))
                seen["listed"] += int((w_pos >= 0).sum())
                live = w_pos[:, :2].min(1) >= 0
                seen["ties"] += int((w_score[live, 0] == w_score[live, 1]).sum())
    assert (seen["listed"] > 0 or (values == "nan" and n_rows == 1)) and seen["flag0"] == ({0, 1} if n_rows > 3 else {0})  # up to 3 rows: "oob" moves no position to M or above
    if values == "nan" and n_rows > 1:
        assert seen["flag1"] == {0, 1}  # the NaN inside a window, and outside every window
    if values == "dyadic" and n_rows > 3:
        assert seen["ties"] > 0  # the position decides


def test_the_chain_stores_its_first_product_and_every_column_is_listed():
    # -0.0 stays -0.0 (0 + -0.0 would be +0.0); negative scores are listed: B is dense, nothing is "untouched"
    B = np.array([[0.0, -0.0, -2.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    pos, score, flags = ease_topk_host(B, np.array([7, 0]), None, np.array([0, 2]), None, 1, None, 3, None, None, 3)
    assert pos.tolist() == [[0, 1, 2]] and _bits(score[0]).tolist() == _bits(np.array([0.0, -0.0, -2.0], np.float32)).tolist() and not flags.any()
    # a user without a present entry: an empty list, rank 0, count 0
    pos, score, _ = ease_topk_host(B, np.array([7, -1]), None, np.array([0, 2]), None, 1, None, 3, None, None, 3)
    assert (pos == -1).all() and np.isneginf(score).all()
    rank, count, t, _ = ease_target_rank_host(B, np.array([7, -1]), None, np.array([0, 2]), None, 1, None, 3, np.array([0]), None, None)
    assert (rank.tolist(), count.tolist()) == ([0], [0]) and np.isneginf(t[0])


def test_nan_and_inf():
    B = np.array([[np.nan, np.inf, 1.0, -np.inf]] + [[0.0] * 4] * 3, np.float32)
    args = (B, np.array([0]), None, np.array([0, 1]), None, 1, None, 4)
    pos, score, flags = ease_topk_host(*args, None, None, 4)
    assert pos.tolist() == [[1, 2, 3, -1]] and np.isposinf(score[0, 0]) and np.isneginf(score[0, 2]) and flags.tolist() == [0, 1]
    pos, _, flags = ease_topk_host(*args, np.array([[1, 4]]), None, 4)  # the NaN outside the window: not seen
    assert pos.tolist() == [[1, 2, 3, -1]] and flags.tolist() == [0, 0]
    _, _, flags = ease_topk_host(*args, None, np.array([[0]]), 4)  # excluded: not admissible otherwise, no flag
    assert flags.tolist() == [0, 0]
    rank, _, t, flags = ease_target_rank_host(*args, np.array([0]), None, None)  # the target itself is the NaN
    assert rank.tolist() == [0] and np.isneginf(t[0]) and flags.tolist() == [0, 1]
    rank, count, t, _ = ease_target_rank_host(*args, np.array([3]), None, None)  # -inf ranks as a number: last
    assert (rank.tolist(), count.tolist()) == ([3], [3]) and np.isneginf(t[0])


def test_twin_argument_errors():
    c = tc.kernel_case(3)
    with pytest.raises(ValueError, match="k must lie"):
        ease_topk_host(c["B"], *_hist(c), None, 3, None, None, 65)
    with pytest.raises(ValueError, match="cand_pos"):
        ease_topk_host(c["B"], *_hist(c), None, 2, None, None, 5)
    with pytest.raises(ValueError, match="cand_pos"):
        ease_topk_host(c["B"], *_hist(c), np.zeros(2, np.int32), 2, None, None, 5)
    with pytest.raises(ValueError, match="B must be"):
        ease_topk_host(np.zeros((3, 2), np.float32), *_hist(c), None, 3, None, None, 5)


# ---- the class on the fixture frames -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet"), pd.read_parquet(GOLDEN / "history.parquet")


@pytest.fixture(scope="module")
def fitted(frames):
    return EASE(regularization=20.0, device=None).fit(frames[1])


def _published(ease, frames):
    """publish times for the fitted articles: spread over the two weeks before the first impression"""
    t0 = frames[0][C.DEFAULT_IMPRESSION_TIMESTAMP_COL].min()
    rng = np.random.default_rng(3)
    return {int(a): t0 - pd.Timedelta(hours=int(h)) for a, h in zip(ease.article_ids, rng.integers(1, 14 * 24, ease.article_ids.size))}


def test_ease_is_a_topn_baseline(fitted):
    assert isinstance(fitted, TopN) and np.array_equal(fitted._topn_ids(), fitted.article_ids)
    s = fitted._topn_session(RaggedLists(fitted.article_ids[:3], np.array([0, 3])))
    assert isinstance(s, ease_mod.EaseSession) and not s.on_device and s.device is None


def test_the_three_call_forms_agree(fitted, frames):
    df, hist = frames
    df = df.head(40)
    ids, scores = fitted.recommend(df, history=hist, top_n=7, return_scores=True)
    assert ids.shape == (40, 7) and scores.shape == (40, 7) and scores.dtype == np.float32
    by_user = dict(zip(hist[C.DEFAULT_USER_COL].tolist(), hist[C.DEFAULT_HISTORY_ARTICLE_ID_COL].tolist()))
    lists = [list(by_user.get(u, [])) for u in df[C.DEFAULT_USER_COL].tolist()]
    own = df.assign(**{C.DEFAULT_HISTORY_ARTICLE_ID_COL: lists})
    ids2, scores2 = fitted.recommend(own, top_n=7, return_scores=True)
    ids3, scores3 = fitted.recommend(lists, top_n=7, return_scores=True)
    for i, s in ((ids2, scores2), (ids3, scores3)):
        assert np.array_equal(i, ids) and np.array_equal(_bits(s), _bits(scores))
    assert (ids >= 0).any() and np.all(np.diff(scores, axis=1)[np.isfinite(scores[:, 1:])] <= 0)
    # exclusion: no listed article is among the history's last 256 distinct ones (TopN's rule); without it some are
    recent = [list(dict.fromkeys(h[::-1]))[:256] for h in lists]
    assert not any(set(row[row >= 0].tolist()) & set(h) for row, h in zip(ids, recent))
    free = fitted.recommend(lists, top_n=7, exclude_history=False)
    assert any(set(row[row >= 0].tolist()) & set(h) for row, h in zip(free, lists))
    small = fitted.recommend(lists, top_n=7, batch_users=7)
    assert np.array_equal(small, ids)
    r1 = fitted.rank_targets(df, history=hist)
    r2 = fitted.rank_targets(own)
    r3 = fitted.rank_targets(lists, targets=df[C.DEFAULT_CLICKED_ARTICLES_COL].tolist())
    for r in (r2, r3):
        assert np.array_equal(r.rank, r1.rank) and np.array_equal(r.count, r1.count) and np.array_equal(_bits(r.score), _bits(r1.score))
    # the fixture's clicked articles are newer than its histories: none is a fitted article, so none has a rank
    assert not r1.rank.any() and np.isneginf(r1.score).all() and r1.impression.size >= 40
    r4 = fitted.rank_targets(df, targets=ids[:, 2].tolist(), history=hist)
    assert np.array_equal(r4.rank, np.where(ids[:, 2] >= 0, 3, 0)) and (r4.rank == 3).any()


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
    n = fitted.article_ids.size  # per impression: two of its own slots and two fitted articles from anywhere
    targets = [[int(ids[i, i % k]), int(ids[i, k - 1]), int(fitted.article_ids[(37 * i) % n]), int(fitted.article_ids[(101 * i + 5) % n])]
               for i in range(len(df))]
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
        unwindowed = fitted.recommend(df, top_n=k, history=hist, exclude_history=exclude_history)
        assert not np.array_equal(unwindowed, ids)


def test_return_scores_agree_with_predict_within_the_bound_of_two_summation_orders(fitted, frames):
    df, hist = frames
    by_user = dict(zip(hist[C.DEFAULT_USER_COL].tolist(), hist[C.DEFAULT_HISTORY_ARTICLE_ID_COL].tolist()))
    lists = [list(by_user.get(u, [])) for u in df[C.DEFAULT_USER_COL].head(50).tolist()]
    for hw in (None, "exponential"):
        m = EASE.from_weights(fitted.article_ids, fitted.weights, device=None, history_weights=hw)
        ids, scores = m.recommend(lists, top_n=12, exclude_history=False, return_scores=True)
        cand = [row[row >= 0].tolist() for row in ids]
        pred = m.predict(cand, lists)
        flat = np.asarray(pred.flat, np.float64)
        B = m.host_weights().astype(np.float64)
        h_rows, h_off, w = m._histories(RaggedLists(np.concatenate([np.asarray(l, np.int64) for l in lists]), np.cumsum([0] + [len(l) for l in lists])))
        at = 0
        for u, row in enumerate(cand):
            r = h_rows[h_off[u]:h_off[u + 1]]
            ww = np.ones(r.size) if w is None else w[h_off[u]:h_off[u + 1]].astype(np.float64)
            ok = r >= 0
            for j, a in enumerate(row):
                col = int(m.rows_of(np.asarray([a]))[0])
                bound = 2 * (int(ok.sum()) + 2) * U32 * float(np.abs(ww[ok] * B[r[ok], col]).sum())
                assert abs(float(scores[u, j]) - flat[at]) <= bound, (hw, u, j)
                at += 1
        assert at == flat.size and at > 100


def test_errors(fitted, frames):
    lists = [[int(fitted.article_ids[0])]]
    with pytest.raises(ValueError, match="not among the fitted"):
        fitted.recommend(lists, candidate_ids=[int(fitted.article_ids.max()) + 1])
    with pytest.raises(ValueError, match="twice"):
        fitted.recommend(lists, candidate_ids=[int(fitted.article_ids[0])] * 2)
    for top_n in (0, 65, True, 2.5):
        with pytest.raises(ValueError, match="top_n"):
            fitted.recommend(lists, top_n=top_n)
    for call in (lambda m: m.recommend(lists), lambda m: m.rank_targets(lists, targets=[1])):
        with pytest.raises(RuntimeError, match="fit has not been called"):
            call(EASE(device=None))
    with pytest.raises(ValueError, match="window must be"):
        fitted.recommend(lists, window=3)


def test_candidate_ids_and_from_weights():
    ids = np.array([40, 10, 30, 20])
    B = np.array([[0, 3, 1, 2], [5, 0, 7, 6], [1, 1, 0, 1], [9, 8, 7, 0]], np.float32)  # rows / columns in the order of ids
    m = EASE.from_weights(ids, B, device=None)
    got, scores = m.recommend([[40], [10, 10], [99], []], top_n=3, return_scores=True)
    assert got.tolist() == [[10, 20, 30], [30, 20, 40], [-1, -1, -1], [-1, -1, -1]]  # the history's own article is excluded
    assert scores[0].tolist() == [3.0, 2.0, 1.0] and scores[1].tolist() == [14.0, 12.0, 10.0] and np.isneginf(scores[2:]).all()
    got = m.recommend([[40]], candidate_ids=[30, 20, 40], top_n=3, fill_id=-7)
    assert got.tolist() == [[20, 30, -7]]
    got = m.recommend([[40]], candidate_ids=[30, 20, 40], top_n=3, exclude_history=False)
    assert got.tolist() == [[20, 30, 40]]  # B[40, 40] = 0 ranks last
    r = m.rank_targets([[40], [40], [99]], targets=[20, [40, 30], 10])
    assert r.rank.tolist() == [2, 0, 3, 0] and r.count.tolist() == [3, 3, 3, 0] and r.target_id.tolist() == [20, 40, 30, 10]
    tied = EASE.from_weights(ids, np.ones((4, 4), np.float32), device=None)
    assert tied.recommend([[10]], top_n=3).tolist() == [[20, 30, 40]]  # ties by position: the ids ascend with the rows
    weighted = EASE.from_weights(ids, B, device=None, history_weights="linear", history_size=2)
    got, s = weighted.recommend([[30, 40, 10]], top_n=2, return_scores=True, exclude_history=False)
    # the last two entries, weights 1/2 and 1 (utils/_decay.py: linear): 0.5 * B[40] + B[10] in the order of ids
    assert got.tolist() == [[30, 20]] and s[0].tolist() == [7.5, 7.0]


def test_example_script_with_ease_and_topn_on_the_host(tmp_path, capsys):
    import sys

    sys.path.insert(0, str(ROOT / "tools"))
    sys.path.insert(0, str(ROOT / "examples" / "baseline"))
    import ebnerd_feat_baselines
    from make_synthetic_ebnerd import make

    data = make(tmp_path / "data", split="ebnerd_demo", n_impressions=120, n_users=20, n_articles=60, seed=2)
    argv = ["--data_path", str(data), "--datasplit", "ebnerd_demo", "--dump_dir", str(tmp_path / "out"), "--ease", "--ease_reg", "10"]
    plain, _ = ebnerd_feat_baselines.main(argv)
    results, _ = ebnerd_feat_baselines.main(argv + ["--topn", "5"])
    out = capsys.readouterr().out
    assert set(results) == set(plain) | {"ease_top5"} and all(results[k] == plain[k] for k in plain)
    row = results["ease_top5"]
    assert {"coverage", "novelty"} <= set(row) and any(k.startswith("hit") for k in row) and 0.0 < row["coverage"] <= 1.0
    assert re.search(r"^ease top-5 over \d+ articles: ", out, flags=re.M)
