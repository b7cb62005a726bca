"""The float32 twins of the co-visitation top-N kernels (covisit_topk_host / covisit_target_rank_host) against the plain-Python brute
force of tests/covisit_topn_cases.py -- lists, scores (as bits), ranks, counts and flags EXACTLY -- the transpose, and the twins on
the kernel cases' edge shapes.  No GPU."""
import numpy as np
import pytest

from ebrec.models.baselines import covisit as cv
from tests import covisit_topn_cases as tc

R = 8192  # the rows of one LDS tile of the kernels (ebn_cv_topk_range()); the twins do not depend on it


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _twin_topk(c, cand_pos, M, window, exclude, k, mode):
    return cv.covisit_topk_host(c["t_indptr"], c["t_cols"], c["t_vals"], c["hist_rows"], c["hist_weights"], c["hist_offsets"], c["user_hist"],
                                c["n_users"], cand_pos, M, window, exclude, k, mode)


def _twin_rank(c, cand_pos, M, target, window, exclude, mode):
    return cv.covisit_target_rank_host(c["t_indptr"], c["t_cols"], c["t_vals"], c["hist_rows"], c["hist_weights"], c["hist_offsets"],
                                       c["user_hist"], c["n_users"], cand_pos, M, target, window, exclude, mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("weights", [None, "positive", "negative"])
@pytest.mark.parametrize("values", ["random", "count"])
@pytest.mark.parametrize("pos_kind", [None, "perm", "holes", "oob"])
def test_twins_equal_the_brute_force(pos_kind, values, weights, mode):
    for seed in (1, 2):
        c = tc.small_case(seed, weights=weights, values=values)
        cand_pos, M = tc.positions(c["n_rows"], pos_kind, seed)
        for window, exclude, k in ((None, None, 5), (tc.windows(c["n_users"], M), tc.exclusions(c, 3, seed), 64),
                                   (tc.windows(c["n_users"], M), None, 1), (None, tc.exclusions(c, 1, seed), 5)):
            pos, score, flags = _twin_topk(c, cand_pos, M, window, exclude, k, mode)
            w_pos, w_score, w_flags = tc.brute_topk(c, cand_pos, M, window, exclude, k, mode)
            assert pos.dtype == np.int32 and score.dtype == np.float32
            assert np.array_equal(pos, w_pos) and np.array_equal(_bits(score), _bits(w_score)) and np.array_equal(flags, w_flags)
            assert int(flags[0]) == int(pos_kind == "oob" and (w_pos >= 0).any())
            # targets: each user's slots 0 and 2, a position nobody holds, none, one past the list
            for target in (w_pos[:, 0], w_pos[:, min(2, k - 1)], np.full(c["n_users"], M - 1), np.full(c["n_users"], -1),
                           np.full(c["n_users"], M + 3)):
                got = _twin_rank(c, cand_pos, M, target, window, exclude, mode)
                want = tc.brute_rank(c, cand_pos, M, target, window, exclude, mode)
                for g, w, what in zip(got, want, ("rank", "count", "score", "flags")):
                    assert np.array_equal(_bits(g) if what == "score" else g, _bits(w) if what == "score" else w), what


def test_rank_is_the_index_in_the_list_plus_one():
    c = tc.small_case(5, weights="negative")
    pos, score, _ = _twin_topk(c, None, c["n_rows"], None, None, 64, 0)
    assert (pos >= 0).sum() > 40 and (score[pos >= 0] < 0).any()  # a touched row with a negative score is listed
    for slot in range(8):
        rank, count, t, _ = _twin_rank(c, None, c["n_rows"], pos[:, slot], None, None, 0)
        listed = pos[:, slot] >= 0
        assert np.array_equal(rank[listed], np.full(int(listed.sum()), slot + 1)) and not rank[~listed].any()
        assert np.array_equal(_bits(t[listed]), _bits(score[listed, slot])) and np.all(np.isneginf(t[~listed]))
        assert np.array_equal(count, (pos >= 0).sum(1))


def test_an_untouched_row_is_never_listed_and_a_stored_zero_is():
    # T: row 0 holds columns {1: 0.0, 2: -2.0}; the history [0]: rows 1 and 2 are touched, row 0 and 3 are not
    t_indptr, t_cols, t_vals = np.array([0, 2, 2, 2, 2]), np.array([1, 2], np.int32), np.array([0.0, -2.0], np.float32)
    pos, score, flags = cv.covisit_topk_host(t_indptr, t_cols, t_vals, np.array([0]), None, np.array([0, 1]), None, 1, None, 4, None, None, 4, 0)
    assert pos.tolist() == [[1, 2, -1, -1]] and score[0, :2].tolist() == [0.0, -2.0] and not flags.any()
    rank, count, t, _ = cv.covisit_target_rank_host(t_indptr, t_cols, t_vals, np.array([0]), None, np.array([0, 1]), None, 1, None, 4,
                                                    np.array([3]), None, None, 0)
    assert (rank.tolist(), count.tolist()) == ([0], [2]) and np.isneginf(t[0])


def test_nan_and_inf():
    t_indptr, t_cols = np.array([0, 3, 3, 3]), np.array([0, 1, 2], np.int32)
    t_vals = np.array([np.nan, np.inf, 1.0], np.float32)
    args = (t_indptr, t_cols, t_vals, np.array([0]), None, np.array([0, 1]), None, 1, None, 3)
    pos, score, flags = cv.covisit_topk_host(*args, None, None, 3, 0)
    assert pos.tolist() == [[1, 2, -1]] and np.isposinf(score[0, 0]) and flags.tolist() == [0, 1]
    pos, _, flags = cv.covisit_topk_host(*args, np.array([[1, 3]]), None, 3, 0)  # the NaN outside the window: not seen
    assert pos.tolist() == [[1, 2, -1]] and flags.tolist() == [0, 0]
    _, _, flags = cv.covisit_topk_host(*args, None, np.array([[0]]), 3, 1)  # excluded: not admissible otherwise, no flag
    assert flags.tolist() == [0, 0]
    rank, _, t, flags = cv.covisit_target_rank_host(*args, np.array([0]), None, None, 0)  # the target itself is the NaN
    assert rank.tolist() == [0] and np.isneginf(t[0]) and flags.tolist() == [0, 1]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_transpose_round_trip(seed):
    c = tc.small_case(seed)
    t = (c["t_indptr"], c["t_cols"], c["t_vals"])
    once = cv.covisit_transpose_host(*t)
    twice = cv.covisit_transpose_host(*once)
    for a, b in zip(t, twice):
        assert a.dtype == b.dtype and np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b)
    assert all(np.all(np.diff(once[1][once[0][r]:once[0][r + 1]]) > 0) for r in range(c["n_rows"]))  # strictly ascending per row
    S = tc.matrix_dict(*t)
    assert tc.matrix_dict(*once) == {h: {c_: v for c_ in S if h in S[c_] for v in [S[c_][h]]} for h in {h for r in S.values() for h in r}}


@pytest.mark.parametrize("n_rows", [1, R - 1, R + 1])
def test_twin_on_the_kernel_cases(n_rows):
    """the edge shapes of the kernel grid make sense on the host: full-row users list k rows, history-less users none"""
    c = tc.kernel_case(n_rows, R, "count", None)
    pos, score, flags = _twin_topk(c, None, n_rows, None, None, 5, 0)
    assert not flags.any() and (pos[[0, 1, 7, 8]] == -1).all() and (pos[2, :min(5, n_rows)] >= 0).all()
    assert np.all(np.diff(score[2, :min(5, n_rows)]) <= 0)


def test_argument_errors():
    c = tc.small_case(0)
    with pytest.raises(ValueError, match="k must lie"):
        _twin_topk(c, None, c["n_rows"], None, None, 65, 0)
    with pytest.raises(ValueError, match="mode"):
        _twin_topk(c, None, c["n_rows"], None, None, 5, 2)
    with pytest.raises(ValueError, match="cand_pos"):
        _twin_topk(c, None, c["n_rows"] - 1, None, None, 5, 0)
    with pytest.raises(ValueError, match="cand_pos"):
        _twin_topk(c, np.zeros(3, np.int32), 3, None, None, 5, 0)
