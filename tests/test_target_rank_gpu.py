"""ebn_target_rank_f32 (csrc/ebn_target_rank.hip) and model.rank_targets() on the GPU: against the float64 restatement of
tests/target_rank_cases.py, against the lists of ebn_topk_score_f32 / ebn_topk_score_window_f32 (the same score bits, the same
total order) and against model.recommend()."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import target_rank_cases as tc
from tests.guarded import guard_in, guard_out, poison
from tests.hip_testutil import P, S, dev
from tests.test_recommend_gpu import _lstur_case, _nrms_case, run_topk
from tests.test_recommend_window_gpu import _candidates, _timed_behaviours, run_window

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3
TAIL = 5  # output elements behind U that must stay as they were


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _opt(a):
    return None if a is None else dev(a, torch.int32)


def launch_rank(hip, users_d, news_d, cand_d, target_d, window_d, ex_d, mode=0, n_splits=0):
    """one call on device tensors -> (rank [U] int32, count [U] int32, score [U] float32, flags [2]) as numpy arrays; the outputs
    are allocated TAIL elements longer, which must come back untouched"""
    U, F = users_d.shape
    n_rows = news_d.shape[0]
    M = n_rows if cand_d is None else len(cand_d)
    X = 0 if ex_d is None else ex_d.shape[1]
    rank_d = torch.full((U + TAIL,), -7, dtype=torch.int32, device="cuda")
    count_d = torch.full((U + TAIL,), -9, dtype=torch.int32, device="cuda")
    score_d = torch.full((U + TAIL,), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    splits = n_splits if n_splits > 0 else int(hip.lib().ebn_topk_auto_splits(U, M))
    ws_bytes = int(hip.lib().ebn_target_rank_workspace_bytes(U, splits))
    assert ws_bytes > 0
    ws_d = poison(torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"))
    code = hip.lib().ebn_target_rank_f32(P(users_d), P(news_d), n_rows, P(cand_d), M, P(target_d), P(window_d), P(ex_d), X, mode, n_splits,
                                         P(rank_d), P(count_d), P(score_d), P(flags_d), P(ws_d), ws_bytes, U, F, S())
    assert code == OK, code
    torch.cuda.synchronize()
    assert (rank_d[U:] == -7).all() and (count_d[U:] == -9).all() and (score_d[U:] == 123.0).all()
    return rank_d[:U].cpu().numpy(), count_d[:U].cpu().numpy(), score_d[:U].cpu().numpy(), flags_d.cpu().numpy()


def run_rank(hip, users, news, cand_rows, target, window, exclude, mode=0, n_splits=0):
    return launch_rank(hip, dev(users), dev(news), _opt(cand_rows), dev(target, torch.int32), _opt(window), _opt(exclude), mode, n_splits)


def _shape_id(s):
    return "x".join(map(str, s))


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("pattern", [None] + tc.PATTERNS)
@pytest.mark.parametrize("exclude", [None, "x3", "all"])
@pytest.mark.parametrize("cand", ["null", "subset"])
@pytest.mark.parametrize("shape", tc.EXACT_SHAPES, ids=_shape_id)
def test_integer_cases_equal_the_restatement(hip, shape, cand, exclude, pattern):
    """Integer-valued inputs: fp32 is exact in any order and ties are frequent, so rank, count and flags must equal the float64
    restatement, and the raw score of a ranked target its float64 score.  "subset" lists carry two rows outside the table."""
    U, M, F = shape
    users, news, cand_rows, ex = tc.integer_case(U, M, F, seed=U + M, cand=cand, exclude=exclude)
    n_rows = news.shape[0]
    if cand_rows is not None:
        cand_rows = tc.with_bad_rows(cand_rows, n_rows)
    window = None if pattern is None else tc.windows(pattern, U, M, seed=U)
    target = tc.targets(U, M, M, window, cand_rows, n_rows, ex)
    s64 = tc.scores64(users, news, cand_rows)
    want_rank, want_count, want_flags = tc.rank_reference(s64, target, window, cand_rows, n_rows, ex)
    rank, count, score, flags = run_rank(hip, users, news, cand_rows, target, window, ex)
    assert np.array_equal(count, want_count)
    assert np.array_equal(rank, want_rank)
    if want_flags[0] == 0 and tc.row_flag_is_open(window, cand_rows, n_rows, M):
        assert flags[0] in (0, 1) and flags[1] == 0
    else:
        assert tuple(flags) == want_flags
    ranked = want_rank > 0
    assert np.array_equal(score[ranked].astype(np.float64), s64[np.flatnonzero(ranked), target[ranked]])
    assert np.isneginf(score[~ranked]).all()
    if pattern == "empty":
        assert (count == 0).all() and (rank == 0).all()
    if exclude == "all" and M <= 256 and pattern in (None, "all", "outside"):
        assert count[0] == 0 and rank[0] == 0  # the user whose every candidate row is excluded


# ------------------------------------------------------------------------------------------------ against the existing kernel
@pytest.mark.parametrize("pattern", [None, "random", "sliding"])
@pytest.mark.parametrize("shape", [tc.ROUNDED_SHAPES[1][:3], (65, 257, 36)], ids=_shape_id)
def test_ranks_and_score_bits_are_those_of_the_top_k_lists(hip, shape, pattern):
    """standard-normal operands, k = 64: rank r <= 64 iff the list of ebn_topk_score[_window]_f32 has the target at index r - 1, and
    out_score has the bits of that slot's score in both modes -- the bits requirement made observable, no tolerance.  Half of the
    targets are taken out of the lists themselves, the others are the generator's mix."""
    U, M, F = shape
    k = 64
    rng = np.random.default_rng(11)
    users, news = rng.standard_normal((U, F)).astype(np.float32), rng.standard_normal((M, F)).astype(np.float32)
    ex = rng.integers(0, M, (U, 5)).astype(np.int32)
    window = None if pattern is None else tc.windows(pattern, U, M, seed=4)
    lists = {}
    for mode in (0, 1):
        lists[mode] = run_topk(hip, users, news, None, ex, k, mode=mode) if window is None else run_window(hip, users, news, None, window, ex, k, mode=mode)
    pos = lists[0][0]
    target = tc.targets(U, M, 3, window, None, M, ex)
    for u in range(0, U, 2):
        kept = pos[u][pos[u] >= 0]
        if len(kept):
            target[u] = kept[(7 * u) % len(kept)]
    n_in_list = 0
    for mode in (0, 1):
        rank, count, score, flags = run_rank(hip, users, news, None, target, window, ex, mode=mode)
        lpos, lscore, _ = lists[mode]
        assert np.array_equal(lpos, pos) and flags[1] == 0
        assert np.array_equal(np.minimum(count, k), (pos >= 0).sum(1))
        for u in range(U):
            r, tp = int(rank[u]), int(target[u])
            if 1 <= r <= k:
                assert pos[u, r - 1] == tp, (u, r)
                assert bits(score[u:u + 1])[0] == bits(lscore[u, r - 1:r])[0], (u, r)
                n_in_list += 1
            else:
                assert tp not in pos[u].tolist() or tp < 0, (u, r)
                assert (r == 0) == bool(np.isneginf(score[u])), u
    assert n_in_list >= U // 2  # the case exercises the lists


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("shape", [s[:3] for s in tc.ROUNDED_SHAPES], ids=_shape_id)
def test_standard_normal_ranks_lie_in_the_float64_interval(hip, shape):
    """Every rank lies in [1 + #{s64 > t64 + 2 b}, 1 + #{s64 >= t64 - 2 b}] over the admissible candidates other than the target
    (b: the fp32 summation bound of the inputs, recommend_cases.summation_bound; two scores, each within b of its float64 value);
    count and the set of ranked users are exact."""
    U, M, F = shape
    rng = np.random.default_rng(13)
    users, news = rng.standard_normal((U, F)).astype(np.float32), rng.standard_normal((M, F)).astype(np.float32)
    ex = rng.integers(0, M, (U, 5)).astype(np.int32)
    window = tc.windows("random", U, M, seed=5)
    window[::3] = [0, M]
    target = tc.targets(U, M, 2, window, None, M, ex)
    b = tc.summation_bound(users, news)
    s64 = tc.scores64(users, news)
    want_rank, want_count, want_flags = tc.rank_reference(s64, target, window, None, M, ex)
    rank, count, score, flags = run_rank(hip, users, news, None, target, window, ex)
    assert np.array_equal(count, want_count) and np.array_equal(rank > 0, want_rank > 0) and tuple(flags) == want_flags
    c = tc.clamp(window, M)
    widest = 0
    for u in np.flatnonzero(rank > 0):
        adm = np.zeros(M, bool)
        adm[c[u, 0]:c[u, 1]] = True
        adm[ex[u]] = False
        adm[target[u]] = False
        t = s64[u, target[u]]
        lo, hi = 1 + int((s64[u, adm] > t + 2 * b).sum()), 1 + int((s64[u, adm] >= t - 2 * b).sum())
        widest = max(widest, hi - lo)
        assert lo <= rank[u] <= hi, (u, lo, int(rank[u]), hi)
        assert abs(float(score[u]) - t) <= b, u
    print(f"shape {shape}: b = {b:.3e}, widest interval {widest}, {int((rank != want_rank).sum())} ranks differ from float64's")


# ------------------------------------------------------------------------------------------------ invariance
@pytest.mark.parametrize("pattern", [None, "random"])
@pytest.mark.parametrize("shape", tc.SPLIT_SHAPES, ids=_shape_id)
def test_splits_runs_and_launch_company_do_not_change_a_bit(hip, shape, pattern):
    U, M, F = shape
    rng = np.random.default_rng(5)
    users, news = rng.standard_normal((U, F)).astype(np.float32), rng.standard_normal((M, F)).astype(np.float32)
    ex = rng.integers(-1, M, (U, 4)).astype(np.int32)
    window = None if pattern is None else tc.windows(pattern, U, M, seed=6)
    target = tc.targets(U, M, 0, window, None, M, ex)
    target[target >= M] = -1
    c = tc.clamp(window, M) if window is not None else np.tile([[0, M]], (U, 1))
    even = np.arange(U) % 2 == 0
    target[even] = np.where(c[even, 0] < c[even, 1], (c[even, 0] + c[even, 1]) // 2, target[even])  # inside the window, if it has an inside
    users_d, news_d, ex_d, target_d, window_d = dev(users), dev(news), dev(ex, torch.int32), dev(target, torch.int32), _opt(window)
    base = launch_rank(hip, users_d, news_d, None, target_d, window_d, ex_d, mode=1, n_splits=1)
    assert tuple(base[3]) == (0, 0) and (base[0] > 0).sum() > U // 3 and (base[0] == 0).any()
    for s in (2, 3, 64, 0, 3):  # 64: more ranges than tiles, clamped; the second 3: another run
        got = launch_rank(hip, users_d, news_d, None, target_d, window_d, ex_d, mode=1, n_splits=s)
        assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, base)), s
    # a launch over a subset of the users: other neighbours in the workgroup, another union of windows
    pick = np.sort(rng.choice(U, U // 2, replace=False))
    got = run_rank(hip, users[pick], news, None, target[pick], None if window is None else window[pick], ex[pick], mode=1, n_splits=2)
    assert all(np.array_equal(bits(g), bits(w[pick])) for g, w in zip(got[:3], base[:3]))
    for u in (0, U - 1):  # and one user alone
        got = launch_rank(hip, users_d[u:u + 1], news_d, None, target_d[u:u + 1], None if window is None else window_d[u:u + 1], ex_d[u:u + 1], mode=1)
        assert all(np.array_equal(bits(g), bits(w[u:u + 1])) for g, w in zip(got[:3], base[:3])), u


# ------------------------------------------------------------------------------------------------ flags
def test_a_nan_counts_only_inside_a_window_and_a_nan_target_has_no_rank(hip):
    U, M, F = 9, 300, 8
    users, news, _c, _e = tc.integer_case(U, M, F, seed=3)
    news[200] = np.nan
    with np.errstate(invalid="ignore"):
        s64 = tc.scores64(users, news)
    target = np.array([200, 199, 201, 5, 160, 200, 0, 299, 200], np.int32)
    for window, want_flags in ((None, (0, 1)),
                               (np.tile([[150, 250]], (U, 1)), (0, 1)),
                               (np.tile([[0, 150]], (U, 1)), (0, 0)),      # the NaN column is in a visited tile, outside every window
                               (np.array([[0, 150]] * (U - 1) + [[200, 201]]), (0, 1))):
        window = None if window is None else window.astype(np.int32)
        want_rank, want_count, flags64 = tc.rank_reference(s64, target, window)
        rank, count, score, flags = run_rank(hip, users, news, None, target, window, None)
        assert flags64 == want_flags and tuple(flags) == want_flags
        assert np.array_equal(rank, want_rank) and np.array_equal(count, want_count)
        assert (rank[target == 200] == 0).all() and np.isneginf(score[target == 200]).all()
    assert count[-1] == 0  # the user whose window holds the NaN row alone


def test_rows_outside_the_table_and_targets_past_the_end_are_flagged(hip):
    U, M, F = 9, 300, 8
    users, news, _c, _e = tc.integer_case(U, M, F, seed=2)
    cand_rows = np.arange(M, dtype=np.int32)[::-1].copy()
    cand_rows[[200, 210]] = [M, -1]  # n_rows and -1
    s64 = tc.scores64(users, news, cand_rows)
    target = np.array([200, 199, 210, 5, 160, 211, 0, 299, 205], np.int32)
    for window, want_flags in ((None, (1, 0)),
                               (np.tile([[150, 250]], (U, 1)), (1, 0)),
                               (np.array([[0, 10]] * (U - 1) + [[205, 211]]), (1, 0)),
                               (np.tile([[0, 150]], (U, 1)), (0, 0)),      # in a visited tile, outside [min lo, max hi)
                               # in nobody's window but inside [min lo, max hi): the header allows either value
                               (np.array([[0, 150]] * (U - 1) + [[211, 300]]), None)):
        window = None if window is None else window.astype(np.int32)
        want_rank, want_count, flags64 = tc.rank_reference(s64, target, window, cand_rows, M)
        rank, count, score, flags = run_rank(hip, users, news, cand_rows, target, window, None)
        if want_flags is not None:
            assert flags64 == want_flags and tuple(flags) == want_flags
        else:
            assert flags64 == (0, 0) and tc.row_flag_is_open(window, cand_rows, M, M) and flags[0] in (0, 1) and flags[1] == 0
        assert np.array_equal(rank, want_rank) and np.array_equal(count, want_count)
        assert (rank[np.isin(target, [200, 210])] == 0).all()
    # a target position >= M: no rank, flags[0]; every window closed around clean rows, so nothing else can raise it
    window = np.tile([[0, 150]], (U, 1)).astype(np.int32)
    for past in (M, M + 1, 2 ** 31 - 1):
        t2 = target.copy()
        t2[4] = past
        rank, count, score, flags = run_rank(hip, users, news, cand_rows, t2, window, None)
        assert tuple(flags) == (1, 0) and rank[4] == 0 and np.isneginf(score[4]) and count[4] == 150
    t2[4] = -(2 ** 31)
    assert tuple(run_rank(hip, users, news, cand_rows, t2, window, None)[3]) == (0, 0)


def test_infinities_rank_like_numbers(hip):
    users, news, _c, _e = tc.integer_case(9, 40, 8, seed=3)
    users = np.abs(users) + 1  # positive users: an infinite news component gives an infinite score, never inf - inf
    news[7, 0] = np.inf
    news[8, 0] = np.inf
    news[9, 0] = -np.inf
    target = np.array([7, 8, 9, 0, 7, 8, 9, 1, 2], np.int32)
    want_rank, want_count, want_flags = tc.rank_reference(tc.scores64(users, news), target)
    rank, count, score, flags = run_rank(hip, users, news, None, target, None, None)
    assert np.array_equal(rank, want_rank) and np.array_equal(count, want_count) and tuple(flags) == want_flags == (0, 0)
    assert rank[0] == 1 and rank[1] == 2 and rank[2] == 40 and np.isposinf(score[0]) and np.isneginf(score[2])
    sig = run_rank(hip, users, news, None, target, None, None, mode=1)[2]
    assert sig[0] == 1.0 and sig[2] == 0.0


# ------------------------------------------------------------------------------------------------ edges and errors
def test_no_users_and_no_candidates(hip):
    users_d = dev(np.ones((3, 8), np.float32))
    target_d = dev(np.array([-1, 0, -1]), torch.int32)
    rank_d = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    count_d = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    score_d = torch.full((4,), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    call = lambda U, M, target: hip.lib().ebn_target_rank_f32(P(users_d), P(users_d), M, None, M, P(target), None, None, 0, 1, 0, P(rank_d),
                                                              P(count_d), P(score_d), P(flags_d), None, 0, U, 8, S())
    assert call(0, 3, target_d) == OK  # U == 0: nothing to do
    torch.cuda.synchronize()
    assert (rank_d == -7).all() and (count_d == -9).all() and (score_d == 123.0).all() and (flags_d == 0).all()
    assert call(3, 0, dev(np.array([-1, -1, -3]), torch.int32)) == OK  # M == 0: rank 0, count 0, score -inf
    torch.cuda.synchronize()
    assert (rank_d[:3] == 0).all() and (count_d[:3] == 0).all() and torch.isneginf(score_d[:3]).all() and (flags_d == 0).all()
    assert rank_d[3] == -7 and count_d[3] == -9 and score_d[3] == 123.0
    assert call(3, 0, target_d) == OK  # a target position 0 >= M = 0
    torch.cuda.synchronize()
    assert (rank_d[:3] == 0).all() and flags_d.tolist() == [1, 0]


def test_failing_calls_return_their_code_and_write_nothing(hip):
    import ctypes

    U, M, F = 5, 300, 8
    users, news, _c, _e = tc.integer_case(U, M, F, seed=4)
    a = dict(users=dev(users), news=dev(news), n_rows=M, cand=None, M=M, target=dev(np.arange(U), torch.int32), window=None, ex=None, X=0,
             mode=0, n_splits=1, rank=torch.full((U,), -7, dtype=torch.int32, device="cuda"),
             count=torch.full((U,), -9, dtype=torch.int32, device="cuda"), score=torch.full((U,), 123.0, device="cuda"),
             flags=torch.zeros(2, dtype=torch.int32, device="cuda"), ws=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"),
             ws_bytes=1 << 16, U=U, F=F)
    ptr = lambda v: P(v) if isinstance(v, torch.Tensor) else v
    call = lambda **kw: hip.lib().ebn_target_rank_f32(*[ptr(v) for v in {**a, **kw}.values()], S())
    need = int(hip.lib().ebn_target_rank_workspace_bytes(U, 2))
    assert call(target=None) == BAD_ARG and call(M=M - 1) == BAD_ARG and call(mode=3) == BAD_ARG
    assert call(ex=dev(np.full((U, 257), -1), torch.int32), X=257) == UNSUPPORTED
    assert call(users=ctypes.c_void_p(a["users"].data_ptr() + 4)) == ALIGN
    assert call(n_splits=2, ws_bytes=need - 1) == BAD_ARG and call(n_splits=2, ws=None) == BAD_ARG
    torch.cuda.synchronize()
    assert (a["rank"] == -7).all() and (a["count"] == -9).all() and (a["score"] == 123.0).all() and (a["flags"] == 0).all()
    assert call(n_splits=2, ws_bytes=need) == OK  # the same call with enough workspace runs
    torch.cuda.synchronize()
    assert (a["rank"] > 0).all() and (a["count"] == M).all()


# ------------------------------------------------------------------------------------------------ untouched memory
@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("n_splits", [1, 2])
@pytest.mark.parametrize("shape", [(65, 257, 36), (3, 7, 4)], ids=_shape_id)
def test_guarded_operands(hip, shape, n_splits, windowed):
    """Operands behind and in front of harmful values -- users / news_all NaN (flags[1] stays 0), cand_rows n_rows (flags[0] stays
    0), target_pos a position past the end (flags[0]), window the whole list, exclude the rows of the first and the last user's
    target (an over-read takes their rank away) -- outputs in canaries, workspace poisoned."""
    U, M, F = shape
    users, news, cand_rows, ex = tc.integer_case(U, M, F, seed=U + M, cand="subset", exclude="x3")
    n_rows = news.shape[0]
    window = tc.windows("random", U, M, seed=1) if windowed else None
    target = np.random.default_rng(3).integers(0, M, U).astype(np.int32)
    for u in (0, U - 1):  # an admissible target for the two users whose neighbours are the guards
        c = tc.clamp(window, M)[u] if windowed else (0, M)
        ok = [p for p in range(c[0], c[1]) if cand_rows[p] not in ex[u]]
        target[u] = ok[0] if ok else target[u]
    s64 = tc.scores64(users, news, cand_rows)
    want_rank, want_count, want_flags = tc.rank_reference(s64, target, window, cand_rows, n_rows, ex)
    assert want_flags == (0, 0)
    (ud, hu), (nd, hn) = guard_in(users), guard_in(news)
    (cd, hcr), (ed, he), (td, ht) = guard_in(cand_rows, fill=n_rows), guard_in(ex, fill=-1), guard_in(target, fill=M)
    he.set_guards(int(cand_rows[target[0]]), int(cand_rows[target[U - 1]]))
    handles = dict(users=hu, news_all=hn, cand_rows=hcr, exclude=he, target_pos=ht)
    wd = None
    if windowed:
        wd, hw = guard_in(window, fill=0)
        hw.set_guards(0, M)
        handles["window"] = hw
    (rd, hr), (kd, hk), (sd, hs), (fd, hf) = (guard_out((U,), dtype=torch.int32), guard_out((U,), dtype=torch.int32), guard_out((U,)),
                                              guard_out((2,), dtype=torch.int32))
    hf.fill_payload([0, 0])
    ws_bytes = int(hip.lib().ebn_target_rank_workspace_bytes(U, n_splits))
    ws = poison(torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"))
    code = hip.lib().ebn_target_rank_f32(P(ud), P(nd), n_rows, P(cd), M, P(td), P(wd), P(ed), ex.shape[1], 0, n_splits, P(rd), P(kd), P(sd),
                                         P(fd), P(ws), ws_bytes, U, F, S())
    assert code == OK
    torch.cuda.synchronize()
    assert tuple(hf.payload().reshape(-1).tolist()) == (0, 0)
    assert np.array_equal(hr.payload().cpu().numpy().reshape(-1), want_rank)
    assert np.array_equal(hk.payload().cpu().numpy().reshape(-1), want_count)
    for name, h in {**handles, "out_rank": hr, "out_count": hk, "out_score": hs, "flags": hf}.items():
        h.check(name)


# ------------------------------------------------------------------------------------------------ whole models
from tests.test_data_pipeline import DATA, frames  # noqa: E402,F401  (the fixture parquets under tests/golden/ebnerd)

N_IMPRESSIONS, N_CANDIDATES = 40, 30
TWO_DAYS, SIX_HOURS = pd.Timedelta(days=2), pd.Timedelta(hours=6)


@pytest.mark.parametrize("which", ["nrms", "lstur-ini"])
def test_model_rank_targets_agrees_with_model_recommend(hip, frames, which):  # noqa: F811
    """rank_targets() against recommend(top_n=K, return_scores=True), K = every candidate (44 <= 64, so the lists hold all that is
    admissible): every pair with rank r > 0 has its target at index r - 1 of the impression's list with the same score bits, every
    other pair's target is absent from the list, and the ranks are cut to k = 8 the same way -- with and without
    window=Freshness(...), with exclude_history False and True.  Impressions with two clicks give two pairs; a target in the
    impression's own history, outside the candidate list or unknown to the loader comes back with rank 0."""
    from ebrec.evaluation import Freshness, rank_metrics
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_LABELS_COL

    model, mk = {"nrms": _nrms_case, "lstur-ini": _lstur_case("ini")}[which](frames)
    beh = _timed_behaviours(frames).copy()
    assert len(beh) == N_IMPRESSIONS
    labels = [list(l) for l in beh[DEFAULT_LABELS_COL]]
    for u in (3, 17):  # two clicks
        labels[u] = [1, 1] + [0] * (len(labels[u]) - 2)
    beh[DEFAULT_LABELS_COL] = labels
    loader = mk(beh)
    index = model._recommend_index(loader)
    rng = np.random.default_rng(7)
    clicked = [[a for a, l in zip(ids, lab) if l == 1] for ids, lab in zip(beh[DEFAULT_INVIEW_ARTICLES_COL], labels)]
    known = sorted({a for c in clicked for a in c} & set(index))
    assert len(known) >= 10
    base = _candidates(model, loader, beh, rng, N_CANDIDATES)
    cand = np.concatenate([base, [a for a in known if a not in set(base.tolist())][:12]])
    cand = np.concatenate([cand, cand[:2]])  # two ids twice: the first occurrence is the target
    K = len(cand)
    assert K <= 64
    pub = {int(a): pd.Timestamp("2023-02-25") + int(s) * SIX_HOURS for a, s in zip(cand.tolist(), rng.integers(0, 20, len(cand)))}
    fresh = Freshness(pub, max_age=TWO_DAYS)
    history = [list(h) for h in beh[DEFAULT_HISTORY_ARTICLE_ID_COL]]
    in_history = [next((a for a in history[u] if a in set(cand.tolist())), None) for u in range(N_IMPRESSIONS)]
    assert sum(a is not None for a in in_history) >= 3, "the case must exercise the exclusion"
    outsider = next(a for a in sorted(index) if a not in set(cand.tolist()))
    explicit = [[a for a in (in_history[u],) if a is not None] + [outsider, -12345, int(cand[u % len(cand)])] for u in range(N_IMPRESSIONS)]
    n_ranked, history_ranks = 0, {True: [], False: []}
    for window in (None, fresh):
        for exclude_history in (True, False):
            kw = dict(exclude_history=exclude_history, window=window)
            ids, sc = model.recommend(loader, cand, top_n=K, return_scores=True, **kw)
            for targets in (None, explicit):
                got = model.rank_targets(loader, targets, cand, **kw)
                pairs = [(u, a) for u in range(N_IMPRESSIONS) for a in (clicked[u] if targets is None else explicit[u])]
                assert list(zip(got.impression.tolist(), got.target_id.tolist())) == pairs
                assert got.rank.dtype == got.count.dtype == np.int32 and got.score.dtype == np.float32 and len(got) == len(pairs)
                if targets is None:
                    assert got.impression.tolist().count(3) == 2 and got.impression.tolist().count(17) == 2
                for (u, a), r, n, s in zip(pairs, got.rank.tolist(), got.count.tolist(), got.score):
                    row = ids[u].tolist()
                    if r > 0:
                        assert row[r - 1] == a and bits(np.float32(s))[0] == bits(sc[u, r - 1:r])[0], (u, a, r)
                        n_ranked += 1
                    else:
                        assert a not in row, (u, a, r)
                    assert (r == 0) == bool(np.isneginf(s)) and r <= n <= K and n == sum(i != -1 for i in row)
                    if a in (outsider, -12345):
                        assert r == 0, (u, a)
                    if targets is not None and a == in_history[u]:
                        history_ranks[exclude_history].append(r)
                    if window is None and not exclude_history and a in set(cand.tolist()):
                        assert r > 0 and n == len(cand), (u, a)
                # more than one launch, each sorting its own pairs: the same answer in loader order
                again = model.rank_targets(loader, targets, cand, users_per_call=16, **kw)
                assert all(np.array_equal(bits(getattr(again, f)), bits(getattr(got, f))) for f in ("rank", "count", "score"))
            raw = model.rank_targets(loader, None, cand, scores="raw", **kw)
            assert np.array_equal(raw.rank, model.rank_targets(loader, None, cand, **kw).rank)
    assert n_ranked >= 40, "the case must exercise the lists"
    # a target in the impression's own history: no rank under the exclusion, a rank without it (when its window holds it)
    assert len(history_ranks[True]) >= 6 and not any(history_ranks[True]) and any(history_ranks[False])
    m = rank_metrics(got.rank, ks=(5, 10), counts=got.count)
    assert 0.0 <= m["hit_rate@5"] <= m["hit_rate@10"] <= 1.0 and 0.0 < m["mrr"] <= 1.0 and 0.0 < m["unranked"] < 1.0
