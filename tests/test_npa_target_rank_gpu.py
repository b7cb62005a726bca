"""ebn_npa_target_rank_f32 (csrc/ebn_npa_target_rank.hip) and NPAModel.rank_targets_pairwise on the GPU: against the lists of
ebn_npa_topk_score_f32 (the same score bits, the same total order), against the float64 rule of tests/npa_target_rank_cases.py and
against NPAModel.recommend_pairwise."""
import ctypes

import numpy as np
import pytest
import torch

from tests import npa_target_rank_cases as nt
from tests.guarded import guard_in, guard_out, poison
from tests.hip_testutil import P, S, dev
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)
from tests.test_npa_recommend_gpu import _count_calls, _history_ids, run_npa_topk

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3
TAIL = 5  # output elements behind U that must stay as they were


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _opt(a):
    return None if a is None else dev(a, torch.int32)


def launch_rank(hip, operands, n_rows, cand_d, target_d, window_d, ex_d, mode=0, n_splits=0):
    """one call on device tensors (operands: users, Q, Ua [n_rows * L, A] or [n_rows, L, A], Vd) -> (rank [U] int32, count [U] int32,
    score [U] float32, flags [2]) as numpy arrays; the outputs are TAIL elements longer, which must come back untouched, and the
    workspace is poisoned"""
    users_d, Q_d, Ua_d, Vd_d = operands
    U, F = users_d.shape
    A = Q_d.shape[1]
    L = Ua_d.numel() // (n_rows * A)
    M = n_rows if cand_d is None else len(cand_d)
    X = 0 if ex_d is None else ex_d.shape[1]
    rank_d = torch.full((U + TAIL,), -7, dtype=torch.int32, device="cuda")
    count_d = torch.full((U + TAIL,), -9, dtype=torch.int32, device="cuda")
    score_d = torch.full((U + TAIL,), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    splits = n_splits if n_splits > 0 else int(hip.lib().ebn_npa_topk_auto_splits(U, M, L))
    ws_bytes = int(hip.lib().ebn_npa_target_rank_workspace_bytes(U, splits))
    assert ws_bytes > 0
    ws_d = poison(torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"))
    code = hip.lib().ebn_npa_target_rank_f32(P(users_d), P(Q_d), P(Ua_d), P(Vd_d), n_rows, P(cand_d), M, P(target_d), P(window_d), P(ex_d), X,
                                             mode, n_splits, P(rank_d), P(count_d), P(score_d), P(flags_d), P(ws_d), ws_bytes, U, L, F, A, S())
    assert code == OK, code
    torch.cuda.synchronize()
    assert (rank_d[U:] == -7).all() and (count_d[U:] == -9).all() and (score_d[U:] == 123.0).all()
    return rank_d[:U].cpu().numpy(), count_d[:U].cpu().numpy(), score_d[:U].cpu().numpy(), flags_d.cpu().numpy()


def run_rank(hip, c, target, window=None, cand_rows="case", exclude="case", mode=0, n_splits=0, users=None):
    """a case of npa_target_rank_cases.case(); users: indices of the users that take part (target / window / exclude are theirs)"""
    cand_rows = c["cand_rows"] if isinstance(cand_rows, str) else cand_rows
    exclude = c["exclude"] if isinstance(exclude, str) else exclude
    us, Q = (c["users"], c["Q"]) if users is None else (c["users"][users], c["Q"][users])
    return launch_rank(hip, (dev(us), dev(Q), dev(c["Ua"]), dev(c["Vd"])), c["n_rows"], _opt(cand_rows), dev(target, torch.int32), _opt(window),
                       _opt(exclude), mode, n_splits)


def _valid(target, adm):
    """[U] bool: the target is a position and admissible"""
    U, M = adm.shape
    inside = (target >= 0) & (target < M)
    return inside & adm[np.arange(U), np.clip(target, 0, M - 1)]


def _check_band(rank, b, what=""):
    for u in range(len(rank)):
        assert b[u, 0] <= rank[u] <= b[u, 1], (what, u, b[u].tolist(), int(rank[u]))


# ------------------------------------------------------------------------------------------------ 1. exact, against the top-k kernel
@pytest.mark.parametrize("exclude", [None, "x3"])
@pytest.mark.parametrize("cand", ["null", "subset"])
@pytest.mark.parametrize("shape", nt.SHAPES, ids=nt.shape_id)
def test_ranks_and_score_bits_are_those_of_the_top_k_lists(hip, shape, cand, exclude):
    """k = min(64, M): count is the numpy count of admissible positions; a target in the list of ebn_npa_topk_score_f32 at index i
    has rank i + 1 and that slot's score bits; a target not in the list has rank 0 (absent or inadmissible) or a rank above k (only
    possible when M > 64).  M <= 64: the list is the whole order.  Mode 1 keeps the ranks and has the sigmoid slot's bits.  Every
    second user's target is taken out of its own list, the others are the generator's eight kinds."""
    U, M = shape[:2]
    k = min(64, M)
    c = nt.case(shape, seed=sum(shape), cand=cand, exclude=exclude)
    topk = {mode: run_npa_topk(hip, {**c, "k": k}, mode=mode) for mode in (0, 1)}
    pos = topk[0][0]
    assert tuple(topk[0][2]) == (0, 0) and np.array_equal(topk[1][0], pos)
    target = nt.targets(U, M, M, None, c["cand_rows"], c["n_rows"], c["exclude"])
    for u in range(0, U, 2):
        kept = pos[u][pos[u] >= 0]
        if len(kept):
            target[u] = kept[(7 * u) % len(kept)]
    adm = nt.admissible(c)
    valid = _valid(target, adm)
    n_in_list = 0
    for mode in (0, 1):
        rank, count, score, flags = run_rank(hip, c, target, mode=mode)
        assert tuple(flags) == (int((target >= M).any()), 0)
        assert np.array_equal(count, adm.sum(1))
        for u in range(U):
            r, tp = int(rank[u]), int(target[u])
            at = np.flatnonzero(pos[u] == tp) if tp >= 0 else []
            if len(at):
                assert r == at[0] + 1 and bits(score[u:u + 1])[0] == bits(topk[mode][1][u, at[0]:at[0] + 1])[0], (mode, u, r)
                n_in_list += 1
            elif valid[u]:
                assert M > 64 and r > k, (mode, u, r)
            else:
                assert r == 0, (mode, u, r)
            assert (r == 0) == bool(np.isneginf(score[u])), (mode, u)
    assert n_in_list >= 2 * int((pos[::2] >= 0).any(1).sum())  # both modes: every second user with a list at all is in it


# ------------------------------------------------------------------------------------------------ 2. exact, deep ranks
def test_deep_ranks_equal_the_order_of_three_chained_top_k_calls(hip):
    """(65, 130, 30, 36, 24), null cand: the complete order of every user from three top-k calls with k = 64, the second excluding the
    first's 64 rows (X = 64), the third those 128 (X = 128: 2 are left).  Every target's rank is its index + 1 in that order, with
    the slot's bits.  With the first call's rows as the exclusion list (X = 64, read through the cache, not staged) the ranks are
    those of the remaining order.  A 3-row list: excluded targets get rank 0."""
    shape = nt.SHAPES[2]
    U, M = shape[:2]
    c = nt.case(shape, seed=31)
    c64 = {**c, "k": 64}
    p1, s1, f1 = run_npa_topk(hip, c64, exclude=None)
    p2, s2, f2 = run_npa_topk(hip, c64, exclude=p1.astype(np.int32))
    p3, s3, f3 = run_npa_topk(hip, c64, exclude=np.concatenate([p1, p2], 1).astype(np.int32))
    assert tuple(f1) == tuple(f2) == tuple(f3) == (0, 0)
    order, obits = np.concatenate([p1, p2, p3[:, :M - 128]], 1), np.concatenate([bits(s1), bits(s2), bits(s3)[:, :M - 128]], 1)
    assert (p3[:, M - 128:] == -1).all() and all(sorted(order[u].tolist()) == list(range(M)) for u in range(U))
    target = np.random.default_rng(1).integers(0, M, U).astype(np.int32)
    where = np.array([int(np.flatnonzero(order[u] == target[u])[0]) for u in range(U)])
    rank, count, score, flags = run_rank(hip, c, target, exclude=None)
    assert tuple(flags) == (0, 0) and (count == M).all()
    assert np.array_equal(rank, where + 1) and np.array_equal(bits(score), obits[np.arange(U), where])
    assert (rank > 64).sum() > U // 4  # deep ranks are exercised
    rank, count, score, flags = run_rank(hip, c, target, exclude=p1.astype(np.int32))
    assert tuple(flags) == (0, 0) and (count == M - 64).all()
    assert np.array_equal(rank, np.where(where < 64, 0, where + 1 - 64))
    assert np.array_equal(bits(score[where >= 64]), obits[np.arange(U), where][where >= 64]) and np.isneginf(score[where < 64]).all()
    ex = np.random.default_rng(2).integers(0, M, (U, 3)).astype(np.int32)
    ex[::2, 1] = target[::2]
    rank, count, score, flags = run_rank(hip, c, target, exclude=ex)
    assert (rank[::2] == 0).all() and np.isneginf(score[::2]).all() and tuple(flags) == (0, 0)
    want = nt.admissible(c, exclude=ex)
    assert np.array_equal(count, want.sum(1)) and np.array_equal(rank > 0, _valid(target, want))
    for u in np.flatnonzero(rank > 0):  # the order with the excluded rows taken out
        left = [p for p in order[u].tolist() if want[u, p]]
        assert left[rank[u] - 1] == target[u], u


# ------------------------------------------------------------------------------------------------ 3. float64 band
@pytest.mark.parametrize("shape", nt.SPLIT_SHAPES, ids=nt.shape_id)
def test_ranks_lie_in_the_float64_band(hip, shape):
    """tol = npa_recommend_cases.tolerance(s64), each fp32 score within tol of its float64 value:
    1 + #{admissible c: s64 > t64 + 2 tol} <= rank <= 1 + #{admissible c != target: s64 >= t64 - 2 tol}; count is exact.  The band
    is a single value for at least half of the ranked pairs (from the float64 scores alone: 0.715 of them at 130x300x30x400x200,
    0.908 at 65x130x30x36x24), so it does not hide failures.  Null cand: a list drawn with replacement has exact ties between the
    duplicates of a row, which the band cannot resolve (about a third of its bands are single values); those ties are pinned
    exactly by the tests against the top-k lists."""
    cand = "null"
    U, M = shape[:2]
    c = nt.case(shape, seed=nt.BAND_SEED[shape], cand=cand)
    target = np.random.default_rng(1).integers(0, M, U).astype(np.int32)
    s64 = nt.scores64(c)
    tol = nt.tolerance(s64)
    adm = nt.admissible(c)
    b = nt.band(s64, adm, target, tol)
    rank, count, score, flags = run_rank(hip, c, target)
    single = float((b[:, 0] == b[:, 1]).mean())
    print(f"shape {shape} cand {cand}: tol {tol:.3e}, single-valued bands {single:.3f}, widest {int((b[:, 1] - b[:, 0]).max())}")
    assert tuple(flags) == (0, 0) and np.array_equal(count, adm.sum(1)) and (rank > 0).all()
    _check_band(rank, b)
    assert (np.abs(score - s64[np.arange(U), target]) <= tol).all()
    assert single >= 0.5


# ------------------------------------------------------------------------------------------------ 4. windows
@pytest.mark.parametrize("pattern", nt.PATTERNS)
def test_windows(hip, pattern):
    """(65, 130, 30, 36, 24), subset cand with two rows outside the table, exclude x3, the eight target kinds: count, the set of ranked
    users and the flags are rank_reference's (the either-value clause honoured), ranks lie in the float64 band; for 8 users the
    result equals the unwindowed kernel on cand_rows[lo:hi] with target_pos - lo, bit for bit (a pair's bits do not depend on its
    position); windows that hold everything equal window == NULL in all three outputs."""
    shape = nt.WINDOW_SHAPE
    U, M = shape[:2]
    c = nt.case(shape, seed=41, cand="subset", exclude="x3")
    n_rows = c["n_rows"]
    cand_rows = nt.with_bad_rows(c["cand_rows"], n_rows)
    window = nt.windows(pattern, U, M, seed=U)
    target = nt.targets(U, M, 5, window, cand_rows, n_rows, c["exclude"])
    s64 = nt.scores64(c, cand_rows)
    want_rank, want_count, want_flags = nt.rank_reference(s64, target, window, cand_rows, n_rows, c["exclude"])
    rank, count, score, flags = run_rank(hip, c, target, window, cand_rows=cand_rows)
    assert np.array_equal(count, want_count) and np.array_equal(rank > 0, want_rank > 0)
    if want_flags[0] == 0 and nt.row_flag_is_open(window, cand_rows, n_rows, M):
        assert flags[0] in (0, 1) and flags[1] == 0
    else:
        assert tuple(flags) == want_flags
    adm = nt.admissible(c, window, cand_rows=cand_rows)
    assert np.array_equal(adm.sum(1), want_count)
    _check_band(rank, nt.band(s64, adm, target, nt.tolerance(s64)), pattern)
    assert np.isneginf(score[rank == 0]).all()
    if pattern == "empty":
        assert (count == 0).all() and (rank == 0).all()
    w = nt.clamp(window, M)
    chosen = [u for u in list(np.flatnonzero(rank > 0)[:5]) + list(np.flatnonzero((rank == 0) & (w[:, 0] < w[:, 1]))[:3])]
    for u in chosen:
        lo, hi = int(w[u, 0]), int(w[u, 1])
        tp = int(target[u]) - lo if lo <= target[u] < hi else -1
        one = run_rank(hip, c, np.array([tp], np.int32), None, cand_rows=cand_rows[lo:hi], exclude=c["exclude"][u:u + 1], users=[u])
        assert one[0][0] == rank[u] and one[1][0] == count[u] and bits(one[2])[0] == bits(score[u:u + 1])[0], (pattern, u)
    if pattern in ("all", "outside"):
        plain = run_rank(hip, c, target, None, cand_rows=cand_rows)
        assert all(np.array_equal(bits(g), bits(p)) for g, p in zip((rank, count, score), plain[:3]))
    else:
        assert len(chosen) >= (0 if pattern == "empty" else 3)


# ------------------------------------------------------------------------------------------------ 5. splits and runs
@pytest.mark.parametrize("pattern", [None, "random"])
@pytest.mark.parametrize("shape", nt.SPLIT_SHAPES, ids=nt.shape_id)
def test_every_split_and_every_run_gives_the_same_bits(hip, shape, pattern):
    U, M = shape[:2]
    c = nt.case(shape, seed=5, cand="subset", exclude="x3")
    window = None if pattern is None else nt.windows(pattern, U, M, seed=6)
    target = nt.targets(U, M, 0, window, c["cand_rows"], c["n_rows"], c["exclude"])
    target[target >= M] = -1
    w = nt.clamp(window, M) if window is not None else np.tile([[0, M]], (U, 1))
    even = np.arange(U) % 2 == 0
    target[even] = np.where(w[even, 0] < w[even, 1], (w[even, 0] + w[even, 1]) // 2, target[even])
    base = run_rank(hip, c, target, window, mode=1, n_splits=1)
    assert tuple(base[3]) == (0, 0) and (base[0] > 0).sum() > U // 3 and (base[0] == 0).any()
    for s in (2, 3, 64, 0, 3):  # 64: clamped to the steps; the second 3: another run
        got = run_rank(hip, c, target, window, mode=1, n_splits=s)
        assert all(np.array_equal(bits(g), bits(b)) for g, b in zip(got, base)), s
    # other neighbours in the workgroup, another union of windows
    pick = np.sort(np.random.default_rng(8).choice(U, U // 2, replace=False))
    got = run_rank(hip, c, target[pick], None if window is None else window[pick], exclude=c["exclude"][pick], mode=1, n_splits=2, users=pick)
    assert all(np.array_equal(bits(g), bits(b[pick])) for g, b in zip(got[:3], base[:3]))


# ------------------------------------------------------------------------------------------------ 6. guard bands
@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("cand", ["null", "subset"])
def test_operands_between_guards(hip, cand, windowed):
    """Ua_all, Vd_all, users and Q inside NaN guards (L = 30: two padded token rows per candidate; U = 65: 63 user columns past the
    last), target_pos between positions past the end (flags[0]), window between whole-list ranges, exclude between the rows of the
    first and the last user's target (an over-read takes their rank away), outputs in canaries: bit-equal to the unguarded run,
    flags (0, 0), every guard intact."""
    shape = nt.SHAPES[2]
    U, M, L, F, A = shape
    c = nt.case(shape, seed=13, cand=cand, exclude="x3")
    n_rows = c["n_rows"]
    rows = np.arange(M) if c["cand_rows"] is None else c["cand_rows"]
    window = nt.windows("random", U, M, seed=1) if windowed else None
    target = np.random.default_rng(3).integers(0, M, U).astype(np.int32)
    for u in (0, U - 1):  # an admissible target for the two users whose neighbours are the guards
        lo, hi = nt.clamp(window, M)[u] if windowed else (0, M)
        ok = [p for p in range(lo, hi) if rows[p] not in c["exclude"][u]]
        target[u] = ok[0] if ok else target[u]
    want = run_rank(hip, c, target, window)
    assert tuple(want[3]) == (0, 0) and (want[0] > 0).sum() > U // 4
    Ua_d, hU = guard_in(c["Ua"].reshape(n_rows * L, A))
    Vd_d, hV = guard_in(c["Vd"].reshape(n_rows * L, F))
    (us_d, hu), (Q_d, hQ) = guard_in(c["users"]), guard_in(c["Q"])
    (ed, he), (td, ht) = guard_in(c["exclude"], fill=-1), guard_in(target, fill=M)
    he.set_guards(int(rows[target[0]]), int(rows[target[U - 1]]))
    handles = dict(Ua_all=hU, Vd_all=hV, users=hu, Q=hQ, exclude=he, target_pos=ht)
    cd = None
    if c["cand_rows"] is not None:
        cd, handles["cand_rows"] = guard_in(c["cand_rows"], fill=n_rows)
    wd = None
    if windowed:
        wd, hw = guard_in(window, fill=0)
        hw.set_guards(0, M)
        handles["window"] = hw
    (rd, hr), (kd, hk), (sd, hs), (fd, hf) = (guard_out((U,), dtype=torch.int32), guard_out((U,), dtype=torch.int32), guard_out((U,)),
                                              guard_out((2,), dtype=torch.int32))
    hf.fill_payload([0, 0])
    for n_splits in (1, 2):
        ws_bytes = int(hip.lib().ebn_npa_target_rank_workspace_bytes(U, n_splits))
        ws = poison(torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"))
        code = hip.lib().ebn_npa_target_rank_f32(P(us_d), P(Q_d), P(Ua_d), P(Vd_d), n_rows, P(cd), M, P(td), P(wd), P(ed), 3, 0, n_splits, P(rd),
                                                 P(kd), P(sd), P(fd), P(ws), ws_bytes, U, L, F, A, S())
        assert code == OK
        torch.cuda.synchronize()
        assert tuple(hf.payload().reshape(-1).tolist()) == (0, 0)
        got = (hr.payload().cpu().numpy().reshape(-1), hk.payload().cpu().numpy().reshape(-1), hs.payload().cpu().numpy().reshape(-1))
        assert all(np.array_equal(bits(g), bits(w_)) for g, w_ in zip(got, want[:3])), n_splits
        for name, h in {**handles, "out_rank": hr, "out_count": hk, "out_score": hs, "flags": hf}.items():
            h.check(name)


# ------------------------------------------------------------------------------------------------ 7. edges
def test_rows_outside_the_catalogue_are_skipped_flagged_and_not_counted(hip):
    c = nt.case(nt.SHAPES[2], seed=17, cand="subset")
    U, M = nt.SHAPES[2][:2]
    n_rows = c["n_rows"]
    bad = c["cand_rows"].copy()
    where = [3, 64, 129]
    bad[where] = [-1, n_rows, n_rows + 1]
    target = np.random.default_rng(4).integers(0, M, U).astype(np.int32)
    target[np.isin(target, where)] = 5
    target[:3] = where  # the first three users alone have a target on a row outside the table
    clean = run_rank(hip, c, target)
    rank, count, score, flags = run_rank(hip, c, target, cand_rows=bad)
    assert tuple(clean[3]) == (0, 0) and (clean[1] == M).all() and tuple(flags) == (1, 0)
    assert (count == M - 3).all() and (rank[:3] == 0).all() and np.isneginf(score[:3]).all() and (rank[3:] > 0).all()
    s64 = nt.scores64(c, bad)
    _check_band(rank, nt.band(s64, nt.admissible(c, cand_rows=bad), target, nt.tolerance(s64)))
    assert np.array_equal(bits(score[3:]), bits(clean[2][3:]))  # the others' own scores: the same pairs, the same bits
    # a window around clean rows: nothing is flagged
    window = np.tile([[4, 60]], (U, 1)).astype(np.int32)
    assert tuple(run_rank(hip, c, target, window, cand_rows=bad)[3]) == (0, 0)


def test_a_nan_in_one_catalogue_row_is_flagged_unranked_and_not_counted(hip):
    c = nt.case(nt.SHAPES[2], seed=19, cand="subset")
    U, M = nt.SHAPES[2][:2]
    row = int(c["cand_rows"][10])
    n_dup = int((c["cand_rows"] == row).sum())
    target = np.random.default_rng(5).integers(0, M, U).astype(np.int32)
    target[::4] = 10
    clean = run_rank(hip, c, target)
    for which, at in (("Vd", (row, 7, 5)), ("Ua", (row, 29, 23))):
        d = {**c, which: c[which].copy()}
        d[which][at] = np.nan
        rank, count, score, flags = run_rank(hip, d, target)
        assert tuple(flags) == (0, 1), which
        hit = c["cand_rows"][target] == row
        assert hit[::4].all() and (rank[hit] == 0).all() and np.isneginf(score[hit]).all() and (rank[~hit] > 0).all(), which
        assert (count == M - n_dup).all(), which
        # as if that row were excluded for everybody: the other pairs keep their bits, so the ranks are exactly those
        ex = run_rank(hip, c, target, exclude=np.full((U, 1), row, np.int32))
        assert np.array_equal(rank, ex[0]) and np.array_equal(count, ex[1]) and np.array_equal(bits(score), bits(ex[2])), which
        assert np.array_equal(bits(score[~hit]), bits(clean[2][~hit]))
        # outside every window the NaN is never looked at
        window = np.tile([[11, M]], (U, 1)).astype(np.int32)
        if not (c["cand_rows"][11:] == row).any():
            assert tuple(run_rank(hip, d, np.maximum(target, 11), window)[3]) == (0, 0), which


def test_an_all_excluded_user_has_count_0_and_rank_0(hip):
    c = nt.case(nt.SHAPES[1], seed=23, cand="subset")
    U, M = nt.SHAPES[1][:2]
    distinct = np.unique(c["cand_rows"])
    ex = np.full((U, len(distinct)), -1, np.int32)
    ex[1] = distinct
    rank, count, score, flags = run_rank(hip, c, np.array([0, 1, 2], np.int32), exclude=ex)
    assert tuple(flags) == (0, 0) and count.tolist() == [M, 0, M] and rank[1] == 0 and np.isneginf(score[1]) and rank[0] > 0 and rank[2] > 0


def test_no_users_and_no_candidates(hip):
    ones = dev(np.ones((3, 4, 8), np.float32))
    target_d = dev(np.array([-1, 0, -1]), torch.int32)
    rank_d = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    count_d = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    score_d = torch.full((4,), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    call = lambda U, M, target: hip.lib().ebn_npa_target_rank_f32(P(ones), P(ones), P(ones), P(ones), M, None, M, P(target), None, None, 0, 1, 0,
                                                                  P(rank_d), P(count_d), P(score_d), P(flags_d), None, 0, U, 4, 8, 8, S())
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


def test_a_failing_call_writes_nothing(hip):
    """the cases of test_npa_recommend_gpu.test_a_failing_call_writes_nothing (k has no counterpart here), plus this entry point's
    own: target_pos, mode, X, the alignment and the workspace one range needs"""
    c = nt.case(nt.SHAPES[1], seed=29)
    U, M, L, F, A = nt.SHAPES[1]
    us, Q, Ua, Vd = dev(c["users"]), dev(c["Q"]), dev(c["Ua"]), dev(c["Vd"])
    rank_d = torch.full((U,), -7, dtype=torch.int32, device="cuda")
    count_d = torch.full((U,), -9, dtype=torch.int32, device="cuda")
    score_d = torch.full((U,), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    target = dev(np.arange(U), torch.int32)
    base = dict(users=P(us), Q=P(Q), Ua=P(Ua), Vd=P(Vd), n_rows=M, cand=None, M=M, target=P(target), window=None, ex=None, X=0, mode=0,
                n_splits=1, rank=P(rank_d), count=P(count_d), score=P(score_d), flags=P(flags_d), ws=P(ws), ws_bytes=1 << 16, U=U, L=L, F=F, A=A,
                stream=S())
    call = lambda **kw: hip.lib().ebn_npa_target_rank_f32(*{**base, **kw}.values())
    need1, need2 = (int(hip.lib().ebn_npa_target_rank_workspace_bytes(U, s)) for s in (1, 2))
    assert call(L=65) == UNSUPPORTED and call(A=A + 2) == UNSUPPORTED and call(M=M - 1) == BAD_ARG
    assert call(target=None) == BAD_ARG and call(mode=3) == BAD_ARG
    assert call(ex=P(dev(np.full((U, 257), -1), torch.int32)), X=257) == UNSUPPORTED
    assert call(users=ctypes.c_void_p(us.data_ptr() + 4)) == ALIGN
    assert call(n_splits=2, ws_bytes=need2 - 1) == BAD_ARG and call(n_splits=2, ws=None) == BAD_ARG
    assert call(ws_bytes=need1 - 1) == BAD_ARG and call(ws=None) == BAD_ARG
    torch.cuda.synchronize()
    assert (rank_d == -7).all() and (count_d == -9).all() and (score_d == 123.0).all() and (flags_d == 0).all()
    assert call(n_splits=2, ws_bytes=need2) == OK and call(U=0) == OK  # the same call with enough workspace runs
    torch.cuda.synchronize()
    assert (rank_d > 0).all() and (count_d == M).all() and (flags_d == 0).all()


# ------------------------------------------------------------------------------------------------ 8. the model
N_CANDIDATES = 30


@pytest.mark.parametrize("kind", ["fixture", "synthetic"])
def test_rank_targets_pairwise_agrees_with_recommend_pairwise(hip, frames, kind, monkeypatch):  # noqa: F811
    """rank_targets_pairwise against recommend_pairwise(top_n=30, return_scores=True) over the 30-candidate list: the lists are the
    complete order, so for every pair the id at index rank - 1 is the target with the same score bits, a pair with rank 0 has its
    target nowhere in the list, and count is the number of non-fill entries -- with and without exclude_history, in one launch and
    in several.  Under window=Freshness(...) there is no list to compare with: count is exact and the rank lies in the band of the
    scores scorer.predict gives the same pairs (both sides are within 1e-4 |s| + 1e-6 of the float64 oracle, so a score of one side
    is within tol = 2 (1e-4 max|s| + 1e-6) of the other's, and the band is +- 2 tol)."""
    from ebrec.evaluation import Freshness, rank_metrics
    from ebrec.utils._constants import DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_LABELS_COL
    from tests.test_npa_cached_scoring_gpu import _npa_case

    model, loader0, _Pw, _hp, _V = _npa_case(kind, frames)
    n_imp = len(loader0.X)
    rng = np.random.default_rng(7)
    index = model._recommend_index(loader0)
    history = _history_ids(loader0, n_imp)
    read = sorted(set().union(*history) & set(index))
    assert len(read) >= 10 and len(index) > N_CANDIDATES
    cand = rng.choice(read, 10, replace=False)
    cand = rng.permutation(np.concatenate([cand, rng.choice(sorted(set(index) - set(cand.tolist())), N_CANDIDATES - 10, replace=False)]))
    col = {a: j for j, a in enumerate(cand.tolist())}
    # the same impressions with the candidate list as every in-view list (so scorer.predict scores every pair), one click each,
    # two for impressions 3 and 17, and an impression time
    clicks = [[(7 * u) % N_CANDIDATES] + ([(7 * u + 11) % N_CANDIDATES] if u in (3, 17) else []) for u in range(n_imp)]
    beh = loader0.behaviors.copy()
    beh[DEFAULT_INVIEW_ARTICLES_COL] = [cand.tolist()] * n_imp
    beh[DEFAULT_LABELS_COL] = [[int(j in cl) for j in range(N_CANDIDATES)] for cl in clicks]
    beh["impression_time"] = rng.integers(10, 40, n_imp).astype(np.float64)
    loader = type(loader0)(behaviors=beh, article_dict=loader0.article_dict, user_id_mapping=loader0.user_id_mapping,
                           unknown_representation="zeros", history_column=loader0.history_column, batch_size=16, eval_mode=True)
    assert len(loader) >= 3
    clicked = [[int(cand[j]) for j in sorted(cl)] for cl in clicks]
    pairs = [(u, a) for u in range(n_imp) for a in clicked[u]]

    before = model.scorer.predict(loader)
    pred = before.reshape(n_imp, N_CANDIDATES).astype(np.float64)
    ids_ex, sc_ex = model.recommend_pairwise(loader, cand, top_n=N_CANDIDATES, return_scores=True)
    ids_all, sc_all = model.recommend_pairwise(loader, cand, top_n=N_CANDIDATES, return_scores=True, exclude_history=False)
    counts = _count_calls(monkeypatch, hip)
    got_ex = model.rank_targets_pairwise(loader, None, cand)
    assert counts["ebn_conv1d_fwd_f32"] == 1 and counts["ebn_npa_target_rank_f32"] == 1  # one catalogue chunk, one counting launch
    assert counts["ebn_pap_indexed_f32"] == len(loader) and "ebn_npa_topk_score_f32" not in counts  # the histories only
    counts.clear()
    got_all = model.rank_targets_pairwise(loader, None, cand, exclude_history=False, users_per_call=16)
    assert counts["ebn_conv1d_fwd_f32"] == 1 and counts["ebn_npa_target_rank_f32"] == len(loader)  # a launch per flush
    assert counts["ebn_pap_indexed_f32"] == len(loader)
    monkeypatch.undo()

    def against_lists(got, ids, sc, want_pairs):
        assert list(zip(got.impression.tolist(), got.target_id.tolist())) == want_pairs and len(got) == len(want_pairs)
        assert got.rank.dtype == got.count.dtype == np.int32 and got.score.dtype == np.float32
        n_ranked = 0
        for (u, a), r, n, s in zip(want_pairs, got.rank.tolist(), got.count.tolist(), got.score):
            row = ids[u].tolist()
            assert n == sum(i != -1 for i in row), (u, a)
            if r > 0:
                assert row[r - 1] == a and bits(np.float32(s))[0] == bits(sc[u, r - 1:r])[0], (u, a, r)
                n_ranked += 1
            else:
                assert a not in row and np.isneginf(s), (u, a)
        return n_ranked

    assert against_lists(got_ex, ids_ex, sc_ex, pairs) >= n_imp // 2
    assert against_lists(got_all, ids_all, sc_all, pairs) == len(pairs) and (got_all.count == N_CANDIDATES).all()
    assert got_ex.impression.tolist().count(3) == 2 and got_ex.impression.tolist().count(17) == 2
    again = model.rank_targets_pairwise(loader, None, cand, users_per_call=16)
    assert all(np.array_equal(bits(getattr(again, f)), bits(getattr(got_ex, f))) for f in ("rank", "count", "score"))
    raw = model.rank_targets_pairwise(loader, None, cand, scores="raw")
    assert np.array_equal(raw.rank, got_ex.rank) and np.array_equal(raw.count, got_ex.count)
    ranked = raw.rank > 0
    assert (np.abs(1 / (1 + np.exp(-raw.score[ranked].astype(np.float64))) - got_ex.score[ranked]) <= 4 * 2.0 ** -23).all()

    # explicit targets: an article of the impression's own history, one outside the candidates, one the loader does not know
    in_history = [next((a for a in sorted(history[u]) if a in col), None) for u in range(n_imp)]
    assert sum(a is not None for a in in_history) >= 3, "the case must exercise the exclusion"
    outsider = next(a for a in sorted(index) if a not in col)
    explicit = [[a for a in (in_history[u],) if a is not None] + [outsider, -12345, int(cand[u % N_CANDIDATES])] for u in range(n_imp)]
    epairs = [(u, a) for u in range(n_imp) for a in explicit[u]]
    for exclude_history, ids, sc in ((True, ids_ex, sc_ex), (False, ids_all, sc_all)):
        got = model.rank_targets_pairwise(loader, explicit, cand, exclude_history=exclude_history)
        against_lists(got, ids, sc, epairs)
        for (u, a), r in zip(epairs, got.rank.tolist()):
            if a in (outsider, -12345) or (exclude_history and a in history[u]):
                assert r == 0, (u, a)
            if not exclude_history and a in col:
                assert r > 0, (u, a)
    m = rank_metrics(got_ex.rank, ks=(5, 10), counts=got_ex.count)
    assert 0.0 <= m["hit_rate@5"] <= m["hit_rate@10"] <= 1.0 and 0.0 < m["mrr"] <= 1.0 and 0.0 <= m["unranked"] < 1.0

    # freshness windows: candidates by publish time, every impression one range of them
    pub = {int(a): float(t) for a, t in zip(cand.tolist(), rng.integers(0, 40, N_CANDIDATES))}
    fresh = Freshness(pub, max_age=15.0)
    order, lo, hi = fresh.windows(cand, loader.X["impression_time"])
    sorted_ids = cand[order]
    s_sorted = pred[:, order]
    where = {int(a): j for j, a in enumerate(sorted_ids.tolist())}
    tol = 2 * nt.tolerance(pred)
    n_ranked = 0
    for exclude_history in (True, False):
        got = model.rank_targets_pairwise(loader, None, cand, window=fresh, exclude_history=exclude_history)
        assert list(zip(got.impression.tolist(), got.target_id.tolist())) == pairs
        position = np.arange(N_CANDIDATES)
        adm = (position[None, :] >= lo[:, None]) & (position[None, :] < hi[:, None])
        if exclude_history:
            adm &= ~np.array([[a in history[u] for a in sorted_ids.tolist()] for u in range(n_imp)])
        imp = got.impression
        tp = np.array([where[a] for a in got.target_id.tolist()])
        b = nt.band(s_sorted[imp], adm[imp], tp, tol)
        assert np.array_equal(got.count, adm[imp].sum(1))
        assert np.array_equal(got.rank > 0, adm[imp, tp])
        _check_band(got.rank, b, f"window, exclude_history={exclude_history}")
        ranked = got.rank > 0
        assert (np.abs(got.score[ranked] - s_sorted[imp, tp][ranked]) <= tol).all() and np.isneginf(got.score[~ranked]).all()
        n_ranked += int(ranked.sum())
        several = model.rank_targets_pairwise(loader, None, cand, window=fresh, exclude_history=exclude_history, users_per_call=16)
        assert all(np.array_equal(bits(getattr(several, f)), bits(getattr(got, f))) for f in ("rank", "count", "score"))
    assert n_ranked >= 10 and (hi - lo).min() < N_CANDIDATES, "the case must exercise the windows"
    with pytest.raises(NotImplementedError, match="window= is not supported for NPAModel"):
        model.recommend_pairwise(loader, cand, top_n=5, window=fresh)
    with pytest.raises(NotImplementedError, match="rank_targets is not supported for NPAModel"):
        model.rank_targets(loader, None, cand)

    np.testing.assert_array_equal(model.scorer.predict(loader), before)  # score_cached is untouched
    model.catalogue_max_bytes = 1
    with pytest.raises(ValueError, match="catalogue_max_bytes"):
        model.rank_targets_pairwise(loader, None, cand)
