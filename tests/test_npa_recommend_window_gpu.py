"""ebn_npa_topk_score_window_f32 (csrc/ebn_npa_topk.hip, the windowed instantiations) and NPAModel.recommend_pairwise_windowed on the
GPU.  The oracle needs no tolerance: a pair's score bits depend only on its rows and the order is score descending, then position
ascending, so user u's windowed list IS the unchanged ebn_npa_topk_score_f32 run for that one user on cand_rows[lo:hi], positions
shifted by lo, bit for bit."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from tests import npa_target_rank_cases as nt
from tests import recommend_window_cases as rw
from tests.guarded import guard_in, guard_out, poison
from tests.hip_testutil import P, S, dev
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3
SHAPE_K = [((65, 130, 30, 36, 24), 10), ((40, 50, 33, 32, 24), 5)]  # four candidates a step | two (L = 33: two row tiles each)
# the classes (of min(k, admissible positions)) a pattern must populate with at least 5 users, so that a change of generator
# cannot empty the test: counted on the host for seed = U
POPULATED = {((65, 130), "random"): ("short", "full"), ((65, 130), "edges"): ("empty", "short", "full"), ((65, 130), "one"): ("short",),
             ((40, 50), "random"): ("short", "full")}


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _opt(a):
    return None if a is None else dev(a, torch.int32)


def launch(hip, operands, n_rows, cand_d, window_d, ex_d, k, mode=0, n_splits=0, poisoned=False):
    """one call on device tensors (operands: users, Q, Ua, Vd); window_d None: the unchanged ebn_npa_topk_score_f32
    -> (pos [U, k] int32, score [U, k] float32, flags [2]) as numpy arrays"""
    users_d, Q_d, Ua_d, Vd_d = operands
    U, F = users_d.shape
    A = Q_d.shape[1]
    L = Ua_d.numel() // (n_rows * A)
    M = n_rows if cand_d is None else len(cand_d)
    X = 0 if ex_d is None else ex_d.shape[1]
    pos_d = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
    score_d = torch.full((U, k), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    splits = n_splits if n_splits > 0 else int(hip.lib().ebn_npa_topk_auto_splits(U, M, L))
    ws_bytes = int(hip.lib().ebn_topk_workspace_bytes(U, k, splits))
    assert ws_bytes > 0
    ws_d = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    if poisoned:
        poison(ws_d)
    if window_d is None:
        code = hip.lib().ebn_npa_topk_score_f32(P(users_d), P(Q_d), P(Ua_d), P(Vd_d), n_rows, P(cand_d), M, P(ex_d), X, k, mode, n_splits,
                                                P(pos_d), P(score_d), P(flags_d), P(ws_d), ws_bytes, U, L, F, A, S())
    else:
        code = hip.lib().ebn_npa_topk_score_window_f32(P(users_d), P(Q_d), P(Ua_d), P(Vd_d), n_rows, P(cand_d), M, P(window_d), P(ex_d), X, k,
                                                       mode, n_splits, P(pos_d), P(score_d), P(flags_d), P(ws_d), ws_bytes, U, L, F, A, S())
    assert code == OK, code
    torch.cuda.synchronize()
    return pos_d.cpu().numpy(), score_d.cpu().numpy(), flags_d.cpu().numpy()


class Case:
    """a case of npa_target_rank_cases.case() on the device, with its candidate list (always explicit: a slice of it is what the
    plain entry is run on)"""

    def __init__(self, c, cand_rows=None):
        self.c, self.n_rows = c, c["n_rows"]
        self.rows = np.asarray(cand_rows if cand_rows is not None else
                               (c["cand_rows"] if c["cand_rows"] is not None else np.arange(c["n_rows"])), dtype=np.int32)
        self.ops = (dev(c["users"]), dev(c["Q"]), dev(c["Ua"]), dev(c["Vd"]))
        self.cand_d = dev(self.rows, torch.int32)
        self.ex_d = _opt(c["exclude"])
        self.U, self.M = c["users"].shape[0], len(self.rows)

    def with_catalogue(self, **changed):
        other = Case({**self.c, **changed}, self.rows)
        return other

    def windowed(self, hip, window, k, users=None, cand_null=False, **kw):
        us_d, Q_d, Ua_d, Vd_d = self.ops
        ex_d = self.ex_d
        if users is not None:
            idx = torch.as_tensor(np.asarray(users), device="cuda")
            us_d, Q_d = us_d[idx].contiguous(), Q_d[idx].contiguous()
            ex_d = None if ex_d is None else ex_d[idx].contiguous()
        return launch(hip, (us_d, Q_d, Ua_d, Vd_d), self.n_rows, None if cand_null else self.cand_d, dev(window, torch.int32), ex_d, k, **kw)

    def plain(self, hip, k, **kw):
        return launch(hip, self.ops, self.n_rows, self.cand_d, None, self.ex_d, k, **kw)

    def plain_slice(self, hip, u, lo, hi, k, mode=0):
        """the unchanged entry for user u alone on cand_rows[lo:hi] (lo < hi), positions shifted back by lo -> (pos [k], score [k])"""
        us_d, Q_d, Ua_d, Vd_d = self.ops
        ex_d = None if self.ex_d is None else self.ex_d[u:u + 1]
        pos, score, flags = launch(hip, (us_d[u:u + 1], Q_d[u:u + 1], Ua_d, Vd_d), self.n_rows, self.cand_d[lo:hi].contiguous(), None, ex_d, k,
                                   mode=mode, n_splits=1)
        return np.where(pos[0] >= 0, pos[0] + lo, -1), score[0], flags


def check_against_plain_slices(hip, case, window, got, k, users=None, mode=0):
    """every user's (or the given users') windowed list and score bits are the plain entry's on the user's slice; -> the number of
    non-empty windows compared"""
    pos, score = got[:2]
    w = nt.clamp(window, case.M)
    n = 0
    for u in (range(case.U) if users is None else users):
        lo, hi = int(w[u, 0]), int(w[u, 1])
        if lo >= hi:
            assert (pos[u] == -1).all() and np.isneginf(score[u]).all(), u
            continue
        want_pos, want_score, _flags = case.plain_slice(hip, u, lo, hi, k, mode)
        assert np.array_equal(pos[u], want_pos), (u, lo, hi, pos[u], want_pos)
        assert np.array_equal(bits(score[u]), bits(want_score)), (u, lo, hi)
        n += 1
    return n


# ------------------------------------------------------------------------------------------------ 1. every user against the plain entry
@pytest.mark.parametrize("pattern", nt.PATTERNS)
@pytest.mark.parametrize("shape,k", SHAPE_K, ids=[nt.shape_id(s) for s, _ in SHAPE_K])
def test_every_list_is_the_plain_entry_on_the_users_slice(hip, shape, k, pattern):
    """subset cand_rows with two rows outside the table, exclude x3, all seven window patterns: every user's positions and score
    bits equal ebn_npa_topk_score_f32 for that user on cand_rows[lo:hi]; an empty window gives -1 / -inf; the number of kept slots is
    min(k, admissible positions) exactly; the flags are window_reference's, the either-value clause honoured; windows that hold
    everything equal the plain entry on the whole list in both outputs.  At 65 x 130 the sliding pattern exercises the per-wave
    skip: wave 0's union ends near position 80, user 64 is alone in wave 2."""
    U, M = shape[:2]
    c = nt.case(shape, seed=41, cand="subset", exclude="x3")
    n_rows = c["n_rows"]
    cand_rows = nt.with_bad_rows(c["cand_rows"], n_rows)
    case = Case(c, cand_rows)
    window = nt.windows(pattern, U, M, seed=U)
    adm = nt.admissible(c, window, cand_rows=cand_rows)
    n_adm = adm.sum(1)
    classes = dict(empty=int((n_adm == 0).sum()), short=int(((n_adm > 0) & (n_adm < k)).sum()), full=int((n_adm >= k).sum()))
    print(f"shape {shape} pattern {pattern}: users with an empty / short / full list {classes}")
    for name in POPULATED.get(((U, M), pattern), ()):
        assert classes[name] >= 5, (pattern, name, classes)
    for mode in (0, 1):
        got = case.windowed(hip, window, k, mode=mode)
        pos, score, flags = got
        assert np.array_equal((pos >= 0).sum(1), np.minimum(k, n_adm))
        assert (np.isneginf(score) == (pos < 0)).all()
        kept = pos >= 0
        assert adm[np.nonzero(kept)[0], pos[kept]].all()  # nothing outside a window, out of the table or excluded
        _p, _s, want_flags = rw.window_reference(nt.scores64(c, cand_rows), k, window, cand_rows, n_rows, c["exclude"])
        if want_flags[0] == 0 and nt.row_flag_is_open(window, cand_rows, n_rows, M):
            assert flags[0] in (0, 1) and flags[1] == 0
        else:
            assert tuple(flags) == want_flags
        n = check_against_plain_slices(hip, case, window, got, k, mode=mode)
        assert n == int((nt.clamp(window, M)[:, 0] < nt.clamp(window, M)[:, 1]).sum())
        if pattern == "empty":
            assert n == 0 and (pos == -1).all() and tuple(flags) == (0, 0)
        if pattern in ("all", "outside"):
            plain = case.plain(hip, k, mode=mode)
            assert np.array_equal(pos, plain[0]) and np.array_equal(bits(score), bits(plain[1])) and tuple(plain[2]) == tuple(flags) == (1, 0)


# ------------------------------------------------------------------------------------------------ 2. a narrow union
def _narrow_windows(U, lo, hi, seed, own=None):
    """random non-empty sub-ranges of [lo, hi); own = (user, split): that user alone owns [lo, split), the others lie in [split, hi)"""
    rng = np.random.default_rng(seed)
    base = lo if own is None else own[1]
    a, b = rng.integers(base, hi, U), rng.integers(base, hi, U)
    w = np.stack([np.minimum(a, b), np.maximum(a, b) + 1], 1).astype(np.int32)
    if own is not None:
        w[own[0]] = lo, own[1]
    w[(own[0] + 1) % U if own is not None else 0, 1] = hi  # the union reaches hi
    w[own[0] if own is not None else 1, 0] = lo          # and starts at lo
    return w


@pytest.mark.parametrize("U,M,span", [(65, 130, (41, 71)), (130, 300, (120, 165))], ids=["65x130", "130x300"])
def test_a_union_inside_the_list_is_walked_alone_and_split_evenly(hip, U, M, span):
    """every window inside [41, 71) of 130 positions (and [120, 165) of 300, two workgroups): the workgroup walks 8 (12) of the
    list's 33 (75) steps.  n_splits 1, 2, 7, 64 and 0 -- 7 and 64 exceed the steps some unions hold, so some ranges are empty --
    give the bits of n_splits = 1, as does a second run, and every list is the plain entry's on the user's slice."""
    k = 10
    c = nt.case((U, M, 30, 36, 24), seed=43, cand="subset", exclude="x3")
    case = Case(c)
    window = _narrow_windows(U, span[0], span[1], seed=3)
    assert window[:, 0].min() == span[0] and window[:, 1].max() == span[1] and (window[:, 0] < window[:, 1]).all()
    base = case.windowed(hip, window, k, n_splits=1)
    assert tuple(base[2]) == (0, 0) and (base[0][:, 0] >= 0).sum() > U // 2
    for s in (2, 7, 64, 0, 1):  # the last: another run
        got = case.windowed(hip, window, k, n_splits=s)
        assert all(np.array_equal(bits(g), bits(b)) for g, b in zip(got, base)), s
    assert check_against_plain_slices(hip, case, window, base, k) == U


def test_rows_outside_the_union_are_never_seen_and_one_inside_one_window_is_that_users_alone(hip):
    """65 x 130, distinct candidate rows, windows inside [41, 71), user 7 alone owning [41, 50).  A NaN catalogue row and a row
    outside the table at positions outside [41, 71): flags (0, 0), every list unchanged.  The same at position 45, inside user 7's
    window only: user 7's list lacks the position, flags[1] (flags[0]) is set, every other list is unchanged."""
    U, M, k = 65, 130, 10
    lo, hi, owner, at = 41, 71, 7, 45
    c = nt.case((U, M, 30, 36, 24), seed=47, cand="subset", exclude="x3")
    c["exclude"][owner] = -1
    rows = np.random.default_rng(5).permutation(c["n_rows"])[:M].astype(np.int32)  # every row once: a planted row is one position
    case = Case(c, rows)
    window = _narrow_windows(U, lo, hi, seed=4, own=(owner, 50))
    inside = (window[:, 0] <= at) & (at < window[:, 1])
    assert inside.sum() == 1 and inside[owner] and window[:, 0].min() == lo and window[:, 1].max() == hi
    for n_splits in (1, 3):
        clean = case.windowed(hip, window, k, n_splits=n_splits)
        assert tuple(clean[2]) == (0, 0) and at in clean[0][owner]
        for far in (3, 40, 71, 129):  # outside the union; 40 and 71 share a step with positions inside it
            nan_case = case.with_catalogue(Vd=_with(c["Vd"], (int(rows[far]), 7, 5), np.nan))
            got = nan_case.windowed(hip, window, k, n_splits=n_splits)
            assert tuple(got[2]) == (0, 0) and all(np.array_equal(bits(g), bits(w_)) for g, w_ in zip(got[:2], clean[:2])), far
            got = Case(c, _with(rows, far, c["n_rows"])).windowed(hip, window, k, n_splits=n_splits)
            assert tuple(got[2]) == (0, 0) and all(np.array_equal(bits(g), bits(w_)) for g, w_ in zip(got[:2], clean[:2])), far
        others = np.arange(U) != owner
        for which, planted in ((1, case.with_catalogue(Ua=_with(c["Ua"], (int(rows[at]), 29, 23), np.nan))), (0, Case(c, _with(rows, at, -1)))):
            pos, score, flags = planted.windowed(hip, window, k, n_splits=n_splits)
            assert flags[which] == 1 and flags[1 - which] == 0
            assert at not in pos[owner] and (pos[owner] >= 0).sum() == (clean[0][owner] >= 0).sum() - 1
            assert np.array_equal(pos[owner][:-1], clean[0][owner][clean[0][owner] != at][:k - 1])
            assert np.array_equal(pos[others], clean[0][others]) and np.array_equal(bits(score[others]), bits(clean[1][others]))


def _with(a, at, value):
    out = np.array(a)
    out[at] = value
    return out


# ------------------------------------------------------------------------------------------------ 3. other neighbours
@pytest.mark.parametrize("pattern", ["random", "sliding"])
def test_a_list_does_not_depend_on_the_other_users_of_the_launch(hip, pattern):
    """(130, 300, 30, 400, 200), k = 64: a launch over a random half of the users, with their windows and exclusion rows -- other
    neighbours in the workgroup, another union -- gives those users the same bits; the first and the last user of each 128-user
    workgroup are the plain entry's on their slices."""
    shape, k = nt.SHAPES[-1], 64
    U, M = shape[:2]
    c = nt.case(shape, seed=5, cand="subset", exclude="x3")
    case = Case(c)
    window = nt.windows(pattern, U, M, seed=6)
    base = case.windowed(hip, window, k, mode=1)
    assert tuple(base[2]) == (0, 0)
    pick = np.sort(np.random.default_rng(8).choice(U, U // 2, replace=False))
    got = case.windowed(hip, window[pick], k, users=pick, mode=1, n_splits=2)
    assert np.array_equal(got[0], base[0][pick]) and np.array_equal(bits(got[1]), bits(base[1][pick])) and tuple(got[2]) == (0, 0)
    assert check_against_plain_slices(hip, case, window, base, k, users=[0, 127, 128, U - 1], mode=1) >= 3


# ------------------------------------------------------------------------------------------------ 4. agreement with the rank kernel
def test_the_rank_kernel_ranks_a_listed_target_at_its_slot(hip):
    """the window test shape, random windows, every user's target drawn from its own windowed list: ebn_npa_target_rank_f32 with the
    same window and exclude returns rank = slot + 1 and the slot's score bits; a target outside the window has rank 0"""
    from tests.test_npa_target_rank_gpu import run_rank

    shape, k = nt.WINDOW_SHAPE, 10
    U, M = shape[:2]
    c = nt.case(shape, seed=41, cand="subset", exclude="x3")
    case = Case(c)
    window = nt.windows("random", U, M, seed=U)
    w = nt.clamp(window, M)
    for mode in (0, 1):
        pos, score, flags = case.windowed(hip, window, k, mode=mode)
        assert tuple(flags) == (0, 0)
        n_kept = (pos >= 0).sum(1)
        slot = np.where(n_kept > 0, (7 * np.arange(U)) % np.maximum(n_kept, 1), -1)
        outside = np.where(w[:, 0] > 0, w[:, 0] - 1, np.minimum(w[:, 1], M - 1))  # a position just outside (inside only for [0, M))
        out = (np.arange(U) % 5 == 0) | (n_kept == 0)
        out &= ~((w[:, 0] == 0) & (w[:, 1] == M))
        target = np.where(out | (slot < 0), outside, pos[np.arange(U), np.maximum(slot, 0)]).astype(np.int32)
        rank, _count, tscore, rflags = run_rank(hip, c, target, window, mode=mode)
        assert tuple(rflags) == (0, 0)
        listed = ~out & (slot >= 0)
        assert listed.sum() > U // 2 and out.sum() >= 5
        assert np.array_equal(rank[listed], slot[listed] + 1) and (rank[~listed] == 0).all()
        assert np.array_equal(bits(tscore[listed]), bits(score[np.arange(U), np.maximum(slot, 0)][listed]))
        assert np.isneginf(tscore[~listed]).all()


# ------------------------------------------------------------------------------------------------ 5. guard bands
@pytest.mark.parametrize("cand", ["null", "subset"])
def test_operands_between_guards(hip, cand):
    """Ua_all, Vd_all, users and Q inside NaN guards (L = 30: two padded token rows per candidate; U = 65: 63 user columns past the
    last), window between whole-list ranges, exclude and cand_rows between harmful rows, outputs in canaries, the workspace
    poisoned: bit-equal to the unguarded run, flags (0, 0), every guard intact."""
    shape, k = nt.SHAPES[2], 10
    U, M, L, F, A = shape
    c = nt.case(shape, seed=13, cand=cand, exclude="x3")
    n_rows = c["n_rows"]
    case = Case(c)
    window = nt.windows("random", U, M, seed=1)
    want = case.windowed(hip, window, k, cand_null=cand == "null")
    assert tuple(want[2]) == (0, 0) and (want[0][:, 0] >= 0).sum() > U // 2
    Ua_d, hU = guard_in(c["Ua"].reshape(n_rows * L, A))
    Vd_d, hV = guard_in(c["Vd"].reshape(n_rows * L, F))
    (us_d, hu), (Q_d, hQ) = guard_in(c["users"]), guard_in(c["Q"])
    ed, he = guard_in(c["exclude"], fill=-1)
    he.set_guards(int(case.rows[want[0][0, 0]]), int(case.rows[want[0][U - 1, 0]]))  # an over-read takes the neighbour's best away
    wd, hw = guard_in(window, fill=0)
    hw.set_guards(0, M)
    handles = dict(Ua_all=hU, Vd_all=hV, users=hu, Q=hQ, exclude=he, window=hw)
    cd = None
    if c["cand_rows"] is not None:
        cd, handles["cand_rows"] = guard_in(c["cand_rows"], fill=n_rows)
    for n_splits in (1, 2):
        (pd_, hp), (sd, hs), (fd, hf) = guard_out((U, k), dtype=torch.int32), guard_out((U, k)), guard_out((2,), dtype=torch.int32)
        hf.fill_payload([0, 0])
        ws_bytes = int(hip.lib().ebn_topk_workspace_bytes(U, k, n_splits))
        ws = poison(torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"))
        code = hip.lib().ebn_npa_topk_score_window_f32(P(us_d), P(Q_d), P(Ua_d), P(Vd_d), n_rows, P(cd), M, P(wd), P(ed), 3, k, 0, n_splits,
                                                       P(pd_), P(sd), P(fd), P(ws), ws_bytes, U, L, F, A, S())
        assert code == OK
        torch.cuda.synchronize()
        assert tuple(hf.payload().reshape(-1).tolist()) == (0, 0)
        assert np.array_equal(hp.payload().cpu().numpy(), want[0]) and np.array_equal(bits(hs.payload().cpu().numpy()), bits(want[1])), n_splits
        for name, h in {**handles, "out_pos": hp, "out_score": hs, "flags": hf}.items():
            h.check(name)


# ------------------------------------------------------------------------------------------------ 6. edges
def test_no_users_no_candidates_and_a_failing_call_writes_nothing(hip):
    c = nt.case(nt.SHAPES[1], seed=29)
    U, M, L, F, A = nt.SHAPES[1]
    k = 4
    us, Q, Ua, Vd = dev(c["users"]), dev(c["Q"]), dev(c["Ua"]), dev(c["Vd"])
    window = dev(np.tile([[0, M]], (U, 1)), torch.int32)
    pos_d = torch.full((U * k + 3,), -7, dtype=torch.int32, device="cuda")
    score_d = torch.full((U * k + 3,), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    base = dict(users=P(us), Q=P(Q), Ua=P(Ua), Vd=P(Vd), n_rows=M, cand=None, M=M, window=P(window), ex=None, X=0, k=k, mode=0, n_splits=1,
                pos=P(pos_d), score=P(score_d), flags=P(flags_d), ws=P(ws), ws_bytes=1 << 16, U=U, L=L, F=F, A=A, stream=S())
    call = lambda **kw: hip.lib().ebn_npa_topk_score_window_f32(*{**base, **kw}.values())
    need = int(hip.lib().ebn_topk_workspace_bytes(U, k, 2))
    assert call(window=None) == BAD_ARG
    assert call(Q=ctypes.c_void_p(Q.data_ptr() + 4)) == ALIGN
    assert call(k=65) == UNSUPPORTED and call(k=0) == UNSUPPORTED and call(L=65) == UNSUPPORTED and call(A=A + 2) == UNSUPPORTED
    assert call(M=M - 1) == BAD_ARG and call(mode=3) == BAD_ARG and call(pos=None) == BAD_ARG
    assert call(n_splits=2, ws_bytes=need - 1) == BAD_ARG and call(n_splits=2, ws=None) == BAD_ARG
    assert call(U=0) == OK and call(U=0, window=None) == OK  # U == 0: nothing to do
    torch.cuda.synchronize()
    assert (pos_d == -7).all() and (score_d == 123.0).all() and (flags_d == 0).all()
    assert call(n_splits=2, ws_bytes=need) == OK  # the same call with enough workspace runs
    torch.cuda.synchronize()
    assert (pos_d[:U * k] >= 0).all() and (pos_d[U * k:] == -7).all() and (score_d[U * k:] == 123.0).all() and (flags_d == 0).all()
    assert call(n_rows=0, M=0) == OK  # M == 0: the outputs are filled as empty
    torch.cuda.synchronize()
    assert (pos_d[:U * k] == -1).all() and torch.isneginf(score_d[:U * k]).all() and (pos_d[U * k:] == -7).all() and (flags_d == 0).all()


# ------------------------------------------------------------------------------------------------ 7. the model
N_CANDIDATES, TOP_N = 30, 8
TWO_DAYS, SIX_HOURS = pd.Timedelta(days=2), pd.Timedelta(hours=6)


def test_recommend_pairwise_windowed_is_the_full_ranking_filtered_by_time(hip, frames):  # noqa: F811
    """recommend_pairwise_windowed(window=Freshness(pub, max_age = 2 days)) against recommend_pairwise(top_n = every candidate)
    filtered on the host by  t - 2 days <= published <= t  and cut to top_n: the same ids and score bits, with and without the
    history exclusion, in one launch and in several; rank_targets_pairwise(window=...) has rank r <= top_n exactly when the list
    has the target at r - 1 (the slot's score bits); MMR(lam = 1) on top returns the plain windowed lists; scorer.predict is
    untouched.  The candidates are passed sorted by publish time, so a tie goes to the earlier position on both sides."""
    from ebrec.evaluation import MMR, Freshness
    from ebrec.evaluation.beyond_accuracy import DeviceLookup
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_IMPRESSION_TIMESTAMP_COL
    from tests.test_npa_cached_scoring_gpu import _npa_case
    from tests.test_recommend_window_gpu import _candidates, _timed_behaviours

    model, loader0, _Pw, _hp, _V = _npa_case("fixture", frames)
    beh = _timed_behaviours(frames)
    loader = type(loader0)(behaviors=beh, article_dict=loader0.article_dict, user_id_mapping=loader0.user_id_mapping,
                           unknown_representation="zeros", history_column=loader0.history_column, batch_size=16, eval_mode=True)
    n_imp = len(loader.X)
    assert len(loader) >= 3 and DEFAULT_IMPRESSION_TIMESTAMP_COL in loader.X.columns
    rng = np.random.default_rng(7)
    cand = _candidates(model, loader, beh, rng, N_CANDIDATES)
    steps = rng.integers(0, 20, len(cand))
    order = np.argsort(steps, kind="stable")
    cand, steps = cand[order], steps[order]  # by publish time already: positions are the same on both sides
    pub = {int(a): pd.Timestamp("2023-02-25") + int(s) * SIX_HOURS for a, s in zip(cand.tolist(), steps)}
    assert len(set(pub.values())) < len(pub) <= 64
    fresh = Freshness(pub, max_age=TWO_DAYS)
    times = beh[DEFAULT_IMPRESSION_TIMESTAMP_COL].tolist()
    _order, lo, hi = fresh.windows(cand, loader.X[DEFAULT_IMPRESSION_TIMESTAMP_COL])
    assert (hi - lo).min() < len(cand) and (hi - lo).max() >= TOP_N, "the case must exercise the windows"
    history = [set(h) for h in beh[DEFAULT_HISTORY_ARTICLE_ID_COL]]
    where = {int(a): j for j, a in enumerate(cand.tolist())}
    explicit = [[int(cand[(7 * u + 3 * j) % N_CANDIDATES]) for j in range(4)] for u in range(n_imp)]
    pairs = [(u, a) for u in range(n_imp) for a in explicit[u]]

    before = model.scorer.predict(loader)
    n_ranked = 0
    for exclude_history in (True, False):
        full_ids, full_sc = model.recommend_pairwise(loader, cand, top_n=len(cand), return_scores=True, exclude_history=exclude_history)
        ids, sc = model.recommend_pairwise_windowed(loader, cand, window=fresh, top_n=TOP_N, return_scores=True,
                                                    exclude_history=exclude_history, fill_id=-9)
        assert ids.shape == sc.shape == (n_imp, TOP_N) and sc.dtype == np.float32
        for u, t in enumerate(times):
            kept = [(a, s) for a, s in zip(full_ids[u].tolist(), full_sc[u]) if a != -1 and t - TWO_DAYS <= pub[a] <= t]
            kept.sort(key=lambda e: (-e[1], where[e[0]]))
            kept = kept[:TOP_N]
            assert ids[u].tolist() == [a for a, _ in kept] + [-9] * (TOP_N - len(kept)), (u, ids[u])
            assert np.array_equal(bits(sc[u]), bits(np.array([s for _, s in kept] + [-np.inf] * (TOP_N - len(kept)), np.float32))), u
            assert not (exclude_history and set(ids[u].tolist()) & history[u])
        several = model.recommend_pairwise_windowed(loader, cand, window=fresh, top_n=TOP_N, return_scores=True,
                                                    exclude_history=exclude_history, fill_id=-9, users_per_call=16)
        assert np.array_equal(several[0], ids) and np.array_equal(bits(several[1]), bits(sc))
        assert np.array_equal(model.recommend_pairwise_windowed(loader, cand, window=fresh, top_n=TOP_N, exclude_history=exclude_history,
                                                                fill_id=-9), ids)
        got = model.rank_targets_pairwise(loader, explicit, cand, window=fresh, exclude_history=exclude_history)
        assert list(zip(got.impression.tolist(), got.target_id.tolist())) == pairs
        for (u, a), r, s in zip(pairs, got.rank.tolist(), got.score):
            row = ids[u].tolist()
            if 0 < r <= TOP_N:
                assert row[r - 1] == a and bits(np.float32(s))[0] == bits(sc[u, r - 1:r])[0], (u, a, r)
                n_ranked += 1
            else:
                assert a not in row, (u, a, r)
    assert n_ranked >= 10, "the case must exercise the ranks"

    articles = {int(a): {"emb": rng.standard_normal(8).astype(np.float32)} for a in model._recommend_index(loader)}
    lookup = DeviceLookup(articles, ["emb"])
    ids, sc = model.recommend_pairwise_windowed(loader, cand, window=fresh, top_n=TOP_N, return_scores=True)
    mmr_ids, mmr_sc = model.recommend_pairwise_windowed(loader, cand, window=fresh, top_n=TOP_N, return_scores=True,
                                                        rerank=MMR(lookup, "emb", lam=1.0, pool=12))
    assert np.array_equal(mmr_ids, ids) and np.array_equal(bits(mmr_sc), bits(sc))
    np.testing.assert_array_equal(model.scorer.predict(loader), before)
    with pytest.raises(NotImplementedError, match="window= is not supported for NPAModel"):
        model.recommend_pairwise(loader, cand, top_n=5, window=fresh)
