"""ebn_cv_topk_f32 / ebn_cv_target_rank_f32 (csrc/ebn_covisit_topk.hip) through the C ABI on guard-banded operands, BITWISE against
the float32 twins of ebrec/models/baselines/covisit.py (which tests/test_covisit_topn_cpu.py holds against the plain-Python brute
force): the positions, and the scores as int32 views -- there is no tolerance.

Operands as in tests/test_covisit_gpu.py (tests/guarded.py): int64 arrays as pairs of int32 words inside zero words, index arrays
inside VALID indices (an over-read entry is used and shows), values and weights inside 3e18, outputs in canary buffers: guards
intact, every payload element written.

One test case = (n_rows, mode, values).  Inside it EVERY combination of history weights (none, positive, negative; the integer
"count" values and the NaN / +inf variants without weights), cand_pos (NULL, a permutation, one with negative and >= M entries),
X in {0, 1, 256}, n_splits in {0, 1, 2, 64} and k in {1, 5, 64} is launched; the users of a launch carry the histories (empty, all
absent, 1, 65, 300 entries, repeats, entries outside the table, user_hist outside [0, n_hists)) and the windows (full, empty,
clamped, lo >= hi, inner; none at all with X = 0).  The matrix of a case holds rows of T of 0, 1, 255, 256, 257 and 1000 columns,
a row on both sides of every range boundary, a row touching every catalogue row, a stored 0.0 and -0.0.  The rank kernel gets the
same grid, against its twin and against the top-k kernel's own k = 64 lists.  One combination per cand_pos also runs at a second
placement of every operand (front = 3)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from ebrec.models.baselines import covisit as cv
from tests import covisit_topn_cases as tc
from tests import guarded

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3
POISON = 3.0e18
GUARD = 4096
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _i64(x, front=0):
    words = np.concatenate([np.zeros(2 * front, np.int32), np.ascontiguousarray(np.asarray(x, np.int64)).view(np.int32)])
    view, h = guarded.guard_in(words, fill=0, guard=GUARD)
    return ctypes.c_void_p(view.data_ptr() + 8 * front), h


def _i32(x, fill, front=0):
    x = np.ascontiguousarray(x, dtype=np.int32)
    view, h = guarded.guard_in(np.concatenate([np.full(front * (x.shape[1] if x.ndim == 2 else 1), fill, np.int32), x.ravel()]), fill=fill,
                               guard=GUARD)
    return ctypes.c_void_p(view.data_ptr() + 4 * front * (x.shape[1] if x.ndim == 2 else 1)), h


def _f32(x, front=0):
    view, h = guarded.guard_in(np.concatenate([np.full(front, POISON, np.float32), np.asarray(x, np.float32)]), fill=POISON, guard=GUARD)
    return ctypes.c_void_p(view.data_ptr() + 4 * front), h


class _Matrix:
    """the guarded matrix and histories of one case at one placement"""

    def __init__(self, c, front=0):
        self.c, self.h = c, {}
        self.n_rows, self.nnz = c["n_rows"], c["t_cols"].size
        self.n_hists, self.n_hist_items, self.U = c["hist_offsets"].size - 1, c["hist_rows"].size, c["n_users"]
        self.t_indptr, self.h["t_indptr"] = _i64(c["t_indptr"], front)
        self.t_cols, self.h["t_cols"] = _i32(c["t_cols"], 0, front)  # a valid column
        self.t_vals, self.h["t_vals"] = _f32(c["t_vals"], front)
        self.hist_rows, self.h["hist_rows"] = _i32(c["hist_rows"], c["special_row"], front)  # a valid row: the one touching everything
        self.hist_weights = None
        if c["hist_weights"] is not None:
            self.hist_weights, self.h["hist_weights"] = _f32(c["hist_weights"], front)
        self.hist_offsets, self.h["hist_offsets"] = _i64(c["hist_offsets"], front)
        self.user_hist, self.h["user_hist"] = _i32(c["user_hist"], 5, front)  # a valid history: the longest

    def head(self, **k):
        names = ("t_indptr", "t_cols", "t_vals", "n_rows", "nnz", "hist_rows", "hist_weights", "hist_offsets", "n_hists", "n_hist_items", "user_hist")
        return [k.get(n, getattr(self, n)) for n in names]

    def check(self):
        for what, h in self.h.items():
            h.check(what)


def _workspace(nbytes):
    return guarded.poison(torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device="cuda"))


def _run_topk(hip, m, cand_pos, M, window, exclude, X, k, mode, n_splits):
    L = hip.lib()
    pos, h_pos = guarded.guard_out((m.U, k), dtype=torch.int32)
    score, h_score = guarded.guard_out((m.U, k))
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    splits = n_splits if n_splits > 0 else L.ebn_cv_topk_auto_splits(m.U, m.n_rows)
    ws = _workspace(L.ebn_cv_topk_workspace_bytes(m.U, k, splits))
    rc = L.ebn_cv_topk_f32(*m.head(), cand_pos, M, window, exclude, X, k, mode, n_splits, P(pos), P(score), P(flags), P(ws), ws.numel(), m.U,
                           hip.stream_handle())
    assert rc == OK, rc
    torch.cuda.synchronize()
    h_pos.check("out_pos")
    h_score.check("out_score")
    return h_pos.payload().cpu().numpy(), h_score.payload().cpu().numpy(), flags.cpu().numpy()


def _run_rank(hip, m, cand_pos, M, target, window, exclude, X, mode, n_splits):
    L = hip.lib()
    outs = [guarded.guard_out((m.U,), dtype=d) for d in (torch.int32, torch.int32, torch.float32)]
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    splits = n_splits if n_splits > 0 else L.ebn_cv_topk_auto_splits(m.U, m.n_rows)
    ws = _workspace(L.ebn_cv_target_rank_workspace_bytes(m.U, splits, 0 if cand_pos is None else M))
    rc = L.ebn_cv_target_rank_f32(*m.head(), cand_pos, M, target, window, exclude, X, mode, n_splits, *[P(o[0]) for o in outs], P(flags), P(ws),
                                  ws.numel(), m.U, hip.stream_handle())
    assert rc == OK, rc
    torch.cuda.synchronize()
    for (_, h), what in zip(outs, ("out_rank", "out_count", "out_score")):
        h.check(what)
    return [h.payload().cpu().numpy() for _, h in outs] + [flags.cpu().numpy()]


def _targets(list64, M, U):
    """per user: one of its own slots (0, 1, 4, 63 -- often empty: -1), a position next to one, none, one past M"""
    t = np.array([list64[u, (0, 1, 4, 63)[u % 4]] for u in range(U)], np.int64)
    t[3::5] = np.minimum(t[3::5] + 1, M - 1)
    t[4::6] = M + 2
    return t.astype(np.int32)


def _grid(hip, c, mode, front, full):
    """every combination for one matrix and history set; ``full``: all of n_splits / k / X, else one of each"""
    R = hip.lib().ebn_cv_topk_range()
    m = _Matrix(c, front)
    n_rows, U = c["n_rows"], c["n_users"]
    chains = cv.covisit_chains_host(c["t_indptr"], c["t_cols"], c["t_vals"], c["hist_rows"], c["hist_weights"], c["hist_offsets"], mode)
    twin = (c["t_indptr"], c["t_cols"], c["t_vals"], c["hist_rows"], c["hist_weights"], c["hist_offsets"], c["user_hist"], U)
    is_nan = bool(np.isnan(c["t_vals"]).any())
    seen = dict(flag0=set(), flag1=set(), short=0, negative=0, launches=0)
    for pos_kind, X in itertools.product((None, "perm", "oob"), (0, 1, 256) if full else (1,)):
        cand_pos, M = tc.positions(n_rows, pos_kind)
        cp, h_cp = (None, None) if cand_pos is None else _i32(cand_pos, 0, front)
        exclude = tc.exclusions(c, X)
        ex, h_ex = (None, None) if exclude is None else _i32(exclude, c["special_col"], front)
        p_special = c["special_col"] if cand_pos is None else int(cand_pos[c["special_col"]])
        variants = [tc.windows(U, M)] + ([None] if X == 0 else []) + ([tc.windows(U, M, avoid=p_special)] if is_nan and 0 <= p_special < M else [])
        for window in variants:
            wd, h_wd = (None, None) if window is None else _i32(window, 0, front)
            w_pos, w_score, w_flags = cv.covisit_topk_host(*twin, cand_pos, M, window, exclude, 64, mode, chains)
            target = _targets(w_pos, M, U)
            tg, h_tg = _i32(target, 0, front)
            w_rank = cv.covisit_target_rank_host(*twin, cand_pos, M, target, window, exclude, mode, chains)
            assert int(w_flags[0]) == int(pos_kind == "oob" and (np.asarray(cand_pos)[np.any([t for t, _ in chains], 0)] >= M).any())
            seen["flag0"].add(int(w_flags[0]))
            seen["flag1"].add(int(w_flags[1]))
            seen["short"] += int(((w_pos >= 0).sum(1) < 5).sum())
            seen["negative"] += int((w_score[w_pos >= 0] < 0).sum())
            lists = {}
            for n_splits in (0, 1, 2, 64) if full else (2,):
                for k in (1, 5, 64) if full else (5, 64):
                    pos, score, flags = _run_topk(hip, m, cp, M, wd, ex, X, k, mode, n_splits)
                    what = (pos_kind, X, window is None, n_splits, k)
                    assert np.array_equal(pos, w_pos[:, :k]), what
                    assert np.array_equal(_bits(score), _bits(w_score[:, :k])), what
                    assert np.array_equal(flags, w_flags), what
                    if k == 64:
                        lists[n_splits] = (pos, score)
                rank, count, t, flags = _run_rank(hip, m, cp, M, tg, wd, ex, X, mode, n_splits)
                for g, w, name in zip((rank, count, _bits(t), flags), (w_rank[0], w_rank[1], _bits(w_rank[2]), w_rank[3]), ("rank", "count", "t", "flags")):
                    assert np.array_equal(g, w), (name, pos_kind, X, window is None, n_splits)
                # against the top-k kernel's own lists: a rank within 64 is that slot, with that slot's score bits
                pos64, score64 = lists[n_splits]
                for u in np.flatnonzero((rank >= 1) & (rank <= 64)):
                    assert pos64[u, rank[u] - 1] == target[u] and _bits(score64[u, rank[u] - 1]) == _bits(t[u])
                assert np.array_equal(count >= 64, pos64[:, 63] >= 0)
                seen["launches"] += 1
            assert all(np.array_equal(a[0], lists[2][0]) and np.array_equal(_bits(a[1]), _bits(lists[2][1])) for a in lists.values())
            for h, what in ((h_wd, "window"), (h_tg, "target_pos")):
                if h is not None:
                    h.check(what)
        for h, what in ((h_cp, "cand_pos"), (h_ex, "exclude")):
            if h is not None:
                h.check(what)
    m.check()
    return seen, R


WEIGHTS = {"random": (None, "positive", "negative"), "count": (None,), "nan": (None,), "inf": (None,)}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("values", ["random", "count", "nan", "inf"])
@pytest.mark.parametrize("rows", ["1", "R-1", "R", "R+1", "2R+37"])
def test_lists_and_ranks_equal_the_twin_bit_for_bit(hip, rows, values, mode):
    R = int(hip.lib().ebn_cv_topk_range())
    n_rows = {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+37": 2 * R + 37}[rows]
    total = dict(flag0=set(), flag1=set(), short=0, negative=0)
    for weights in WEIGHTS[values]:
        c = tc.kernel_case(n_rows, R, values, weights)
        seen, _ = _grid(hip, c, mode, front=0, full=True)
        for key in ("flag0", "flag1"):
            total[key] |= seen[key]
        total["short"] += seen["short"]
        total["negative"] += seen["negative"]
        _grid(hip, c, mode, front=3, full=False)  # another placement of every operand
    assert total["flag0"] == ({0, 1} if n_rows > 1 else {0}) and total["short"] > 0  # one row: no position can lie at or above M
    if values == "nan" and n_rows > 1:
        assert total["flag1"] == {0, 1}  # the NaN inside a window, and outside every window
    if values == "random" and n_rows > 1:
        assert total["negative"] > 0  # touched rows with negative scores are listed (untouched ones never: the twin's lists)


def test_position_beyond_M_on_an_untouched_row_sets_no_flag(hip):
    # T: row 0 holds columns 1 and 2; cand_pos sends the untouched row 3 beyond M and the touched row 2 to position 0
    t_indptr, t_cols, t_vals = np.array([0, 2, 2, 2, 2], np.int64), np.array([1, 2], np.int32), np.array([0.0, -2.0], np.float32)
    c = dict(t_indptr=t_indptr, t_cols=t_cols, t_vals=t_vals, hist_rows=np.array([0], np.int32), hist_weights=None,
             hist_offsets=np.array([0, 1], np.int64), user_hist=np.array([0], np.int32), n_users=1, n_rows=4, special_row=0, special_col=0)
    m = _Matrix(c)
    for cand_pos, want_flag, want in (([2, 1, 0, 7], 0, [1, 0, -1]), ([2, 7, 0, -1], 1, [0, -1, -1])):
        cp, h = _i32(np.array(cand_pos, np.int32), 0)
        pos, score, flags = _run_topk(hip, m, cp, 3, None, None, 0, 3, 0, 0)
        assert pos.tolist() == [want] and flags.tolist() == [want_flag, 0], cand_pos
        h.check("cand_pos")
    assert _bits(score[0, 0]) == _bits(np.float32(-2.0))  # a touched negative row is listed, the untouched rows 0 and 3 are not


def test_two_runs_and_other_co_launched_users_give_the_same_bits(hip):
    R = int(hip.lib().ebn_cv_topk_range())
    c = dict(tc.kernel_case(R + 1, R, "random", "negative"))
    first = _run_topk(hip, _Matrix(c), None, R + 1, None, None, 0, 64, 0, 0)
    again = _run_topk(hip, _Matrix(c), None, R + 1, None, None, 0, 64, 0, 0)
    assert np.array_equal(first[0], again[0]) and np.array_equal(_bits(first[1]), _bits(again[1]))
    keep = np.array([5, 2, 12, 4], np.int64)  # a subset, in another order: other users share the launch
    sub = dict(c, user_hist=c["user_hist"][keep], n_users=int(keep.size))
    other = _run_topk(hip, _Matrix(sub), None, R + 1, None, None, 0, 64, 0, 2)
    assert np.array_equal(other[0], first[0][keep]) and np.array_equal(_bits(other[1]), _bits(first[1][keep]))
    target = np.ascontiguousarray(first[0][:, 1])
    tg, h_tg = _i32(target, 0)
    r_all = _run_rank(hip, _Matrix(c), None, R + 1, tg, None, None, 0, 0, 0)
    tg_sub, h_sub = _i32(target[keep], 0)
    r_sub = _run_rank(hip, _Matrix(sub), None, R + 1, tg_sub, None, None, 0, 0, 64)
    for a, b in zip(r_all[:3], r_sub[:3]):
        assert np.array_equal(_bits(a[keep]) if a.dtype == np.float32 else a[keep], _bits(b) if b.dtype == np.float32 else b)
    h_tg.check("target_pos")
    h_sub.check("target_pos")


def test_argument_checks_return_codes_and_write_nothing(hip):
    L, st = hip.lib(), hip.stream_handle()
    R = int(L.ebn_cv_topk_range())
    assert R >= 1024 and L.ebn_cv_topk_auto_splits(1, 3 * R) == 3 and L.ebn_cv_topk_auto_splits(10 ** 6, 3 * R) == 1 and L.ebn_cv_topk_auto_splits(4096, 9 * R) == 4
    assert L.ebn_cv_topk_auto_splits(1, 100 * R) == 64 and L.ebn_cv_topk_auto_splits(0, 0) == 1
    assert L.ebn_cv_topk_workspace_bytes(7, 5, 3) == L.ebn_topk_workspace_bytes(7, 5, 3) == 7 * 5 * 3 * 8 + 16
    assert L.ebn_cv_topk_workspace_bytes(7, 65, 3) == 0 and L.ebn_cv_topk_workspace_bytes(-1, 5, 3) == 0
    assert L.ebn_cv_target_rank_workspace_bytes(7, 3, 0) == (2 * 3 * 7 + 7) * 4 + 16 and L.ebn_cv_target_rank_workspace_bytes(7, 1, 0) == 16
    assert L.ebn_cv_target_rank_workspace_bytes(7, 3, 11) == (2 * 3 * 7 + 7 + 11) * 4 + 16 and L.ebn_cv_target_rank_workspace_bytes(7, 1, 11) == 60
    assert L.ebn_cv_target_rank_workspace_bytes(7, 0, 0) == 0 and L.ebn_cv_target_rank_workspace_bytes(2 ** 31, 2, 0) == 0
    assert L.ebn_cv_target_rank_workspace_bytes(7, 2, -1) == 0 and L.ebn_cv_target_rank_workspace_bytes(7, 2, 2 ** 31) == 0
    c = tc.kernel_case(R + 1, R, "random", "positive")
    m = _Matrix(c)
    U, n_rows, big = m.U, m.n_rows, 2 ** 31
    cand_pos, M = tc.positions(n_rows, "holes")  # M != n_rows: cand_pos is needed
    cp, h_cp = _i32(cand_pos, 0)
    wd, h_wd = _i32(tc.windows(U, M), 0)
    ex, h_ex = _i32(tc.exclusions(c, 4), 0)
    tg, h_tg = _i32(np.zeros(U, np.int32), 0)
    pos, h_pos = guarded.guard_out((U, 5), dtype=torch.int32)
    score, h_score = guarded.guard_out((U, 5))
    rank, h_rank = guarded.guard_out((U,), dtype=torch.int32)
    count, h_count = guarded.guard_out((U,), dtype=torch.int32)
    t, h_t = guarded.guard_out((U,))
    flags, h_flags = guarded.guard_out((2,), dtype=torch.int32)
    ws = _workspace(1 << 16)
    base = dict(cand_pos=cp, M=M, window=wd, exclude=ex, X=4, k=5, mode=0, n_splits=2, ws=P(ws), ws_bytes=ws.numel(), U=U)

    def topk(**k):
        a = dict(base, **k)
        return L.ebn_cv_topk_f32(*m.head(**k), a["cand_pos"], a["M"], a["window"], a["exclude"], a["X"], a["k"], a["mode"], a["n_splits"],
                                 a.get("pos", P(pos)), a.get("score", P(score)), a.get("flags", P(flags)), a["ws"], a["ws_bytes"], a["U"], st)

    def rnk(**k):
        a = dict(base, **k)
        return L.ebn_cv_target_rank_f32(*m.head(**k), a["cand_pos"], a["M"], a.get("target", tg), a["window"], a["exclude"], a["X"], a["mode"],
                                        a["n_splits"], a.get("rank", P(rank)), a.get("count", P(count)), a.get("t", P(t)),
                                        a.get("flags", P(flags)), a["ws"], a["ws_bytes"], a["U"], st)

    before = L.ebn_launch_count()
    bad = [dict([(n, v)]) for n in ("n_rows", "nnz", "n_hists", "n_hist_items", "M", "U") for v in (-1, big)]
    bad += [dict(X=-1), dict(n_splits=-1), dict(ws_bytes=-1), dict(mode=-1), dict(mode=2), dict(n_hists=0), dict(cand_pos=None),
            dict(flags=None), dict(t_indptr=None), dict(t_cols=None), dict(t_vals=None), dict(hist_rows=None), dict(hist_offsets=None),
            dict(ws=None), dict(ws_bytes=15)]
    for kw in bad:
        assert topk(**kw) == BAD_ARG, kw
        assert rnk(**kw) == BAD_ARG, kw
    for kw in (dict(pos=None), dict(score=None)):
        assert topk(**kw) == BAD_ARG, kw
    for kw in (dict(target=None), dict(rank=None), dict(count=None), dict(t=None)):
        assert rnk(**kw) == BAD_ARG, kw
    for kw in (dict(k=0), dict(k=65), dict(X=257)):
        assert topk(**kw) == UNSUPPORTED, kw
        assert topk(mode=3, **kw) == BAD_ARG, kw  # BAD_ARG comes first
    assert rnk(X=257) == UNSUPPORTED and rnk(X=257, U=-1) == BAD_ARG
    odd = ctypes.c_void_p(ws.data_ptr() + 4)
    assert topk(ws=odd) == ALIGN and rnk(ws=odd) == ALIGN
    assert topk(ws_bytes=L.ebn_cv_topk_workspace_bytes(U, 5, 2) - 1) == BAD_ARG
    assert rnk(ws_bytes=L.ebn_cv_target_rank_workspace_bytes(U, 2, M) - 1) == BAD_ARG
    assert rnk(n_splits=1, ws=None) == BAD_ARG and rnk(n_splits=1, ws_bytes=L.ebn_cv_target_rank_workspace_bytes(U, 1, M) - 1) == BAD_ARG  # the inverse of cand_pos
    # U == 0: nothing to do, nothing is needed
    assert topk(U=0, pos=None, score=None, flags=None, ws=None, ws_bytes=0) == OK and rnk(U=0, target=None, rank=None, ws=None, ws_bytes=0) == OK
    assert L.ebn_launch_count() == before
    torch.cuda.synchronize()
    for h, what in ((h_pos, "out_pos"), (h_score, "out_score"), (h_rank, "out_rank"), (h_count, "out_count"), (h_t, "out_score"),
                    (h_flags, "flags")):
        h.check_untouched(what)
    # the empty matrix and the empty candidate list: empty outputs in one launch, no workspace and no matrix needed
    legal = (dict(n_rows=0, M=0, cand_pos=None, t_indptr=None), dict(nnz=0, t_cols=None, t_vals=None), dict(M=0),
             dict(n_rows=0, M=0, nnz=0, cand_pos=None, t_indptr=None, t_cols=None, t_vals=None, ws=None, ws_bytes=0))
    tgt = np.array([-1, 0, 5] + [0] * (U - 3), np.int32)
    tg2, h_tg2 = _i32(tgt, 0)
    for kw in legal:
        p2, hp2 = guarded.guard_out((U, 5), dtype=torch.int32)
        s2, hs2 = guarded.guard_out((U, 5))
        f2 = torch.zeros(2, dtype=torch.int32, device="cuda")
        assert topk(pos=P(p2), score=P(s2), flags=P(f2), **kw) == OK, kw
        torch.cuda.synchronize()
        hp2.check("out_pos")
        hs2.check("out_score")
        assert (hp2.payload() == -1).all() and torch.isneginf(hs2.payload()).all() and not f2.any(), kw
        outs = [guarded.guard_out((U,), dtype=d) for d in (torch.int32, torch.int32, torch.float32)]
        assert rnk(target=tg2, rank=P(outs[0][0]), count=P(outs[1][0]), t=P(outs[2][0]), flags=P(f2), **kw) == OK, kw
        torch.cuda.synchronize()
        for _, h in outs:
            h.check("rank outputs")
        assert not outs[0][1].payload().any() and not outs[1][1].payload().any() and torch.isneginf(outs[2][1].payload()).all()
        assert f2.tolist() == [1 if kw.get("M", M) <= 5 else 0, 0], kw  # a target position >= M is reported
    assert L.ebn_launch_count() == before + 2 * len(legal)
    m.check()
    for h, what in ((h_cp, "cand_pos"), (h_wd, "window"), (h_ex, "exclude"), (h_tg, "target_pos"), (h_tg2, "target_pos")):
        h.check(what)
