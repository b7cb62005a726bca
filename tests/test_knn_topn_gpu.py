"""ebn_knn_topk_f32 / ebn_knn_target_rank_f32 (csrc/ebn_knn_topk.hip) through the C ABI on guard-banded operands, BITWISE against the
float32 twins of ebrec/models/baselines/knn.py (which tests/test_knn_topn_cpu.py holds against the plain-Python brute force): the
positions, and the scores as int32 views -- there is no tolerance.

Operands as in tests/test_covisit_topn_gpu.py (tests/guarded.py): int64 arrays as pairs of int32 words inside zero words, index
arrays inside VALID indices (an over-read entry is used and shows), sims and scales inside 3e18, outputs in canary buffers: guards
intact, every payload element written.

One test case = (n_rows, k_nbr, sims, item_scale).  Inside it EVERY combination of cand_pos (NULL, a permutation, one with negative
and >= M entries), X in {0, 1, 256}, n_splits in {0, 1, 2, 64} and k in {1, 5, 64} is launched; the users of a launch carry the
neighbour rows of tests/knn_topn_cases.py and the windows (full, empty, clamped, lo >= hi, inner; none at all with X = 0).  The rank
kernel gets the same grid, against its twin and against the top-k kernel's own k = 64 lists.  One combination per cand_pos also runs
at a second placement of every operand (front = 3)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from ebrec.models.baselines import knn as knn_mod
from tests import guarded
from tests import knn_topn_cases as tc

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
    width = x.shape[1] if x.ndim == 2 else 1
    view, h = guarded.guard_in(np.concatenate([np.full(front * width, fill, np.int32), x.ravel()]), fill=fill, guard=GUARD)
    return ctypes.c_void_p(view.data_ptr() + 4 * front * width), h


def _f32(x, front=0):
    x = np.ascontiguousarray(x, dtype=np.float32)
    width = x.shape[1] if x.ndim == 2 else 1
    view, h = guarded.guard_in(np.concatenate([np.full(front * width, POISON, np.float32), x.ravel()]), fill=POISON, guard=GUARD)
    return ctypes.c_void_p(view.data_ptr() + 4 * front * width), h


class _Index:
    """the guarded sets and neighbour rows of one case at one placement"""

    def __init__(self, c, front=0):
        self.c, self.h = c, {}
        self.n_seqs, self.nnz_s, self.n_rows = c["n_seqs"], c["s_items"].size, c["n_rows"]
        self.n_hists, self.k_nbr, self.U = c["nbr_seq"].shape[0], c["nbr_seq"].shape[1], c["n_users"]
        self.s_indptr, self.h["s_indptr"] = _i64(c["s_indptr"], front)
        self.s_items, self.h["s_items"] = _i32(c["s_items"], c["special_col"], front)  # a valid row: the one many sets hold
        self.item_scale = None
        if c["item_scale"] is not None:
            self.item_scale, self.h["item_scale"] = _f32(c["item_scale"], front)
        self.nbr_seq, self.h["nbr_seq"] = _i32(c["nbr_seq"], c["full_seq"], front)  # a valid sequence: the set of every row
        self.nbr_sim, self.h["nbr_sim"] = _f32(c["nbr_sim"], front)
        self.user_hist = None
        if c["user_hist"] is not None:
            self.user_hist, self.h["user_hist"] = _i32(c["user_hist"], 5, front)  # a valid neighbour row: the one that touches everything

    def head(self, **k):
        names = ("s_indptr", "s_items", "n_seqs", "nnz_s", "n_rows", "item_scale", "nbr_seq", "nbr_sim", "n_hists", "k_nbr", "user_hist")
        return [k.get(n, getattr(self, n)) for n in names]

    def check(self):
        for what, h in self.h.items():
            h.check(what)


def _workspace(nbytes):
    return guarded.poison(torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device="cuda"))


def _run_topk(hip, m, cand_pos, M, window, exclude, X, k, n_splits):
    L = hip.lib()
    pos, h_pos = guarded.guard_out((m.U, k), dtype=torch.int32)
    score, h_score = guarded.guard_out((m.U, k))
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    splits = n_splits if n_splits > 0 else L.ebn_knn_topk_auto_splits(m.U, m.n_rows)
    ws = _workspace(L.ebn_knn_topk_workspace_bytes(m.U, k, splits))
    rc = L.ebn_knn_topk_f32(*m.head(), cand_pos, M, window, exclude, X, k, n_splits, P(pos), P(score), P(flags), P(ws), ws.numel(), m.U,
                            hip.stream_handle())
    assert rc == OK, rc
    torch.cuda.synchronize()
    h_pos.check("out_pos")
    h_score.check("out_score")
    return h_pos.payload().cpu().numpy(), h_score.payload().cpu().numpy(), flags.cpu().numpy()


def _run_rank(hip, m, cand_pos, M, target, window, exclude, X, n_splits):
    L = hip.lib()
    outs = [guarded.guard_out((m.U,), dtype=d) for d in (torch.int32, torch.int32, torch.float32)]
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    splits = n_splits if n_splits > 0 else L.ebn_knn_topk_auto_splits(m.U, m.n_rows)
    ws = _workspace(L.ebn_knn_target_rank_workspace_bytes(m.U, splits, 0 if cand_pos is None else M))
    rc = L.ebn_knn_target_rank_f32(*m.head(), cand_pos, M, target, window, exclude, X, n_splits, *[P(o[0]) for o in outs], P(flags), P(ws),
                                   ws.numel(), m.U, hip.stream_handle())
    assert rc == OK, rc
    torch.cuda.synchronize()
    for (_, h), what in zip(outs, ("out_rank", "out_count", "out_score")):
        h.check(what)
    return [h.payload().cpu().numpy() for _, h in outs] + [flags.cpu().numpy()]


def _grid(hip, c, front, full):
    """every combination for one index and one set of neighbour rows; ``full``: all of n_splits / k / X, else one of each"""
    m = _Index(c, front)
    n_rows, U = c["n_rows"], c["n_users"]
    chains = knn_mod.knn_chains_host(c["s_indptr"], c["s_items"], n_rows, c["item_scale"], c["nbr_seq"], c["nbr_sim"])
    twin = tc.twin_args(c)
    is_nan = bool(np.isnan(c["nbr_sim"]).any())
    seen = dict(flag0=set(), flag1=set(), short=0, launches=0)
    for pos_kind, X in itertools.product((None, "perm", "oob"), (0, 1, 256) if full else (1,)):
        cand_pos, M = tc.positions(n_rows, pos_kind)
        cp, h_cp = (None, None) if cand_pos is None else _i32(cand_pos, 0, front)
        exclude = tc.exclusions(c, X)
        ex, h_ex = (None, None) if exclude is None else _i32(exclude, c["special_col"], front)
        p_special = c["special_col"] if cand_pos is None else int(cand_pos[c["special_col"]])
        variants = [tc.windows(U, M)] + ([None] if X == 0 else []) + ([tc.windows(U, M, avoid=p_special)] if is_nan and X == 0 and 0 <= p_special < M else [])
        for window in variants:
            wd, h_wd = (None, None) if window is None else _i32(window, 0, front)
            w_pos, w_score, w_flags = knn_mod.knn_topk_host(*twin, cand_pos, M, window, exclude, 64, chains)
            target = tc.targets(w_pos, M, U)
            tg, h_tg = _i32(target, 0, front)
            w_rank = knn_mod.knn_target_rank_host(*twin, cand_pos, M, target, window, exclude, chains)
            seen["flag0"].add(int(w_flags[0]))
            seen["flag1"].add(int(w_flags[1]))
            seen["short"] += int(((w_pos >= 0).sum(1) < 5).sum())
            lists = {}
            for n_splits in (0, 1, 2, 64) if full else (2,):
                for k in (1, 5, 64) if full else (5, 64):
                    pos, score, flags = _run_topk(hip, m, cp, M, wd, ex, X, k, n_splits)
                    what = (pos_kind, X, window is None, n_splits, k)
                    assert np.array_equal(pos, w_pos[:, :k]), what
                    assert np.array_equal(_bits(score), _bits(w_score[:, :k])), what
                    assert np.array_equal(flags, w_flags), what
                    if k == 64:
                        lists[n_splits] = (pos, score)
                rank, count, t, flags = _run_rank(hip, m, cp, M, tg, wd, ex, X, n_splits)
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
    return seen


def _rows(hip, rows):
    R = int(hip.lib().ebn_knn_topk_range())
    return R, {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+37": 2 * R + 37}[rows]


@pytest.mark.parametrize("rows", ["1", "R-1", "R", "R+1", "2R+37"])
def test_lists_and_ranks_equal_the_twin_bit_for_bit(hip, rows):
    R, n_rows = _rows(hip, rows)
    c = tc.kernel_case(n_rows, R, 65, "random", True)
    seen = _grid(hip, c, front=0, full=True)
    _grid(hip, c, front=3, full=False)  # another placement of every operand
    assert seen["flag0"] == ({0, 1} if n_rows > 3 else {0}) and seen["short"] > 0 and seen["flag1"] == {0}


@pytest.mark.parametrize("k_nbr,sims,scaled", [(1, "random", True), (64, "integer", True), (65, "nan", False), (512, "random", False),
                                               (512, "nan", True)])
@pytest.mark.parametrize("rows", ["R+1", "2R+37"])
def test_every_neighbour_count_and_kind_of_sims(hip, rows, k_nbr, sims, scaled):
    R, n_rows = _rows(hip, rows)
    c = tc.kernel_case(n_rows, R, k_nbr, sims, scaled)
    seen = _grid(hip, c, front=0, full=rows == "R+1")
    if sims == "nan" and rows == "R+1":
        assert seen["flag1"] == {0, 1}  # the NaN inside a window; excluded, no candidate or outside every window


def test_user_hist_null_is_the_identity(hip):
    R, n_rows = _rows(hip, "R+1")
    c = tc.kernel_case(n_rows, R, 65, "random", True, identity=True)
    assert c["user_hist"] is None and c["n_users"] == c["nbr_seq"].shape[0]
    _grid(hip, c, front=0, full=False)


def test_the_chain_runs_in_list_order(hip):
    R, n_rows = _rows(hip, "R+1")
    c, forward = tc.order_case(n_rows, R)  # folded in reversed order the special row's sum has other bits (asserted there)
    m = _Index(c)
    only = np.tile(np.array([c["special_col"], c["special_col"] + 1], np.int32), (m.U, 1))  # a window of the special row alone
    wd, h_wd = _i32(only, 0)
    for n_splits in (1, 2):
        pos, score, _ = _run_topk(hip, m, None, n_rows, wd, None, 0, 64, n_splits)
        assert pos[1, 0] == c["special_col"] and pos[1, 1] == -1 and _bits(score[1, 0]) == _bits(forward), n_splits
        tg, h_tg = _i32(np.full(m.U, c["special_col"], np.int32), 0)
        rank, count, t, _ = _run_rank(hip, m, None, n_rows, tg, None, None, 0, n_splits)  # among all rows: the same chain, the same bits
        assert rank[1] >= 1 and count[1] > 64 and _bits(t[1]) == _bits(forward)
        h_tg.check("target_pos")
    h_wd.check("window")
    m.check()


def test_position_beyond_M_on_an_untouched_row_sets_no_flag(hip):
    # one neighbour whose set holds the rows 1 and 2; cand_pos sends the untouched row 3 beyond M and the touched row 2 to position 0
    c = dict(s_indptr=np.array([0, 2], np.int64), s_items=np.array([1, 2], np.int32), n_rows=4, n_seqs=1, item_scale=np.array([1, 0, -2, 1], np.float32),
             nbr_seq=np.array([[0]], np.int32), nbr_sim=np.array([[1.5]], np.float32), user_hist=np.array([0], np.int32), n_users=1,
             special_col=0, full_seq=0)
    m = _Index(c)
    for cand_pos, want_flag, want in (([2, 1, 0, 7], 0, [1, 0, -1]), ([2, 7, 0, -1], 1, [0, -1, -1])):
        cp, h = _i32(np.array(cand_pos, np.int32), 0)
        pos, score, flags = _run_topk(hip, m, cp, 3, None, None, 0, 3, 0)
        assert pos.tolist() == [want] and flags.tolist() == [want_flag, 0], cand_pos
        h.check("cand_pos")
    assert _bits(score[0, 0]) == _bits(np.float32(-3.0))  # touched rows with the scores 0 and -3 are listed, the untouched rows 0 and 3 are not
    m.check()


def test_two_runs_and_other_co_launched_users_give_the_same_bits(hip):
    R, n_rows = _rows(hip, "R+1")
    c = dict(tc.kernel_case(n_rows, R, 65, "random", True))
    first = _run_topk(hip, _Index(c), None, n_rows, None, None, 0, 64, 0)
    again = _run_topk(hip, _Index(c), None, n_rows, None, None, 0, 64, 0)
    assert np.array_equal(first[0], again[0]) and np.array_equal(_bits(first[1]), _bits(again[1]))
    keep = np.array([5, 2, 12, 4], np.int64)  # a subset, in another order: other users share the launch
    sub = dict(c, user_hist=c["user_hist"][keep], n_users=int(keep.size))
    other = _run_topk(hip, _Index(sub), None, n_rows, None, None, 0, 64, 2)
    assert np.array_equal(other[0], first[0][keep]) and np.array_equal(_bits(other[1]), _bits(first[1][keep]))
    target = np.ascontiguousarray(first[0][:, 1])
    tg, h_tg = _i32(target, 0)
    r_all = _run_rank(hip, _Index(c), None, n_rows, tg, None, None, 0, 0)
    tg_sub, h_sub = _i32(target[keep], 0)
    r_sub = _run_rank(hip, _Index(sub), None, n_rows, tg_sub, None, None, 0, 64)
    for a, b in zip(r_all[:3], r_sub[:3]):
        assert np.array_equal(_bits(a[keep]) if a.dtype == np.float32 else a[keep], _bits(b) if b.dtype == np.float32 else b)
    h_tg.check("target_pos")
    h_sub.check("target_pos")


def test_argument_checks_return_codes_and_write_nothing(hip):
    L, st = hip.lib(), hip.stream_handle()
    R = int(L.ebn_knn_topk_range())
    c = tc.kernel_case(R + 1, R, 65, "random", True)
    m = _Index(c)
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
    base = dict(cand_pos=cp, M=M, window=wd, exclude=ex, X=4, k=5, n_splits=2, ws=P(ws), ws_bytes=ws.numel(), U=U)

    def topk(**k):
        a = dict(base, **k)
        return L.ebn_knn_topk_f32(*m.head(**k), a["cand_pos"], a["M"], a["window"], a["exclude"], a["X"], a["k"], a["n_splits"],
                                  a.get("pos", P(pos)), a.get("score", P(score)), a.get("flags", P(flags)), a["ws"], a["ws_bytes"], a["U"], st)

    def rnk(**k):
        a = dict(base, **k)
        return L.ebn_knn_target_rank_f32(*m.head(**k), a["cand_pos"], a["M"], a.get("target", tg), a["window"], a["exclude"], a["X"],
                                         a["n_splits"], a.get("rank", P(rank)), a.get("count", P(count)), a.get("t", P(t)),
                                         a.get("flags", P(flags)), a["ws"], a["ws_bytes"], a["U"], st)

    before = L.ebn_launch_count()
    bad = [dict([(n, v)]) for n in ("n_seqs", "nnz_s", "n_rows", "n_hists", "M", "U") for v in (-1, big)]
    bad += [dict(X=-1), dict(n_splits=-1), dict(ws_bytes=-1), dict(k_nbr=0), dict(k_nbr=-1), dict(cand_pos=None), dict(flags=None),
            dict(s_indptr=None), dict(s_items=None), dict(nbr_seq=None), dict(nbr_sim=None), dict(ws=None), dict(ws_bytes=15)]
    for kw in bad:
        assert topk(**kw) == BAD_ARG, kw
        assert rnk(**kw) == BAD_ARG, kw
    for kw in (dict(pos=None), dict(score=None)):
        assert topk(**kw) == BAD_ARG, kw
    for kw in (dict(target=None), dict(rank=None), dict(count=None), dict(t=None)):
        assert rnk(**kw) == BAD_ARG, kw
    for kw in (dict(k=0), dict(k=65), dict(X=257), dict(k_nbr=513)):
        assert topk(**kw) == UNSUPPORTED, kw
        assert topk(n_splits=-3, **kw) == BAD_ARG, kw  # BAD_ARG comes first
    assert rnk(X=257) == UNSUPPORTED and rnk(k_nbr=513) == UNSUPPORTED and rnk(X=257, U=-1) == BAD_ARG
    odd = ctypes.c_void_p(ws.data_ptr() + 4)
    assert topk(ws=odd) == ALIGN and rnk(ws=odd) == ALIGN
    assert topk(ws_bytes=L.ebn_knn_topk_workspace_bytes(U, 5, 2) - 1) == BAD_ARG
    assert rnk(ws_bytes=L.ebn_knn_target_rank_workspace_bytes(U, 2, M) - 1) == BAD_ARG
    assert rnk(n_splits=1, ws=None) == BAD_ARG and rnk(n_splits=1, ws_bytes=L.ebn_knn_target_rank_workspace_bytes(U, 1, M) - 1) == BAD_ARG  # the inverse of cand_pos
    # U == 0: nothing to do, nothing is needed
    assert topk(U=0, pos=None, score=None, flags=None, ws=None, ws_bytes=0) == OK and rnk(U=0, target=None, rank=None, ws=None, ws_bytes=0) == OK
    assert L.ebn_launch_count() == before
    torch.cuda.synchronize()
    for h, what in ((h_pos, "out_pos"), (h_score, "out_score"), (h_rank, "out_rank"), (h_count, "out_count"), (h_t, "out_score"),
                    (h_flags, "flags")):
        h.check_untouched(what)
    # the empty index and the empty candidate list: empty outputs in one launch, no workspace and no index needed
    legal = (dict(n_rows=0, M=0, cand_pos=None), dict(nnz_s=0, s_items=None), dict(M=0), dict(n_seqs=0, s_indptr=None),
             dict(n_rows=0, M=0, nnz_s=0, n_seqs=0, cand_pos=None, s_indptr=None, s_items=None, nbr_seq=None, nbr_sim=None, ws=None, ws_bytes=0))
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


def test_fitted_class_on_the_device_equals_the_host_path():
    from ebrec.models import HistoryKNN
    from tests import knn_cases as kc

    seqs = kc.random_sequences(11, n_seqs=300, n_ids=90, longest=14)
    keys = np.arange(len(seqs))
    dev = HistoryKNN(k=20, sample_size=60, idf=True, device="cuda").fit(seqs, keys=keys)
    assert dev.index.on_device
    host = HistoryKNN(k=20, sample_size=60, idf=True, device=None)
    host.index = knn_mod.KNNIndex(dev.index.article_ids, *dev.index.host(), dev.index.sequence_of, dev.index.keys)  # one fitted state
    hists = seqs[:50] + [[], [7]]
    hkeys = np.concatenate([keys[:50], [-1, -2]])
    for kw in (dict(), dict(exclude_history=False, candidate_ids=dev.index.article_ids[::-1][:70])):
        d_ids, d_scores = dev.recommend(hists, top_n=10, return_scores=True, history_keys=hkeys, batch_users=17, **kw)
        h_ids, h_scores = host.recommend(hists, top_n=10, return_scores=True, history_keys=hkeys, **kw)
        assert np.array_equal(d_ids, h_ids) and np.array_equal(_bits(d_scores.cpu().numpy()), _bits(h_scores)) and (h_ids >= 0).any()
        targets = [[int(h_ids[i, i % 10]), int(dev.index.article_ids[(7 * i) % 90])] for i in range(len(hists))]
        d, h = (m.rank_targets(hists, targets=targets, history_keys=hkeys, **kw) for m in (dev, host))
        assert np.array_equal(d.rank, h.rank) and np.array_equal(d.count, h.count) and np.array_equal(_bits(d.score), _bits(h.score))
        assert (h.rank > 0).any()
