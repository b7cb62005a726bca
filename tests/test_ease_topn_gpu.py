"""ebn_ease_topk_f32 / ebn_ease_target_rank_f32 (csrc/ebn_ease_topk.hip) through the C ABI on guard-banded operands, BITWISE against
the float32 twins of ebrec/models/baselines/ease.py (which tests/test_ease_topn_cpu.py holds against the plain-Python brute force):
the positions, and the scores as int32 views -- there is no tolerance.

Operands as in tests/test_covisit_topn_gpu.py (tests/guarded.py): B as rows of n_rows payload columns at row stride ldb inside 3e18,
int64 arrays as pairs of int32 words inside zero words, index arrays inside VALID indices (an over-read entry is used and shows),
weights inside 3e18, outputs in canary buffers: guards intact, every payload element written.

One test case = (n_rows, values, weights).  Inside it B is placed four ways -- ldb = n_rows rounded up to 4 (16-byte loads), ldb =
n_rows (16-byte loads only when n_rows is a multiple of 4), ldb = n_rows rounded up to 4, + 4, and 4 bytes off a 16-byte boundary (the
4-byte path) -- and at every placement EVERY combination of cand_pos (NULL, a permutation, one with negative and >= M entries),
X in {0, 1, 256}, n_splits in {0, 1, 2, 64} and k in {1, 5, 64} is launched; at the last placement every other operand is moved as
well (front = 3).  The users of a launch carry the histories of tests/ease_topn_cases.py and the windows (full,
empty, clamped, lo >= hi, inner; none at all with X = 0).  The rank kernel gets the same grid, against its twin and against the top-k
kernel's own k = 64 lists."""
import ctypes
import itertools

import numpy as np
import pandas as pd
import pytest
import torch

from ebrec.models import EASE
from ebrec.models.baselines import ease as ez
from tests import ease_topn_cases as tc
from tests import guarded

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3
POISON = 3.0e18
GUARD = 4096
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
pad4 = lambda n: (n + 3) // 4 * 4
PLACEMENTS = (("pad4", 0, 0), ("n", 0, 0), ("pad4+4", 0, 0), ("pad4", 1, 3))  # (ldb, floats off a 16-byte boundary, front of the others)


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
    view, h = guarded.guard_in(np.concatenate([np.full(front, POISON, np.float32), np.asarray(x, np.float32)]), fill=POISON, guard=GUARD)
    return ctypes.c_void_p(view.data_ptr() + 4 * front), h


class _Operands:
    """the guarded matrix and histories of one case at one placement"""

    def __init__(self, c, ld="pad4", offset=0, front=0):
        self.c, self.h = c, {}
        n = self.n_rows = c["n_rows"]
        self.ldb = {"n": n, "pad4": pad4(n), "pad4+4": pad4(n) + 4}[ld]
        view, self.h["B"] = guarded.guard_in(c["B"], ld=self.ldb, fill=POISON, offset=offset)
        self.B = ctypes.c_void_p(view.data_ptr())
        self.n_hists, self.n_hist_items, self.U = c["hist_offsets"].size - 1, c["hist_rows"].size, c["n_users"]
        self.hist_rows, self.h["hist_rows"] = _i32(c["hist_rows"], c["special_row"], front)  # a valid row
        self.hist_weights = None
        if c["hist_weights"] is not None:
            self.hist_weights, self.h["hist_weights"] = _f32(c["hist_weights"], front)
        self.hist_offsets, self.h["hist_offsets"] = _i64(c["hist_offsets"], front)
        self.user_hist, self.h["user_hist"] = _i32(c["user_hist"], 9, front)  # a valid history: the longest

    def head(self, **k):
        names = ("B", "n_rows", "ldb", "hist_rows", "hist_weights", "hist_offsets", "n_hists", "n_hist_items", "user_hist")
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
    splits = n_splits if n_splits > 0 else L.ebn_ease_topk_auto_splits(m.U, m.n_rows)
    ws = _workspace(L.ebn_ease_topk_workspace_bytes(m.U, k, splits))
    rc = L.ebn_ease_topk_f32(*m.head(), cand_pos, M, window, exclude, X, k, n_splits, P(pos), P(score), P(flags), P(ws), ws.numel(), m.U,
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
    splits = n_splits if n_splits > 0 else L.ebn_ease_topk_auto_splits(m.U, m.n_rows)
    ws = _workspace(L.ebn_ease_target_rank_workspace_bytes(m.U, splits, 0 if cand_pos is None else M))
    rc = L.ebn_ease_target_rank_f32(*m.head(), cand_pos, M, target, window, exclude, X, n_splits, *[P(o[0]) for o in outs], P(flags), P(ws),
                                    ws.numel(), m.U, hip.stream_handle())
    assert rc == OK, rc
    torch.cuda.synchronize()
    for (_, h), what in zip(outs, ("out_rank", "out_count", "out_score")):
        h.check(what)
    return [h.payload().cpu().numpy() for _, h in outs] + [flags.cpu().numpy()]


def _grid(hip, c, chains, ld, offset, front):
    """every combination for one matrix and history set at one placement"""
    m = _Operands(c, ld, offset, front)
    n_rows, U = c["n_rows"], c["n_users"]
    twin = (c["B"], c["hist_rows"], c["hist_weights"], c["hist_offsets"], c["user_hist"], U)
    is_nan = bool(np.isnan(c["B"]).any())
    seen = dict(flag0=set(), flag1=set(), short=0)
    for pos_kind, X in itertools.product((None, "perm", "oob"), (0, 1, 256)):
        cand_pos, M = tc.positions(n_rows, pos_kind)
        cp, h_cp = (None, None) if cand_pos is None else _i32(cand_pos, 0, front)
        exclude = tc.exclusions(c, X)
        ex, h_ex = (None, None) if exclude is None else _i32(exclude, c["special_col"], front)
        p_special = c["special_col"] if cand_pos is None else int(cand_pos[c["special_col"]])
        variants = [tc.windows(U, M)] + ([None] if X == 0 else []) + ([tc.windows(U, M, avoid=p_special)] if is_nan and X == 0 else [])
        for window in variants:
            wd, h_wd = (None, None) if window is None else _i32(window, 0, front)
            w_pos, w_score, w_flags = ez.ease_topk_host(*twin, cand_pos, M, window, exclude, 64, chains)
            target = tc.targets(w_pos, M, U)
            tg, h_tg = _i32(target, 0, front)
            w_rank = ez.ease_target_rank_host(*twin, cand_pos, M, target, window, exclude, chains)
            seen["flag0"].add(int(w_flags[0]))
            seen["flag1"].add(int(w_flags[1]))
            seen["short"] += int(((w_pos >= 0).sum(1) < 5).sum())
            lists = {}
            for n_splits in (0, 1, 2, 64):
                for k in (1, 5, 64):
                    pos, score, flags = _run_topk(hip, m, cp, M, wd, ex, X, k, n_splits)
                    what = (ld, offset, pos_kind, X, window is None, n_splits, k)
                    assert np.array_equal(pos, w_pos[:, :k]), what
                    assert np.array_equal(_bits(score), _bits(w_score[:, :k])), what
                    assert np.array_equal(flags, w_flags), what
                    if k == 64:
                        lists[n_splits] = (pos, score)
                rank, count, t, flags = _run_rank(hip, m, cp, M, tg, wd, ex, X, n_splits)
                for g, w, name in zip((rank, count, _bits(t), flags), (w_rank[0], w_rank[1], _bits(w_rank[2]), w_rank[3]), ("rank", "count", "t", "flags")):
                    assert np.array_equal(g, w), (name, ld, offset, pos_kind, X, window is None, n_splits)
                # against the top-k kernel's own lists: a rank within 64 is that slot, with that slot's score bits
                pos64, score64 = lists[n_splits]
                for u in np.flatnonzero((rank >= 1) & (rank <= 64)):
                    assert pos64[u, rank[u] - 1] == target[u] and _bits(score64[u, rank[u] - 1]) == _bits(t[u])
                assert np.array_equal(count >= 64, pos64[:, 63] >= 0)
            assert all(np.array_equal(a[0], lists[2][0]) and np.array_equal(_bits(a[1]), _bits(lists[2][1])) for a in lists.values())
            for h, what in ((h_wd, "window"), (h_tg, "target_pos")):
                if h is not None:
                    h.check(what)
        for h, what in ((h_cp, "cand_pos"), (h_ex, "exclude")):
            if h is not None:
                h.check(what)
    m.check()
    return seen


CASES = [(rows, values, weights) for rows in tc.ROWS for values in tc.VALUES for weights in tc.WEIGHTS[values]]


@pytest.mark.parametrize("rows,values,weights", CASES)
def test_lists_and_ranks_equal_the_twin_bit_for_bit(hip, rows, values, weights):
    assert int(hip.lib().ebn_ease_topk_range()) == tc.R
    n_rows = tc.ROWS[rows]
    c = tc.kernel_case(n_rows, values, weights)
    chains = ez.ease_chains_host(c["B"], c["hist_rows"], c["hist_weights"], c["hist_offsets"])
    for i, (ld, offset, front) in enumerate(PLACEMENTS):
        seen = _grid(hip, c, chains, ld, offset, front)
        if i == 0:
            assert seen["flag0"] == ({0, 1} if n_rows > 3 else {0}) and seen["short"] > 0
            if values == "nan" and n_rows > 1:
                assert seen["flag1"] == {0, 1}  # the NaN inside a window, and outside every window


def test_two_runs_and_other_co_launched_users_give_the_same_bits(hip):
    R = tc.R
    c = dict(tc.kernel_case(R + 1, "normal", "negative"))
    first = _run_topk(hip, _Operands(c), None, R + 1, None, None, 0, 64, 0)
    again = _run_topk(hip, _Operands(c), None, R + 1, None, None, 0, 64, 0)
    assert np.array_equal(first[0], again[0]) and np.array_equal(_bits(first[1]), _bits(again[1]))
    keep = np.array([9, 2, 12, 4], np.int64)  # a subset, in another order: other users share the launch
    sub = dict(c, user_hist=c["user_hist"][keep], n_users=int(keep.size))
    other = _run_topk(hip, _Operands(sub, "n", 1), None, R + 1, None, None, 0, 64, 2)  # and B on the 4-byte path
    assert np.array_equal(other[0], first[0][keep]) and np.array_equal(_bits(other[1]), _bits(first[1][keep]))
    target = np.ascontiguousarray(first[0][:, 1])
    tg, h_tg = _i32(target, 0)
    r_all = _run_rank(hip, _Operands(c), None, R + 1, tg, None, None, 0, 0)
    tg_sub, h_sub = _i32(target[keep], 0)
    r_sub = _run_rank(hip, _Operands(sub), None, R + 1, tg_sub, None, None, 0, 64)
    for a, b in zip(r_all[:3], r_sub[:3]):
        assert np.array_equal(_bits(a[keep]) if a.dtype == np.float32 else a[keep], _bits(b) if b.dtype == np.float32 else b)
    assert np.array_equal(r_all[0][first[0][:, 1] >= 0], np.full(int((first[0][:, 1] >= 0).sum()), 2))
    h_tg.check("target_pos")
    h_sub.check("target_pos")


def test_argument_checks_return_codes_and_write_nothing(hip):
    L, st = hip.lib(), hip.stream_handle()
    R = int(L.ebn_ease_topk_range())
    c = tc.kernel_case(R + 1, "normal", "positive")
    m = _Operands(c)
    U, n_rows, big = m.U, m.n_rows, 2 ** 31
    cand_pos, M = tc.positions(n_rows, "oob")  # M != n_rows: cand_pos is needed
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
        return L.ebn_ease_topk_f32(*m.head(**k), a["cand_pos"], a["M"], a["window"], a["exclude"], a["X"], a["k"], a["n_splits"],
                                   a.get("pos", P(pos)), a.get("score", P(score)), a.get("flags", P(flags)), a["ws"], a["ws_bytes"], a["U"], st)

    def rnk(**k):
        a = dict(base, **k)
        return L.ebn_ease_target_rank_f32(*m.head(**k), a["cand_pos"], a["M"], a.get("target", tg), a["window"], a["exclude"], a["X"],
                                          a["n_splits"], a.get("rank", P(rank)), a.get("count", P(count)), a.get("t", P(t)),
                                          a.get("flags", P(flags)), a["ws"], a["ws_bytes"], a["U"], st)

    before = L.ebn_launch_count()
    bad = [dict([(n, v)]) for n in ("n_rows", "ldb", "n_hists", "n_hist_items", "M", "U") for v in (-1, big)]
    bad += [dict(X=-1), dict(n_splits=-1), dict(ws_bytes=-1), dict(ldb=n_rows - 1), dict(n_hists=0), dict(cand_pos=None), dict(flags=None),
            dict(B=None), dict(hist_rows=None), dict(hist_offsets=None), dict(ws=None), dict(ws_bytes=15)]
    for kw in bad:
        assert topk(**kw) == BAD_ARG, kw
        assert rnk(**kw) == BAD_ARG, kw
    for kw in (dict(pos=None), dict(score=None)):
        assert topk(**kw) == BAD_ARG, kw
    for kw in (dict(target=None), dict(rank=None), dict(count=None), dict(t=None)):
        assert rnk(**kw) == BAD_ARG, kw
    too_many = dict(n_rows=32769, ldb=32772, cand_pos=cp)
    for kw in (dict(k=0), dict(k=65), dict(X=257), too_many):
        assert topk(**kw) == UNSUPPORTED, kw
        assert topk(n_splits=-1, **kw) == BAD_ARG, kw  # BAD_ARG comes first
    assert rnk(X=257) == UNSUPPORTED and rnk(X=257, U=-1) == BAD_ARG and rnk(**too_many) == UNSUPPORTED
    assert topk(k=65, pos=None) == UNSUPPORTED and topk(k=65, U=0) == UNSUPPORTED  # UNSUPPORTED before the NULL outputs and U == 0
    odd = ctypes.c_void_p(ws.data_ptr() + 4)
    assert topk(ws=odd) == ALIGN and rnk(ws=odd) == ALIGN
    assert topk(ws_bytes=L.ebn_ease_topk_workspace_bytes(U, 5, 2) - 1) == BAD_ARG
    assert rnk(ws_bytes=L.ebn_ease_target_rank_workspace_bytes(U, 2, M) - 1) == BAD_ARG
    assert rnk(n_splits=1, ws=None) == BAD_ARG and rnk(n_splits=1, ws_bytes=L.ebn_ease_target_rank_workspace_bytes(U, 1, M) - 1) == BAD_ARG  # the inverse of cand_pos
    # U == 0: nothing to do, nothing is needed
    assert topk(U=0, pos=None, score=None, flags=None, ws=None, ws_bytes=0) == OK and rnk(U=0, target=None, rank=None, ws=None, ws_bytes=0) == OK
    assert L.ebn_launch_count() == before
    torch.cuda.synchronize()
    for h, what in ((h_pos, "out_pos"), (h_score, "out_score"), (h_rank, "out_rank"), (h_count, "out_count"), (h_t, "out_score"),
                    (h_flags, "flags")):
        h.check_untouched(what)
    # the empty matrix and the empty candidate list: empty outputs in one launch, no workspace and no matrix needed; NULL outputs
    # are still BAD_ARG there
    assert topk(M=0, pos=None) == BAD_ARG and rnk(M=0, target=None) == BAD_ARG
    legal = (dict(n_rows=0, ldb=0, M=0, cand_pos=None, B=None), dict(M=0), dict(n_rows=0, ldb=5, M=0, cand_pos=None, B=None, ws=None, ws_bytes=0))
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
        assert f2.tolist() == [1, 0], kw  # a target position >= M (= 0) is reported
    assert L.ebn_launch_count() == before + 2 * len(legal)
    m.check()
    for h, what in ((h_cp, "cand_pos"), (h_wd, "window"), (h_ex, "exclude"), (h_tg, "target_pos"), (h_tg2, "target_pos")):
        h.check(what)


def test_device_model_equals_the_host_model_over_its_own_weights():
    from pathlib import Path

    from ebrec.evaluation.freshness import Freshness
    from ebrec.utils import _constants as C

    golden = Path(__file__).resolve().parents[1] / "tests" / "golden" / "ebnerd"
    df, hist = pd.read_parquet(golden / "behaviors.parquet").head(200), pd.read_parquet(golden / "history.parquet")
    for hw in (None, "exponential"):
        dev = EASE(regularization=20.0, device="cuda", history_weights=hw).fit(hist)
        assert not isinstance(dev.weights, np.ndarray) and dev.weights.stride(0) == pad4(dev.article_ids.size)
        host = EASE.from_weights(dev.article_ids, dev.weights, device=None, history_weights=hw)
        assert isinstance(host.weights, np.ndarray)
        t0 = df[C.DEFAULT_IMPRESSION_TIMESTAMP_COL].min()
        rng = np.random.default_rng(3)
        published = {int(a): t0 - pd.Timedelta(hours=int(h)) for a, h in zip(dev.article_ids, rng.integers(1, 14 * 24, dev.article_ids.size))}
        for kw in (dict(), dict(exclude_history=False), dict(candidate_ids=dev.article_ids[::3][::-1]),
                   dict(window=Freshness(published, max_age=pd.Timedelta(days=9), min_age=pd.Timedelta(hours=2)))):
            d_ids, d_scores = dev.recommend(df, history=hist, top_n=10, return_scores=True, **kw)
            h_ids, h_scores = host.recommend(df, history=hist, top_n=10, return_scores=True, **kw)
            assert d_scores.is_cuda and np.array_equal(d_ids, h_ids) and np.array_equal(_bits(d_scores.cpu().numpy()), _bits(h_scores)), (hw, list(kw))
            assert (d_ids >= 0).any()
            targets = [[int(d_ids[i, i % 10]), int(dev.article_ids[(37 * i) % dev.article_ids.size])] for i in range(len(df))]
            d_r, h_r = dev.rank_targets(df, targets=targets, history=hist, **kw), host.rank_targets(df, targets=targets, history=hist, **kw)
            assert np.array_equal(d_r.rank, h_r.rank) and np.array_equal(d_r.count, h_r.count) and np.array_equal(_bits(d_r.score), _bits(h_r.score))
            assert (d_r.rank > 0).any()
