"""ebn_npa_topk_score_f32 (csrc/ebn_npa_topk.hip) and NPAModel.recommend_pairwise on the GPU, against the float64 restatement
of tests/npa_recommend_cases.py, against ebn_pap_indexed_f32 and against scorer.predict."""
import numpy as np
import pytest
import torch

from tests import npa_recommend_cases as nc
from tests.guarded import guard_in
from tests.hip_testutil import P, S, dev
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)

pytestmark = pytest.mark.gpu

OK = 0
SHAPE_IDS = lambda s: "x".join(map(str, s))  # noqa: E731


def run_npa_topk(hip, c, k=None, mode=0, n_splits=0, cand_rows="case", exclude="case", operands=None):
    """-> (pos [U, k] int32, score [U, k] float32, flags [2]) as numpy arrays for a case of npa_recommend_cases.case();
    operands: device tensors (users, Q, Ua, Vd) to use in place of the case's (the guarded ones)"""
    k = c["k"] if k is None else k
    cand_rows = c["cand_rows"] if isinstance(cand_rows, str) else cand_rows
    exclude = c["exclude"] if isinstance(exclude, str) else exclude
    U, F = c["users"].shape
    n_rows, L, A = c["Ua"].shape
    M = n_rows if cand_rows is None else len(cand_rows)
    users_d, Q_d, Ua_d, Vd_d = operands if operands is not None else (dev(c["users"]), dev(c["Q"]), dev(c["Ua"]), dev(c["Vd"]))
    cand_d = None if cand_rows is None else dev(cand_rows, torch.int32)
    ex_d = None if exclude is None else dev(exclude, torch.int32)
    X = 0 if exclude is None else exclude.shape[1]
    pos_d = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
    score_d = torch.full((U, k), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    splits = n_splits if n_splits > 0 else int(hip.lib().ebn_npa_topk_auto_splits(U, M, L))
    ws_bytes = int(hip.lib().ebn_topk_workspace_bytes(U, k, splits))
    assert ws_bytes > 0
    ws_d = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    code = hip.lib().ebn_npa_topk_score_f32(P(users_d), P(Q_d), P(Ua_d), P(Vd_d), n_rows, P(cand_d), M, P(ex_d), X, k, mode, n_splits,
                                            P(pos_d), P(score_d), P(flags_d), P(ws_d), ws_bytes, U, L, F, A, S())
    assert code == OK, code
    torch.cuda.synchronize()
    return pos_d.cpu().numpy(), score_d.cpu().numpy(), flags_d.cpu().numpy()


def check_lists(pos, score, s64, k, tol, cand_rows, n_rows, exclude):
    """The properties of a result against the float64 scores s64 [U, M]; returns the largest |score - float64| seen"""
    U, M = s64.shape
    rows = np.arange(M) if cand_rows is None else np.asarray(cand_rows, dtype=np.int64)
    worst = 0.0
    for u in range(U):
        ok = (rows >= 0) & (rows < n_rows)
        if exclude is not None:
            ok &= ~np.isin(rows, exclude[u])
        n_kept = min(k, int(ok.sum()))
        p, s = pos[u, :n_kept].astype(np.int64), score[u, :n_kept]
        assert (pos[u, n_kept:] == -1).all() and np.isneginf(score[u, n_kept:]).all(), u  # the empty trailing slots
        assert (p >= 0).all() and (p < M).all() and len(set(p.tolist())) == n_kept, u  # no position twice
        assert ok[p].all(), (u, "an excluded or out-of-range candidate was kept")
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (p[:-1] < p[1:]))).all(), (u, "order: score descending, position ascending")
        if n_kept == 0:
            continue
        dev_ = np.abs(s.astype(np.float64) - s64[u, p])
        worst = max(worst, float(dev_.max()))
        assert (dev_ <= tol).all(), (u, dev_.max(), tol)
        left = ok.copy()
        left[p] = False
        if left.any():
            assert n_kept == k and s64[u, left].max() <= s64[u, p[-1]] + 2 * tol, (u, "an admissible candidate left out beats the k-th kept")
    return worst


# ------------------------------------------------------------------------------------------------ properties against float64
@pytest.mark.parametrize("exclude", [None, "x3"])
@pytest.mark.parametrize("cand", ["null", "subset"])
@pytest.mark.parametrize("shape", nc.SHAPES, ids=SHAPE_IDS)
def test_lists_by_properties_against_float64(hip, shape, cand, exclude):
    """tol = 1e-4 max|score64| + 1e-6: the project's tolerance for this score against float64.  Flags (0, 0); ordered lists; no
    position twice, no excluded row; every returned score within tol of the float64 score of the returned candidate; nothing
    admissible left out beats the k-th kept by more than 2 tol; sigmoid mode keeps the positions.
    The 1 x 1 shape has ONE score, so its spread is 0 by construction: there the score itself must be off zero."""
    c = nc.case(shape, seed=sum(shape), cand=cand, exclude=exclude)
    s64 = nc.pair_scores64(c["users"], c["Q"], c["Ua"], c["Vd"], c["cand_rows"])
    tol = nc.tolerance(s64)
    pos, score, flags = run_npa_topk(hip, c)
    kept = pos >= 0
    seen = np.abs(score[kept] - np.take_along_axis(s64, np.maximum(pos, 0).astype(np.int64), 1)[kept])
    print(f"shape {shape} cand {cand} exclude {exclude}: tol {tol:.3e}, max |score - float64| = {seen.max() if seen.size else 0.0:.3e}")
    assert tuple(flags) == (0, 0)
    if s64.size > 1:
        assert np.ptp(s64) > 1e-2
    else:
        assert abs(s64[0, 0]) > 1e-2
    check_lists(pos, score, s64, c["k"], tol, c["cand_rows"], c["n_rows"], c["exclude"])
    pos1, score1, flags1 = run_npa_topk(hip, c, mode=1)
    assert np.array_equal(pos1, pos) and tuple(flags1) == (0, 0)
    want = 1.0 / (1.0 + np.exp(-score[kept].astype(np.float64)))
    assert np.isneginf(score1[~kept]).all() and (np.abs(score1[kept] - want) <= 4 * 2.0 ** -23 * want).all()


# ------------------------------------------------------------------------------------------------ ties, position independence
@pytest.mark.parametrize("shape", [nc.SHAPES[2], nc.SHAPES[4]], ids=SHAPE_IDS)
def test_duplicate_rows_tie_bit_for_bit_and_a_permutation_only_permutes_positions(hip, shape):
    """cand_rows repeats every row several times: the duplicates of a kept row carry bit-equal scores and are ordered by position;
    permuting cand_rows permutes out_pos and leaves every kept (row, score bits) pair unchanged -- a pair's bits do not depend on
    where the candidate stands."""
    U, M, L, F, A, _k = shape
    k = 40
    c = nc.case(shape, seed=21, cand="subset")
    rng = np.random.default_rng(22)
    cand_rows = rng.integers(0, 12, M).astype(np.int32)  # 12 distinct rows, each about M / 12 times
    pos, score, flags = run_npa_topk(hip, c, k=k, cand_rows=cand_rows, exclude=None)
    assert tuple(flags) == (0, 0) and (pos >= 0).all()
    bits = score.view(np.int32)
    rows = cand_rows[pos]
    n_dup = 0
    for u in range(U):
        for r in np.unique(rows[u]):
            at = np.flatnonzero(rows[u] == r)
            assert len(set(bits[u, at].tolist())) == 1, (u, r)  # duplicates of a row: the same bits
            assert (np.diff(at) == 1).all() and (np.diff(pos[u, at]) > 0).all(), (u, r)  # adjacent, by position ascending
            n_dup += len(at) > 1
    assert n_dup > U  # the case exercises the tie rule
    perm = rng.permutation(M)
    pos2, score2, flags2 = run_npa_topk(hip, c, k=k, cand_rows=cand_rows[perm], exclude=None)
    assert tuple(flags2) == (0, 0)
    rows2 = cand_rows[perm][pos2]
    # ties are between duplicates of one row, so the kept (row, bits) sequence is the same; the positions are the permuted ones
    assert np.array_equal(rows2, rows) and np.array_equal(score2.view(np.int32), bits)
    for u in range(U):
        for r in np.unique(rows[u]):
            at = np.flatnonzero(rows[u] == r)
            # the kept duplicates of r are its first len(at) positions in each order
            assert np.array_equal(pos[u, at], np.flatnonzero(cand_rows == r)[:len(at)])
            assert np.array_equal(pos2[u, at], np.flatnonzero(cand_rows[perm] == r)[:len(at)])


# ------------------------------------------------------------------------------------------------ split invariance
@pytest.mark.parametrize("shape", nc.SPLIT_SHAPES, ids=SHAPE_IDS)
def test_every_split_and_every_run_gives_the_same_bits(hip, shape):
    c = nc.case(shape, seed=5, cand="subset", exclude="x3")
    runs = {s: run_npa_topk(hip, c, mode=1, n_splits=s) for s in (1, 2, 3, 64, 0)}
    again = run_npa_topk(hip, c, mode=1, n_splits=3)
    for s, (pos, score, flags) in list(runs.items()) + [("again", again)]:
        assert np.array_equal(pos, runs[1][0]), s
        assert np.array_equal(score.view(np.int32), runs[1][1].view(np.int32)), s
        assert tuple(flags) == (0, 0)
    assert (runs[1][0] >= 0).all()


# ------------------------------------------------------------------------------------------------ the existing kernel
def test_kept_scores_agree_with_the_indexed_pooling_kernel(hip):
    """At the real widths: the kept pairs scored by ebn_pap_indexed_f32 (mode 0), which pools first and dots second.  Both are within
    tol of float64, so they agree within 2 tol."""
    shape = nc.SHAPES[-1]
    c = nc.case(shape, seed=9, cand="subset")
    s64 = nc.pair_scores64(c["users"], c["Q"], c["Ua"], c["Vd"], c["cand_rows"])
    tol = nc.tolerance(s64)
    pos, score, flags = run_npa_topk(hip, c)
    assert tuple(flags) == (0, 0) and (pos >= 0).all()
    U, k = pos.shape
    n_rows, L, A = c["Ua"].shape
    F = c["Vd"].shape[2]
    rows = c["cand_rows"][pos.reshape(-1)]
    q_idx = np.repeat(np.arange(U), k)
    out = torch.full((U * k,), float("nan"), device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.call("ebn_pap_indexed_f32", P(dev(c["Ua"])), P(dev(c["Vd"])), n_rows, P(dev(rows, torch.int32)), P(dev(c["Q"])),
             P(dev(q_idx, torch.int32)), U, None, P(dev(c["users"])), P(out), 0, P(flag), U * k, L, F, A, S())
    torch.cuda.synchronize()
    other = out.cpu().numpy().reshape(U, k)
    diff = np.abs(other.astype(np.float64) - score)
    print(f"fused vs ebn_pap_indexed_f32 on the kept pairs: max |difference| = {diff.max():.3e} (2 tol = {2 * tol:.3e})")
    assert int(flag.item()) == 0 and np.isfinite(other).all()
    assert (diff <= 2 * tol).all()


# ------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("cand", ["null", "subset"])
def test_operands_between_nan_guards(hip, cand):
    """Ua_all, Vd_all, users and Q inside NaN guards (L = 30: two padded token rows per candidate; U = 65: 63 user columns past the
    last): a kernel that reads a padded token row, or past the last user, picks up a NaN and raises flags[1]."""
    shape = nc.SHAPES[2]
    c = nc.case(shape, seed=13, cand=cand, exclude="x3")
    n_rows, L, A = c["Ua"].shape
    F = c["Vd"].shape[2]
    Ua_d, hU = guard_in(c["Ua"].reshape(n_rows * L, A))
    Vd_d, hV = guard_in(c["Vd"].reshape(n_rows * L, F))
    us_d, hu = guard_in(c["users"])
    Q_d, hQ = guard_in(c["Q"])
    want = run_npa_topk(hip, c)
    pos, score, flags = run_npa_topk(hip, c, operands=(us_d, Q_d, Ua_d, Vd_d))
    assert tuple(flags) == (0, 0) and np.isfinite(score[pos >= 0]).all()
    assert np.array_equal(pos, want[0]) and np.array_equal(score.view(np.int32), want[1].view(np.int32))
    s64 = nc.pair_scores64(c["users"], c["Q"], c["Ua"], c["Vd"], c["cand_rows"])
    check_lists(pos, score, s64, c["k"], nc.tolerance(s64), c["cand_rows"], c["n_rows"], c["exclude"])
    for h, what in ((hU, "Ua_all"), (hV, "Vd_all"), (hu, "users"), (hQ, "Q")):
        h.check(what)


# ------------------------------------------------------------------------------------------------ flags and edges
def test_rows_outside_the_catalogue_are_skipped_and_flagged(hip):
    c = nc.case(nc.SHAPES[2], seed=17, cand="subset")
    k, n_rows = c["k"], c["n_rows"]
    clean = run_npa_topk(hip, c)
    bad = c["cand_rows"].copy()
    where = [3, 64, 129]
    bad[where] = [-1, n_rows, n_rows + 1]
    pos, score, flags = run_npa_topk(hip, c, cand_rows=bad)
    assert tuple(clean[2]) == (0, 0) and tuple(flags) == (1, 0)
    assert not np.isin(pos, where).any()
    s64 = nc.pair_scores64(c["users"], c["Q"], c["Ua"], c["Vd"], bad)
    check_lists(pos, score, s64, k, nc.tolerance(s64), bad, n_rows, None)
    # users whose clean list holds none of the three positions: the list is unchanged, bit for bit
    same = ~np.isin(clean[0], where).any(1)
    assert same.any() and np.array_equal(pos[same], clean[0][same])
    assert np.array_equal(score[same].view(np.int32), clean[1][same].view(np.int32))
    # the others keep their remaining entries, with the same bits, and take the next best
    for u in np.flatnonzero(~same):
        keep = ~np.isin(clean[0][u], where)
        n = int(keep.sum())
        assert np.array_equal(pos[u, :n], clean[0][u][keep]) and np.array_equal(score[u, :n].view(np.int32), clean[1][u][keep].view(np.int32))


def test_a_nan_in_one_catalogue_row_is_flagged_and_enters_no_list(hip):
    c = nc.case(nc.SHAPES[2], seed=19, cand="subset")
    clean = run_npa_topk(hip, c)
    row = int(c["cand_rows"][clean[0][0, 0]])  # user 0's best candidate
    for which, at in (("Vd", (row, 7, 5)), ("Ua", (row, 29, 23))):
        d = {**c, which: c[which].copy()}
        d[which][at] = np.nan
        pos, score, flags = run_npa_topk(hip, d)
        assert tuple(flags) == (0, 1), which
        kept_rows = np.where(pos >= 0, c["cand_rows"][np.maximum(pos, 0)], -1)
        assert not (kept_rows == row).any() and np.isfinite(score[pos >= 0]).all(), which
        s64 = nc.pair_scores64(c["users"], c["Q"], c["Ua"], c["Vd"], c["cand_rows"])
        ex = np.full((c["users"].shape[0], 1), row, np.int32)  # as if that row were excluded for everybody
        check_lists(pos, score, s64, c["k"], nc.tolerance(s64), c["cand_rows"], c["n_rows"], ex)


def test_an_all_excluded_user_gets_an_empty_list(hip):
    c = nc.case(nc.SHAPES[1], seed=23, cand="subset")
    U = c["users"].shape[0]
    distinct = np.unique(c["cand_rows"])
    ex = np.full((U, len(distinct)), -1, np.int32)
    ex[1] = distinct
    pos, score, flags = run_npa_topk(hip, c, exclude=ex)
    assert tuple(flags) == (0, 0)
    assert (pos[1] == -1).all() and np.isneginf(score[1]).all()
    others = [u for u in range(U) if u != 1]
    assert (pos[others, :7] >= 0).all() and (pos[others, 7:] == -1).all()  # M = 7 < k = 10: short lists


def test_no_candidates_fills_the_outputs_as_empty(hip):
    ones = dev(np.ones((3, 4, 8), np.float32))
    pos_d = torch.full((3, 5), -7, dtype=torch.int32, device="cuda")
    score_d = torch.full((3, 5), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    code = hip.lib().ebn_npa_topk_score_f32(P(ones), P(ones), P(ones), P(ones), 0, None, 0, None, 0, 5, 1, 0, P(pos_d), P(score_d),
                                            P(flags_d), None, 0, 3, 4, 8, 8, S())
    torch.cuda.synchronize()
    assert code == OK and (pos_d == -1).all() and torch.isneginf(score_d).all() and (flags_d == 0).all()


def test_a_failing_call_writes_nothing(hip):
    c = nc.case(nc.SHAPES[1], seed=29)
    U, F = c["users"].shape
    n_rows, L, A = c["Ua"].shape
    us, Q, Ua, Vd = dev(c["users"]), dev(c["Q"]), dev(c["Ua"]), dev(c["Vd"])
    pos_d = torch.full((U, 65), -7, dtype=torch.int32, device="cuda")
    score_d = torch.full((U, 65), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    base = dict(users=P(us), Q=P(Q), Ua=P(Ua), Vd=P(Vd), n_rows=n_rows, cand=None, M=n_rows, ex=None, X=0, k=4, mode=0, n_splits=1,
                pos=P(pos_d), score=P(score_d), flags=P(flags_d), ws=P(ws), ws_bytes=1 << 16, U=U, L=L, F=F, A=A, stream=S())
    call = lambda **kw: hip.lib().ebn_npa_topk_score_f32(*{**base, **kw}.values())
    need = int(hip.lib().ebn_topk_workspace_bytes(U, 4, 2))
    assert call(k=65) == -2 and call(L=65) == -2 and call(A=A + 2) == -2 and call(M=n_rows - 1) == -1
    assert call(n_splits=2, ws_bytes=need - 1) == -1 and call(n_splits=2, ws=None) == -1
    torch.cuda.synchronize()
    assert (pos_d == -7).all() and (score_d == 123.0).all() and (flags_d == 0).all()
    assert call(n_splits=2, ws_bytes=need) == OK and call(U=0) == OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the model
N_CANDIDATES, TOP_N = 30, 5


def _count_calls(monkeypatch, hip):
    counts = {}
    real = hip.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(hip, "call", counting)
    return counts


def _history_ids(loader, n):
    """per impression the article ids of its history (those the loader's index knows)"""
    row_to_id = {r: a for a, r in loader.lookup_article_index.items()}
    out = []
    for i in range(len(loader)):
        his_idx = np.asarray(loader.user_index_eval_batch(i)[1])
        out += [{row_to_id[r] for r in h.tolist() if r in row_to_id} for h in his_idx]
    assert len(out) == n
    return out


@pytest.mark.parametrize("kind", ["fixture", "synthetic"])
def test_recommend_pairwise_agrees_with_scorer_predict(hip, frames, kind, monkeypatch):  # noqa: F811
    """recommend_pairwise against scorer.predict over a loader whose every in-view list is the candidate list: the scores of the same
    (user, article) agree within 2 (1e-4 |s| + 1e-6) -- each side is within the project's tolerance of the float64 oracle --, nothing
    left out beats the fifth kept one by more than twice that, no history article is kept under exclusion; raw scores give the same
    ids; the lists go into IntralistDiversity unchanged; MMR with lam = 1 returns the plain lists, Calibrated returns candidates; the
    catalogue is encoded once whatever the number of batches and no candidate goes through ebn_pap_indexed_f32; scorer.predict is
    the same array before and after."""
    from ebrec.evaluation.beyond_accuracy import DeviceLookup, IntralistDiversity
    from ebrec.evaluation.rerank import MMR, Calibrated
    from tests.test_npa_cached_scoring_gpu import _npa_case

    model, loader, _Pw, _hp, _V = _npa_case(kind, frames)
    n_imp = sum(len(loader.user_index_eval_batch(i)[0]) for i in range(len(loader)))
    assert len(loader) >= 3
    rng = np.random.default_rng(7)
    index = model._recommend_index(loader)
    history = _history_ids(loader, n_imp)
    read = sorted(set().union(*history) & set(index))
    assert len(read) >= 10 and len(index) >= N_CANDIDATES
    cand = rng.choice(read, 10, replace=False)
    cand = rng.permutation(np.concatenate([cand, rng.choice(sorted(set(index) - set(cand.tolist())), N_CANDIDATES - 10, replace=False)]))

    before = model.scorer.predict(loader)
    counts = _count_calls(monkeypatch, hip)
    ids_ex, sc_ex = model.recommend_pairwise(loader, cand, top_n=TOP_N, return_scores=True)
    assert counts["ebn_conv1d_fwd_f32"] == 1 and counts["ebn_npa_topk_score_f32"] == 1  # one catalogue chunk, one scoring launch
    assert counts["ebn_pap_indexed_f32"] == len(loader) and counts["ebn_pap_fwd_f32"] == len(loader)  # the histories only
    counts.clear()
    ids_all, sc_all = model.recommend_pairwise(loader, cand, top_n=TOP_N, return_scores=True, exclude_history=False, users_per_call=16)
    assert counts["ebn_conv1d_fwd_f32"] == 1 and counts["ebn_npa_topk_score_f32"] == len(loader)  # a launch per flush
    assert counts["ebn_pap_indexed_f32"] == len(loader)
    monkeypatch.undo()
    assert ids_ex.shape == sc_ex.shape == ids_all.shape == sc_all.shape == (n_imp, TOP_N) and sc_ex.dtype == np.float32
    assert np.array_equal(model.recommend_pairwise(loader, cand, top_n=TOP_N), ids_ex)
    np.testing.assert_array_equal(model.scorer.predict(loader), before)  # score_cached is untouched

    # scorer.predict over the same impressions with the candidate list as every in-view list
    from ebrec.utils._constants import DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_LABELS_COL

    same_users = loader.behaviors.copy()
    same_users[DEFAULT_INVIEW_ARTICLES_COL] = [cand.tolist()] * n_imp
    same_users[DEFAULT_LABELS_COL] = [[0] * N_CANDIDATES] * n_imp
    twin = type(loader)(behaviors=same_users, article_dict=loader.article_dict, user_id_mapping=loader.user_id_mapping,
                        unknown_representation="zeros", history_column=loader.history_column, batch_size=16, eval_mode=True)
    pred = model.scorer.predict(twin).reshape(n_imp, N_CANDIDATES).astype(np.float64)
    tol = lambda s: 2 * (1e-4 * np.abs(s) + 1e-6)
    col = {c_: j for j, c_ in enumerate(cand.tolist())}
    assert any(history[u] & set(col) for u in range(n_imp)), "the case must exercise the exclusion"
    worst = 0.0
    for ids, sc, excluded in ((ids_ex, sc_ex, history), (ids_all, sc_all, [set()] * n_imp)):
        for u in range(n_imp):
            kept = [col[a] for a in ids[u].tolist()]
            assert len(set(kept)) == TOP_N and not set(ids[u].tolist()) & excluded[u]
            worst = max(worst, float(np.abs(sc[u] - pred[u, kept]).max()))
            assert (np.abs(sc[u] - pred[u, kept]) <= tol(pred[u, kept])).all(), (u, sc[u], pred[u, kept])
            assert (np.diff(sc[u]) <= 0).all()
            left_out = [j for c_, j in col.items() if j not in kept and c_ not in excluded[u]]
            assert pred[u, left_out].max() <= pred[u, kept[-1]] + 2 * tol(pred[u, kept[-1]]), u
    print(f"{kind}: max |recommend_pairwise - scorer.predict| on the kept pairs = {worst:.3e}")
    assert np.ptp(pred) > 1e-3
    raw_ids, raw = model.recommend_pairwise(loader, cand, top_n=TOP_N, return_scores=True, scores="raw")
    assert np.array_equal(raw_ids, ids_ex) and (np.abs(1 / (1 + np.exp(-raw.astype(np.float64))) - sc_ex) <= 4 * 2.0 ** -23).all()

    # the lists as they are in the beyond-accuracy metrics, and through the two re-rankers
    arng = np.random.default_rng(9)
    articles = {int(a): {"emb": arng.standard_normal(8).astype(np.float32), "cat": "abcd"[int(arng.integers(0, 4))]} for a in index}
    lookup = DeviceLookup(articles, ["emb"], label_keys=["cat"])
    on_device = IntralistDiversity()(ids_ex, lookup_dict=lookup, lookup_key="emb")
    on_host = IntralistDiversity()(ids_ex, lookup_dict=articles, lookup_key="emb")
    np.testing.assert_allclose(on_device, on_host, rtol=1e-4, atol=1e-5)
    mmr_ids, mmr_sc = model.recommend_pairwise(loader, cand, top_n=TOP_N, return_scores=True, rerank=MMR(lookup, "emb", lam=1.0, pool=20))
    assert np.array_equal(mmr_ids, ids_ex) and np.array_equal(mmr_sc, sc_ex)
    div_ids = model.recommend_pairwise(loader, cand, top_n=TOP_N, rerank=MMR(lookup, "emb", lam=0.3, pool=20))
    assert div_ids.shape == ids_ex.shape and np.isin(div_ids, cand).all() and not np.array_equal(div_ids, ids_ex)
    cal_ids = model.recommend_pairwise(loader, cand, top_n=TOP_N, rerank=Calibrated(lookup, "cat", lam=0.5, pool=20))
    assert cal_ids.shape == ids_ex.shape and np.isin(cal_ids, cand).all()
    assert all(not set(cal_ids[u].tolist()) & history[u] and len(set(cal_ids[u].tolist())) == TOP_N for u in range(n_imp))

    # ranking has no per-batch fallback
    model.catalogue_max_bytes = 1
    with pytest.raises(ValueError, match="catalogue_max_bytes"):
        model.recommend_pairwise(loader, cand, top_n=TOP_N)
