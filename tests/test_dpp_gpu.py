"""ebn_dpp_rerank_f32 (csrc/ebn_dpp.hip), dpp_rerank() over a DeviceLookup and recommend(rerank=DPP(...)) on the GPU, against the
restatement of tests/dpp_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dpp_cases as dc
from tests.hip_testutil import P as PTR, S, dev

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3


def run_pool(hip, entry, unit, rows, rel, k, lam, want_obj=True):
    """-> (sel [U, k] int32, obj [U, k] float32, flags [2]) as numpy arrays"""
    U, P = rows.shape
    unit_d, rows_d, rel_d = dev(unit), dev(rows, torch.int32), dev(rel)
    sel_d = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
    obj_d = torch.full((U, k), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    code = getattr(hip.lib(), entry)(PTR(unit_d), unit.shape[0], unit.shape[1], PTR(rows_d), PTR(rel_d), P, k, lam, PTR(sel_d),
                                     PTR(obj_d) if want_obj else None, PTR(flags_d), U, S())
    assert code == OK, code
    torch.cuda.synchronize()
    return sel_d.cpu().numpy(), obj_d.cpu().numpy(), flags_d.cpu().numpy()


def run_dpp(hip, unit, rows, rel, k, lam, want_obj=True):
    return run_pool(hip, "ebn_dpp_rerank_f32", unit, rows, rel, k, lam, want_obj)


@pytest.fixture(scope="module")
def margin_cases():
    """{shape: (seed, unit, rows, rel, reference picks)} for the shapes that have, among seeds 0..49, a case whose float64
    reference leads its runner-up by 100 (tol(best) + tol(runner-up)) in every round at lam = 0.7.  Found on the CPU."""
    found = {}
    for shape in dc.SHAPES:
        U, P, D, k = shape
        for seed in range(50):
            unit, rows, rel = dc.dpp_case(U, P, D, seed)
            ok, sel = dc.margin_ok(unit, rows, rel, k, 0.7)
            if ok:
                found[shape] = (seed, unit, rows, rel, sel)
                break
    return found


# ------------------------------------------------------------------------------------------------ the greedy property
@pytest.mark.parametrize("lam", dc.LAMS)
@pytest.mark.parametrize("shape", dc.SHAPES, ids=dc.shape_id)
def test_standard_normal_cases_by_the_greedy_property(hip, shape, lam):
    """Every pick's objective, recomputed in float64 GIVEN the kernel's earlier picks, is within tol(s) + tol(best) of the best
    one left, and out_obj within tol(s) of it; no pick repeats, no absent entry is picked (dpp_cases.check_greedy_dpp).  The
    tolerance comes from the float32 numpy restatement's own error along the same prefix, times four.
    Measured on an MI355X (worst over the four lam): see DESIGN.md section 23."""
    U, P, D, k = shape
    unit, rows, rel = dc.dpp_case(U, P, D, seed=11)
    sel, obj, flags = run_dpp(hip, unit, rows, rel, k, lam)
    assert tuple(flags) == (0, 0)
    gap, err, e32 = dc.check_greedy_dpp(unit, rows, rel, sel, obj, lam)
    print(f"DPP shape {shape} lam {lam}: E32 = {e32:.3e}, worst shortfall {gap:.3e}, worst |obj - float64| {err:.3e}")
    present = np.stack([dc.present_mask(rows[u], rel[u], len(unit)) for u in range(U)])
    assert ((sel >= 0).sum(1) == np.minimum(present.sum(1), k)).all()  # full length: spanned entries are clamped, not dropped
    sel_only, untouched, _ = run_dpp(hip, unit, rows, rel, k, lam, want_obj=False)
    assert np.array_equal(sel_only, sel) and (untouched == 123.0).all()


def test_picks_equal_the_reference_where_every_round_has_a_margin(hip, margin_cases):
    assert len(margin_cases) >= 3, sorted(margin_cases)
    for shape, (seed, unit, rows, rel, want) in margin_cases.items():
        sel, _, flags = run_dpp(hip, unit, rows, rel, shape[3], 0.7)
        assert np.array_equal(sel, want), (shape, seed)
        assert tuple(flags) == (0, 0)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=dc.shape_id)
def test_lam_one_is_mmr_at_lam_one_bit_for_bit(hip, shape):
    U, P, D, k = shape
    unit, rows, rel = dc.dpp_case(U, P, D, seed=13)
    rel[:, P // 2] = rel[:, 0]  # a tie
    sel, obj, flags = run_dpp(hip, unit, rows, rel, k, 1.0)
    mmr_sel, _, _ = run_pool(hip, "ebn_mmr_rerank_f32", unit, rows, rel, k, 1.0)
    assert np.array_equal(sel, mmr_sel) and tuple(flags) == (0, 0)
    want_obj = np.where(sel >= 0, np.take_along_axis(rel, np.maximum(sel, 0).astype(np.int64), 1), -np.inf).astype(np.float32)
    assert np.array_equal(obj, want_obj)


# ------------------------------------------------------------------------------------------------ absent entries
@pytest.mark.parametrize("shape", [(7, 32, 36, 10), (3, 33, 64, 33)], ids=dc.shape_id)
def test_absent_entries_are_never_picked_and_flagged_as_for_mmr(hip, shape):
    U, P, D, k = shape
    base = dc.dpp_case(U, P, D, seed=7)
    for bad_row, bad_rel in ((True, False), (False, True), (True, True), (False, False)):
        unit, rows, rel = (a.copy() for a in base)
        rows[0, 1], rel[0, 2] = -1, -np.inf  # the padding: sets nothing
        rows[1], rel[1] = -1, -np.inf        # a user whose every entry is absent
        if bad_row:
            rows[0, 3], rows[2, 0] = len(unit), -2
        if bad_rel:
            rel[0, 4], rel[2, 1] = np.nan, np.inf
        sel, obj, flags = run_dpp(hip, unit, rows, rel, k, 0.5)
        assert tuple(flags) == (int(bad_row), int(bad_rel)) == dc.dpp_reference(unit, rows, rel, k, 0.5)[2]
        dc.check_greedy_dpp(unit, rows, rel, sel, obj, 0.5)
        for u in range(U):
            gone = np.flatnonzero(~dc.present_mask(rows[u], rel[u], len(unit)))
            assert not np.isin(sel[u], gone).any()
        assert (sel[1] == -1).all() and np.isneginf(obj[1]).all()


def test_a_nan_table_row_is_distance_zero_and_flagged(hip):
    U, P, D, k = 3, 33, 64, 33
    unit, rows, rel = dc.dpp_case(U, P, D, seed=9)
    unit[rows[0, 0], 7] = np.nan  # user 0 holds the row twice (entry 0 and its duplicate)
    want_flags = dc.dpp_reference(unit, rows, rel, k, 0.5)[2]
    sel, obj, flags = run_dpp(hip, unit, rows, rel, k, 0.5)
    assert want_flags == (0, 1) and tuple(flags) == (0, 1)
    assert np.isfinite(obj[sel >= 0]).all()
    dc.check_greedy_dpp(unit, rows, rel, sel, obj, 0.5)  # the restatement too gives a NaN dot product d = 0, S = 1
    lone = np.full((1, 5), -1, np.int32)
    lone[0, 2] = rows[0, 0]  # the NaN row alone: its own dot product is the only one
    sel, obj, flags = run_dpp(hip, unit, lone, np.ones((1, 5), np.float32), 3, 0.5)
    assert sel.tolist() == [[2, -1, -1]] and tuple(flags) == (0, 1) and obj[0, 0] == 0.5


# ------------------------------------------------------------------------------------------------ determinism
def test_two_runs_and_any_set_of_co_launched_users_give_the_same_bits(hip):
    """A user's output depends neither on U nor on who shares its launch or workgroup: users [0, 7) alone against the first 7 of
    19, at two users per workgroup (P = 20, where 7 users leave a workgroup half empty) and at one (P = 40)."""
    for P, D, k in ((20, 36, 20), (40, 36, 40)):
        unit, rows, rel = dc.dpp_case(19, P, D, seed=17)
        full = run_dpp(hip, unit, rows, rel, k, 0.7)
        again = run_dpp(hip, unit, rows, rel, k, 0.7)
        head = run_dpp(hip, unit, rows[:7], rel[:7], k, 0.7)
        odd = run_dpp(hip, unit, rows[1:8], rel[1:8], k, 0.7)  # the same users paired differently inside workgroups
        assert np.array_equal(full[0], again[0]) and np.array_equal(full[1].view(np.int32), again[1].view(np.int32))
        assert np.array_equal(head[0], full[0][:7]) and np.array_equal(head[1].view(np.int32), full[1][:7].view(np.int32))
        assert np.array_equal(odd[0], full[0][1:8]) and np.array_equal(odd[1].view(np.int32), full[1][1:8].view(np.int32))


# ------------------------------------------------------------------------------------------------ error codes
def test_unsupported_bad_and_misaligned_calls_return_their_code_and_write_nothing(hip):
    U, P, D, k, n_rows = 5, 33, 8, 4, 24
    unit_d = dev(np.zeros(n_rows * 8 + 4, np.float32))
    rows_d, rel_d = dev(np.zeros((U, 65)), torch.int32), dev(np.zeros((U, 65)))
    sel_d = torch.full((U, 65), -7, dtype=torch.int32, device="cuda")
    obj_d = torch.full((U, 65), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")

    def call(**kw):
        a = {**dict(unit=PTR(unit_d), n_rows=n_rows, D=D, rows=PTR(rows_d), rel=PTR(rel_d), P=P, k=k, lam=0.5, sel=PTR(sel_d),
                    obj=PTR(obj_d), flags=PTR(flags_d), U=U, stream=S()), **kw}
        return hip.lib().ebn_dpp_rerank_f32(*a.values())

    assert call(P=0) == UNSUPPORTED and call(P=65) == UNSUPPORTED and call(k=0) == UNSUPPORTED and call(k=65) == UNSUPPORTED
    assert call(D=6) == UNSUPPORTED and call(D=8196) == UNSUPPORTED
    assert call(lam=-0.1) == BAD_ARG and call(lam=float("nan")) == BAD_ARG
    assert call(unit=ctypes.c_void_p(unit_d.data_ptr() + 4)) == ALIGN
    torch.cuda.synchronize()
    assert (sel_d == -7).all() and (obj_d == 123.0).all() and (flags_d == 0).all()
    assert call(U=0) == OK
    torch.cuda.synchronize()
    assert (sel_d == -7).all() and (flags_d == 0).all()
    assert call() == OK  # the same call within the limits runs
    torch.cuda.synchronize()
    assert (sel_d.view(-1)[:U * k] != -7).all()


# ------------------------------------------------------------------------------------------------ dpp_rerank() over a DeviceLookup
def test_dpp_rerank_on_the_device_equals_the_host_path(hip, margin_cases):
    from ebrec.evaluation import dpp_rerank
    from ebrec.evaluation.beyond_accuracy import DeviceLookup

    shape = (7, 32, 36, 10)
    assert shape in margin_cases
    _, table, rows, rel, want_sel = margin_cases[shape]
    k = shape[3]
    articles = {100 + r: {"emb": table[r]} for r in range(len(table))}
    ids = np.where(rows >= 0, rows + 100, -1)
    lookup = DeviceLookup(articles, ["emb"])
    kept = np.maximum(want_sel, 0).astype(np.int64)
    got_ids, got_scores = dpp_rerank(ids, rel, lookup, "emb", k, 0.7, return_scores=True)
    assert np.array_equal(got_ids, np.where(want_sel >= 0, np.take_along_axis(ids, kept, 1), -1))
    assert np.array_equal(got_scores, np.where(want_sel >= 0, np.take_along_axis(rel, kept, 1), -np.inf))
    assert np.array_equal(dpp_rerank(ids, rel, articles, "emb", k, 0.7), got_ids)  # the host path


# ------------------------------------------------------------------------------------------------ whole model
from tests.test_data_pipeline import frames  # noqa: E402,F401  (the fixture parquets under tests/golden/ebnerd)
from tests.test_recommend_gpu import N_CANDIDATES, N_IMPRESSIONS, TOP_N, _nrms_case  # noqa: E402

POOL = 20


def test_nrms_recommend_with_dpp(hip, frames):  # noqa: F811
    """lam = 1 is plain recommend(); lam = 1/2 gives duplicate-free subsets of the plain top-20 that hold no history article and
    satisfy the greedy property recomputed in float64 from the plain top-20 and the lookup's vectors; top_n > pool raises."""
    from ebrec.evaluation import DPP
    from ebrec.evaluation.beyond_accuracy import DeviceLookup
    from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL

    model, mk = _nrms_case(frames)
    beh = frames[0].iloc[:N_IMPRESSIONS].reset_index(drop=True)
    loader = mk(beh)
    rng = np.random.default_rng(7)
    index = model._recommend_index(loader)
    read = sorted({a for h in beh[DEFAULT_HISTORY_ARTICLE_ID_COL] for a in h} & set(index))
    cand = rng.choice(read, 10, replace=False)
    cand = rng.permutation(np.concatenate([cand, rng.choice(sorted(set(index) - set(cand.tolist())), N_CANDIDATES - 10, replace=False)]))
    articles = {int(a): {"emb": rng.standard_normal(8).astype(np.float32)} for a in index}
    lookup = DeviceLookup(articles, ["emb"])

    plain_ids, plain_sc = model.recommend(loader, cand, top_n=TOP_N, return_scores=True)
    same_ids, same_sc = model.recommend(loader, cand, top_n=TOP_N, return_scores=True, rerank=DPP(lookup, "emb", lam=1.0, pool=POOL))
    assert np.array_equal(same_ids, plain_ids) and np.array_equal(same_sc.view(np.int32), plain_sc.view(np.int32))

    ids20, sc20 = model.recommend(loader, cand, top_n=POOL, return_scores=True)
    ids, sc = model.recommend(loader, cand, top_n=TOP_N, return_scores=True, rerank=DPP(lookup, "emb", lam=0.5, pool=POOL))
    assert ids.shape == sc.shape == (N_IMPRESSIONS, TOP_N) and sc.dtype == np.float32
    assert np.array_equal(model.recommend(loader, cand, top_n=TOP_N, rerank=DPP(lookup, "emb", lam=0.5, pool=POOL)), ids)
    assert not np.array_equal(ids, plain_ids), "the case must exercise the diversity term"
    history = [set(h) for h in beh[DEFAULT_HISTORY_ARTICLE_ID_COL]]
    unit = lookup.device_table("emb").cpu().numpy()
    rows20 = lookup.rows_of(ids20).reshape(ids20.shape)
    sel = np.empty((N_IMPRESSIONS, TOP_N), np.int64)
    for u in range(N_IMPRESSIONS):
        pos = {a: i for i, a in enumerate(ids20[u].tolist()) if a != -1}
        assert set(ids[u].tolist()) <= set(pos) and len(set(ids[u].tolist())) == TOP_N and not set(ids[u].tolist()) & history[u]
        sel[u] = [pos[a] for a in ids[u].tolist()]
    assert np.array_equal(sc, np.take_along_axis(sc20, sel, 1))  # the model's scores of the kept items, in selection order
    gap, _, e32 = dc.check_greedy_dpp(unit, rows20, sc20, sel, None, 0.5)
    print(f"DPP whole model: E32 = {e32:.3e}, worst shortfall {gap:.3e}")
    with pytest.raises(ValueError, match=rf"the DPP pool must lie in \[top_n, 64\] = \[{POOL + 1}, 64\]"):
        model.recommend(loader, cand, top_n=POOL + 1, rerank=DPP(lookup, "emb", pool=POOL))
