"""ebn_mmr_rerank_f32 (csrc/ebn_rerank.hip), mmr_rerank() over a DeviceLookup and recommend(rerank=MMR(...)) on the GPU, against
the float64 restatement of tests/rerank_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import rerank_cases as rr
from tests.hip_testutil import P as PTR, S, dev

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3


def run_rerank(hip, unit, rows, rel, k, lam, want_obj=True):
    """-> (sel [U, k] int32, obj [U, k] float32, flags [2]) as numpy arrays"""
    U, P = rows.shape
    unit_d, rows_d, rel_d = dev(unit), dev(rows, torch.int32), dev(rel)
    sel_d = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
    obj_d = torch.full((U, k), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    code = hip.lib().ebn_mmr_rerank_f32(PTR(unit_d), unit.shape[0], unit.shape[1], PTR(rows_d), PTR(rel_d), P, k, lam, PTR(sel_d),
                                        PTR(obj_d) if want_obj else None, PTR(flags_d), U, S())
    assert code == OK, code
    torch.cuda.synchronize()
    return sel_d.cpu().numpy(), obj_d.cpu().numpy(), flags_d.cpu().numpy()


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("shape", rr.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_cases_equal_the_restatement(hip, shape):
    """Dyadic inputs: every dot product, distance and objective is exact in fp32 in any order, so picks AND objectives must equal
    the float64 restatement -- ties, duplicates, padding, the all-absent user and k > P included."""
    U, P, D, k = shape
    unit, rows, rel = rr.exact_case(U, P, D, seed=U + P)
    for lam in rr.EXACT_LAMS:
        want_sel, want_obj, want_flags = rr.mmr_reference(unit, rows, rel, k, lam)
        sel, obj, flags = run_rerank(hip, unit, rows, rel, k, lam)
        assert np.array_equal(sel, want_sel), lam
        assert np.array_equal(obj.astype(np.float64), want_obj), lam
        assert tuple(flags) == want_flags == (0, 0)
    if U > 1:
        assert (sel[1] == -1).all() and np.isneginf(obj[1]).all()  # the user whose every entry is padding
    sel_only, untouched, _ = run_rerank(hip, unit, rows, rel, k, 0.5, want_obj=False)
    assert np.array_equal(sel_only, rr.mmr_reference(unit, rows, rel, k, 0.5)[0]) and (untouched == 123.0).all()


@pytest.mark.parametrize("shape", [(7, 33, 36, 10), (5, 32, 16, 5)], ids=lambda s: "x".join(map(str, s)))
def test_rows_outside_the_table_and_nan_relevances_are_absent_and_flagged(hip, shape):
    U, P, D, k = shape
    for bad_row, nan_rel in ((True, False), (False, True), (True, True)):
        unit, rows, rel = rr.exact_case(U, P, D, seed=3, bad_row=bad_row, nan_rel=nan_rel)
        want_sel, want_obj, want_flags = rr.mmr_reference(unit, rows, rel, k, 0.5)
        sel, obj, flags = run_rerank(hip, unit, rows, rel, k, 0.5)
        assert want_flags == (int(bad_row), int(nan_rel)) and tuple(flags) == want_flags
        assert np.array_equal(sel, want_sel) and np.array_equal(obj.astype(np.float64), want_obj)
        gone = ~rr.present_mask(rows[U - 1], rel[U - 1], len(unit))
        assert not np.isin(sel[U - 1], np.flatnonzero(gone)).any()


def test_a_nan_dot_product_is_distance_zero_and_flagged(hip):
    unit, rows, rel = rr.exact_case(4, 33, 36, seed=5)
    unit[2, 7] = np.nan
    rows[0, :3] = [2, 0, 1]
    rel[0, :3] = [1.0, 0.5, 0.25]
    want_sel, want_obj, want_flags = rr.mmr_reference(unit, rows, rel, 10, 0.5)
    sel, obj, flags = run_rerank(hip, unit, rows, rel, 10, 0.5)
    assert want_flags == (0, 1) and tuple(flags) == (0, 1)
    assert np.array_equal(sel, want_sel) and np.array_equal(obj.astype(np.float64), want_obj)


# ------------------------------------------------------------------------------------------------ rounded cases
@pytest.mark.parametrize("lam", rr.ROUNDED_LAMS)
@pytest.mark.parametrize("shape", rr.ROUNDED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_standard_normal_cases_by_the_greedy_property(hip, shape, lam):
    """Every pick's objective, recomputed in float64 GIVEN the kernel's earlier picks, is within 2 tol of the best one left, and
    out_obj within tol of it; no pick repeats, no absent entry is picked (rerank_cases.check_greedy);
    tol = (1 - lam) b + 4 * 2^-23 with b the fp32 summation bound of the table's rows."""
    U, P, D, k = shape
    unit, rows, rel = rr.rounded_case(U, P, D, seed=11)
    tol = rr.tolerance(unit, lam)
    sel, obj, flags = run_rerank(hip, unit, rows, rel, k, lam)
    assert tuple(flags) == (0, 0)
    lam32 = float(np.float32(lam))
    gap, err = rr.check_greedy(unit, rows, rel, sel, obj, lam32, tol)
    print(f"shape {shape} lam {lam}: tol = {tol:.3e}, worst shortfall {gap:.3e}, worst |obj - float64| {err:.3e}")
    assert (sel[:, 0] >= 0).all()


# ------------------------------------------------------------------------------------------------ determinism
def test_two_runs_and_any_set_of_co_launched_users_give_the_same_bits(hip):
    """A user's output depends neither on U nor on who shares its launch or workgroup: users [0, 7) alone against the first 7 of
    130, at one user per workgroup (P = 64) and at two (P = 32, where 7 users leave a workgroup half empty)."""
    for P, D, k in ((64, 64, 64), (32, 36, 10)):
        unit, rows, rel = rr.rounded_case(130, P, D, seed=17)
        full = run_rerank(hip, unit, rows, rel, k, 0.7)
        again = run_rerank(hip, unit, rows, rel, k, 0.7)
        head = run_rerank(hip, unit, rows[:7], rel[:7], k, 0.7)
        odd = run_rerank(hip, unit, rows[1:8], rel[1:8], k, 0.7)  # the same users paired differently inside workgroups
        assert np.array_equal(full[0], again[0]) and np.array_equal(full[1].view(np.int32), again[1].view(np.int32))
        assert np.array_equal(head[0], full[0][:7]) and np.array_equal(head[1].view(np.int32), full[1][:7].view(np.int32))
        assert np.array_equal(odd[0], full[0][1:8]) and np.array_equal(odd[1].view(np.int32), full[1][1:8].view(np.int32))


# ------------------------------------------------------------------------------------------------ error codes
def test_unsupported_bad_and_misaligned_calls_return_their_code_and_write_nothing(hip):
    U, P, D, k = 5, 33, 8, 4
    unit, rows, rel = rr.exact_case(U, P, D, seed=4)
    unit_d = dev(np.zeros(len(unit) * 8 + 4, np.float32))
    rows_d, rel_d = dev(np.zeros((U, 65)), torch.int32), dev(np.zeros((U, 65)))
    sel_d = torch.full((U, 65), -7, dtype=torch.int32, device="cuda")
    obj_d = torch.full((U, 65), 123.0, device="cuda")
    flags_d = torch.zeros(2, dtype=torch.int32, device="cuda")

    def call(**kw):
        a = {**dict(unit=PTR(unit_d), n_rows=len(unit), D=D, rows=PTR(rows_d), rel=PTR(rel_d), P=P, k=k, lam=0.5, sel=PTR(sel_d),
                    obj=PTR(obj_d), flags=PTR(flags_d), U=U, stream=S()), **kw}
        return hip.lib().ebn_mmr_rerank_f32(*a.values())

    assert call(P=65) == UNSUPPORTED and call(k=65) == UNSUPPORTED and call(D=6) == UNSUPPORTED
    assert call(lam=1.5) == BAD_ARG and call(lam=float("nan")) == BAD_ARG
    assert call(unit=ctypes.c_void_p(unit_d.data_ptr() + 4)) == ALIGN
    torch.cuda.synchronize()
    assert (sel_d == -7).all() and (obj_d == 123.0).all() and (flags_d == 0).all()
    assert call(U=0) == OK
    torch.cuda.synchronize()
    assert (sel_d == -7).all() and (flags_d == 0).all()
    assert call() == OK  # the same call within the limits runs
    torch.cuda.synchronize()
    assert (sel_d.view(-1)[:U * k] != -7).all()


# ------------------------------------------------------------------------------------------------ mmr_rerank() over a DeviceLookup
def test_mmr_rerank_on_the_device_equals_the_restatement(hip):
    from ebrec.evaluation import mmr_rerank
    from ebrec.evaluation.beyond_accuracy import DeviceLookup

    U, P, D, k = 7, 33, 36, 10
    _, rows, rel = rr.exact_case(U, P, D, seed=9)
    table = rr.exact_unit_table(max(3, (3 * P) // 4), D, np.random.default_rng(9))  # unit rows in dyadic numbers: normalising is exact
    articles = {100 + r: {"emb": table[r]} for r in range(len(table))}
    ids = np.where(rows >= 0, rows + 100, -1)
    lookup = DeviceLookup(articles, ["emb"])
    assert np.array_equal(lookup.device_table("emb").cpu().numpy(), table)
    for lam in (0.25, 1.0):
        want_sel, _, _ = rr.mmr_reference(table, rows, rel, k, lam)
        kept = np.maximum(want_sel, 0).astype(np.int64)
        got_ids, got_scores = mmr_rerank(ids, rel, lookup, "emb", k, lam, return_scores=True)
        assert np.array_equal(got_ids, np.where(want_sel >= 0, np.take_along_axis(ids, kept, 1), -1))
        assert np.array_equal(got_scores, np.where(want_sel >= 0, np.take_along_axis(rel, kept, 1), -np.inf))
        assert np.array_equal(mmr_rerank(ids, rel, articles, "emb", k, lam), got_ids)  # the host path


# ------------------------------------------------------------------------------------------------ whole model
from tests.test_data_pipeline import frames  # noqa: E402,F401  (the fixture parquets under tests/golden/ebnerd)
from tests.test_recommend_gpu import N_CANDIDATES, N_IMPRESSIONS, TOP_N, _nrms_case  # noqa: E402

POOL = 20


def test_nrms_recommend_with_mmr(hip, frames):  # noqa: F811
    """lam = 1 is plain recommend(); lam = 1/2 gives subsets of the plain top-20 that start with the plain first item, hold no
    history article and satisfy the greedy property recomputed in float64 from the plain top-20 and the lookup's vectors;
    mmr_rerank() over the plain top-20 gives the same lists."""
    from ebrec.evaluation import MMR, mmr_rerank
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
    same_ids, same_sc = model.recommend(loader, cand, top_n=TOP_N, return_scores=True, rerank=MMR(lookup, "emb", lam=1.0, pool=POOL))
    assert np.array_equal(same_ids, plain_ids) and np.array_equal(same_sc.view(np.int32), plain_sc.view(np.int32))

    ids20, sc20 = model.recommend(loader, cand, top_n=POOL, return_scores=True)
    ids, sc = model.recommend(loader, cand, top_n=TOP_N, return_scores=True, rerank=MMR(lookup, "emb", lam=0.5, pool=POOL))
    assert ids.shape == sc.shape == (N_IMPRESSIONS, TOP_N) and sc.dtype == np.float32
    assert np.array_equal(model.recommend(loader, cand, top_n=TOP_N, rerank=MMR(lookup, "emb", lam=0.5, pool=POOL)), ids)
    assert np.array_equal(ids[:, 0], plain_ids[:, 0])
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
    tol = rr.tolerance(unit, 0.5)
    gap, _ = rr.check_greedy(unit, rows20, sc20, sel, None, 0.5, tol)
    print(f"whole model: tol = {tol:.3e}, worst shortfall {gap:.3e}")
    assert np.array_equal(mmr_rerank(ids20, sc20, lookup, "emb", TOP_N, 0.5), ids)
