"""The float64 stage references of tests/docvec_kernel_refs.py, checked without a GPU:

  * every backward stage against torch.autograd in float64 at the shapes of tests/test_guarded_docvec_gpu.py (1e-10 relative), batch
    statistics inside the graph, per call site; the BatchNormalization backward also against training_tail_refs.bn_bwd_ref;
  * every magnitude dominates its value;
  * the float32 numpy stand-in of the two calls (dk.standin_step) passes check_step -- the comparator of the GPU tests -- and the
    whole-chain check against the oracle at every listed case, so the references, the `stat` layout and the comparator are exercised
    before a GPU sees them;
  * planted defects in the stand-in, run through the same comparator.  Six are caught at a listed case and MISSED at every shape
    tests/test_docvec_model.py runs (NEW_ONLY: the evidence that the listed shapes matter).  Five defects of the issue's list are, in
    their plain form, caught at the old shapes as well (the comparator would notice them there too: CAUGHT_BY_OLD says which) and are
    replaced by a form only the listed shapes catch:
      site 1 normalised with site 0's statistics        -> the same, where the history tiles are counted as n0 / 32 + 1
      one moving-average update for both sites          -> an update for an EMPTY site too
      dropout index relative to the site                -> the mean | istd block of an empty site written (no dropout path is new: every
                                                           old shape has history rows in front of the candidates and runs with p = 0.2)
      last four columns of a B tile duplicated          -> a last row tile of exactly ONE row never launched (n = 1, 33, 65)
      Aout slab kt without an owning column tile skipped -> the constant term of the d(BatchNormalization) operand indexed by LDS buffer
                                                           instead of by slab (needs a hidden layer l >= 1 wider than 256: units 512)"""
import numpy as np
import pytest
import torch

from tests import docvec_kernel_refs as dk
from tests import training_tail_refs as tr
from tests.hip_testutil import assert_close

REL = 1e-10


def t64(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def same(got, want, what, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want.detach().numpy() if torch.is_tensor(want) else want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-300) if scale is None else scale
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= REL * scale, (what, err, scale)


def dominates(ref, what):
    v, m = ref
    assert v.shape == m.shape and (m >= np.abs(v) * (1 - 1e-12)).all(), what


def test_the_listed_cases_are_what_the_table_says():
    assert len(dk.CASES) == 10 and all(n0 + n1 <= 98 and max(units + [din, e]) <= 1024 for n0, n1, din, units, e in dk.CASES.values())
    assert dk.stat_floats([4]) == 20 * 4 + 64 and dk.ONE_M_MOM32 < 0.01 < dk.ONE_M_MOM32 * (1 + 2e-6)
    st = np.arange(dk.stat_floats([4, 8]), dtype=np.float32)
    v = dk.stat_view(st, [4, 8], 1)
    assert v["fwd"].shape == (2, 2, 8) and v["mean"][0, 0] == 16 * 12 + 4 * 4 and v["istd"][0, 0] == 16 * 12 + 16 + 16 and dk.l2_view(st, [4, 8])[0, 0] == 240
    assert v["bwd"].view(np.float32).reshape(-1)[0] == 8 * 12 + 8 * 4


@pytest.mark.parametrize("p,l2", dk.P_L2)
@pytest.mark.parametrize("name", list(dk.CASES))
def test_stage_references_vs_autograd(name, p, l2):
    n0, n1, din, units, e_out = dk.CASES[name]
    L, n, ns = len(units), n0 + n1, (n0, n1)
    inp = dk.case_inputs(n0, n1, din, units, e_out)
    mults = [m.astype(np.float64) for m in dk.drop_mults(n0, n1, units, p)]
    W, b = [t64(w) for w in inp["W"]], [t64(x) for x in inp["b"]]
    gam, bet = [t64(x) for x in inp["gamma"]], [t64(x) for x in inp["beta"]]
    # ---- torch: the model, statistics inside the graph per site
    x, pres, bns, xns = t64(inp["X0"], False), [], [], []
    for l in range(L):
        pre = x @ W[l] + b[l]
        pre.retain_grad()
        r = torch.relu(pre)
        rows = []
        for a, e in dk.sites(n0, n1):
            if e > a:
                rs = r[a:e]
                rows.append((rs - rs.mean(0)) / torch.sqrt(rs.var(0, unbiased=False) + dk.EPS32) * gam[l] + bet[l])
        bn = torch.cat(rows, 0)
        bn.retain_grad()
        x = bn * t64(mults[l], False)
        pres.append(pre)
        bns.append(bn)
        xns.append(x)
    pre = x @ W[L] + b[L]
    pre.retain_grad()
    pres.append(pre)
    ne = torch.relu(pre)
    (ne * t64(inp["dNE"], False)).sum().backward()
    # ---- the references, chained on their own exact values
    A = inp["X0"]
    Rs, means, istds = [], [], []
    for l in range(L):
        R = dk.dense_ref(A, inp["W"][l], inp["b"][l])
        dominates(R, "R")
        same(R[0], torch.relu(pres[l]), f"R{l}")
        st = dk.stats_ref(R[0], n0, n1)
        for s in range(2):
            assert (st[s] is None) == (ns[s] == 0)
            if st[s] is not None:
                for k in ("mean", "var", "istd"):
                    dominates(st[s][k], k)
                a, e = dk.sites(n0, n1)[s]
                same(st[s]["var"][0], R[0][a:e].var(0), "var", scale=max(float((R[0][a:e] ** 2).mean(0).max()), 1e-300))
        mean = np.stack([np.zeros(units[l]) if s is None else s["mean"][0] for s in st])
        istd = np.stack([np.zeros(units[l]) if s is None else s["istd"][0] for s in st])
        Xn = dk.xn_ref(R[0], mean, istd, inp["gamma"][l], inp["beta"][l], mults[l], n0, n1)
        dominates(Xn, "Xn")
        same(Xn[0], xns[l], f"Xn{l}")
        mm, mv = dk.moving_ref(inp["mm"][l], inp["mv"][l], R[0], mean, n0, n1)
        dominates(mm, "moving mean")
        dominates(mv, "moving var")
        wm, wv = inp["mm"][l].astype(np.float64), inp["mv"][l].astype(np.float64)
        for s, (a, e) in enumerate(dk.sites(n0, n1)):  # one update per non-empty site, history first
            if e > a:
                wm, wv = wm * dk.MOM32 + R[0][a:e].mean(0) * dk.ONE_M_MOM32, wv * dk.MOM32 + R[0][a:e].var(0) * dk.ONE_M_MOM32
        same(mm[0], wm, "moving mean")
        same(mv[0], wv, "moving var", scale=float(np.abs(wv).max()) + float((R[0] ** 2).max()))
        Rs.append(R[0]); means.append(mean); istds.append(istd)
        A = Xn[0]
    NE = dk.dense_ref(A, inp["W"][L], inp["b"][L])
    dominates(NE, "NE")
    same(NE[0], ne, "NE")
    dP = dk.relu_gate_ref(inp["dNE"], NE[0])
    same(dP[0], pres[L].grad, f"dP{L}")
    dPl = dP[0]
    for l in range(L, 0, -1):
        dY = dk.dy_ref(dPl, inp["W"][l], mults[l - 1])
        dominates(dY, "dY")
        same(dY[0], bns[l - 1].grad, f"dY{l - 1}", scale=max(float(np.abs(dY[1]).max()), 1e-300))
        bb = dk.bn_bwd_stage(dY[0], Rs[l - 1], means[l - 1], istds[l - 1], inp["gamma"][l - 1], n0, n1)
        for k in ("ggamma", "gbeta", "dP"):
            dominates(bb[k], k)
        sc = max(float(bb["dP"][1].max()), 1e-300)
        same(bb["dP"][0], pres[l - 1].grad, f"dP{l - 1}", scale=sc)
        same(bb["ggamma"][0], gam[l - 1].grad, "ggamma", scale=max(float(bb["ggamma"][1].max()), 1e-300))
        same(bb["gbeta"][0], bet[l - 1].grad, "gbeta", scale=max(float(bb["gbeta"][1].max()), 1e-300))
        for s, (a, e) in enumerate(dk.sites(n0, n1)):  # the batch-norm pair of the training tail, per site, from the same xhat / istd
            if e > a:
                xh = (Rs[l - 1][a:e] - means[l - 1][s]) * istds[l - 1][s]
                t = tr.bn_bwd_ref(dY[0][a:e], xh, inp["gamma"][l - 1], istds[l - 1][s])
                same(bb["dP"][0][a:e], np.where(Rs[l - 1][a:e] > 0, t["dX"][0], 0.0), "dP vs bn_bwd_ref", scale=sc)
        dPl = bb["dP"][0]
    loss, parts = dk.l2_ref(inp["W"][:L], l2)
    want = dk.LOSS0 + float(np.float32(l2)) * sum(float((w.astype(np.float64) ** 2).sum()) for w in inp["W"][:L])
    same(loss[0], np.array([want]), "loss")
    assert (parts is None) == (l2 == 0)


# ------------------------------------------------------------------------------------------------------------ the stand-in, clean
def _run(shape, p, l2, defect=None, chain=False):
    n0, n1, din, units, e_out = shape
    inp = dk.case_inputs(n0, n1, din, units, e_out)
    with np.errstate(invalid="ignore"):
        out = dk.standin_step(inp, n0, n1, units, p, l2, defect=defect)
    seen = dk.check_step(out, inp, n0, n1, units, p, l2, what=f"{shape} p {p} l2 {l2}")
    if chain:
        dk.chain_check(out, inp, n0, n1, units, p, l2, assert_close, what=f"{shape}")
    return seen


@pytest.mark.parametrize("p,l2", dk.P_L2)
@pytest.mark.parametrize("name", list(dk.CASES))
def test_standin_passes_the_comparator_of_the_gpu_tests_and_the_chain_check(name, p, l2):
    seen = _run(dk.CASES[name], p, l2, chain=True)
    assert set(seen) >= {"dvn.R", "dvn.Xn", "dvn.NE", "dvn.dY", "dvn.dP", "dvn.ggamma", "dvn.gbeta", "dvn.moving_mean", "dvn.moving_var"}
    assert all(v < dk.C_SUM for v in seen.values()), seen


def test_standin_second_step_on_the_used_scratch_is_the_step_on_a_zero_scratch():
    n0, n1, din, units, e_out = dk.CASES["exact"]
    prev = dk.standin_step(dk.case_inputs(n0, n1, din, units, e_out, seed=5), n0, n1, units, 0.2, 1e-4)
    assert any(dk.stat_view(prev["stat"], units, l)["bwd"].any() for l in range(len(units)))  # the next forward call re-zeroes them
    inp = dk.case_inputs(n0, n1, din, units, e_out)
    a, b = dk.standin_step(inp, n0, n1, units, 0.2, 1e-4, stat0=prev["stat"]), dk.standin_step(inp, n0, n1, units, 0.2, 1e-4)
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.int32), np.asarray(b[k]).view(np.int32)), k


# ------------------------------------------------------------------------------------------------------------ planted defects
P_DEF, L2_DEF = 0.2, 1e-4
NEW_ONLY = {  # defect -> the listed cases that must catch it
    "slab_dropped": {"reload"},
    "site_from_floor_tiles": {"empty-history", "reload"},
    "moving_empty_twice": {"min", "empty-history"},
    "empty_site_stats_written": {"min", "empty-history"},
    "tile_of_one_row_dropped": {"min", "empty-history", "slab+4", "reload"},
    "dbn_constant_by_buffer": {"reload"},
}
CAUGHT_BY_OLD = ("site0_stats", "moving_once", "mask_site_relative", "clamp_dup", "aout_unowned_slab_skipped")


def _caught(shape, defect):
    try:
        _run(shape, P_DEF, L2_DEF, defect)
    except AssertionError:
        return True
    return False


def test_old_shapes_pass_clean():
    for shape in dk.OLD_SHAPES:
        _run(shape, P_DEF, L2_DEF)


@pytest.mark.parametrize("defect", list(NEW_ONLY))
def test_defect_caught_at_a_listed_case_and_missed_at_every_old_shape(defect):
    assert not any(_caught(shape, defect) for shape in dk.OLD_SHAPES), defect
    caught = {name for name, shape in dk.CASES.items() if _caught(shape, defect)}
    assert caught == NEW_ONLY[defect], (defect, caught)


@pytest.mark.parametrize("defect", CAUGHT_BY_OLD)
def test_plain_form_of_a_listed_defect_is_caught_at_the_old_shapes_too(defect):
    """said so, and replaced (module docstring): the comparator catches these at shapes tests/test_docvec_model.py already runs"""
    assert any(_caught(shape, defect) for shape in dk.OLD_SHAPES), defect
    assert any(_caught(shape, defect) for shape in dk.CASES.values()), defect
