"""Device path of the beyond-accuracy evaluation: the ebn_ba_* entry points through the C ABI, and the classes called with a
DeviceLookup, against the REFERENCE's outputs (tests/golden/beyond_accuracy_golden*.npz).

Bounds (derived, not measured).  Diversity, serendipity, candidate diversity: |hip - reference| <= (2 D + 80) * 2^-24 absolute
per list (9.6e-5 at D = 768, 1.6e-5 at D = 96): rounding the unit rows to fp32 and normalising in fp32 contribute at most about
(D + 8) * 2^-24 to a dot product of two unit vectors, a worst-case serial fp32 accumulation of D products another D * 2^-24, a
tree mean over at most 2^18 values in [0, 2] the rest; clipping and averaging do not enlarge it.  Anything structurally wrong
(diagonal, normalisation, divisor, a dropped id) is off by 1e-2 or more on these inputs.  Novelty and sentiment: 2^-20 of the
list's largest |term| (16 fp32 ulps: input rounding, a 2-ulp log2, a tree mean).  NaN positions: exact."""
import json

import numpy as np
import pytest

from tests import beyond_accuracy_cases as bc

pytestmark = pytest.mark.gpu
FAST_MAX = 10  # EBN_BA_FAST_MAX of csrc/ebn_beyond.hip: the last list length of the wave-per-list form


def dist_tol(D):
    return (2 * D + 80) * 2.0 ** -24


def check_dist(got, want, D, what):
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ from the reference"
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print(f"{what}: max abs err {err:.3e} (bound {dist_tol(D):.3e}, D = {D}, {int(ok.sum())} finite values)")
    assert err <= dist_tol(D), what
    return err


def check_mean(got, want, scale, what):
    """scale = the largest |term| of each list"""
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ from the reference"
    ok = ~np.isnan(want)
    rel = np.abs(got[ok] - want[ok]) / scale[ok]
    print(f"{what}: max err {float(rel.max()):.3e} of the largest term (bound {2.0 ** -20:.3e})")
    assert np.all(rel <= 2.0 ** -20), what


@pytest.fixture(scope="module", params=list(bc.CASES))
def case(request):
    from ebrec.evaluation.beyond_accuracy import DeviceLookup

    g = bc.load(request.param)
    lookup = bc.build_lookup(g)
    return {"g": g, "lookup": lookup, "R": bc.ragged(g, "R"), "H": bc.ragged(g, "H"), "U": g["universe"],
            "meta": json.loads(str(g["meta"])), "D": g["vec"].shape[1],
            "dl": DeviceLookup(lookup, vector_keys=(bc.VEC,), scalar_keys=(bc.POP, bc.SENT))}


def term_scale(lists, lookup, key, fn):
    out = np.full(len(lists), np.nan)
    for i, ids in enumerate(lists):
        t = [abs(fn(lookup[x][key])) for x in ids if x in lookup]
        if t:
            out[i] = max(max(t), 2.0 ** -126)
    return out


# ---- the classes with a DeviceLookup, on the whole golden input set -------------------------------------------------------
def test_classes_with_device_lookup_match_the_reference_and_the_dict_path(hip, case):
    from ebrec.evaluation.beyond_accuracy import IntralistDiversity, Novelty, Sentiment, Serendipity

    g, lookup, dl, D = case["g"], case["lookup"], case["dl"], case["D"]
    R, H, R2 = case["R"], case["H"], case["U"][g["R2"]]
    assert dl.holds(bc.VEC) and dl.holds(bc.POP) and not dl.holds(bc.CAT)
    for what, got, want, plain in (
            ("diversity", IntralistDiversity()(R, dl, bc.VEC), g["exp_diversity"], IntralistDiversity()(R, lookup, bc.VEC)),
            ("serendipity", Serendipity()(R, H, dl, bc.VEC), g["exp_serendipity"], Serendipity()(R, H, lookup, bc.VEC)),
            ("diversity 2-D", IntralistDiversity()(R2, dl, bc.VEC), g["exp_diversity_R2"], IntralistDiversity()(R2, lookup, bc.VEC))):
        check_dist(got, want, D, f"{what} vs reference")
        check_dist(got, plain, D, f"{what} vs plain dict")
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
        plain_s, plain_n = Sentiment()(R, lookup, bc.SENT), Novelty()(R, lookup, bc.POP)
    s_scale, n_scale = term_scale(R, lookup, bc.SENT, float), term_scale(R, lookup, bc.POP, np.log2)
    for what, got, want, plain, scale in (("sentiment", Sentiment()(R, dl, bc.SENT), g["exp_sentiment"], plain_s, s_scale),
                                          ("novelty", Novelty()(R, dl, bc.POP), g["exp_novelty"], plain_n, n_scale)):
        check_mean(got, want, scale, f"{what} vs reference")
        check_mean(got, plain, scale, f"{what} vs plain dict")
    check_mean(Sentiment()(R2, dl, bc.SENT), g["exp_sentiment_R2"], term_scale(R2, lookup, bc.SENT, float), "sentiment 2-D")
    check_mean(Novelty()(R2, dl, bc.POP), g["exp_novelty_R2"], term_scale(R2, lookup, bc.POP, np.log2), "novelty 2-D")
    with pytest.raises(ValueError):
        Serendipity()(R[:3], H[:2], dl, bc.VEC)


def test_candidate_diversity_on_the_device_matches_the_reference(hip, case):
    from ebrec.evaluation.beyond_accuracy import IntralistDiversity

    g, dl, m, D = case["g"], case["dl"], case["meta"], case["D"]
    small, large = case["U"][g["cand_small"]], case["U"][g["cand_large"]]
    before = hip.lib().ebn_launch_count()
    ex = m["cand_div_exhaustive"]
    got = IntralistDiversity()._candidate_diversity(small, ex["n"], dl, bc.VEC, max_number_combinations=ex["max"])
    assert hip.lib().ebn_launch_count() > before, "the candidate search did not run on the device"
    check_dist(np.asarray(got), ex["out"], D, "candidate diversity, every combination")
    sa = m["cand_div_sampled"]
    got = IntralistDiversity()._candidate_diversity(large, sa["n"], dl, bc.VEC, max_number_combinations=sa["max"], seed=sa["seed"])
    check_dist(np.asarray(got), sa["out"], D, "candidate diversity, seeded sampling")
    with pytest.raises(ValueError):
        IntralistDiversity()._candidate_diversity(small[:4], 5, dl, bc.VEC)


# ---- the entry points through the C ABI ---------------------------------------------------------------------------------
def _dev(a, dtype):
    from tests.hip_testutil import dev

    return dev(np.asarray(a), dtype=dtype) if np.asarray(a).size else dev(np.zeros(1), dtype=dtype)[:0]


def _csr(lists):
    import torch

    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.empty(0, np.int64)])
    return _dev(flat, torch.int32), _dev(off, torch.int64), int(off[-1])


def intralist(hip, unit, lists, form=0):
    import torch

    from tests.hip_testutil import P, S, host

    ids, off, n_ids = _csr(lists)
    out = torch.full((len(lists),), -7.0, device="cuda")
    hip.call("ebn_ba_intralist_f32", P(unit), unit.shape[0], unit.shape[1], P(ids), n_ids, P(off), len(lists), form, P(out), S())
    return host(out)


def cross(hip, unit, R, H, form=0):
    import torch

    from tests.hip_testutil import P, S, host

    ids_r, off_r, n_r = _csr(R)
    ids_h, off_h, n_h = _csr(H)
    out = torch.full((len(R),), -7.0, device="cuda")
    hip.call("ebn_ba_cross_f32", P(unit), unit.shape[0], unit.shape[1], P(ids_r), n_r, P(off_r), P(ids_h), n_h, P(off_h), len(R), form, P(out), S())
    return host(out)


def unit_table(hip, vec):
    import torch

    from tests.hip_testutil import P, S

    src = _dev(vec, torch.float32)
    dst = torch.empty_like(src)
    hip.call("ebn_ba_unit_rows_f32", P(src), P(dst), src.shape[0], src.shape[1], S())
    return dst


def host_diversity(vec, lists):
    """float64 host path of the package (pinned to the reference by tests/test_beyond_accuracy.py); ids are table rows, ids
    outside the table are missing"""
    from ebrec.evaluation.beyond_accuracy import IntralistDiversity

    lookup = {r: {"v": vec[r].astype(np.float64)} for r in range(len(vec))}
    return IntralistDiversity()([np.asarray(x, np.int64) for x in lists], lookup, "v")


def host_serendipity(vec, R, H):
    from ebrec.evaluation.beyond_accuracy import Serendipity

    lookup = {r: {"v": vec[r].astype(np.float64)} for r in range(len(vec))}
    return Serendipity()([np.asarray(x, np.int64) for x in R], [np.asarray(x, np.int64) for x in H], lookup, "v")


def test_unit_rows(hip):
    from tests.hip_testutil import host

    vec = bc.load("d96")["vec"]
    u = host(unit_table(hip, vec))
    want = vec.astype(np.float64)
    nrm = np.sqrt((want * want).sum(1))
    nrm[nrm == 0] = 1.0
    assert np.abs(u - want / nrm[:, None]).max() <= 2.0 ** -22  # |u| <= 1: an fp32 sum of squares, a square root, a division
    assert np.all(u[7] == 0.0)  # the zero row is divided by 1
    assert np.array_equal(u[10], u[11])


@pytest.mark.parametrize("D", [2, 30, 70, 96, 260, 516, 1028])
def test_every_width_and_both_forms_match_the_host_path(hip, D):
    """D % 4 != 0 takes the 4-byte loads, D = 70, 260, 516 have a partial last slab, D = 1028 is past the register form of the
    cross mean; lengths 0 ... 40 cover both forms."""
    rng = np.random.default_rng(D)
    vec = (rng.standard_normal((60, D)) + 0.5).astype(np.float32)
    vec[5] = 0.0
    vec[9] = vec[8]
    unit = unit_table(hip, vec)
    lists = [rng.integers(0, 60, n) for n in list(range(0, 41)) + [64, 65, 130]]
    lists[7][2], lists[20][5], lists[30][:] = 60, -1, 2**31 - 1  # missing ids; a list of missing ids only
    want = host_diversity(vec, lists)
    for form in (0, 1):
        check_dist(intralist(hip, unit, lists, form), want, D, f"D = {D}, form {form}")
    H = [rng.integers(0, 60, n) for n in rng.integers(0, 90, len(lists))]
    H[3][:] = 99
    want = host_serendipity(vec, lists, H)
    for form in (0, 1):
        check_dist(cross(hip, unit, lists, H, form), want, D, f"cross, D = {D}, form {form}")
        check_dist(cross(hip, unit, H, lists, form), want, D, f"cross, sides swapped, D = {D}, form {form}")


def test_fast_and_general_form_agree_where_they_hand_over(hip, case):
    """Lists of FAST_MAX positions are the last the wave-per-list form takes, FAST_MAX + 1 the first of the tiled form; form 1
    sends every list to the tiled form, so the same lists run through both."""
    g, D = case["g"], case["D"]
    rng = np.random.default_rng(5)
    n_rows = g["vec"].shape[0]
    unit = unit_table(hip, g["vec"])
    lists = [rng.integers(0, n_rows, n) for n in (FAST_MAX - 1, FAST_MAX, FAST_MAX + 1, FAST_MAX + 2) for _ in range(25)]
    lists += [np.array([7, 10, 11, 3, 4, 5, 6, 8, 9, 12][:n]) for n in (FAST_MAX, 5, 2)] + [np.array([7, 10, 11] + list(range(20, 28)))]
    auto, tiled, want = intralist(hip, unit, lists, 0), intralist(hip, unit, lists, 1), host_diversity(g["vec"], lists)
    check_dist(auto, tiled, D, "auto form vs tiled form")
    check_dist(auto, want, D, "auto form vs host")
    check_dist(tiled, want, D, "tiled form vs host")
    # the cross mean hands over on the SHORTER side of a pair
    hist = [rng.integers(0, n_rows, n) for n in (1, FAST_MAX, FAST_MAX + 1, 20, 64, 700) for _ in range(len(lists) // 6 + 1)][:len(lists)]
    for A, B in ((lists, hist), (hist, lists)):
        auto, tiled, want = cross(hip, unit, A, B, 0), cross(hip, unit, A, B, 1), host_serendipity(g["vec"], A, B)
        check_dist(auto, tiled, D, "cross: auto form vs tiled form")
        check_dist(auto, want, D, "cross: auto form vs host")
        check_dist(tiled, want, D, "cross: tiled form vs host")


def test_zero_row_repeated_ids_and_out_of_table_ids(hip, case):
    import torch

    from tests.hip_testutil import P, S, host

    g, D = case["g"], case["D"]
    n_rows = g["vec"].shape[0]
    unit = unit_table(hip, g["vec"])
    others = [r for r in range(n_rows) if r != 7]
    # the zero row: distance exactly 1 to everything
    assert np.all(intralist(hip, unit, [[7, r] for r in others[:40]]) == 1.0)
    assert np.all(intralist(hip, unit, [[7, r] for r in others[:40]], form=1) == 1.0)
    assert np.all(cross(hip, unit, [[7], others, [7, 7]], [others, [7], [7]]) == 1.0)
    ids = _dev(np.arange(n_rows), torch.int32)
    dist = torch.empty(n_rows * n_rows, device="cuda")
    hip.call("ebn_ba_pairdist_f32", P(unit), n_rows, D, P(ids), n_rows, P(dist), S())
    dist = host(dist).reshape(n_rows, n_rows)
    assert np.all(dist[7, others] == 1.0) and np.all(dist[others, 7] == 1.0) and np.all(np.diag(dist) == 0.0)
    assert dist.min() >= 0.0 and dist.max() <= 2.0 and np.abs(dist - dist.T).max() == 0.0
    # one id repeated n times: the off-diagonal copies keep their (about 0) distances, the list is defined
    for form in (0, 1):
        rep = intralist(hip, unit, [[3] * n for n in (2, 5, FAST_MAX, FAST_MAX + 1, 40, 250)], form)
        assert not np.isnan(rep).any() and np.all(np.abs(rep) <= dist_tol(D)), rep
    assert np.isnan(intralist(hip, unit, [[3], [], [n_rows], [-1, 3]])).all()  # fewer than two valid ids
    # ids outside the table are skipped as missing: same result as the list without them
    rng = np.random.default_rng(11)
    clean = [rng.integers(0, n_rows, n) for n in (2, 5, 8, 10, 11, 33, 64, 65, 250)]
    dirty = []
    for x in clean:
        y = list(x)
        for bad in (-1, n_rows, 2**31 - 1):
            y.insert(int(rng.integers(0, len(y) + 1)), bad)
        dirty.append(y)
    for form in (0, 1):
        check_dist(intralist(hip, unit, dirty, form), intralist(hip, unit, clean, form), D, f"ids outside the table, form {form}")
    hist = [rng.integers(0, n_rows, n) for n in (700, 1, 20, 20, 3, 64, 65, 16, 17)]
    check_dist(cross(hip, unit, dirty, hist), cross(hip, unit, clean, hist), D, "ids outside the table, cross")
    check_dist(cross(hip, unit, hist, dirty), cross(hip, unit, hist, clean), D, "ids outside the table, cross (history side)")
    assert np.isnan(cross(hip, unit, [[1, 2], [], [n_rows]], [[], [1], [2]])).all()


def test_offsets_outside_the_id_array_make_an_empty_list(hip):
    """The kernels never form an address from offsets they cannot trust: a span that runs backwards or past n_ids is empty."""
    import torch

    from tests.hip_testutil import P, S, host

    vec = bc.load("d96")["vec"]
    unit = unit_table(hip, vec)
    ids = _dev(np.array([1, 2, 3, 4, 5, 6, 8, 9]), torch.int32)
    off = _dev(np.array([0, 5, 3, 100]), torch.int64)
    out = torch.full((3,), -7.0, device="cuda")
    hip.call("ebn_ba_intralist_f32", P(unit), unit.shape[0], unit.shape[1], P(ids), 8, P(off), 3, 0, P(out), S())
    got = host(out)
    assert np.isnan(got[1]) and np.isnan(got[2])
    check_dist(got[:1], host_diversity(vec, [[1, 2, 3, 4, 5]]), 96, "the intact list")
    vals = _dev(np.arange(10) / 10 + 0.1, torch.float32)
    hip.call("ebn_ba_list_mean_f32", P(vals), 10, P(ids), 8, P(off), 3, 0, P(out), S())
    got = host(out)
    assert abs(got[0] - np.mean(np.array([1, 2, 3, 4, 5]) / 10 + 0.1)) < 1e-6 and np.isnan(got[1]) and np.isnan(got[2])


def test_list_mean_and_subset_sums_through_the_abi(hip):
    import torch

    from tests.hip_testutil import P, S, host

    rng = np.random.default_rng(3)
    vals = rng.uniform(1e-4, 1.0, 500).astype(np.float32)
    lists = [rng.integers(0, 500, n) for n in (0, 1, 2, 10, 63, 64, 65, 700)] + [[500, -1], [5, 500, 5]]
    ids, off, n_ids = _csr(lists)
    dv = _dev(vals, torch.float32)
    out = torch.full((len(lists),), -7.0, device="cuda")
    for transform, fn in ((0, lambda v: v), (1, lambda v: -np.log2(v))):
        hip.call("ebn_ba_list_mean_f32", P(dv), 500, P(ids), n_ids, P(off), len(lists), transform, P(out), S())
        terms = [fn(vals[[i for i in x if 0 <= i < 500]].astype(np.float64)) for x in lists]
        want = np.array([t.mean() if len(t) else np.nan for t in terms])
        scale = np.array([np.abs(t).max() if len(t) else np.nan for t in terms])
        check_mean(host(out), want, scale, f"list mean, transform {transform}")
    m, k = 37, 6
    dist = rng.uniform(0, 2, (m, m)).astype(np.float32)
    subsets = np.stack([rng.choice(m, k, replace=False) for _ in range(300)])
    subsets[4, 2], subsets[9, :] = m, -1  # an index outside the matrix is skipped; a tuple without a valid index is undefined
    subsets[11, 1:] = -1
    want = []
    for s in subsets:
        v = [i for i in s if 0 <= i < m]
        want.append(sum(float(dist[a, b]) for a in v for b in v if a != b) / (len(v) * (len(v) - 1)) if len(v) >= 2 else np.nan)
    out = torch.full((300,), -7.0, device="cuda")
    hip.call("ebn_ba_subset_sums_f32", P(_dev(dist, torch.float32)), m, P(_dev(subsets, torch.int32)), k, 300, P(out), S())
    got = host(out)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.nanmax(np.abs(got - np.array(want))) <= 2.0 * 2.0 ** -20


def test_empty_calls_launch_nothing_and_streams_agree(hip, case):
    import torch

    from tests.hip_testutil import P, S, host

    g = case["g"]
    unit = unit_table(hip, g["vec"])
    n_rows, D = unit.shape
    lib = hip.lib()
    one = torch.zeros(4, device="cuda")
    i32, i64 = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    before = lib.ebn_launch_count()
    assert lib.ebn_ba_unit_rows_f32(P(unit), P(unit), 0, D, S()) == 0
    assert lib.ebn_ba_intralist_f32(P(unit), n_rows, D, P(i32), 0, P(i64), 0, 0, P(one), S()) == 0
    assert lib.ebn_ba_cross_f32(P(unit), n_rows, D, P(i32), 0, P(i64), P(i32), 0, P(i64), 0, 0, P(one), S()) == 0
    assert lib.ebn_ba_pairdist_f32(P(unit), n_rows, D, P(i32), 0, P(one), S()) == 0
    assert lib.ebn_ba_list_mean_f32(P(one), 4, P(i32), 0, P(i64), 0, 1, P(one), S()) == 0
    assert lib.ebn_ba_subset_sums_f32(P(one), 2, P(i32), 2, 0, P(one), S()) == 0
    assert lib.ebn_launch_count() == before, "an empty call launched a kernel"
    assert lib.ebn_ba_intralist_f32(None, n_rows, D, P(i32), 4, P(i64), 1, 0, P(one), S()) == -1
    assert lib.ebn_ba_intralist_f32(P(unit), n_rows, D, P(i32), 4, P(i64), 1, 2, P(one), S()) == -1
    assert lib.ebn_ba_list_mean_f32(P(one), 4, P(i32), 4, P(i64), -1, 0, P(one), S()) == -1
    # a non-default stream computes the same bits
    R, H = case["R"], case["H"]
    rows = {str(i): r for r, i in enumerate(g["ids"])}
    Rr = [[rows.get(str(x), -1) for x in r] for r in R]
    Hr = [[rows.get(str(x), -1) for x in h] for h in H]
    base_d, base_c = intralist(hip, unit, Rr), cross(hip, unit, Rr, Hr)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        side_d, side_c = intralist(hip, unit, Rr), cross(hip, unit, Rr, Hr)
    side.synchronize()
    assert np.array_equal(base_d, side_d, equal_nan=True) and np.array_equal(base_c, side_c, equal_nan=True)
    check_dist(base_d, g["exp_diversity"], case["D"], "C ABI diversity vs reference")
    check_dist(base_c, g["exp_serendipity"], case["D"], "C ABI serendipity vs reference")
