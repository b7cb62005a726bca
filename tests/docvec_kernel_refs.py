"""Float64 references of the fused NRMSDocVec launches (csrc/ebn_docvec.hip), stage by stage (plain module: no fixtures, nothing
collected): ebn_dvn_fwd_train_f32 = n_layers + 1 launches of dvn_panel_kernel, ebn_dvn_bwd_f32 = n_layers more + dvn_dbn_apply_kernel.

Written from the header comment of include/ebnerd_hip.h, the layout comment at `stat_view` and the formulae of the reference model.
The conventions are those of tests/training_tail_refs.py / tests/model_kernel_refs.py: every reference is a pair (value, magnitude),
the magnitude being the same expression with every term replaced by its absolute value, and the comparison is their check_close:

    |got - want| <= c * magnitude + TINY   element-wise, c = C_SUM = 2e-6 for every output; a NaN or inf in `got` fails.

Every stage is judged on its OWN step, from the launch's own earlier outputs taken as exact inputs (the `given=` idea of
training_tail_refs.head_ref): R[l] from the Xn[l-1] the kernel wrote, the statistics from its R[l], Xn[l] from its R[l] and its
statistics, ... -- a magnitude of one step, and a launch that consumed anything but what the launch in front wrote fails its stage.

  stage            from                                           magnitude
  R[l], NE         Xn[l-1] (X0), W, b                              |x|.|W| + |b|
  mean[s]          R[l], rows of site s                            mean|x| + tiles 2^-33 / n  (*)
  istd[s]          R[l]                                            istd + istd^3 / 2 * (E[x^2] + 2 |mean| mag(mean) + tiles 2^-29 / n (*))
                   -- the kernel's variance is E[x^2] - mean^2 (float64, from two fixed-point sums): its magnitude is E[x^2], not the variance
  Xn[l]            R[l], the kernel's mean / istd, gamma, beta     ((|x| + |mean|) istd |gamma| + |beta|) mult; zero pattern == the keep mask
  moving mean/var  the kernel's mean; the variance from R[l]       history site first, then candidates, an empty site: no update; the
                                                                   float32 model's momentum 0.99f and 1 - 0.99f = 0.0099999905 (not 0.01)
  dP[L]            dNE, the kernel's NE > 0                        exact (a gate)
  dY[l-1]          dP[l], W[l], mask, scale                        (|dP|.|W|^T) mult; zero where dropped
  gbeta / ggamma   dY[l], R[l], the kernel's mean / istd           sum |dy| / sum |dy| (|x| + |mean|) istd, + tiles 2^-41 (*)
  dP[l], l < L     the same; the gate is the kernel's R[l] > 0     |k| (|dy| + mag(s1) + mag(xhat) |s2| + |xhat| mag(s2)), k = gamma istd
  loss, l2_part    W                                               |loss0| + l2 sum W^2; the column-tile sums themselves

(*) the absolute terms of the fixed-point accumulators, DERIVED from their scales (FIX_SUM = 2^32, FIX_SQ = 2^28, FIX_GRAD = 2^40 in the
kernel): every tile addend is rounded to an integer, half a unit each.  check_close has no absolute term, so they are carried inside the
magnitude as term / C_SUM.

The whole chain from the inputs is checked as well, against oracle.nrms_numpy at the bounds of tests/test_docvec_model.py (chain_check).

`standin_step` is a float32 numpy stand-in of the two calls with the kernel's structure (row tiles per site, 128-deep slabs, per-tile
fixed-point sums, the Aout writer rule, the `stat` layout); tests/test_docvec_kernel_refs_cpu.py runs it through check_step -- the
comparator of the GPU tests -- clean and with planted defects."""
import numpy as np

from oracle import nrms_numpy as on
from tests import training_tail_refs as tr
from tests.model_kernel_refs import C_SUM, TINY, check_close, f64, ratio  # noqa: F401  (re-exported)

TM, TN, TK, MAX_K, L2_SLOTS, MAX_LAYERS = 32, 64, 128, 1024, 16, 4
FIX_SUM, FIX_SQ, FIX_GRAD = 2.0 ** 32, 2.0 ** 28, 2.0 ** 40
SITE_MLP0 = 8
EPS32 = float(np.float32(1e-3))                     # BN_EPS as the kernel (and the float32 model) holds it
MOM32 = float(np.float32(0.99))
ONE_M_MOM32 = float(np.float32(1.0) - np.float32(0.99))  # 0.0099999905: exact in float32
LOSS0 = 0.75                                        # the non-zero payload of loss[0]

# (n0, n1, din, units, e_out): the smallest shapes at which each loop takes no, one and a second trip and each clamp is touched
CASES = {
    "min": (1, 0, 4, [4], 4),
    "empty-history": (0, 33, 28, [36], 20),
    "exact": (31, 32, 128, [64, 60], 68),
    "slab+4": (33, 65, 132, [68, 132, 100], 4),
    "reload": (32, 1, 516, [516, 512], 64),
    "max-k": (5, 3, 100, [1024], 260),
    "four-layers": (40, 24, 64, [64, 48, 40, 36], 96),
    "apply-252": (2, 2, 8, [252], 8),
    "apply-256": (2, 2, 8, [256], 8),
    "apply-260": (2, 2, 8, [260], 8),
}
P_L2 = [(0.0, 0.0), (0.2, 1e-4)]
# what tests/test_docvec_model.py::test_train_step_gradients_loss_and_moving_stats runs: n0 = 7 B, n1 = 5 B, E = 32
OLD_SHAPES = [(7 * B, 5 * B, din, units, 32) for units, din, B in
              [([48, 40], 64, 8), ([200, 136, 72], 300, 24), ([36], 20, 3), ([4], 20, 3), ([260, 68], 96, 8), ([64, 48, 40, 36], 64, 8), ([1024], 100, 4)]]
SEED, STEP = 11, 6


def row_tiles(n):
    return -(-int(n) // TM)


def sites(n0, n1):
    return [(0, n0), (n0, n0 + n1)]


def with_abs(mag, abs_term):
    """a magnitude that also admits the absolute error `abs_term` under the constant C_SUM"""
    return mag + abs_term / C_SUM


# ------------------------------------------------------------------------------------------------------------ inputs, stat layout
def case_inputs(n0, n1, din, units, e_out, seed=0):
    """float32 operands of one step; He-scaled kernels keep every layer O(1); row 1 is a zero document vector (a padded slot)."""
    rng = np.random.default_rng(1000 * n0 + 10 * n1 + din + sum(units) + e_out + seed)
    n, dims = n0 + n1, [din] + list(units) + [e_out]
    X0 = rng.standard_normal((n, din)).astype(np.float32)
    if n > 2:
        X0[1] = 0
    inp = dict(X0=X0, W=[], b=[], gamma=[], beta=[], mm=[], mv=[])
    for l in range(len(dims) - 1):
        inp["W"].append((rng.standard_normal((dims[l], dims[l + 1])) * np.sqrt(2.0 / dims[l])).astype(np.float32))
        inp["b"].append((0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32))
    for u in units:
        inp["gamma"].append((1 + 0.1 * rng.standard_normal(u)).astype(np.float32))
        inp["beta"].append((0.1 * rng.standard_normal(u)).astype(np.float32))
        inp["mm"].append((0.1 * rng.standard_normal(u)).astype(np.float32))
        inp["mv"].append((1 + 0.2 * rng.random(u)).astype(np.float32))
    inp["dNE"] = (0.1 * rng.standard_normal((n, e_out))).astype(np.float32)
    return inp


def stat_floats(units):
    return 20 * sum(units) + MAX_LAYERS * L2_SLOTS


def stat_view(stat, units, l):
    """views into a float32 `stat` array (the layout at stat_view in the kernel file): fwd / bwd int64 [2 sums][2 sites][u], mean / istd [2][u]"""
    stat = np.asarray(stat)
    assert stat.dtype == np.float32 and stat.shape == (stat_floats(units),)
    U, before, u = sum(units), sum(units[:l]), units[l]
    acc = lambda o: stat[o:o + 8 * u].view(np.int64).reshape(2, 2, u)
    m0 = 16 * U + 4 * before
    return dict(fwd=acc(8 * before), bwd=acc(8 * U + 8 * before), mean=stat[m0:m0 + 2 * u].reshape(2, u), istd=stat[m0 + 2 * u:m0 + 4 * u].reshape(2, u))


def l2_view(stat, units):
    o = 20 * sum(units)
    return np.asarray(stat)[o:o + MAX_LAYERS * L2_SLOTS].reshape(MAX_LAYERS, L2_SLOTS)


def drop_mults(n0, n1, units, p, seed=SEED, step=STEP):
    """per layer the float32 multipliers [n, u] as the kernels form them; the mask is indexed by GLOBAL row: site 1 starts at n0"""
    n = n0 + n1
    return [tr.drop_mult32(seed, step, SITE_MLP0 + l, n * u, p).reshape(n, u) for l, u in enumerate(units)]


# ------------------------------------------------------------------------------------------------------------ stages
def dense_ref(A, W, b):
    A, W, b = f64(A), f64(W), f64(b)
    return np.maximum(A @ W + b, 0.0), np.abs(A) @ np.abs(W) + np.abs(b)


def stats_ref(R, n0, n1):
    """per site (None for an empty one): mean, istd, var as (value, mag), from E[x] and E[x^2] over the site's rows"""
    R, out = f64(R), []
    for a, e in sites(n0, n1):
        n = e - a
        if n == 0:
            out.append(None)
            continue
        x, t = R[a:e], row_tiles(n)
        mean, mmean = x.mean(0), with_abs(np.abs(x).mean(0), t * 2.0 ** -33 / n)
        e2 = (x * x).mean(0)
        var = np.maximum(e2 - mean * mean, 0.0)
        mvar = with_abs(e2, t * 2.0 ** -29 / n) + 2.0 * np.abs(mean) * mmean
        istd = 1.0 / np.sqrt(var + EPS32)
        out.append(dict(mean=(mean, mmean), var=(var, mvar), istd=(istd, istd + 0.5 * istd ** 3 * mvar)))
    return out


def xn_ref(R, mean, istd, gamma, beta, mult, n0, n1):
    """Dropout(BatchNormalization(R)) with the given per-site statistics [2][u]; rows of an empty site: none"""
    R, mean, istd, gamma, beta, mult = f64(R), f64(mean), f64(istd), f64(gamma), f64(beta), f64(mult)
    v, m = np.zeros_like(R), np.zeros_like(R)
    for s, (a, e) in enumerate(sites(n0, n1)):
        x = R[a:e]
        v[a:e] = ((x - mean[s]) * istd[s] * gamma + beta) * mult[a:e]
        m[a:e] = ((np.abs(x) + np.abs(mean[s])) * istd[s] * np.abs(gamma) + np.abs(beta)) * mult[a:e]
    return v, m


def moving_ref(mm0, mv0, R, mean, n0, n1):
    """one update per non-empty site, history first: from the kernel's means [2][u] and the variance of its R"""
    mm, mv, mean = f64(mm0), f64(mv0), f64(mean)
    gm, gv = np.abs(mm), np.abs(mv)
    for s, st in enumerate(stats_ref(R, n0, n1)):
        if st is None:
            continue
        var, mvar = st["var"]
        mm, gm = mm * MOM32 + mean[s] * ONE_M_MOM32, gm * MOM32 + np.abs(mean[s]) * ONE_M_MOM32
        mv, gv = mv * MOM32 + var * ONE_M_MOM32, gv * MOM32 + (var + mvar) * ONE_M_MOM32
    return (mm, gm), (mv, gv)


def relu_gate_ref(dOut, Out):
    v = np.where(f64(Out) > 0, f64(dOut), 0.0)
    return v, np.abs(v)


def dy_ref(dP, W, mult):
    dP, W, mult = f64(dP), f64(W), f64(mult)
    return (dP @ W.T) * mult, (np.abs(dP) @ np.abs(W).T) * mult


def bn_bwd_stage(dY, R, mean, istd, gamma, n0, n1):
    """ggamma, gbeta (both sites together) and dP = relu'(R) * BatchNormalization-backward(dY) per site, from the kernel's dY, R, mean, istd"""
    dY, R, mean, istd, gamma = f64(dY), f64(R), f64(mean), f64(istd), f64(gamma)
    u = R.shape[1]
    gg, mgg, gb, mgb = np.zeros(u), np.zeros(u), np.zeros(u), np.zeros(u)
    dP, mdP = np.zeros_like(R), np.zeros_like(R)
    for s, (a, e) in enumerate(sites(n0, n1)):
        n = e - a
        if n == 0:
            continue
        g, x = dY[a:e], R[a:e]
        absq = row_tiles(n) * 2.0 ** -41
        xh, mxh = (x - mean[s]) * istd[s], (np.abs(x) + np.abs(mean[s])) * istd[s]
        sd, msd = g.sum(0), with_abs(np.abs(g).sum(0), absq)
        sx, msx = (g * xh).sum(0), with_abs((np.abs(g) * mxh).sum(0), absq)
        k = gamma * istd[s]
        s1, s2 = sd / n, sx / n
        dr = k * (g - s1 - xh * s2)
        mdr = np.abs(k) * (np.abs(g) + msd / n + mxh * np.abs(s2) + np.abs(xh) * msx / n)
        dP[a:e], mdP[a:e] = np.where(x > 0, dr, 0.0), np.where(x > 0, mdr, 0.0)
        gg, mgg, gb, mgb = gg + sx, mgg + msx, gb + sd, mgb + msd
    return dict(ggamma=(gg, mgg), gbeta=(gb, mgb), dP=(dP, mdP))


def l2_ref(Ws, l2, loss0=LOSS0):
    """loss[0] = loss0 + l2 * sum_l sum W[l]^2 over the hidden kernels, and the [MAX_LAYERS][L2_SLOTS] column-tile sums of squares"""
    l2 = float(np.float32(l2))
    parts = np.zeros((MAX_LAYERS, L2_SLOTS))
    for l, W in enumerate(Ws):
        sq = f64(W) ** 2
        for t in range(-(-W.shape[1] // TN)):
            parts[l, t] = sq[:, t * TN:(t + 1) * TN].sum()
    if l2 <= 0:
        return (np.array([loss0]), np.array([abs(loss0)])), None
    return (np.array([loss0 + l2 * parts.sum()]), np.array([abs(loss0) + l2 * parts.sum()])), (parts, parts)


# ------------------------------------------------------------------------------------------------------------ the comparator
def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def check_step(out, inp, n0, n1, units, p, l2, stat0=None, cmp=None, what=""):
    """Every output of one forward + backward pair (`out`: name -> float32 array as the calls left it, `stat` the whole scratch, `stat0`
    the scratch before the step, default zeros) against the stage references.  `cmp(key, got, ref, what)` defaults to check_close at
    C_SUM.  -> {key: largest err / mag}"""
    seen = {}

    def default_cmp(key, got, ref, w):
        seen[key] = max(seen.get(key, 0.0), ratio(np.asarray(got, np.float64).reshape(np.shape(ref[0])), ref[0], ref[1]))
        check_close(got, ref, C_SUM, f"{key} {w}")

    cmp = default_cmp if cmp is None else cmp
    L, n = len(units), n0 + n1
    stat = np.asarray(out["stat"], np.float32)
    stat0 = np.zeros_like(stat) if stat0 is None else np.asarray(stat0, np.float32)
    mults = drop_mults(n0, n1, units, p)
    ns = (n0, n1)
    A = inp["X0"]
    for l in range(L):
        w = f"{what} layer {l}"
        R, sv, sv0 = out[f"R{l}"], stat_view(stat, units, l), stat_view(stat0, units, l)
        cmp("dvn.R", R, dense_ref(A, inp["W"][l], inp["b"][l]), w)
        for s, st in enumerate(stats_ref(R, n0, n1)):
            if st is None:  # an empty site: its mean | istd block is untouched
                assert np.array_equal(_bits(sv["mean"][s]), _bits(sv0["mean"][s])) and np.array_equal(_bits(sv["istd"][s]), _bits(sv0["istd"][s])), \
                    f"{w}: the mean | istd block of the empty site {s} was written"
                continue
            cmp("dvn.mean", sv["mean"][s], st["mean"], f"{w} site {s}")
            cmp("dvn.istd", sv["istd"][s], st["istd"], f"{w} site {s}")
        mean = np.where(np.array(ns)[:, None] > 0, sv["mean"], 0.0)  # (rows of an empty site: none -- its block may hold anything)
        istd = np.where(np.array(ns)[:, None] > 0, sv["istd"], 0.0)
        Xn = np.asarray(out[f"Xn{l}"])
        ref = xn_ref(R, mean, istd, inp["gamma"][l], inp["beta"][l], mults[l], n0, n1)
        cmp("dvn.Xn", Xn, ref, w)
        assert np.array_equal(Xn == 0, (mults[l] == 0) | (ref[1] == 0)), f"{w}: the zero pattern of Xn is not the dropout mask"
        mm, mv = moving_ref(inp["mm"][l], inp["mv"][l], R, mean, n0, n1)
        cmp("dvn.moving_mean", out[f"moving_mean{l}"], mm, w)
        cmp("dvn.moving_var", out[f"moving_var{l}"], mv, w)
        A = Xn
    cmp("dvn.NE", out["NE"], dense_ref(A, inp["W"][L], inp["b"][L]), what)
    want = np.where(np.asarray(out["NE"]) > 0, inp["dNE"], np.float32(0))
    assert np.array_equal(_bits(out[f"dP{L}"]), _bits(want)), f"{what}: dP[{L}] is not dNE gated by the kernel's NE > 0, bit for bit"
    for l in range(L, 0, -1):
        w = f"{what} layer {l - 1}"
        sv = stat_view(stat, units, l - 1)
        mean = np.where(np.array(ns)[:, None] > 0, sv["mean"], 0.0)
        istd = np.where(np.array(ns)[:, None] > 0, sv["istd"], 0.0)
        dY = np.asarray(out[f"dY{l - 1}"])
        ref = dy_ref(out[f"dP{l}"], inp["W"][l], mults[l - 1])
        cmp("dvn.dY", dY, ref, w)
        assert ((dY == 0) | (mults[l - 1] != 0)).all(), f"{w}: dY is not zero where the mask drops"
        assert np.array_equal(dY == 0, (mults[l - 1] == 0) | (ref[1] == 0)), f"{w}: the zero pattern of dY is not the dropout mask"
        bb = bn_bwd_stage(dY, out[f"R{l - 1}"], mean, istd, inp["gamma"][l - 1], n0, n1)
        cmp("dvn.ggamma", out[f"ggamma{l - 1}"], bb["ggamma"], w)
        cmp("dvn.gbeta", out[f"gbeta{l - 1}"], bb["gbeta"], w)
        cmp("dvn.dP", out[f"dP{l - 1}"], bb["dP"], w)
        assert not np.asarray(out[f"dP{l - 1}"])[np.asarray(out[f"R{l - 1}"]) <= 0].any(), f"{w}: dP is not zero where the kernel's R is"
    loss_ref, parts_ref = l2_ref(inp["W"][:L], l2)
    if parts_ref is None:  # no regulariser: the loss keeps its bits, the slots stay as they were
        assert np.array_equal(_bits(out["loss"]), _bits([LOSS0])) and np.array_equal(_bits(l2_view(stat, units)), _bits(l2_view(stat0, units))), what
    else:
        cmp("dvn.loss", out["loss"], loss_ref, what)
        cmp("dvn.l2_part", l2_view(stat, units)[:L], (parts_ref[0][:L], parts_ref[1][:L]), what)
    for l in range(L):  # (the BACKWARD accumulators keep the step's sums until the next forward call re-zeroes them: see the GPU module)
        assert not stat_view(stat, units, l)["fwd"].any(), f"{what}: the forward accumulators of layer {l} are not all-zero bits after the step"
    assert int(np.asarray(out["range_flag"]).reshape(-1)[0]) == 0, f"{what}: range_flag raised"
    return seen


# ------------------------------------------------------------------------------------------------------------ the whole chain
class TieGate:
    """tests/hip_testutil.ReluTieGate for bare arrays: ReLU inputs the float64 oracle puts within `rel` of 0 (relative to the layer's
    largest) take the KERNEL's side; every other element keeps the oracle's.  (Only chain_check uses it: the stage references gate with
    the kernel's own R > 0 and need none.)"""

    def __init__(self, on_mask, rows, rel=3e-6):
        self.on, self.rows, self.rel = on_mask, rows, rel

    def __call__(self, layer, pre):
        tie = (np.abs(pre) <= self.rel * np.abs(pre).max()) & (pre != 0)
        return np.where(tie, self.on[layer][self.rows], pre > 0) if tie.any() else None


def chain_check(out, inp, n0, n1, units, p, l2, assert_close, what=""):
    """the whole chain from the inputs against oracle.nrms_numpy at the bounds tests/test_docvec_model.py sets: NE 2e-5 + 2e-5 |want|,
    parameter gradients (dW = Xn^T . dP and the column sums of dP formed in float64 from the kernel's outputs, ggamma / gbeta as they are)
    rtol 2e-4 + 2e-4 max |want| + 1e-6, moving statistics 1e-5 / 1e-6, the loss 3e-5 max(1, |L|)"""
    L = len(units)
    P = {"units": list(units), "out_W": f64(inp["W"][L]), "out_b": f64(inp["b"][L])}
    for l in range(L):
        P[f"d{l}_W"], P[f"d{l}_b"], P[f"bn{l}_g"], P[f"bn{l}_b"] = f64(inp["W"][l]), f64(inp["b"][l]), f64(inp["gamma"][l]), f64(inp["beta"][l])
        P[f"bn{l}_mean"], P[f"bn{l}_var"] = f64(inp["mm"][l]), f64(inp["mv"][l])
    on_mask = [np.asarray(out[f"R{l}"]) > 0 for l in range(L)] + [np.asarray(out["NE"]) > 0]
    drop = on.Drop(p, SEED, STEP) if p > 0 else None
    g, stats_seq, NE = {}, [], np.zeros_like(f64(out["NE"]))
    for a, e in sites(n0, n1):
        if e == a:
            continue
        ne, cache, st = on.docvec_news_encoder_fwd(f64(inp["X0"][a:e]), P, True, drop, 0, a)
        NE[a:e] = ne
        stats_seq.append(st)
        gs, _ = on.docvec_news_encoder_bwd(f64(inp["dNE"][a:e]), cache, P, TieGate(on_mask, slice(a, e)))
        for k, v in gs.items():
            g[k] = g.get(k, 0.0) + v
    assert_close(out["NE"], NE, rtol=2e-5, atol=2e-5, what=f"chain NE {what}")
    acts = [inp["X0"]] + [out[f"Xn{l}"] for l in range(L)]
    for l in range(L + 1):
        wn, bn = (f"d{l}_W", f"d{l}_b") if l < L else ("out_W", "out_b")
        dP = f64(out[f"dP{l}"])
        got = {wn: f64(acts[l]).T @ dP, bn: dP.sum(0)}
        if l < L:
            got[f"bn{l}_g"], got[f"bn{l}_b"] = f64(out[f"ggamma{l}"]), f64(out[f"gbeta{l}"])
        for k, v in got.items():
            assert_close(v, g[k], rtol=2e-4, atol=1e-6 + 2e-4 * np.abs(g[k]).max(), what=f"chain d{k} {what}")
    Pn = dict(P)
    on.bn_update_moving(Pn, stats_seq)
    for l in range(L):
        assert_close(out[f"moving_mean{l}"], Pn[f"bn{l}_mean"], rtol=1e-5, atol=1e-6, what=f"chain moving mean {l} {what}")
        assert_close(out[f"moving_var{l}"], Pn[f"bn{l}_var"], rtol=1e-5, atol=1e-6, what=f"chain moving var {l} {what}")
    Lw = LOSS0 + l2 * sum(float((P[f"d{l}_W"] ** 2).sum()) for l in range(L))
    assert abs(float(np.asarray(out["loss"]).reshape(-1)[0]) - Lw) <= 3e-5 * max(1.0, abs(Lw)), (what, out["loss"], Lw)


# ------------------------------------------------------------------------------------------------------------ numpy stand-in
F32 = np.float32
DEFECTS = ("slab_dropped", "site0_stats", "site_from_floor_tiles", "moving_once", "moving_empty_twice", "mask_site_relative",
           "empty_site_stats_written", "clamp_dup", "tile_of_one_row_dropped", "aout_unowned_slab_skipped", "dbn_constant_by_buffer")


def _fix(x, scale):
    return np.rint(np.asarray(x, np.float64) * scale).astype(np.int64)


def standin_step(inp, n0, n1, units, p, l2, stat0=None, defect=None):
    """float32 numpy stand-in of ebn_dvn_fwd_train_f32 + ebn_dvn_bwd_f32 (every output starts as NaN: what is never written stays NaN).
    defect (one of DEFECTS):
      slab_dropped               the partial last slab of a matmul is dropped when nk > 4 (the register-set reload)
      site0_stats                site 1's rows are normalised with site 0's statistics
      site_from_floor_tiles      ... only where the number of history tiles is taken as n0 / 32 + 1 (wrong when n0 % 32 == 0)
      moving_once                one moving-average update for both sites (the candidate site's is lost)
      moving_empty_twice         an update for an EMPTY site too (mean 0, variance 0)
      mask_site_relative         the dropout index of site 1 counted from the site's first row
      empty_site_stats_written   the mean | istd block of an empty site is written (0 and 1 / sqrt(eps))
      clamp_dup                  the last four columns of every B tile are loaded from the four in front (the clamp one float4 early)
      tile_of_one_row_dropped    row tiles counted as (n + 30) / 32: a last tile holding exactly one row is never launched
      aout_unowned_slab_skipped  the Aout writer of slab kt is tile kt instead of kt mod #tiles: slabs kt >= #tiles are never written
      dbn_constant_by_buffer     the constant term of the d(BatchNormalization) transform is indexed by LDS buffer (kt & 1), not by slab"""
    assert defect is None or defect in DEFECTS, defect
    L, n, dims = len(units), n0 + n1, [inp["X0"].shape[1]] + list(units) + [inp["W"][-1].shape[1]]
    ns = (n0, n1)
    stat = np.zeros(stat_floats(units), F32) if stat0 is None else np.array(stat0, F32)
    nan = lambda *s: np.full(s, np.nan, F32)
    out = dict(stat=stat, range_flag=np.zeros(1, np.int32), loss=np.array([LOSS0], F32))
    scale = F32(1) / (F32(1) - F32(p)) if p > 0 else F32(1)
    mults = drop_mults(n0, n1, units, p)
    if defect == "mask_site_relative" and p > 0:
        mults = [np.concatenate([m[:n0], tr.drop_mult32(SEED, STEP, SITE_MLP0 + l, n1 * u, p).reshape(n1, u)]) for l, (m, u) in enumerate(zip(mults, units))]

    def tiles():  # (site, first row, end row of the site) of every launched row tile
        cnt = (lambda m: (m + TM - 2) // TM) if defect == "tile_of_one_row_dropped" else row_tiles
        return [(s, a + t * TM, e) for s, (a, e) in enumerate(sites(n0, n1)) for t in range(cnt(e - a))]

    def stat_site(s, row0):
        if defect == "site0_stats":
            return 0
        if defect == "site_from_floor_tiles":  # the tile index against n0 / 32 + 1 history tiles
            ty = row0 // TM if s == 0 else row_tiles(n0) + (row0 - n0) // TM
            return 1 if ty >= n0 // TM + 1 else 0
        return s

    def matmul(A, B):  # A [rows, K] . B [K, N], slab by slab in float32
        K = A.shape[1]
        nk, nk_full = -(-K // TK), K // TK
        if defect == "clamp_dup" and B.shape[1] >= 8:
            cols = np.arange(B.shape[1])
            last = (cols % TN >= TN - 4) | (cols >= B.shape[1] - 4)
            B = B[:, np.where(last, cols - 4, cols)]
        acc = np.zeros((A.shape[0], B.shape[1]), F32)
        for kt in range(nk):
            if defect == "slab_dropped" and nk > 4 and kt >= nk_full:
                continue
            acc += A[:, kt * TK:(kt + 1) * TK] @ B[kt * TK:(kt + 1) * TK]
        return acc

    def write_aout(dst, T, r0, r1, Nout):  # slab kt of the transformed operand is written by column tile kt mod #tiles
        K, ntx = T.shape[1], -(-Nout // TN)
        for kt in range(-(-K // TK)):
            if defect == "aout_unowned_slab_skipped" and kt >= ntx:
                continue
            dst[r0:r1, kt * TK:(kt + 1) * TK] = T[:, kt * TK:(kt + 1) * TK]

    # ---- forward
    A = inp["X0"]
    for l in range(L + 1):
        K, Nout = dims[l], dims[l + 1]
        C = nan(n, Nout)
        if l > 0:  # the A transform: statistics of layer l - 1 from its accumulators
            sv = stat_view(stat, units, l - 1)
            mean, var, istd = np.zeros((2, K), F32), np.zeros((2, K), F32), np.zeros((2, K), F32)
            for s in range(2):
                inv = 1.0 / ns[s] if ns[s] > 0 else 0.0
                m = sv["fwd"][0, s] / FIX_SUM * inv
                v = sv["fwd"][1, s] / FIX_SQ * inv - m * m
                mean[s], var[s] = m.astype(F32), np.maximum(v, 0).astype(F32)
                istd[s] = F32(1) / np.sqrt(var[s] + F32(1e-3))
            mmv, mvv = inp["mm"][l - 1].copy(), inp["mv"][l - 1].copy()
            for s in range(2):
                upd = ns[s] > 0 or defect == "moving_empty_twice"
                if defect == "moving_once" and s == 1:
                    upd = False
                if upd:
                    mmv = mmv * F32(0.99) + mean[s] * (F32(1) - F32(0.99))
                    mvv = mvv * F32(0.99) + var[s] * (F32(1) - F32(0.99))
                if ns[s] > 0 or defect == "empty_site_stats_written":
                    sv["mean"][s], sv["istd"][s] = mean[s], istd[s]
            out[f"moving_mean{l - 1}"], out[f"moving_var{l - 1}"] = mmv, mvv
            Xn = nan(n, K)
        for s, r0, e in tiles():
            r1 = min(r0 + TM, e)
            a = A[r0:r1]
            if l > 0:
                ss = stat_site(s, r0)
                gs = inp["gamma"][l - 1] * istd[ss]
                a = (a * (gs * scale) + (inp["beta"][l - 1] - mean[ss] * gs) * scale).astype(F32)
                a = np.where(mults[l - 1][r0:r1] != 0, a, F32(0))
                write_aout(Xn, a, r0, r1, Nout)
            c = np.maximum(matmul(a, inp["W"][l]) + inp["b"][l], F32(0))
            C[r0:r1] = c
            if l < L:
                acc = stat_view(stat, units, l)["fwd"]
                acc[0, s] += _fix(c.sum(0, dtype=F32), FIX_SUM)
                acc[1, s] += _fix((c * c).sum(0, dtype=F32), FIX_SQ)
        if l > 0:
            out[f"Xn{l - 1}"] = Xn
        out[f"R{l}" if l < L else "NE"] = C
        A = C  # the launch behind transforms the relu output on its way into the tiles
        if l < L and l2 > 0:
            parts = l2_view(stat, units)
            for t in range(-(-Nout // TN)):
                parts[l, t] = (inp["W"][l][:, t * TN:(t + 1) * TN] ** 2).sum(dtype=F32)
        if l == 0:
            for k in range(L):
                stat_view(stat, units, k)["bwd"][...] = 0
    # ---- backward
    for l in range(L, 0, -1):
        K, Nout = dims[l + 1], dims[l]  # dY[l-1] (n, Nout) = transform(A) (n, K) . W[l]^T
        sv_out = stat_view(stat, units, l - 1)
        dY, dP = nan(n, Nout), nan(n, K)
        if l < L:
            sv_in = stat_view(stat, units, l)
            sd, sx = (sv_in["bwd"][0] / FIX_GRAD).astype(F32), (sv_in["bwd"][1] / FIX_GRAD).astype(F32)
            out[f"ggamma{l}"], out[f"gbeta{l}"] = sx[0] + sx[1], sd[0] + sd[1]
        for s, r0, e in tiles():
            r1 = min(r0 + TM, e)
            if l == L:
                t = np.where(out["NE"][r0:r1] > 0, inp["dNE"][r0:r1], F32(0))
            else:
                ss = stat_site(s, r0)
                inv = F32(1.0 / ns[ss]) if ns[ss] > 0 else F32(0)
                is_, mn = sv_in["istd"][ss], sv_in["mean"][ss]
                k = inp["gamma"][l] * is_
                c1, c2 = k * (sx[ss] * inv) * is_, k * (sx[ss] * inv) * (mn * is_) - k * (sd[ss] * inv)
                c2t = np.broadcast_to(c2, (r1 - r0, K)).copy()
                if defect == "dbn_constant_by_buffer":
                    for kt in range(2, -(-K // TK)):
                        w = min(TK, K - kt * TK)
                        c2t[:, kt * TK:kt * TK + w] = c2[(kt & 1) * TK:(kt & 1) * TK + w]
                y = out[f"R{l}"][r0:r1]
                t = np.where(y > 0, out[f"dY{l}"][r0:r1] * k + (c2t - y * c1), F32(0)).astype(F32)
            write_aout(dP, t, r0, r1, Nout)
            c = (matmul(t, inp["W"][l].T.copy()) * mults[l - 1][r0:r1]).astype(F32)
            dY[r0:r1] = c
            ss = stat_site(s, r0)
            xh = out[f"R{l - 1}"][r0:r1] * sv_out["istd"][ss] - sv_out["mean"][ss] * sv_out["istd"][ss]
            sv_out["bwd"][0, s] += _fix(c.sum(0, dtype=F32), FIX_GRAD)
            sv_out["bwd"][1, s] += _fix((c * xh).sum(0, dtype=F32), FIX_GRAD)
        out[f"dY{l - 1}"], out[f"dP{l}"] = dY, dP
    sv = stat_view(stat, units, 0)
    sd, sx = (sv["bwd"][0] / FIX_GRAD).astype(F32), (sv["bwd"][1] / FIX_GRAD).astype(F32)
    out["ggamma0"], out["gbeta0"] = sx[0] + sx[1], sd[0] + sd[1]
    dP = nan(n, units[0])
    for s, r0, e in tiles():
        r1 = min(r0 + TM, e)
        ss = stat_site(s, r0)
        inv = F32(1.0 / ns[ss]) if ns[ss] > 0 else F32(0)
        is_, mn = sv["istd"][ss], sv["mean"][ss]
        k = inp["gamma"][0] * is_
        c1, c2 = k * (sx[ss] * inv) * is_, k * (sx[ss] * inv) * (mn * is_) - k * (sd[ss] * inv)
        y = out["R0"][r0:r1]
        dP[r0:r1] = np.where(y > 0, out["dY0"][r0:r1] * k + (c2 - y * c1), F32(0))
    out["dP0"] = dP
    if l2 > 0:
        out["loss"] = (out["loss"] + F32(l2) * l2_view(stat, units)[:L].sum(dtype=F32)).astype(F32)
    for k in range(L):
        stat_view(stat, units, k)["fwd"][...] = 0
    return out
