"""Float64 references of the kernels that close an NRMS training step (plain module: no fixtures, nothing collected): the fused user
head, the scorer and the three compiled losses, the Keras-form Adam step, the batch-norm pair, the bias + ReLU backward and the
fixed-point embedding-gradient scatter.

Written from the header comments of include/ebnerd_hip.h and the formulae of the reference model, not from the kernels.  The
conventions are those of tests/model_kernel_refs.py: every function returns a dict `name -> (value, magnitude)`, the magnitude being
the same expression with every term replaced by its absolute value, carried through nested expressions (first-order sensitivities
behind tanh / exp / log / a division), and the comparison is

    check_close:  |got - want| <= c * magnitude + TINY   element-wise, and a NaN or inf in `got` fails.

The label rows of every loss are arbitrary: one, two or no positives per row (`label_rows`), so that `sum(y)` is not 1.

The shape lists of tests/test_guarded_training_tail_gpu.py live here as well, so that tests/test_training_tail_refs_cpu.py can show
without a GPU which of them catch a planted defect that the shapes of tests/test_hip_kernels.py miss."""
import numpy as np

from oracle import nrms_numpy as on
from tests.model_kernel_refs import C_SUM, TINY, _softmax_like, _tanh, check_close, f64, ratio  # noqa: F401  (re-exported)

KERAS_EPS = 1e-7
EPS32 = float(np.float32(1e-7))                    # K.epsilon() as the float32 model holds it
HI32 = float(np.float32(1.0) - np.float32(1e-7))   # 1 - K.epsilon() formed in float32: 1 - 2^-23
LOSS_KINDS = {"cross_entropy_loss": 0, "log_loss": 1, "log_loss_probs": 2}  # the C ABI's loss_kind per oracle loss name
KIND_NAMES = {v: k for k, v in LOSS_KINDS.items()}
FIXED_SCALE = 2.0 ** 40


# ------------------------------------------------------------------------------------------------------------ inputs
def label_rows(B, C, first=0):
    """[B, C] float32 labels: row b has (b + first) % 3 -> one, two, no positives (at most C), at positions that move with b."""
    y = np.zeros((B, C), np.float32)
    for b in range(B):
        n_pos = min((1, 2, 0)[(b + first) % 3], C)
        for j in range(n_pos):
            y[b, (3 * b + 5 * j + 1) % C if C > 1 else 0] = 1
        if n_pos == 2 and y[b].sum() < 2:  # the two positions coincided (tiny C)
            y[b, (np.flatnonzero(y[b])[0] + 1) % C] = 1
    return y


def drop_mult32(seed, step, site, n, p, start=0):
    """The inverted-dropout multipliers of elements [start, start + n) as the KERNELS form them: float32 1 / (1 - p) or 0."""
    if p <= 0:
        return np.ones(n, np.float32)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return on.dropout_keep_mask(on.dropout_key(seed, step, site), n, p, start=start).astype(np.float32) * scale


# ------------------------------------------------------------------------------------------------------------ losses
def loss_ref(s, ms, y, kind, inv_batch):
    """The compiled loss on the logits s [B, C] (magnitude ms: the rounding s carries already; zeros when s is an input) with labels y.
    kind 0: categorical CE on the logits; 1: sigmoid CE on the logits, mean over (b, c); 2: binary CE on the softmax outputs clipped to
    [1e-7, 1 - 1e-7] with 1e-7 added inside the logs, no gradient where the clip is active.
    -> probs (softmax), loss_rows [B] (their sum is the batch loss), ds [B, C] = d(batch loss) / d(s)."""
    s, ms, y = f64(s), f64(ms), f64(y)
    B, C = s.shape
    invbc = inv_batch / C
    p, mp, _, _ = _softmax_like(s, ms, 1, shift=True)
    out = dict(probs=(p, mp))
    if kind == 0:
        mx = s.max(1, keepdims=True)
        se = np.exp(s - mx).sum(1, keepdims=True)
        lse = mx + np.log(se)
        mlse = np.abs(mx) + np.log(se) + 1.0 + ms.max(1, keepdims=True)
        logp, mlogp = s - lse, np.abs(s) + ms + mlse
        ysum = y.sum(1, keepdims=True)
        out["loss_rows"] = (-(y * logp).sum(1) * inv_batch, (np.abs(y) * mlogp).sum(1) * inv_batch)
        out["ds"] = ((p * ysum - y) * inv_batch, (mp * np.abs(ysum) + np.abs(y)) * inv_batch)
    elif kind == 1:
        sg = 1.0 / (1.0 + np.exp(-s))
        l = np.maximum(s, 0.0) - s * y + np.log1p(np.exp(-np.abs(s)))
        ml = np.maximum(s, 0.0) + np.abs(s * y) + np.log1p(np.exp(-np.abs(s))) + (1.0 + np.abs(y)) * ms
        out["loss_rows"] = (l.sum(1) * invbc, ml.sum(1) * invbc)
        out["ds"] = ((sg - y) * invbc, (sg * (1.0 + (1.0 - sg) * (1.0 + ms)) + np.abs(y)) * invbc)
    else:
        # K.epsilon() and the clip range are FLOAT32 numbers in the model (Keras computes this loss in float32): 1e-7 is 1.00000001e-7 and
        # 1 - 1e-7 is 0.99999988 = 1 - 2^-23.  Where the clip is active at the top (C = 1: p = 1) the term log(1 - p^ + eps) is
        # log(2.19e-7) with these, log(2e-7) with the double constants: 0.6 % apart, and the float32 model is the definition.
        lo, hi, eps = EPS32, HI32, EPS32
        in_range = (p >= lo) & (p <= hi)
        pc = np.clip(p, lo, hi)
        a, b = pc + eps, 1.0 - pc + eps
        mpc = np.maximum(mp, pc)
        ma, mb = mpc + eps, 1.0 + mpc + eps  # forming a and b rounds too: 1 - p^ is a difference of numbers of magnitude 1
        ay, a1y = np.abs(y), np.abs(1.0 - y)
        l = -(y * np.log(a) + (1.0 - y) * np.log(b))
        ml = ay * (np.abs(np.log(a)) + ma / a) + a1y * (np.abs(np.log(b)) + mb / b)
        dldp = np.where(in_range, -(y / a) + (1.0 - y) / b, 0.0)
        mdldp = np.where(in_range, ay / a * (ma / a) + a1y / b * (mb / b), 0.0)
        dot = (p * dldp).sum(1, keepdims=True)
        mdot = (mp * np.abs(dldp) + p * mdldp).sum(1, keepdims=True)
        out["loss_rows"] = (l.sum(1) * invbc, ml.sum(1) * invbc)
        out["ds"] = (p * (dldp - dot) * invbc, (p * (mdldp + mdot) + mp * (np.abs(dldp) + np.abs(dot))) * invbc)
        # the case is well posed only while no probability sits at a clip threshold (the gate is a step function)
        out["clip_margin"] = float(np.min(np.where(p < 0.5, np.abs(p - lo) / lo, np.where(p == 1.0, 1.0, np.abs(hi - p) / lo))))
    return out


def score_ref(cand, user, scores=None):
    """scores[b, c] = cand[b, c, :] . user[b, :]; probs: softmax over c (mode 0) and sigmoid (mode 1).  `scores` given (the kernel's
    own logits): the activations are judged from them, as exact inputs."""
    cand, user = f64(cand), f64(user)
    s, ms = np.einsum("bce,be->bc", cand, user), np.einsum("bce,be->bc", np.abs(cand), np.abs(user))
    sa, msa = (s, ms) if scores is None else (f64(scores).reshape(s.shape), np.zeros_like(s))
    p, mp, _, _ = _softmax_like(sa, msa, 1, shift=True)
    sg = 1.0 / (1.0 + np.exp(-sa))
    return dict(scores=(s, ms), probs=(p, mp), sigmoid=(sg, sg * (1.0 + (1.0 - sg) * (1.0 + msa))))


def score_loss_ref(cand, user, y, kind, inv_batch, scores=None):
    """scorer (softmax mode) + loss + backward into the representations.  `scores` given: the backward kernel's view -- the logits are
    an input (no rounding of their own) and cand / user only carry the gradients."""
    cand, user = f64(cand), f64(user)
    fwd = score_ref(cand, user)
    s, ms = fwd["scores"] if scores is None else (f64(scores), np.zeros(np.shape(scores)))
    out = loss_ref(s, ms, y, kind, inv_batch)
    ds, mds = out["ds"]
    out["scores"] = (s, ms)
    out["dcand"] = (ds[:, :, None] * user[:, None, :], mds[:, :, None] * np.abs(user)[:, None, :])
    out["duser"] = (np.einsum("bc,bce->be", ds, cand), np.einsum("bc,bce->be", mds, np.abs(cand)))
    out["loss"] = (np.array([out["loss_rows"][0].sum()]), np.array([out["loss_rows"][1].sum()]))
    return out


def pair_score_ref(user, news, u_idx, n_idx):
    u, x = f64(user)[np.asarray(u_idx)], f64(news)[np.asarray(n_idx)]
    s, ms = (u * x).sum(1), np.abs(u * x).sum(1)
    sg = 1.0 / (1.0 + np.exp(-s))
    return dict(dot=(s, ms), sigmoid=(sg, sg * (1.0 + (1.0 - sg) * (1.0 + ms))))


# ------------------------------------------------------------------------------------------------------------ fused user head
def _pm(x, mx, y, my):
    """magnitude of x * y to first order; mx, my include |x|, |y| (an exact input has mx = |x|)"""
    return mx * np.abs(y) + np.abs(x) * my - np.abs(x) * np.abs(y)


HEAD_LINKS = ("w", "user", "scores", "duser", "de")  # the outputs of the head that a later stage of the same launch consumes


def head_ref(Upre, b, q, X, cand, y, kind, inv_batch, given=None):
    """AttLayer2 after its x.W matmul (un-stabilised exp, +1e-7 in the denominator) -> scorer -> loss -> their backward up to
    d(pre-tanh), d(q), d(b).  Upre [B, L, A], X [B, L, E], cand [B, C, E], y [B, C].

    given = None: the whole chain from the inputs; every magnitude carries what the stages before it contribute, so it grows along
    the chain (three nested dot products of random signs: the bound is thousands of times the value at the end).
    given = {w, user, scores, duser, de} (HEAD_LINKS, the KERNEL's own outputs): every stage is computed from the kernel's outputs of
    the stage before, taken as exact inputs -- each link of the fused launch is judged on its own step, as a separate kernel would be,
    with a magnitude of one step.  A link that consumed anything but what the launch wrote fails its stage."""
    Upre, b, q, X, cand = f64(Upre), f64(b), f64(q).reshape(-1), f64(X), f64(cand)
    aq, aX, ac = np.abs(q), np.abs(X), np.abs(cand)

    def link(name, val, mag, exact_mag=None):
        if given is None:
            return val, mag
        g = f64(given[name]).reshape(val.shape)
        return g, (np.abs(g) if exact_mag is None else exact_mag)

    T, mT = _tanh(Upre + b, np.abs(Upre) + np.abs(b))
    e, me = T @ q, mT @ aq
    w, mw, _, _ = _softmax_like(e, me, 1, eps=KERAS_EPS)
    wu, mwu = link("w", w, mw)
    user, muser = np.einsum("bl,ble->be", wu, X), np.einsum("bl,ble->be", mwu, aX)
    uu, muu = link("user", user, muser)
    s, ms = np.einsum("bce,be->bc", cand, uu), np.einsum("bce,be->bc", ac, muu)
    su, msu = link("scores", s, ms, exact_mag=np.zeros_like(s))  # loss_ref's ms: the rounding the logits carry, none for an input
    out = loss_ref(su, msu, y, kind, inv_batch)
    ds, mds = out["ds"]
    dcand, mdcand = ds[:, :, None] * uu[:, None, :], _pm(ds[:, :, None], mds[:, :, None], uu[:, None, :], muu[:, None, :])
    duser, mduser = np.einsum("bc,bce->be", ds, cand), np.einsum("bc,bce->be", mds, ac)
    du, mdu = link("duser", duser, mduser)
    dw, mdw = np.einsum("ble,be->bl", X, du), np.einsum("ble,be->bl", aX, mdu)
    sw, msw = (wu * dw).sum(1, keepdims=True), _pm(wu, mwu, dw, mdw).sum(1, keepdims=True)
    de, mde = wu * (dw - sw), _pm(wu, mwu, dw - sw, mdw + msw)
    deu, mdeu = link("de", de, mde)
    one_t2, m_one_t2 = 1.0 - T * T, 1.0 + T * T + 2.0 * np.abs(T) * (mT - np.abs(T))
    dpre, mdpre = deu[:, :, None] * q * one_t2, _pm(deu[:, :, None], mdeu[:, :, None], q * one_t2, aq * m_one_t2)
    out.update(T=(T, mT), w=(w, mw), user=(user, muser), scores=(s, ms), dcand=(dcand, mdcand), duser=(duser, mduser), de=(de, mde),
               dpre=(dpre, mdpre), dq=((deu[:, :, None] * T).sum((0, 1)), _pm(deu[:, :, None], mdeu[:, :, None], T, mT).sum((0, 1))),
               db=(dpre.sum((0, 1)), mdpre.sum((0, 1))),
               loss=(np.array([out["loss_rows"][0].sum()]), np.array([out["loss_rows"][1].sum()])))
    return out


def head_inputs(B, L, C, E, A, seed=0):
    """float32 inputs of a head case, scaled so that the attention logits and the scores stay O(1) at every shape (E up to 4100): the
    softmax outputs keep clear of the clip thresholds of loss kind 2."""
    rng = np.random.default_rng(1000 * L + 10 * C + E + A + seed)
    Upre = (rng.standard_normal((B, L, A)) * 0.7).astype(np.float32)
    b = (rng.standard_normal(A) * 0.2).astype(np.float32)
    q = (rng.standard_normal(A) * (2.0 / np.sqrt(A))).astype(np.float32)
    X = rng.standard_normal((B, L, E)).astype(np.float32)
    cand = (rng.standard_normal((B, C, E)) * (1.5 / np.sqrt(E))).astype(np.float32)
    return Upre, b, q, X, cand, label_rows(B, C)


# ------------------------------------------------------------------------------------------------------------ Adam (Keras form)
def adam_ref(theta, g, m, v, alpha, beta1=0.9, beta2=0.999, eps=1e-7, gscale=1.0):
    """g' = g gscale; m += (g' - m)(1 - b1); v += (g'^2 - v)(1 - b2); theta -= alpha m / (sqrt(v) + eps), with the NEW m and v.
    `alpha` is the step state's adam_alpha (lr sqrt(1 - b2^t) / (1 - b1^t), a float32 the kernel reads)."""
    theta, g, m, v = f64(theta), f64(g) * gscale, f64(m), f64(v)
    o1, o2 = 1.0 - beta1, 1.0 - beta2
    m1, mm1 = m + (g - m) * o1, np.abs(m) + (np.abs(g) + np.abs(m)) * o1
    v1, mv1 = v + (g * g - v) * o2, np.abs(v) + (g * g + np.abs(v)) * o2
    rt = np.sqrt(v1)
    den = rt + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        mrt = np.where(v1 > 0, mv1 / (2.0 * rt), 0.0)  # an exact zero stays exact
    step = alpha * m1 / den
    mstep = alpha * (mm1 / den + np.abs(m1) / den ** 2 * (mrt + rt + eps))
    return dict(theta=(theta - step, np.abs(theta) + mstep), m=(m1, mm1), v=(v1, mv1))


# ------------------------------------------------------------------------------------------------------------ column reductions
BN_EPS, BN_MOM = 1e-3, 0.99


def relu_bwd_ref(Y, dY):
    Y, dY = f64(Y), f64(dY)
    dX = np.where(Y > 0, dY, 0.0)
    return dict(dX=(dX, np.abs(dX)), dbias=(dX.sum(0), np.abs(dX).sum(0)))


def bn_fwd_ref(X, gamma, beta, mmean, mvar, mult=1.0):
    """training-mode BatchNormalization(momentum .99, eps 1e-3) over the rows, then the dropout multipliers."""
    X, gamma, beta, mmean, mvar = f64(X), f64(gamma), f64(beta), f64(mmean), f64(mvar)
    R = X.shape[0]
    mean, mmu = X.mean(0), np.abs(X).mean(0)
    d, md = X - mean, np.abs(X) + mmu
    var, mv = (d * d).mean(0), (d * d + 2.0 * np.abs(d) * md).mean(0)
    istd = 1.0 / np.sqrt(var + BN_EPS)
    mistd = istd * (1.0 + 0.5 * mv / (var + BN_EPS))
    xhat, mxh = d * istd, md * istd + np.abs(d) * mistd
    return dict(mean=(mean, mmu), istd=(istd, mistd), xhat=(xhat, mxh),
                Y=((xhat * gamma + beta) * mult, (mxh * np.abs(gamma) + np.abs(beta)) * mult),
                moving_mean=(mmean * BN_MOM + mean * (1.0 - BN_MOM), np.abs(mmean) * BN_MOM + mmu * (1.0 - BN_MOM)),
                moving_var=(mvar * BN_MOM + var * (1.0 - BN_MOM), np.abs(mvar) * BN_MOM + (var + mv) * (1.0 - BN_MOM)))


def bn_bwd_ref(dY, xhat, gamma, istd, mult=1.0, dgamma0=None, dbeta0=None):
    """From the forward's saved xhat and istd (inputs of the backward kernel).  dgamma0 / dbeta0: accumulate onto these."""
    dY, xhat, gamma, istd = f64(dY), f64(xhat), f64(gamma), f64(istd)
    R = dY.shape[0]
    g = dY * mult
    dg, mdg = (g * xhat).sum(0), np.abs(g * xhat).sum(0)
    db, mdb = g.sum(0), np.abs(g).sum(0)
    k = gamma * istd
    dX, mdX = (g - db / R - xhat * dg / R) * k, (np.abs(g) + mdb / R + np.abs(xhat) * mdg / R) * np.abs(k)
    if dgamma0 is not None:
        dg, mdg, db, mdb = dg + f64(dgamma0), mdg + np.abs(f64(dgamma0)), db + f64(dbeta0), mdb + np.abs(f64(dbeta0))
    return dict(dgamma=(dg, mdg), dbeta=(db, mdb), dX=(dX, mdX))


# ------------------------------------------------------------------------------------------------------------ embedding
def gather_ref(ids, table, mult=None):
    """out[r] = table[ids[r]] (a zero row for an id outside the table) * the float32 multipliers: float32, to be matched exactly (as
    VALUES: a dropped negative element is +0 on the select path and -0 on the multiply path of the kernel; a NaN never matches)."""
    ids, table = np.asarray(ids).astype(np.int64), np.asarray(table, np.float32)
    ok = (ids >= 0) & (ids < table.shape[0])
    out = np.where(ok[:, None], table[np.clip(ids, 0, table.shape[0] - 1)], np.float32(0))
    if mult is not None:
        m = np.asarray(mult, np.float32).reshape(out.shape)
        out = np.where(m != 0, out * m, np.float32(0))
    return out.astype(np.float32), bool((~ok).any())


def scatter_ref(ids, dX, V, mult=None):
    """dTable[ids[r]] += dX[r] * mult[r] over the ids inside [0, V).  -> the float64 dense gradient with its magnitude, and `fixed`:
    the 2^40-scaled int64 accumulator -- every term is the float32 product dX * mult, scaled exactly and rounded to nearest-even, the
    sums exact integers."""
    ids = np.asarray(ids).astype(np.int64)
    x = np.asarray(dX, np.float32)
    if mult is not None:
        x = x * np.asarray(mult, np.float32).reshape(x.shape)  # one float32 rounding, as in the kernels
    ok = (ids >= 0) & (ids < V)
    D = x.shape[1]
    dense, mag, fixed = np.zeros((V, D)), np.zeros((V, D)), np.zeros((V, D), np.int64)
    np.add.at(dense, ids[ok], x[ok].astype(np.float64))
    np.add.at(mag, ids[ok], np.abs(x[ok]).astype(np.float64))
    np.add.at(fixed, ids[ok], np.rint(x[ok].astype(np.float64) * FIXED_SCALE).astype(np.int64))
    return dict(dense=(dense, mag), fixed=fixed)


def fixed_to_f32_ref(acc):
    return (np.asarray(acc, np.int64).astype(np.float64) / FIXED_SCALE).astype(np.float32)


RUN_CHUNK = 64  # tokens per workgroup of the duplicate-combining scatter; it walks them in id order in groups of 8
ID_PATTERNS = ("same", "cross8", "valid8", "valid9", "all_oob", "oob_between")


def scatter_ids(n_tok, V, kind):
    """Hand-built id patterns for the duplicate-combining scatter, chunk by chunk of 64 tokens (ids outside [0, V) are skipped and
    sort behind the valid ones):
      same         every token the same id
      cross8       5 x id 0 then runs of 6 equal ids: in id order every run crosses a boundary of the 8-token load groups
      valid8/9     exactly 8 / 9 valid tokens in every chunk, the rest outside the table
      all_oob      the first chunk holds no valid id at all (a later chunk does)
      oob_between  ids outside the table at every third position, between valid ones"""
    assert V >= 3
    t = np.arange(n_tok)
    j = t % RUN_CHUNK
    oob = np.where(t % 2 == 0, V, -1)
    if kind == "same":
        ids = np.full(n_tok, V - 1)
    elif kind == "cross8":
        ids = np.where(j < 5, 0, 1 + ((j - 5) // 6) % (V - 1))
    elif kind in ("valid8", "valid9"):
        n_valid = 8 if kind == "valid8" else 9
        ids = np.where((j % 7 == 0) & (j // 7 < n_valid), (j // 7) % 2 + 1, oob)  # scattered positions, two ids: runs of 4 and 4 / 5
    elif kind == "all_oob":
        ids = np.where(t < RUN_CHUNK, oob, t % V)
    elif kind == "oob_between":
        ids = np.where(t % 3 == 1, oob, (t // 3) % V)
    else:
        raise ValueError(kind)
    return ids.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ the shapes of the GPU tests
# What test_hip_kernels.py ran the head at, and the shapes that take every loop of ebn_user_head_train_f32 into a second trip.
HEAD_OLD = [(20, 5, 400, 200), (50, 5, 400, 200), (7, 9, 20, 12), (1, 1, 8, 4), (20, 5, 256, 200)]  # (L, C, E, A)
HEAD_CASES = [
    (64, 64, 8, 8),      # L and C exactly at 64
    (65, 3, 8, 12),      # second trip of the lane loops over L
    (3, 65, 8, 12),      # ... over C
    (17, 2, 8, 8),       # second trip of the wave loops (16 waves)
    (5, 2, 8, 260),      # A4 = 65
    (3, 2, 8, 1028),     # second trip of the k loop (1024 threads)
    (2, 2, 4100, 4),     # E4 = 1025
    (9, 9, 1000, 8),     # second trip of the X and the candidate staging loops (2048 float4 per trip)
    (17, 1, 4, 484),     # second trip of the U staging loop
    (5, 5, 1028, 8),     # first staging batch full, second partial
    (59, 5, 400, 200)]   # the longest history ebn_user_head_supported admits at the reference sizes (LDS 153 312 of 153 600 bytes)
HEAD_REFUSED = (60, 5, 400, 200)
HEAD_B = 3
HEAD_LONG_BATCH = (257, 2, 2, 4, 4)  # (B, L, C, E, A): the loss-row sum of the finishing block takes a second trip

SCORE_OLD_BWD = [(5, 400), (9, 20)]                                        # (C, E) at which the gradients met the oracle
SCORE_OLD_TRAIN = [(5, 400), (5, 256), (64, 20), (1, 8), (70, 16)]         # ... and the fused kernel its parts (labels one-hot)
SCORE_CASES = [(C, E) for C in (1, 63, 64, 65, 129) for E in (1, 63, 65, 257)]
SCORE_LIMIT = (1, 8192, 4)  # (B, C, E): 64 KB of dynamic LDS in the train kernel; C = 8193 is refused

GATHER_CASES = [  # (D, n_tok): item counts on both sides of one block's share (512 16-byte vectors; 256 floats on the scalar path)
    (4, 511), (4, 512), (4, 513), (256, 7), (256, 8), (256, 9), (1024, 1), (1024, 2), (1024, 3), (300, 6), (300, 7), (7, 36), (7, 37)]
SCATTER_NTOK = (1, 63, 64, 65, 129)
SCATTER_D = (1, 33, 1024, 1025, 2052)
COLRED_OLD_R = [160, 1025, 3, 640, 37, 1024, 1500]   # the row counts of the kernel-level tests: at most 47 row blocks
COLRED_CASES = [(R, C) for R in (8193, 8224, 32801) for C in (1, 65)]
FINISH_REST = (1, 4095, 0, 4097)
