"""The float64 references of tests/training_tail_refs.py, checked without a GPU: every backward against torch.autograd in float64 at
the new shapes (1e-10 relative), the Adam step against the oracle's, the fixed-point scatter against the dense gradient, and four
planted defects in numpy stand-ins run through the comparator of the GPU tests -- each is caught at a shape
tests/test_guarded_training_tail_gpu.py lists and missed at every shape (and label / id pattern) tests/test_hip_kernels.py has, which
is the evidence that the listed shapes are the ones that matter."""
import numpy as np
import pytest
import torch

from oracle import nrms_numpy as on
from tests import training_tail_refs as tr
from tests.guarded import guard_out

REL = 1e-10


def t64(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def same(got, want, what, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want.detach().numpy() if torch.is_tensor(want) else want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-300) if scale is None else scale
    err = float(np.abs(got - want).max())
    assert err <= REL * scale, (what, err, scale)


def mags_dominate(ref):
    for k, v in ref.items():
        if isinstance(v, tuple):
            assert v[0].shape == v[1].shape and (v[1] >= np.abs(v[0]) * (1 - 1e-12)).all(), k


def torch_loss(s, y, kind, inv_batch):
    """the three compiled losses in torch, from the formulae of nrms.py:56-67 / Keras' backend"""
    C = s.shape[1]
    if kind == 0:
        return -(y * torch.log_softmax(s, 1)).sum() * inv_batch
    if kind == 1:
        return (torch.clamp(s, min=0) - s * y + torch.log1p(torch.exp(-s.abs()))).sum() * inv_batch / C
    pc = torch.clamp(torch.softmax(s, 1), tr.EPS32, tr.HI32)  # K.epsilon() and 1 - K.epsilon() as float32 holds them
    return -(y * torch.log(pc + tr.EPS32) + (1 - y) * torch.log(1 - pc + tr.EPS32)).sum() * inv_batch / C


# ------------------------------------------------------------------------------------------------------------ label rows, id patterns
def test_label_rows_have_one_two_and_no_positives():
    for C in (1, 2, 3, 5, 64, 65, 129, 8192):
        y = tr.label_rows(3, C)
        assert y.sum(1).tolist() == [1, min(2, C), 0], C
    assert sorted(tr.label_rows(1, 9, first=f).sum() for f in range(3)) == [0, 1, 2]


def test_id_patterns_are_what_they_say():
    V = 7
    ok = lambda ids: (ids >= 0) & (ids < V)
    for n_tok in tr.SCATTER_NTOK:
        for kind in tr.ID_PATTERNS:
            assert tr.scatter_ids(n_tok, V, kind).shape == (n_tok,)
    assert len(set(tr.scatter_ids(129, V, "same").tolist())) == 1
    c8 = tr.scatter_ids(64, V, "cross8")
    order = np.sort(c8[ok(c8)], kind="stable")
    assert ok(c8).all() and order[7] == order[8] and order[15] == order[16]  # runs cross the boundaries of the 8-token groups
    for kind, n in (("valid8", 8), ("valid9", 9)):
        ids = tr.scatter_ids(129, V, kind)
        assert ok(ids[:64]).sum() == n and ok(ids[64:128]).sum() == n and ok(ids[128:]).sum() == 1
    ao = tr.scatter_ids(129, V, "all_oob")
    assert not ok(ao[:64]).any() and ok(ao[64:]).all() and not ok(tr.scatter_ids(63, V, "all_oob")).any()
    ob = tr.scatter_ids(65, V, "oob_between")
    assert not ok(ob[1::3]).any() and ok(ob[0::3]).all() and ok(ob[2::3]).all() and (ob > V - 1).any() and (ob < 0).any()


# ------------------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("L,C,E,A", [(65, 3, 8, 12), (3, 65, 8, 12), (17, 2, 8, 8), (5, 2, 8, 260)])
def test_head_reference_vs_autograd(kind, L, C, E, A):
    B = tr.HEAD_B
    Upre, b, q, X, cand, y = tr.head_inputs(B, L, C, E, A)
    ref = tr.head_ref(Upre, b, q, X, cand, y, kind, 1.0 / B)
    mags_dominate(ref)
    assert kind != 2 or ref["clip_margin"] > 0.5
    u, bt, qt, x, ct = t64(Upre), t64(b), t64(q), t64(X), t64(cand)
    T = torch.tanh(u + bt)
    e = T @ qt
    e.retain_grad()
    a = torch.exp(e)
    w = a / (a.sum(1, keepdim=True) + 1e-7)
    user = (w.unsqueeze(2) * x).sum(1)
    user.retain_grad()
    s = torch.einsum("bce,be->bc", ct, user)
    s.retain_grad()
    loss = torch_loss(s, t64(y, False), kind, 1.0 / B)
    loss.backward()
    for name, want in (("w", w), ("user", user), ("scores", s), ("probs", torch.softmax(s, 1)), ("ds", s.grad), ("dcand", ct.grad), ("duser", user.grad),
                       ("de", e.grad), ("dpre", u.grad), ("dq", qt.grad), ("db", bt.grad)):
        same(ref[name][0], want, name)
    same(ref["loss"][0], loss.reshape(1), "loss")
    same(np.array([ref["loss_rows"][0].sum()]), loss.reshape(1), "loss rows")
    # link by link from exact upstream values: the same numbers, magnitudes of one step (never above the chain's, far below at its end)
    links = tr.head_ref(Upre, b, q, X, cand, y, kind, 1.0 / B, given={k: ref[k][0] for k in tr.HEAD_LINKS})
    mags_dominate(links)
    for name in ("w", "user", "scores", "probs", "loss_rows", "dcand", "duser", "de", "dpre", "dq", "db"):
        same(links[name][0], ref[name][0], f"links {name}", scale=max(float(np.abs(ref[name][0]).max()), 1e-300))
        assert (links[name][1] <= ref[name][1] * (1 + 1e-9) + 1e-300).all(), name
    if ref["dpre"][1].max() > 0:  # (C = 1 with a positive label: the gradient is an exact zero)
        assert np.median(links["dpre"][1] / (ref["dpre"][1] + 1e-300)) < 0.2


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("C,E", [(1, 1), (65, 63), (129, 257), (8192, 4)])
def test_scorer_reference_vs_autograd_and_the_oracle(kind, C, E):
    B = 3 if C < 8192 else 1
    rng = np.random.default_rng(C + E)
    cand, user = rng.standard_normal((B, C, E)) * 0.4, rng.standard_normal((B, E)) * 0.4
    y = tr.label_rows(B, C, first=1)
    ref = tr.score_loss_ref(cand, user, y, kind, 1.0 / B)
    mags_dominate(ref)
    ct, ut = t64(cand), t64(user)
    s = torch.einsum("bce,be->bc", ct, ut)
    s.retain_grad()
    loss = torch_loss(s, t64(y, False), kind, 1.0 / B)
    loss.backward()
    for name, want in (("scores", s), ("ds", s.grad), ("dcand", ct.grad), ("duser", ut.grad)):
        same(ref[name][0], want, name)
    same(ref["loss"][0], loss.reshape(1), "loss")
    L, ds = on.loss_fwd_bwd(ref["scores"][0], y.astype(np.float64), tr.KIND_NAMES[kind])  # the oracle's formulae hold for multi-hot rows too
    if kind != 2:
        same(ref["loss"][0], np.array([L]), "loss vs oracle")
        same(ref["ds"][0], ds, "ds vs oracle")
    elif C > 1:  # the oracle's float64 pass holds the DOUBLE 1e-7: 1e-8 of eps apart while no clip is active, 0.6 % apart at p = 1 (C = 1)
        same(ref["loss"][0], np.array([L]), "loss vs oracle", scale=1e4 * abs(L))
        same(ref["ds"][0], ds, "ds vs oracle", scale=1e4 * float(np.abs(ds).max()))
    else:
        assert abs(ref["loss"][0][0] / L - 1) < 0.01
    fwd = tr.score_ref(cand, user)
    same(fwd["probs"][0], torch.softmax(s, 1), "softmax")
    same(fwd["sigmoid"][0], torch.sigmoid(s), "sigmoid")
    # the backward kernel's view: the logits given
    given = tr.score_loss_ref(cand, user, y, kind, 1.0 / B, scores=ref["scores"][0])
    same(given["dcand"][0], ct.grad, "dcand from given scores")
    pr = tr.pair_score_ref(user, cand[0], [0, B - 1], [C - 1, 0])
    same(pr["dot"][0], np.array([user[0] @ cand[0, C - 1], user[B - 1] @ cand[0, 0]]), "pair score")


def test_adam_reference_is_the_oracles_keras_step():
    rng = np.random.default_rng(3)
    n, t, lr = 1000, 3, 1e-3
    th, g, m, v = rng.standard_normal(n), rng.standard_normal(n) * 2, rng.standard_normal(n) * 0.1, rng.random(n) * 0.01
    g[:100], v[:50], m[:50] = 0.0, 0.0, 0.0  # untouched rows: an exact zero stays exact
    alpha = lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
    ref = tr.adam_ref(th, g * 2, m, v, alpha, gscale=0.5)
    mags_dominate(ref)
    th2, m2, v2 = th.copy(), m.copy(), v.copy()
    on.adam_keras_step(th2, g, m2, v2, t, lr=lr)
    same(ref["theta"][0], th2, "theta")
    same(ref["m"][0], m2, "m")
    same(ref["v"][0], v2, "v")
    assert (ref["theta"][0][:50] == th[:50]).all() and np.isfinite(ref["theta"][1]).all()


@pytest.mark.parametrize("R,C,p", [(37, 5, 0.0), (130, 65, 0.2)])
def test_batchnorm_pair_and_relu_backward_references_vs_autograd(R, C, p):
    rng = np.random.default_rng(R)
    X, dY = np.maximum(rng.standard_normal((R, C)) + 0.3, 0), rng.standard_normal((R, C))
    gamma, beta = 1 + 0.1 * rng.standard_normal(C), 0.1 * rng.standard_normal(C)
    mm0, mv0 = 0.05 * rng.standard_normal(C), 1 + 0.1 * rng.random(C)
    mult = tr.drop_mult32(3, 4, 9, R * C, p, start=1000).reshape(R, C).astype(np.float64)
    fwd = tr.bn_fwd_ref(X, gamma, beta, mm0, mv0, mult)
    mags_dominate(fwd)
    x, gt, bt = t64(X), t64(gamma), t64(beta)
    mu, var = x.mean(0), x.var(0, unbiased=False)
    xh = (x - mu) / torch.sqrt(var + 1e-3)
    y = (xh * gt + bt) * t64(mult, False)
    same(fwd["Y"][0], y, "Y")
    same(fwd["xhat"][0], xh, "xhat")
    same(fwd["moving_mean"][0], mm0 * 0.99 + mu.detach().numpy() * 0.01, "moving mean")
    same(fwd["moving_var"][0], mv0 * 0.99 + var.detach().numpy() * 0.01, "moving var")
    (y * t64(dY, False)).sum().backward()
    g0, b0 = rng.standard_normal(C), rng.standard_normal(C)
    bwd = tr.bn_bwd_ref(dY, fwd["xhat"][0], gamma, fwd["istd"][0], mult, g0, b0)
    mags_dominate(bwd)
    same(bwd["dX"][0], x.grad, "dX")
    same(bwd["dgamma"][0] - g0, gt.grad, "dgamma")
    same(bwd["dbeta"][0] - b0, bt.grad, "dbeta")
    pre = t64(rng.standard_normal((R, C)))
    (torch.relu(pre) * t64(dY, False)).sum().backward()
    rb = tr.relu_bwd_ref(np.maximum(pre.detach().numpy(), 0), dY)
    same(rb["dX"][0], pre.grad, "relu dX")
    same(rb["dbias"][0], pre.grad.sum(0), "dbias")


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("kind", tr.ID_PATTERNS)
def test_scatter_reference_vs_the_oracle_and_its_own_fixed_point(kind, p):
    V, D, n_tok = 7, 33, 129
    rng = np.random.default_rng(5)
    ids = tr.scatter_ids(n_tok, V, kind)
    dX = (rng.standard_normal((n_tok, D)) * 10 ** rng.uniform(-6, 0, (n_tok, 1))).astype(np.float32)
    mult = tr.drop_mult32(4, 3, 0, n_tok * D, p).reshape(n_tok, D)
    ref = tr.scatter_ref(ids, dX, V, mult if p > 0 else None)
    ok = (ids >= 0) & (ids < V)
    same(ref["dense"][0], on.embedding_bwd(ids[ok], (dX * mult)[ok].astype(np.float64), V), "dense gradient", scale=1.0)
    # each term is off by at most half a unit of 2^-40
    assert np.abs(ref["fixed"] / tr.FIXED_SCALE - ref["dense"][0]).max() <= 0.5 * n_tok / tr.FIXED_SCALE
    exact = tr.scatter_ref(ids, np.round(dX * 1024) / 1024, V)  # multiples of 2^-10: the fixed-point sums are exact
    assert np.array_equal(exact["fixed"], np.rint(exact["dense"][0] * tr.FIXED_SCALE).astype(np.int64))
    out, flag = tr.gather_ref(ids, dX[:V], mult[:n_tok * 0 + n_tok, :] if p > 0 else None)
    assert flag == bool((~ok).any()) and (out[~ok] == 0).all() and out.dtype == np.float32


# ------------------------------------------------------------------------------------------------------------ planted defects
CAP_W = 2e-5  # the bound of tests/test_hip_kernels.py on the head's attention weights: the ceiling of the GPU test's constant


def standin_head_weights(e, defect):
    """Stand-in of the head's softmax over the history (wave 0: 64 lanes, l += 64): w = exp(e) / (sum exp(e) + 1e-7) of one impression.
    Defect: the lane loop of the SUM makes one trip only (l < 64)."""
    L = e.shape[0]
    ex = np.exp(e.astype(np.float32))
    part = np.zeros(64, np.float32)
    for lane in range(64):
        for l in range(lane, min(L, 64) if defect else L, 64):
            part[lane] += ex[l]
    return ex / (part.sum(dtype=np.float32) + np.float32(1e-7))


def _head_weights_case(L, C, E, A, defect):
    Upre, b, q, X, cand, y = tr.head_inputs(2, L, C, E, A)
    ref = tr.head_ref(Upre, b, q, X, cand, y, 0, 0.5)
    e = np.tanh(Upre.astype(np.float64) + b) @ q.astype(np.float64)
    got = np.stack([standin_head_weights(e[i], defect) for i in range(2)])
    tr.check_close(got, ref["w"], CAP_W, "w")


def test_defect_history_loop_stops_after_64_rows():
    for shape in tr.HEAD_OLD + tr.HEAD_CASES:
        _head_weights_case(*shape, False)
    for shape in tr.HEAD_OLD:  # L <= 50: one trip is all there is
        _head_weights_case(*shape, True)
    caught = []
    for shape in tr.HEAD_CASES:
        try:
            _head_weights_case(*shape, True)
        except AssertionError:
            caught.append(shape)
    assert caught == [(65, 3, 8, 12)], caught  # L = 64 still passes: the limit is touched from both sides


def standin_ce_dscores(s, y, inv_batch, defect):
    """Stand-in of the categorical gradient ds = (softmax(s) * sum(y) - y) / B in float32.  Defect: sum(y) taken as 1."""
    s, y = s.astype(np.float32), y.astype(np.float32)
    ex = np.exp(s - s.max(1, keepdims=True))
    p = ex / ex.sum(1, keepdims=True)
    ysum = np.float32(1) if defect else y.sum(1, keepdims=True)
    return (p * ysum - y) * np.float32(inv_batch)


def _ce_case(C, E, y_of, defect):
    rng = np.random.default_rng(C * 1000 + E)
    B = 3
    cand, user = (rng.standard_normal((B, C, E)) * 0.4).astype(np.float32), (rng.standard_normal((B, E)) * 0.4).astype(np.float32)
    y = y_of(B, C, rng)
    s = np.einsum("bce,be->bc", cand.astype(np.float64), user.astype(np.float64)).astype(np.float32)
    ref = tr.loss_ref(s, np.zeros_like(s), y, 0, 1.0 / B)
    tr.check_close(standin_ce_dscores(s, y, 1.0 / B, defect), ref["ds"], 3e-5, "ds")  # 3e-5: the gradient bound of test_hip_kernels.py


def _one_hot(B, C, rng):
    y = np.zeros((B, C), np.float32)
    y[np.arange(B), rng.integers(0, C, B)] = 1
    return y


def test_defect_label_sum_taken_as_one():
    multi = lambda B, C, rng: tr.label_rows(B, C)
    for C, E in tr.SCORE_OLD_BWD + tr.SCORE_OLD_TRAIN:
        _ce_case(C, E, _one_hot, False)
        _ce_case(C, E, _one_hot, True)  # missed: the labels of test_hip_kernels.py are one-hot, sum(y) IS 1
    for C, E in tr.SCORE_CASES:
        _ce_case(C, E, multi, False)
        with pytest.raises(AssertionError):
            _ce_case(C, E, multi, True)  # the rows with two and with no positives


def standin_scatter_runs(ids, dX, acc_raw, V, defect):
    """Stand-in of the duplicate-combining scatter over the accumulator as C sees it (flat int64 storage, offset): per chunk of 64
    tokens the valid (id, position) pairs in id order, walked in groups of 8; a run of equal ids is summed and flushed when the id
    changes, and once more behind the walk.  Defect: the early exit at a group that starts with a skipped token leaves the column
    without that last flush -- the pending run is lost whenever a chunk holds 8, 16, ... 56 valid tokens."""
    acc, a0 = acc_raw
    n_tok, D = dX.shape
    q = np.rint(dX.astype(np.float64) * tr.FIXED_SCALE).astype(np.int64)
    for t0 in range(0, n_tok, tr.RUN_CHUNK):
        chunk = ids[t0:t0 + tr.RUN_CHUNK].astype(np.int64)
        pairs = sorted((int(i), j) for j, i in enumerate(chunk) if 0 <= i < V)
        s_id = [i for i, _ in pairs] + [-1] * (tr.RUN_CHUNK + 1 - len(pairs))
        s_pos = [j for _, j in pairs] + [0] * (tr.RUN_CHUNK - len(pairs))
        for c in range(D):
            run, prev, lost, done = 0, -1, False, False
            for j0 in range(0, tr.RUN_CHUNK, 8):
                if done:
                    break
                if s_id[j0] < 0:
                    lost = defect
                    break
                for j in range(8):
                    i = s_id[j0 + j]
                    if i < 0:
                        done = True  # a skipped token inside a group ends the walk: the flush behind it still runs
                        break
                    if prev >= 0 and i != prev:
                        acc[a0 + prev * D + c] += run
                        run = 0
                    run += q[t0 + s_pos[j0 + j], c]
                    prev = i
            if prev >= 0 and not lost:
                acc[a0 + prev * D + c] += run


def _runs_case(ids, V, defect, D=3):
    rng = np.random.default_rng(len(ids))
    dX = rng.standard_normal((len(ids), D)).astype(np.float32)
    _, h = guard_out((V, 2 * D), dtype=torch.int32, device="cpu")
    h.fill_payload(np.zeros((V, 2 * D), np.int32))
    buf, start = h.raw()
    assert start % 2 == 0
    standin_scatter_runs(ids, dX, (buf.view(np.int64), start // 2), V, defect)
    h.check("acc")
    got = h.payload().numpy().view(np.int64)
    assert np.array_equal(got, tr.scatter_ref(ids, dX, V)["fixed"]), "accumulator differs from the exact fixed-point sums"


def _old_ids(n_tok, V, kind, rng):
    """the id sets of test_duplicate_combining_gradient_accumulation_is_the_atomic_one_bit_for_bit"""
    ids = np.full(n_tok, V // 2, np.int32) if kind == "one_id" else rng.integers(0, V, n_tok).astype(np.int32)
    if n_tok > 100 and kind == "hot":
        pad = (rng.random(n_tok // 30 + 1) < 0.15).repeat(30)[:n_tok]
        ids[pad] = 0
        ids[10:14] = [V, -1, V + 5, -7]
        ids[20:60] = V - 1
    return ids


def test_defect_early_exit_loses_the_pending_run():
    V = 7
    old = [(700, 50), (5, 1000), (4099, 3), (130, 70), (64, 9), (65, 250002), (24000, 32000)]
    for n_tok, Vo in old:
        for kind in ("hot", "one_id", "uniform"):
            ids = _old_ids(n_tok, Vo, kind, np.random.default_rng(n_tok))
            if n_tok > 5000:
                ids = ids[:640]  # ten chunks of the long case are as good as all of them: the chunks do not interact
            _runs_case(ids, Vo, False, D=2)
            _runs_case(ids, Vo, True, D=2)  # missed: no chunk of theirs holds a multiple of 8 valid tokens short of 64
    for n_tok in tr.SCATTER_NTOK:
        for kind in tr.ID_PATTERNS:
            _runs_case(tr.scatter_ids(n_tok, V, kind), V, False)
    caught = []
    for kind in tr.ID_PATTERNS:
        try:
            _runs_case(tr.scatter_ids(129, V, kind), V, True)
        except AssertionError:
            caught.append(kind)
    assert caught == ["valid8"], caught


def standin_colsum_stage2(partials, defect):
    """Stand-in of stage 2 of the column reductions: 32 parts, each sums the row blocks part, part + 32, ... eight per trip
    (bk += 256).  Defect: one trip only."""
    nblk, C = partials.shape
    out = np.zeros(C, np.float32)
    for part in range(32):
        acc = np.zeros(C, np.float32)
        for bk in range(part, min(nblk, 256) if defect else nblk, 256):
            for j in range(8):
                if bk + 32 * j < nblk:
                    acc += partials[bk + 32 * j]
        out += acc
    return out


def _stage2_case(R, C, defect):
    rng = np.random.default_rng(R)
    nblk = max(1, min(-(-R // 32), 1024))
    partials = rng.standard_normal((nblk, C)).astype(np.float32)
    p64 = partials.astype(np.float64)
    tr.check_close(standin_colsum_stage2(partials, defect), (p64.sum(0), np.abs(p64).sum(0)), tr.C_SUM, "column sums")


def test_defect_stage_two_makes_one_trip_only():
    for R in tr.COLRED_OLD_R:
        _stage2_case(R, 5, False)
        _stage2_case(R, 5, True)  # missed: at most 47 row blocks
    for R, C in tr.COLRED_CASES:
        _stage2_case(R, C, False)
        with pytest.raises(AssertionError):
            _stage2_case(R, C, True)  # 257 and 1024 row blocks
