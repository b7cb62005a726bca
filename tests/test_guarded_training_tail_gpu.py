"""The kernels that close an NRMS training step on guard-banded operands at their edge shapes, against the float64 references of
tests/training_tail_refs.py: the fused user head (+ its finishing job), the scorer and the three losses, the embedding gather / title
expansion / three gradient scatters, Adam (plain, misaligned, fixed-point fused, inside the finishing launch) and the two-stage
column reductions behind ebn_bias_relu_bwd_f32 and the batch-norm pair.

Every operand goes through tests/guarded.py: float inputs sit between NaN guards, id inputs between HARMFUL integers (a gather id or
an article row outside its table raises the kernel's flag; a scatter id guard is the VALID row 0, so that an over-read token adds the
NaN guard of dX), outputs are pre-filled and sit between canaries, in-place operands are outputs with a payload, the int64
accumulators are int32 operands of twice the width with a zero payload, scratch is NaN.  After each call every handle is checked; a
refused call must leave every operand untouched.  Values are compared element-wise -- |got - want| <= c * mag + 1e-30 with `mag` the
reference's magnitude array; a NaN fails.  Bit-exact claims stay bit-exact: the gather and its dropout mask, the title expansion, the
fixed-point sums (== the float64 reference quantised the same way, and the two fixed kernels == each other), the ReLU gate, the
fused kernels against the separate ones, the head with its own reduction against the head + EBN_FINISH_HEAD job.  The label rows hold
one, two and no positives, so sum(y) is 1, 2 and 0.  The shapes (tests/training_tail_refs.py) are the smallest at which each
lane-, wave-, thread- and grid-strided loop takes a second trip and each limit is touched from both sides;
tests/test_training_tail_refs_cpu.py shows planted defects that only they catch.

The head is six stages in one launch (attention weights -> user -> scores -> loss and d(scores) -> d(user), d(cand) -> de -> d(pre-tanh),
dq, db).  From the inputs alone the magnitudes compound along that chain to thousands of times the values and bound nothing, so every
stage is held to float64 computed from the launch's OWN outputs of the stage before, taken as exact inputs (tr.head_ref(given=...)): a
magnitude of one step, as for a chain of separate kernels, and a stage that consumed anything but what the launch wrote fails.  The
whole chain from the inputs is held to the bounds tests/test_hip_kernels.py sets for the head.  The fused scorer likewise: its logits
from its inputs, everything behind them from its logits.  Loss kind 2 is defined with K.epsilon() and 1 - K.epsilon() as FLOAT32 holds
them (1 - 2^-23): where the clip is active at p = 1 (C = 1) the double constants give a loss 0.6 % away from the float32 model's.

NOT covered (they need tens of GB): the int64 index paths of the gather / scatters (2^32 items and more) and the overflow of the
int64 accumulators.  LIMIT (tests/guarded.py): an over-read whose value a select discards is not seen.

The constant c:
  * C_SUM = 2e-6 for outputs that are fp32 sums of products of the kernel's inputs (scores, the Adam moments, the column sums, the
    batch-norm outputs -- its division and square root are correctly rounded, the magnitudes carry the statistics' rounding);
  * for outputs behind tanhf / expf / logf / log1pf, a division by a softmax sum, or Adam's sqrt: 4 x the largest err / mag measured
    on an MI355X over all cases of this file, never above what tests/test_hip_kernels.py allows for the same quantity (the cap).

MI355X, 2026-10-20, on top of commit ba4ca4c; max err / mag over all cases of this file, and the c in force (no kernel defect found:
all cases pass):
  output           max err/mag  c
  head.w           3.425e-08   1.4e-07   (cap 2e-05)
  head.user        1.851e-07   C_SUM = 2e-6
  head.scores      1.002e-07   C_SUM = 2e-6
  head.probs       1.400e-07   5.6e-07   (cap 5e-05)
  head.loss_rows   9.933e-08   4.0e-07   (cap 5e-06)
  head.loss        7.457e-08   3.0e-07   (cap 5e-06)
  head.dcand       2.992e-07   1.2e-06   (cap 1e-04)
  head.duser       1.654e-07   6.6e-07   (cap 1e-04)
  head.de          8.541e-08   C_SUM = 2e-6
  head.dpre        1.309e-07   5.2e-07   (cap 1e-04)
  head.dq          8.829e-08   3.5e-07   (cap 1e-04)
  head.db          5.244e-08   2.1e-07   (cap 1e-04)
  score.scores     1.278e-07   C_SUM = 2e-6
  score.probs      1.858e-07   7.4e-07   (cap 3e-05)
  score.sigmoid    7.865e-08   3.1e-07   (cap 3e-05)
  score.loss_rows  1.477e-07   5.9e-07   (cap 3e-06)
  score.loss       1.610e-07   6.4e-07   (cap 3e-06)
  score.dcand      4.570e-07   1.8e-06   (cap 3e-05)
  score.duser      1.256e-06   5.0e-06   (cap 3e-05)   (the 8192 sequential terms of the candidate limit)
  pair.dot         1.739e-08   C_SUM = 2e-6
  pair.sigmoid     1.718e-08   6.9e-08   (cap 2e-05)
  scatter.dense    3.609e-07   C_SUM = 2e-6   (fp32 atomics: the order, and with it this figure, varies from run to run)
  adam.m           1.639e-07   C_SUM = 2e-6
  adam.v           1.543e-07   C_SUM = 2e-6
  adam.theta       9.164e-08   3.7e-07   (cap 1e-05)
  relu.dbias       8.024e-09   C_SUM = 2e-6
  bn.mean          2.726e-07   C_SUM = 2e-6
  bn.istd          1.483e-07   C_SUM = 2e-6
  bn.xhat          1.362e-07   C_SUM = 2e-6
  bn.Y             1.381e-07   C_SUM = 2e-6
  bn.moving_mean   9.646e-07   C_SUM = 2e-6   (the kernel's 1 - 0.99f is 0.0099999905, 1e-6 below 0.01)
  bn.moving_var    1.123e-07   C_SUM = 2e-6
  bn.dgamma        8.895e-09   C_SUM = 2e-6
  bn.dbeta         6.508e-09   C_SUM = 2e-6
  bn.dX            1.917e-07   C_SUM = 2e-6
The whole module runs in about 6 s; no case takes more than half a second.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import training_tail_refs as tr
from tests.guarded import guard_in, guard_out
from tests.hip_testutil import P, S, assert_close, host, make_state

pytestmark = pytest.mark.gpu
NAN = float("nan")
OK, BAD_ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -3
FLAT = 4096  # guard elements of a long flat operand (element-wise kernels: nothing strides by its length)
SEED, STEP = 11, 6

# output -> (largest err / mag measured on the MI355X, the cap: the relative bound of tests/test_hip_kernels.py on that quantity)
BEHIND_LIBM = {
    "head.w": (3.425e-08, 2e-5), "head.probs": (1.400e-07, 5e-5), "head.loss_rows": (9.933e-08, 5e-6), "head.loss": (7.457e-08, 5e-6),
    "head.dcand": (2.992e-07, 1e-4), "head.duser": (1.654e-07, 1e-4), "head.dpre": (1.309e-07, 1e-4), "head.dq": (8.829e-08, 1e-4),
    "head.db": (5.244e-08, 1e-4),
    "score.probs": (1.858e-07, 3e-5), "score.sigmoid": (7.865e-08, 3e-5), "score.loss_rows": (1.477e-07, 3e-6), "score.loss": (1.610e-07, 3e-6),
    "score.dcand": (4.570e-07, 3e-5), "score.duser": (1.256e-06, 3e-5), "pair.sigmoid": (1.718e-08, 2e-5),
    "adam.theta": (9.164e-08, 1e-5),
}
# (link by link, the head's user, scores and de are sums of products of the launch's own outputs: no libm call in their step)
SUMS = ("head.user", "head.scores", "head.de", "score.scores", "pair.dot", "adam.m", "adam.v", "scatter.dense", "relu.dbias", "bn.mean", "bn.istd", "bn.xhat", "bn.Y", "bn.moving_mean",
        "bn.moving_var", "bn.dgamma", "bn.dbeta", "bn.dX")
C = {k: (cap if m is None else min(4.0 * m, cap)) for k, (m, cap) in BEHIND_LIBM.items()}
C.update({k: tr.C_SUM for k in SUMS})
MEASURED = {}  # output -> the largest err / mag of this session (printed by every comparison: `pytest -s`)


def cmp(got, ref, key, what=""):
    """print err / mag, then assert |got - want| <= C[key] * mag + TINY element-wise"""
    got = host(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    r = tr.ratio(got.reshape(np.shape(ref[0])), ref[0], ref[1])
    MEASURED[key] = max(MEASURED.get(key, 0.0), r)
    print(f"ERRMAG {key} {r:.3e} {what}")
    tr.check_close(got, ref, C[key], f"{key} {what}")


def r32(a):
    return np.asarray(a, np.float64).astype(np.float32)


class G:
    """the guarded operands of one call sequence, by name"""

    def __init__(self):
        self.h = {}

    def _add(self, name, v, h):
        assert name not in self.h, name
        self.h[name] = h
        return v

    def i(self, x, name, fill=NAN, offset=0, guard=None):
        return self._add(name, *guard_in(x, fill=fill, offset=offset, guard=guard))

    def o(self, shape, name, dtype=torch.float32, offset=0, guard=None):
        return self._add(name, *guard_out(shape, dtype=dtype, offset=offset, guard=guard))

    def io(self, values, name, offset=0, guard=None):
        """an in-place operand (or an output with starting values): an output with a payload"""
        values = np.asarray(values)
        shape = values.shape if values.ndim <= 2 else (int(np.prod(values.shape[:-1])), values.shape[-1])
        v, h = guard_out(shape, dtype=torch.int32 if values.dtype.kind in "iu" else torch.float32, offset=offset, guard=guard)
        h.fill_payload(values.reshape(shape))
        return self._add(name, v, h)

    def ws(self, n, name):
        """scratch of n floats the kernel writes before it reads: NaN inside, canaries around"""
        return self.io(np.full(max(int(n), 1), NAN, np.float32), name, guard=FLAT)

    def acc(self, V, D, name, values=None, guard=None):
        """an int64 accumulator [V, D] as an int32 operand of twice the width (zero unless `values` int64 are given)"""
        v64 = np.zeros((V, D), np.int64) if values is None else np.ascontiguousarray(values, np.int64).reshape(V, D)
        t = self.io(v64.view(np.int32), name, guard=guard)
        assert t.data_ptr() % 16 == 0
        return t

    def flag(self, name="flag"):
        return self.io(np.zeros(1, np.int32), name)

    def get(self, name):
        """the payload of an operand on the host: float64 for floats, the int32 array for ints"""
        p = self.h[name].payload()
        return host(p) if p.dtype.is_floating_point else p.cpu().numpy()

    def bits(self, name):
        return self.h[name].payload().cpu().numpy().view(np.int32)

    def acc64(self, name):
        return self.h[name].payload().cpu().numpy().view(np.int64)

    def check(self, but=()):
        torch.cuda.synchronize()
        for name, h in self.h.items():
            (h.check_untouched if name in but else h.check)(name)

    def untouched(self):
        torch.cuda.synchronize()
        for name, h in self.h.items():
            h.check_untouched(name)


def state(alpha=0.0):
    return make_state(seed=SEED, step=STEP, alpha=alpha)


# ---------------------------------------------------------------------------------------------------------------- fused user head
HEAD_OUT = ("w", "user", "scores", "probs", "loss_rows", "loss", "dcand", "duser", "de", "dq", "db")


def _head_operands(g, data, B, L, C, E, A, hip, x_offset=0):
    Upre, b, q, X, cand, y = data
    a = dict(U=g.io(Upre.reshape(B * L, A), "U"), b=g.i(b, "b"), q=g.i(q, "q"), X=g.i(X.reshape(B * L, E), "X", offset=x_offset),
             cand=g.i(cand.reshape(B * C, E), "cand"), y=g.i(y.reshape(-1), "labels"), w=g.o((B * L,), "w"), user=g.o((B, E), "user"),
             scores=g.o((B * C,), "scores"), probs=g.o((B * C,), "probs"), loss_rows=g.o((B,), "loss_rows"), loss=g.o((1,), "loss"),
             dcand=g.o((B * C, E), "dcand"), duser=g.o((B, E), "duser"), de=g.o((B * L,), "de"), dq=g.o((A,), "dq"), db=g.o((A,), "db"))
    n_part = int(hip.lib().ebn_user_head_partials_len(B, A))
    assert n_part == B * 2 * A
    a["part"] = g.o((n_part,), "partials")  # scratch of exactly this length: every element is written
    return a


def _head_call(hip, a, B, L, C, E, A, kind, own_reduction):
    f = hip.lib().ebn_user_head_train_f32
    return f(P(a["U"]), P(a["b"]), P(a["q"]), P(a["X"]), P(a["cand"]), P(a["y"]), P(a["w"]), P(a["user"]), P(a["scores"]), P(a["probs"]),
             P(a["loss_rows"]), P(a["loss"]), P(a["dcand"]), P(a["duser"]), P(a["de"]), P(a["dq"]) if own_reduction else None,
             P(a["db"]) if own_reduction else None, P(a["part"]), B, L, C, E, A, kind, 1.0 / B, S())


def _head_run(hip, data, B, L, C, E, A, kind, own_reduction):
    g = G()
    a = _head_operands(g, data, B, L, C, E, A, hip)
    assert _head_call(hip, a, B, L, C, E, A, kind, own_reduction) == OK
    if own_reduction:
        g.check()
    else:
        g.check(but=("loss", "dq", "db"))  # left to the finishing launch: not written by this call
        job = hip.FinishJob(hip.FINISH_HEAD, 1, B, A, a["part"].data_ptr(), a["dq"].data_ptr(), a["db"].data_ptr(), A, 0.0, 1.0,
                            a["loss_rows"].data_ptr(), a["loss"].data_ptr())
        hip.call("ebn_grad_finish_f32", (hip.FinishJob * 1)(job), 1, S())
        g.check()
    return g


def _head_compare(g, data, B, kind, what):
    """(1) link by link: every stage of the launch against float64 computed from the launch's OWN outputs of the stage before (taken as
    exact inputs), with the magnitude of that one step -- what a chain of separate kernels would be held to; (2) the whole chain from the
    inputs against float64 at the bounds tests/test_hip_kernels.py sets for the head (the chain's magnitudes compound to thousands of times
    the values: they bound nothing useful)."""
    links = tr.head_ref(*data, kind, 1.0 / B, given={k: g.get(k) for k in tr.HEAD_LINKS})
    for name in HEAD_OUT:
        cmp(g.get(name), links[name], f"head.{name}", what)
    cmp(g.get("U"), links["dpre"], "head.dpre", what)
    ref = tr.head_ref(*data, kind, 1.0 / B)
    assert kind != 2 or ref["clip_margin"] > 0.5
    v = lambda name: ref[name][0]
    close = lambda name, want, rtol, atol: assert_close(g.get(name).reshape(want.shape), want, rtol=rtol, atol=atol, what=f"chain {name} {what}")
    close("w", v("w"), 2e-5, 1e-7)
    close("user", v("user"), 3e-5, 5e-7)
    close("scores", v("scores"), 3e-5, 3e-6)
    close("probs", v("probs"), 5e-5, 1e-7)
    Lw = float(v("loss")[0])
    assert abs(float(g.get("loss")[0]) - Lw) <= 5e-6 * max(1, abs(Lw)) and abs(g.get("loss_rows").sum() - Lw) <= 5e-6 * max(1, abs(Lw))
    close("dcand", v("dcand"), 1e-4, 2e-6 if kind == 2 else 1e-6)
    close("duser", v("duser"), 1e-4, 2e-6 if kind == 2 else 1e-6)
    for name, key, a0 in (("de", "de", 1e-6), ("U", "dpre", 1e-7), ("dq", "dq", 1e-6), ("db", "db", 1e-6)):
        close(name, v(key), 1e-4, a0 + 1e-4 * np.abs(v(key)).max())


def _head_case(hip, B, L, C, E, A, kind):
    assert hip.lib().ebn_user_head_supported(L, C, E, A) == 1
    data = tr.head_inputs(B, L, C, E, A)
    runs = [_head_run(hip, data, B, L, C, E, A, kind, own) for own in (True, False)]
    _head_compare(runs[0], data, B, kind, f"{(B, L, C, E, A)} kind {kind}")
    for name in HEAD_OUT + ("U", "partials"):  # the finishing job sums in the stand-alone pass's order: the same bits
        assert np.array_equal(runs[0].bits(name), runs[1].bits(name)), f"head + EBN_FINISH_HEAD job differs from the head's own reduction: {name}"


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("L,C,E,A", tr.HEAD_CASES)
def test_user_head_at_every_second_trip(hip, L, C, E, A, kind):
    _head_case(hip, tr.HEAD_B, L, C, E, A, kind)


def test_user_head_long_batch_second_trip_of_the_loss_row_sum(hip):
    _head_case(hip, *tr.HEAD_LONG_BATCH, 0)


def test_user_head_refuses_what_does_not_fit_and_what_is_misaligned(hip):
    B = 2
    L, C, E, A = tr.HEAD_REFUSED
    assert hip.lib().ebn_user_head_supported(L, C, E, A) == 0 and hip.lib().ebn_user_head_supported(L - 1, C, E, A) == 1
    for own in (True, False):
        g = G()
        a = _head_operands(g, tr.head_inputs(B, L, C, E, A), B, L, C, E, A, hip)
        assert _head_call(hip, a, B, L, C, E, A, 0, own) == UNSUPPORTED
        g.untouched()
    L, C, E, A = 5, 2, 8, 8
    g = G()
    a = _head_operands(g, tr.head_inputs(B, L, C, E, A), B, L, C, E, A, hip, x_offset=1)
    assert a["X"].data_ptr() % 16 == 4
    assert _head_call(hip, a, B, L, C, E, A, 0, True) == ALIGN
    g.untouched()


# ---------------------------------------------------------------------------------------------------------------- scorer + loss
def _score_data(B, C, E):
    rng = np.random.default_rng(C * 1000 + E)
    cand = (rng.standard_normal((B, C, E)) * 0.4).astype(np.float32)
    user = (rng.standard_normal((B, E)) * (1.5 / np.sqrt(E))).astype(np.float32)  # scores of O(1) at every E: clear of the clip of loss kind 2
    return cand, user


def _score_fwd(hip, cand, user, B, C, E, mode):
    g = G()
    sc, pr = g.o((B, C), "scores"), g.o((B, C), "probs")
    rc = hip.lib().ebn_score_fwd_f32(P(g.i(cand, "cand")), P(g.i(user, "user")), P(sc), P(pr), B, C, E, mode, S())
    return g, rc


def _score_bwd(hip, cand, user, scores, y, B, C, E, kind):
    g = G()
    rows, dc, du = g.o((B,), "loss_rows"), g.o((B * C, E), "dcand"), g.o((B, E), "duser")
    rc = hip.lib().ebn_score_loss_bwd_f32(P(g.i(cand, "cand")), P(g.i(user, "user")), P(g.i(scores, "scores")), P(g.i(y, "labels")), P(rows), P(dc), P(du),
                                          B, C, E, kind, 1.0 / B, S())
    return g, rc


def _score_train(hip, cand, user, y, B, C, E, kind):
    g = G()
    sc, pr, rows, tot, dc, du = g.o((B, C), "scores"), g.o((B, C), "probs"), g.o((B,), "loss_rows"), g.o((1,), "loss"), g.o((B * C, E), "dcand"), g.o((B, E), "duser")
    rc = hip.lib().ebn_score_loss_train_f32(P(g.i(cand, "cand")), P(g.i(user, "user")), P(g.i(y, "labels")), P(sc), P(pr), P(rows), P(tot), P(dc), P(du),
                                            B, C, E, kind, 1.0 / B, S())
    return g, rc


def _scorer_case(hip, B, C, E, y):
    what = f"{(B, C, E)}"
    cand, user = _score_data(B, C, E)
    fwd = tr.score_ref(cand, user)
    g0, rc = _score_fwd(hip, cand, user, B, C, E, 0)
    assert rc == OK
    g0.check()
    cmp(g0.get("scores"), fwd["scores"], "score.scores", what)
    sc32 = g0.h["scores"].payload().cpu().numpy()
    act = tr.score_ref(cand, user, scores=sc32)  # the activations from the kernel's own logits: one step
    cmp(g0.get("probs"), act["probs"], "score.probs", what)
    g1, rc = _score_fwd(hip, cand, user, B, C, E, 1)
    assert rc == OK
    g1.check()
    assert np.array_equal(g1.bits("scores"), g0.bits("scores"))
    cmp(g1.get("probs"), act["sigmoid"], "score.sigmoid", what)
    for kind in (0, 1, 2):
        # the backward kernel on the forward kernel's logits: its reference takes them as given
        ref = tr.score_loss_ref(cand, user, y, kind, 1.0 / B, scores=sc32)
        assert kind != 2 or ref["clip_margin"] > 0.5
        gb, rc = _score_bwd(hip, cand, user, sc32, y, B, C, E, kind)
        assert rc == OK
        gb.check()
        for name in ("loss_rows", "dcand", "duser"):
            cmp(gb.get(name), ref[name], f"score.{name}", f"bwd {what} kind {kind}")
        # the fused kernel: its logits against float64 from its inputs, everything behind them against float64 from ITS logits (one
        # step, like the backward kernel), and all of it against the separate kernels bit for bit
        gt, rc = _score_train(hip, cand, user, y, B, C, E, kind)
        assert rc == OK
        gt.check()
        cmp(gt.get("scores"), fwd["scores"], "score.scores", f"train {what}")
        ref = tr.score_loss_ref(cand, user, y, kind, 1.0 / B, scores=gt.h["scores"].payload().cpu().numpy())
        for name in ("probs", "loss_rows", "loss", "dcand", "duser"):
            cmp(gt.get(name), ref[name], f"score.{name}", f"train {what} kind {kind}")
        for name, other in (("scores", g0), ("probs", g0), ("loss_rows", gb), ("dcand", gb), ("duser", gb)):
            assert np.array_equal(gt.bits(name), other.bits(name)), f"fused scorer differs from the separate kernels: {name}, {what} kind {kind}"


@pytest.mark.parametrize("C,E", tr.SCORE_CASES)
def test_scorer_and_losses_against_float64(hip, C, E):
    _scorer_case(hip, 3, C, E, tr.label_rows(3, C))


@pytest.mark.parametrize("first", [0, 1, 2])
def test_scorer_at_the_candidate_limit(hip, first):
    B, C, E = tr.SCORE_LIMIT
    _scorer_case(hip, B, C, E, tr.label_rows(B, C, first=first))


def test_scorer_refuses_one_candidate_too_many(hip):
    B, C, E = tr.SCORE_LIMIT
    C += 1
    cand, user = _score_data(B, C, E)
    y = tr.label_rows(B, C)
    for mode in (0, 1):
        g, rc = _score_fwd(hip, cand, user, B, C, E, mode)
        assert rc == UNSUPPORTED
        g.untouched()
    g, rc = _score_bwd(hip, cand, user, np.zeros((B, C), np.float32), y, B, C, E, 0)
    assert rc == UNSUPPORTED
    g.untouched()
    g, rc = _score_train(hip, cand, user, y, B, C, E, 0)
    assert rc == UNSUPPORTED
    g.untouched()


def test_pair_score_five_pairs(hip):
    nu, nn, E, n_pairs = 3, 4, 65, 5
    rng = np.random.default_rng(47)
    user, news = (rng.standard_normal((nu, E)) * 0.3).astype(np.float32), (rng.standard_normal((nn, E)) * 0.3).astype(np.float32)
    ui, ni = np.array([2, 0, 1, 2, 0], np.int32), np.array([3, 0, 1, 1, 2], np.int32)
    ref = tr.pair_score_ref(user, news, ui, ni)
    for mode, name in ((0, "dot"), (1, "sigmoid")):
        g = G()
        out = g.o((n_pairs,), "out")
        # an index guard names the row behind the table: the NaN guard of user / news
        hip.call("ebn_pair_score_f32", P(g.i(user, "user")), P(g.i(news, "news")), P(g.i(ui, "u_idx", fill=nu)), P(g.i(ni, "n_idx", fill=nn)), P(out),
                 n_pairs, E, mode, S())
        g.check()
        cmp(g.get("out"), ref[name], f"pair.{name}")


# ---------------------------------------------------------------------------------------------------------------- gather, expansion
def _gather_ids(n_tok, V, rng, oob):
    ids = rng.integers(0, V, n_tok).astype(np.int32)
    ids[0], ids[-1] = 0, V - 1
    if oob:
        ids[n_tok // 2] = V
        ids[(n_tok // 3) if n_tok > 2 else 0] = -1
        if n_tok == 1:
            ids[0] = V
    return ids


def _gather_case(hip, D, n_tok, p, V=11, table_offset=0):
    rng = np.random.default_rng(D * 100 + n_tok)
    table = rng.standard_normal((V, D)).astype(np.float32)
    mult = tr.drop_mult32(SEED, STEP, 0, n_tok * D, p).reshape(n_tok, D) if p > 0 else None
    st = state()
    for oob in (False, True):
        ids = _gather_ids(n_tok, V, rng, oob)
        want, want_flag = tr.gather_ref(ids, table, mult)
        assert want_flag == oob
        g = G()
        out, flag = g.o((n_tok, D), "out"), g.flag()
        t = g.i(table, "table", offset=table_offset)
        # an id guard is a row outside the table: an over-read raises the flag of the clean run
        hip.call("ebn_gather_rows_f32", P(g.i(ids, "ids", fill=V + 3, guard=FLAT)), P(t), P(out), n_tok, D, V, P(st) if p > 0 else None, 0 if p > 0 else -1,
                 p, P(flag), S())
        g.check()
        assert int(g.get("flag")[0]) == int(oob), (D, n_tok, p, oob)
        got = g.h["out"].payload().cpu().numpy()
        # exact as values (+0 == -0: a dropped negative element is -0 on the scalar path; a NaN equals nothing)
        assert np.array_equal(got, want), f"gather differs from table[ids] * mask: D {D}, n_tok {n_tok}, p {p}, oob {oob}"
        if oob:
            assert (got[(ids < 0) | (ids >= V)] == 0).all()


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("D,n_tok", tr.GATHER_CASES)
def test_gather_every_path_both_sides_of_a_block(hip, D, n_tok, p):
    _gather_case(hip, D, n_tok, p)


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_gather_misaligned_table_takes_the_scalar_path(hip, p):
    _gather_case(hip, 8, 70, p, table_offset=1)


def test_gather_scalar_path_past_its_grid_cap(hip):
    _gather_case(hip, 1025, 2049, 0.2, V=5)  # 2 100 225 items > 8192 blocks x 256


def test_expand_titles_past_its_grid_cap(hip):
    n_rows, T, n_titles = 37, 3, 699100  # 2 097 300 items > 8192 blocks x 256
    rng = np.random.default_rng(81)
    matrix = rng.integers(0, 250002, (n_rows, T)).astype(np.int32)
    for oob in (False, True):
        idx = rng.integers(0, n_rows, n_titles).astype(np.int32)
        if oob:
            idx[5], idx[-1] = n_rows, -1
        ok = (idx >= 0) & (idx < n_rows)
        want = np.where(ok[:, None], matrix[np.clip(idx, 0, n_rows - 1)], 0).astype(np.int32)
        g = G()
        out, flag = g.o((n_titles * T,), "ids_out", dtype=torch.int32, guard=FLAT), g.flag()
        hip.call("ebn_expand_titles_i32", P(g.i(idx, "art_idx", fill=n_rows, guard=FLAT)), P(g.i(matrix, "token_matrix", fill=-777)), P(out), n_titles, T,
                 n_rows, P(flag), S())
        g.check()
        assert int(g.get("flag")[0]) == int(oob)
        assert np.array_equal(g.get("ids_out").reshape(n_titles, T), want)


# ---------------------------------------------------------------------------------------------------------------- gradient scatters
def _scatter_three(hip, ids, dX, V, D, p, st, what):
    """the float scatter and the two fixed-point ones on the same operands -> the fixed accumulator (checked against the reference)"""
    n_tok = len(ids)
    mult = tr.drop_mult32(SEED, STEP, 0, n_tok * D, p).reshape(n_tok, D) if p > 0 else None
    ref = tr.scatter_ref(ids, dX, V, mult)
    sp, site = (P(st), 0) if p > 0 else (None, -1)
    g = G()
    # an id guard is the VALID row 0: a token read past the end adds the NaN guard of dX
    d_ids, d_dx = g.i(ids, "ids", fill=0, guard=FLAT), g.i(dX, "dX")
    dT = g.io(np.zeros((V, D), np.float32), "dTable")
    hip.call("ebn_embedding_grad_scatter_f32", P(d_ids), P(d_dx), P(dT), n_tok, D, V, sp, site, p, S())
    g.check()
    cmp(g.get("dTable"), ref["dense"], "scatter.dense", what)
    accs = {}
    for fn in ("ebn_embedding_grad_scatter_fixed", "ebn_embedding_grad_scatter_fixed_atomic"):
        acc, flag = g.acc(V, D, fn), g.flag(fn + ".flag")
        hip.call(fn, P(d_ids), P(d_dx), P(acc), n_tok, D, V, sp, site, p, P(flag), S())
        g.check()
        assert int(g.get(fn + ".flag")[0]) == 0
        accs[fn] = g.acc64(fn)
        assert np.array_equal(accs[fn], ref["fixed"]), f"{fn}: the accumulator is not the exact sum of the quantised terms ({what})"
    a, b = accs.values()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("D", tr.SCATTER_D)
@pytest.mark.parametrize("n_tok", tr.SCATTER_NTOK)
def test_scatters_on_hand_built_id_patterns(hip, n_tok, D, p):
    V = 7
    rng = np.random.default_rng(n_tok * 10000 + D)
    dX = (rng.standard_normal((n_tok, D)) * 10 ** rng.uniform(-4, 0, (n_tok, 1))).astype(np.float32)
    st = state()
    for kind in tr.ID_PATTERNS:
        _scatter_three(hip, tr.scatter_ids(n_tok, V, kind), dX, V, D, p, st, f"{kind} n_tok {n_tok} D {D} p {p}")


def test_atomic_scatters_past_their_grid_cap(hip):
    n_tok, D, V = 2049, 1024, 50  # 2 098 176 items > 8192 blocks x 256
    rng = np.random.default_rng(2049)
    ids = rng.integers(0, V, n_tok).astype(np.int32)
    ids[:300] = 0
    ids[[7, 1000, 2048]] = [V, -1, V + 5]
    dX = rng.standard_normal((n_tok, D)).astype(np.float32)
    _scatter_three(hip, ids, dX, V, D, 0.3, state(), "past the grid cap")


# ---------------------------------------------------------------------------------------------------------------- Adam
ALPHA = float(np.float32(7e-4))


def _adam_data(n, seed):
    rng = np.random.default_rng(seed)
    th, m, v = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32), (rng.random(n) * 0.01).astype(np.float32)
    g = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 0.5, n)).astype(np.float32)
    g[: n // 3] = 0.0  # untouched embedding rows still get the dense moment decay
    m[: n // 7], v[: n // 7] = 0.0, 0.0  # ... and rows nothing has ever touched stay exactly where they are
    return th, g, m, v


def _adam_compare(g, ref, what, sel=None):
    for name in ("theta", "m", "v"):
        got, r = g.get(name), ref[name]
        if sel is not None:
            got, r = got[sel], (r[0][sel], r[1][sel])
        cmp(got, r, f"adam.{name}", what)


@pytest.mark.parametrize("n,theta_offset", [(4194304 + 1029, 0), (1048576 + 3, 1)])
def test_adam_step_past_its_grid_cap(hip, n, theta_offset):
    """aligned: the vector kernel (4 194 304 elements per trip) + its scalar tail; theta misaligned by 4 bytes: the scalar kernel
    (1 048 576 per trip)"""
    th, gr, m, v = _adam_data(n, n)
    ref = tr.adam_ref(th, gr, m, v, ALPHA, gscale=0.5)
    g = G()
    t = g.io(th, "theta", offset=theta_offset, guard=FLAT)
    assert t.data_ptr() % 16 == 4 * theta_offset
    hip.call("ebn_adam_keras_step_f32", P(t), P(g.i(gr, "g", guard=FLAT)), P(g.io(m, "m", guard=FLAT)), P(g.io(v, "v", guard=FLAT)), n, P(state(ALPHA)), 0.9, 0.999,
             1e-7, 0.5, S())
    g.check()
    _adam_compare(g, ref, f"n {n} offset {theta_offset}")
    assert np.array_equal(g.get("theta")[: n // 7], th[: n // 7].astype(np.float64))


def _quantise(gr):
    return np.rint(gr.astype(np.float64) * tr.FIXED_SCALE).astype(np.int64)


def test_fixed_to_f32_past_its_grid_cap(hip):
    n = 1048576 + 3
    acc64 = _quantise(_adam_data(n, n)[1])
    g = G()
    acc, out, flag = g.acc(1, n, "acc", acc64, guard=FLAT), g.o((n,), "out", guard=FLAT), g.flag()
    hip.call("ebn_fixed_to_f32", P(acc), P(out), n, P(flag), S())
    g.check()
    assert np.array_equal(g.h["out"].payload().cpu().numpy().view(np.int32), tr.fixed_to_f32_ref(acc64).view(np.int32))
    assert not g.acc64("acc").any() and int(g.get("flag")[0]) == 0  # the accumulator is left zeroed for the next step


def test_fixed_point_adam_past_its_grid_cap(hip):
    n = 4194304 + 5
    th, gr, m, v = _adam_data(n, n)
    acc64 = _quantise(gr)
    g32 = tr.fixed_to_f32_ref(acc64)  # the gradient the kernel forms: the accumulator as one float32
    ref = tr.adam_ref(th, g32, m, v, ALPHA, gscale=0.5)
    st = state(ALPHA)
    g = G()
    acc, flag = g.acc(1, n, "acc", acc64, guard=FLAT), g.flag()
    hip.call("ebn_adam_keras_step_fixed_f32", P(g.io(th, "theta", guard=FLAT)), P(acc), P(g.io(m, "m", guard=FLAT)), P(g.io(v, "v", guard=FLAT)), n, P(st),
             0.9, 0.999, 1e-7, 0.5, P(flag), S())
    g.check()
    _adam_compare(g, ref, f"fixed n {n}")
    assert not g.acc64("acc").any() and int(g.get("flag")[0]) == 0
    # the two kernels it fuses, on the same inputs: the same bits
    g2 = G()
    hip.call("ebn_adam_keras_step_f32", P(g2.io(th, "theta", guard=FLAT)), P(g2.i(g32, "g", guard=FLAT)), P(g2.io(m, "m", guard=FLAT)),
             P(g2.io(v, "v", guard=FLAT)), n, P(st), 0.9, 0.999, 1e-7, 0.5, S())
    g2.check()
    for name in ("theta", "m", "v"):
        assert np.array_equal(g.bits(name), g2.bits(name)), name


def test_finishing_launch_adam_over_rest_ranges_with_an_empty_one(hip):
    """ebn_grad_finish_adam_f32 with no job and the rest ranges (1, 4095, 0, 4097): a zero-length range and a 4096-element block
    boundary both fall inside the ranges; what no range owns does not move."""
    lens = tr.FINISH_REST
    offs, numel = [], 64
    for n in lens:
        offs.append(numel)
        numel += -(-(n + 37) // 64) * 64  # a gap nobody owns behind every range
    th, gr, m, v = _adam_data(numel, 5)
    own = np.zeros(numel, bool)
    for o, n in zip(offs, lens):
        own[o:o + n] = True
    assert own.sum() == sum(lens) == 8193
    ref = tr.adam_ref(th, gr, m, v, ALPHA)
    g = G()
    ad = hip.AdamFlat()
    ad.theta, ad.grad, ad.m, ad.v = (t.data_ptr() for t in (g.io(th, "theta"), g.i(gr, "grad"), g.io(m, "m"), g.io(v, "v")))
    ad.numel, ad.beta1, ad.beta2, ad.eps, ad.grad_scale, ad.n_rest = numel, 0.9, 0.999, 1e-7, 1.0, len(lens)
    for i, (o, n) in enumerate(zip(offs, lens)):
        ad.rest_off[i], ad.rest_len[i] = o, n
    assert hip.lib().ebn_grad_finish_adam_f32(None, 0, ctypes.byref(ad), P(state(ALPHA)), S()) == OK
    g.check()
    _adam_compare(g, ref, "rest ranges", sel=own)
    for name, was in (("theta", th), ("m", m), ("v", v)):
        assert np.array_equal(g.bits(name)[~own], was.view(np.int32)[~own]), f"{name}: an element no range owns moved"


# ---------------------------------------------------------------------------------------------------------------- column reductions
@pytest.mark.parametrize("R,C", tr.COLRED_CASES)
def test_bias_relu_backward_many_row_blocks(hip, R, C):
    rng = np.random.default_rng(R + C)
    Y = np.maximum(rng.standard_normal((R, C)), 0).astype(np.float32)
    dY = rng.standard_normal((R, C)).astype(np.float32)
    ref = tr.relu_bwd_ref(Y, dY)
    g = G()
    dX, dbias = g.o((R, C), "dX"), g.o((C,), "dbias")
    part = g.ws(hip.lib().ebn_colsum_partials_len(R, C), "partials")
    hip.call("ebn_bias_relu_bwd_f32", P(g.i(Y, "Y")), P(g.i(dY, "dY")), P(dX), P(dbias), P(part), R, C, 0, S())
    g.check()
    assert np.array_equal(g.bits("dX"), r32(ref["dX"][0]).view(np.int32))  # a gate: exact
    cmp(g.get("dbias"), ref["dbias"], "relu.dbias", f"R {R} C {C}")


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("R,C", tr.COLRED_CASES)
def test_batchnorm_pair_many_row_blocks(hip, R, C, p):
    rng = np.random.default_rng(R * 3 + C)
    X = np.maximum(rng.standard_normal((R, C)) + 0.3, 0).astype(np.float32)
    dY = rng.standard_normal((R, C)).astype(np.float32)
    gamma, beta = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    mm0, mv0 = (0.05 * rng.standard_normal(C)).astype(np.float32), (1 + 0.1 * rng.random(C)).astype(np.float32)
    site, off = 9, 1000
    mult = tr.drop_mult32(SEED, STEP, site, R * C, p, start=off).reshape(R, C).astype(np.float64) if p > 0 else 1.0
    st = state()
    what = f"R {R} C {C} p {p}"
    n_part = hip.lib().ebn_colsum_partials_len(R, C)
    fwd = tr.bn_fwd_ref(X, gamma, beta, mm0, mv0, mult)
    g = G()
    Y, xhat, mean, istd = g.o((R, C), "Y"), g.o((R, C), "xhat"), g.o((C,), "mean"), g.o((C,), "istd")
    hip.call("ebn_batchnorm_fwd_f32", P(g.i(X, "X")), P(g.i(gamma, "gamma")), P(g.i(beta, "beta")), P(g.io(mm0, "moving_mean")), P(g.io(mv0, "moving_var")),
             P(Y), P(xhat), P(mean), P(istd), P(g.ws(n_part, "partials")), R, C, 1, P(st), site, p, ctypes.c_int64(off), S())
    g.check()
    for name in ("mean", "istd", "xhat", "Y", "moving_mean", "moving_var"):
        cmp(g.get(name), fwd[name], f"bn.{name}", what)
    # the backward on the float64 forward's outputs rounded to float32: judged on its own step
    xh32, is32 = r32(fwd["xhat"][0]), r32(fwd["istd"][0])
    acc = C == 65
    g0, b0 = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    bwd = tr.bn_bwd_ref(dY, xh32, gamma, is32, mult, g0 if acc else None, b0 if acc else None)
    g = G()
    dX = g.o((R, C), "dX")
    dg, db = (g.io(g0, "dgamma"), g.io(b0, "dbeta")) if acc else (g.o((C,), "dgamma"), g.o((C,), "dbeta"))
    hip.call("ebn_batchnorm_bwd_f32", P(g.i(dY, "dY")), P(g.i(xh32, "xhat")), P(g.i(gamma, "gamma")), P(g.i(is32, "istd")), P(dX), P(dg), P(db),
             P(g.ws(n_part, "partials")), R, C, 1, int(acc), P(st), site, p, ctypes.c_int64(off), S())
    g.check()
    for name in ("dgamma", "dbeta", "dX"):
        cmp(g.get(name), bwd[name], f"bn.{name}", what)


def test_zz_report_measured_constants(hip):
    """last in the module: the err / mag table of this session (`pytest -s`); every constant in force is within its cap"""
    for k in sorted(MEASURED):
        m, cap = BEHIND_LIBM.get(k, (None, None))
        print(f"TABLE {k:18s} {MEASURED[k]:.3e}   " + ("C_SUM = 2e-6" if cap is None else f"{min(4 * MEASURED[k], cap):.1e}   (cap {cap:g}; in force {C[k]:.1e})"))
    assert all(c <= BEHIND_LIBM[k][1] for k, c in C.items() if k in BEHIND_LIBM)
