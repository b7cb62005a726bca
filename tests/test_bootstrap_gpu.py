"""ebn_poisson_bootstrap_f64 (csrc/ebn_bootstrap.hip) through the C ABI, against the numpy twin of the weight stream.

Every call runs on guard-banded operands: `values` sits in a NaN-filled buffer with ld = n + 3 (NaN behind every column and on both
sides), both outputs and the workspace sit inside sentinel-filled buffers, the outputs are pre-filled with the sentinel and the
workspace is poisoned with 0xFF bytes (NaN as fp64).  After the call: the sentinels around outputs and workspace survive, every
output was written, and every sum is finite.

Bound on a sum: the twin accumulates sum_i w_i x_i in np.longdouble; any summation order of n float64 terms has a first-order error
of at most (n - 1) u sum |terms| with u = 2^-53, and each term w_i x_i carries one more rounding at most (the kernel's fma has none),
so |got - want| <= n * 2^-52 * sum_i w_i |x_i| holds with room for every order.  weight_sums are integers and must be equal."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ebrec.evaluation import bootstrap as bs

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
T, R = bs.TILE, bs.RESAMPLES
SENTINEL = 0x5A5AC3C35A5AC3C3  # as a double: 8.3e125, finite; as bytes: never what a sum of these inputs is
GUARD = 4096                    # elements on each side
SEED, FIRST_KEY, FIRST_RESAMPLE = 7, 777, 12345
N_ITEMS = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
N_RESAMPLES = [1, 63, 64, 65, R - 1, R + 1]
N_COLS = [1, 2, 16]
BIG_N = 512 * T * 2 + 5  # 1025 tiles: three tiles a range, 342 ranges, a ragged last range and a ragged last tile


@functools.lru_cache(maxsize=None)
def _case(n, clustered):
    """values [16, n] float64 and the item keys (cluster codes with repeats, or first_key + i): computed once, shared, read-only"""
    rng = np.random.default_rng(1000 + n + (1 << 20) * clustered)
    x = rng.normal(size=(16, n)) * np.exp(rng.normal(size=(16, 1)) * 3.0)  # columns of very different scales
    codes = rng.integers(0, max(n // 3, 1), n).astype(np.uint32) if clustered else None
    keys = codes if clustered else (np.arange(n, dtype=np.uint64) + FIRST_KEY).astype(np.uint32)
    x.setflags(write=False)
    keys.setflags(write=False)
    return x, codes, keys


@functools.lru_cache(maxsize=None)
def _weights(n, clustered, first_resample, n_resamples, seed=SEED):
    w = bs.poisson_weights(_case(n, clustered)[2], seed, first_resample, n_resamples)
    w.setflags(write=False)
    return w


def _reference(x, w):
    """(sums [B, m] in long double, bound [B, m], weight sums [B] int64) for values x [m, n] and weights w [B, n]"""
    wl = w.astype(np.longdouble)
    want = wl @ x.T.astype(np.longdouble)
    bound = x.shape[1] * 2.0 ** -52 * (w.astype(np.float64) @ np.abs(x).T)
    return want, bound, w.astype(np.int64).sum(1)


class Guarded:
    """an int64-viewable device buffer of `count` 8-byte payload elements inside GUARD sentinels on each side"""

    def __init__(self, count, dtype):
        self.count = count
        self.raw = torch.full((2 * GUARD + max(count, 1),), SENTINEL, dtype=torch.int64, device="cuda")
        self.view = self.raw[GUARD:GUARD + count].view(dtype)
        assert self.view.data_ptr() % 16 == 0

    def check(self, what, written=True):
        assert bool((self.raw[:GUARD] == SENTINEL).all()), f"{what}: sentinels in front were overwritten"
        assert bool((self.raw[GUARD + self.count:] == SENTINEL).all()), f"{what}: sentinels behind were overwritten"
        if written:
            assert not bool((self.raw[GUARD:GUARD + self.count] == SENTINEL).any()), f"{what}: an output was never written"

    def untouched(self, what):
        assert bool((self.raw == SENTINEL).all()), f"{what}: written by a call that returned an error"


def _guarded_values(x, pad):
    """x [m, n] -> (float64 device buffer full of NaN with column c at GUARD + c * ld, ld)"""
    m, n = x.shape
    ld = n + pad
    buf = torch.full((2 * GUARD + m * ld,), float("nan"), dtype=torch.float64, device="cuda")
    buf[GUARD:GUARD + m * ld].view(m, ld)[:, :n].copy_(torch.from_numpy(np.array(x)))
    return buf, ld


def _run(hip, x, codes, first_key, seed, first_resample, B, pad=3):
    """one guarded call -> (sums [B, m] float64, weight_sums [B] int64) as numpy arrays"""
    m, n = x.shape
    vbuf, ld = _guarded_values(x, pad)
    snap = vbuf.view(torch.int64).clone()
    keys = None if codes is None else torch.from_numpy(np.array(codes).view(np.int32)).cuda()
    sums, wsum = Guarded(B * m, torch.float64), Guarded(B, torch.int64)
    ws_bytes = int(hip.lib().ebn_poisson_bootstrap_workspace_bytes(n, B, m))
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    ws = Guarded(ws_bytes // 8, torch.int64)
    ws.view.fill_(-1)  # every byte 0xFF: NaN for a partial sum that would be read before it is written
    rc = hip.lib().ebn_poisson_bootstrap_f64(ctypes.c_void_p(vbuf.data_ptr() + 8 * GUARD), ld, n, m, hip.ptr(keys), first_key, seed,
                                            first_resample, B, hip.ptr(sums.view), hip.ptr(wsum.view), hip.ptr(ws.view), ws_bytes,
                                            hip.stream_handle())
    assert rc == OK, rc
    torch.cuda.synchronize()
    sums.check("sums"), wsum.check("weight_sums"), ws.check("workspace", written=False)
    assert torch.equal(vbuf.view(torch.int64), snap), "values were written"
    got = sums.view.cpu().numpy().reshape(B, m)
    assert np.isfinite(got).all(), "a NaN of the padding or of the poisoned workspace reached a sum"
    return got, wsum.view.cpu().numpy()


def _assert_sums(got, want, bound, what):
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} sums off; worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3e}"


@pytest.mark.parametrize("clustered", [False, True], ids=["rows", "clusters"])
@pytest.mark.parametrize("n", N_ITEMS + [BIG_N])
def test_sums_and_weights_against_the_twin(hip, n, clustered):
    x, codes, _ = _case(n, clustered)
    combos = [(65, 2)] if n == BIG_N else [(B, m) for B in N_RESAMPLES for m in N_COLS]
    for B, m in combos:
        w = _weights(n, clustered, FIRST_RESAMPLE, B)
        want, bound, wsum = _reference(x[:m], w)
        got, got_w = _run(hip, x[:m], codes, 0 if clustered else FIRST_KEY, SEED, FIRST_RESAMPLE, B)
        print(f"n={n} B={B} m={m}: max err/bound {float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()):.3e}")
        assert np.array_equal(got_w, wsum), (n, B, m)
        _assert_sums(got, want, bound, f"n={n} B={B} m={m}")


def test_last_resample_numbers_of_the_stream(hip):
    """first_resample + n_resamples == 2^32: the resample number is a uint32 counter used up to its last value"""
    n, B = T + 1, 65
    x, _, keys = _case(n, False)
    first = 2 ** 32 - B
    w = bs.poisson_weights(keys, SEED, first, B)
    want, bound, wsum = _reference(x[:2], w)
    got, got_w = _run(hip, x[:2], None, FIRST_KEY, SEED, first, B)
    assert np.array_equal(got_w, wsum)
    _assert_sums(got, want, bound, "last resamples")


@pytest.mark.parametrize("n", [2 * T + 3, BIG_N])
def test_bits_do_not_depend_on_run_columns_or_blocking(hip, n):
    x, codes, _ = _case(n, True)
    B = R + 1
    whole, whole_w = _run(hip, x[:3], codes, 0, SEED, FIRST_RESAMPLE, B)
    again, again_w = _run(hip, x[:3], codes, 0, SEED, FIRST_RESAMPLE, B, pad=5)  # another run, another leading dimension
    assert np.array_equal(whole.view(np.int64), again.view(np.int64)) and np.array_equal(whole_w, again_w)
    for c in range(3):  # a column alone, and in other company (16 columns: another instantiation of the kernel)
        alone, alone_w = _run(hip, x[c:c + 1], codes, 0, SEED, FIRST_RESAMPLE, B)
        assert np.array_equal(alone[:, 0].view(np.int64), whole[:, c].view(np.int64)), c
        assert np.array_equal(alone_w, whole_w)
    wide, _ = _run(hip, x, codes, 0, SEED, FIRST_RESAMPLE, B)
    assert np.array_equal(wide[:, :3].view(np.int64), whole.view(np.int64))
    # blocks over resamples: rows [first, first + b) of one call
    at = 0
    for b in (1, 63, R - 128, 65):
        part, part_w = _run(hip, x[:3], codes, 0, SEED, FIRST_RESAMPLE + at, b)
        assert np.array_equal(part.view(np.int64), whole[at:at + b].view(np.int64)), (at, b)
        assert np.array_equal(part_w, whole_w[at:at + b])
        at += b
    assert at == B


@pytest.mark.parametrize("clustered", [False, True], ids=["rows", "clusters"])
def test_item_shards_add_to_the_whole(hip, clustered):
    n, cut, B, m = 2 * T + 3, T + 77, 65, 2
    x, codes, _ = _case(n, clustered)
    w = _weights(n, clustered, FIRST_RESAMPLE, B)
    want, bound, wsum = _reference(x[:m], w)
    s0, w0 = _run(hip, x[:m, :cut], None if codes is None else codes[:cut], 0 if clustered else FIRST_KEY, SEED, FIRST_RESAMPLE, B)
    s1, w1 = _run(hip, x[:m, cut:], None if codes is None else codes[cut:], 0 if clustered else FIRST_KEY + cut, SEED, FIRST_RESAMPLE, B)
    whole, whole_w = _run(hip, x[:m], codes, 0 if clustered else FIRST_KEY, SEED, FIRST_RESAMPLE, B)
    assert np.array_equal(w0 + w1, wsum) and np.array_equal(whole_w, wsum)
    _assert_sums(s0 + s1, want, bound, "shards")  # one more rounding, of the final add: far inside the bound's factor n
    _assert_sums(whole, want, bound, "whole")


def test_argument_checks_return_codes_and_launch_nothing(hip):
    L = hip.lib()
    n, B, m = 100, 10, 2
    x, _, _ = _case(T, False)
    vbuf, ld = _guarded_values(x[:m, :n], 3)
    v = ctypes.c_void_p(vbuf.data_ptr() + 8 * GUARD)
    sums, wsum = Guarded(B * m, torch.float64), Guarded(B, torch.int64)
    ws_bytes = int(L.ebn_poisson_bootstrap_workspace_bytes(n, B, m))
    ws = Guarded(ws_bytes // 8, torch.int64)
    S, W, WS, st = hip.ptr(sums.view), hip.ptr(wsum.view), hip.ptr(ws.view), hip.stream_handle()
    call = L.ebn_poisson_bootstrap_f64
    before = L.ebn_launch_count()
    assert call(v, ld, n, 0, None, 0, 1, 0, B, S, W, WS, ws_bytes, st) == BAD_ARG          # no columns
    assert call(v, ld, n, 17, None, 0, 1, 0, B, S, W, WS, ws_bytes, st) == UNSUPPORTED     # more than EBN_BS_MAX_COLS
    assert call(v, ld, -1, m, None, 0, 1, 0, B, S, W, WS, ws_bytes, st) == BAD_ARG
    assert call(v, ld, 2 ** 31 - 256, m, None, 0, 1, 0, B, S, W, WS, ws_bytes, st) == BAD_ARG
    assert call(v, n - 1, n, m, None, 0, 1, 0, B, S, W, WS, ws_bytes, st) == BAD_ARG       # ld < n_items
    assert call(v, ld, n, m, None, 0, 1, 0, -1, S, W, WS, ws_bytes, st) == BAD_ARG
    assert call(v, ld, n, m, None, 0, 1, -1, B, S, W, WS, ws_bytes, st) == BAD_ARG
    assert call(v, ld, n, m, None, 0, 1, 2 ** 32 - B + 1, B, S, W, WS, ws_bytes, st) == BAD_ARG  # past the last resample number
    assert call(None, ld, n, m, None, 0, 1, 0, B, S, W, WS, ws_bytes, st) == BAD_ARG
    assert call(v, ld, n, m, None, 0, 1, 0, B, None, W, WS, ws_bytes, st) == BAD_ARG
    assert call(v, ld, n, m, None, 0, 1, 0, B, S, None, WS, ws_bytes, st) == BAD_ARG
    assert call(v, ld, n, m, None, 0, 1, 0, B, S, W, None, ws_bytes, st) == BAD_ARG
    assert call(v, ld, n, m, None, 0, 1, 0, B, S, W, WS, ws_bytes - 1, st) == BAD_ARG       # workspace too small
    assert call(v, ld, n, m, None, 0, 1, 0, B, S, W, ctypes.c_void_p(ws.view.data_ptr() + 8), ws_bytes, st) == BAD_ARG  # misaligned
    assert call(v, ld, n, m, None, 0, 1, 0, 0, S, W, WS, ws_bytes, st) == OK                # no resamples: nothing to do
    assert L.ebn_launch_count() == before
    torch.cuda.synchronize()
    sums.untouched("sums"), wsum.untouched("weight_sums"), ws.untouched("workspace")
    # n_items == 0 is a legal call of the ABI (the host layer raises earlier): all sums are zero
    assert call(None, 0, 0, m, None, 0, 1, 0, B, S, W, WS, ws_bytes, st) == OK
    torch.cuda.synchronize()
    sums.check("sums"), wsum.check("weight_sums")
    assert not sums.view.any() and not wsum.view.any()


def test_bootstrap_evaluator_through_the_classes(hip):
    from ebrec.evaluation import AucScore, DeviceMetricEvaluator, MrrScore, NdcgScore, RaggedLists, bootstrap_evaluator

    rng = np.random.default_rng(11)
    n_lists, B = 2000, 300
    lengths = rng.integers(2, 40, n_lists)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    scores = rng.random(offsets[-1])
    labels = np.zeros(offsets[-1], np.int64)
    labels[offsets[:-1] + rng.integers(0, lengths)] = 1  # one click per impression; every list has both classes
    users = rng.integers(0, 400, n_lists)
    ev = DeviceMetricEvaluator(RaggedLists(labels, offsets), RaggedLists(scores, offsets), [AucScore(), MrrScore(), NdcgScore(k=5)])
    ev.evaluate(per_impression=True)
    assert ev.on_device and len(ev.per_impression) == 3
    dev_res = bootstrap_evaluator(ev, n_resamples=B, seed=5, clusters=users)
    host_res = bootstrap_evaluator(ev, n_resamples=B, seed=5, clusters=users, device=None)
    codes = np.unique(users, return_inverse=True)[1].astype(np.uint32)
    w = bs.poisson_weights(codes, 5, 0, B).astype(np.float64)
    for name, x in ev.per_impression.items():
        bound = n_lists * 2.0 ** -52 * (w @ np.abs(x))  # on the sums; a replicate is sum / weight, each side one more rounding
        tol = bound / w.sum(1) + 2.0 ** -52 * np.abs(host_res.replicates[name])
        assert dev_res.n_empty[name] == host_res.n_empty[name] == 0
        assert np.all(np.abs(dev_res.replicates[name] - host_res.replicates[name]) <= tol), name
        assert dev_res.estimate[name] == host_res.estimate[name] == pytest.approx(ev.evaluations[name], rel=1e-12)
        lo, hi = dev_res.ci(0.95)[name]
        assert lo < ev.evaluations[name] < hi, name
        assert 0.0 < dev_res.std_error[name] < 0.05


def test_ebnerd_nrms_driver_prints_intervals_with_bootstrap_flag(hip, tmp_path, capsys):
    """--device_metrics --bootstrap N: one line per validation metric, its 95 % interval around the metric the driver returns"""
    import re
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    sys.path.insert(0, str(root / "tools"))
    sys.path.insert(0, str(root / "examples" / "reproducibility_scripts"))
    import ebnerd_nrms
    from make_synthetic_ebnerd import make

    data = make(tmp_path / "data", split="ebnerd_demo", n_impressions=300, n_users=40, n_articles=200, seed=1)
    _, metrics = ebnerd_nrms.main(["--data_path", str(data), "--datasplit", "ebnerd_demo", "--epochs", "1", "--bs_train", "32",
                                   "--n_chunks_test", "1", "--tokenizer", "hash", "--vocab_size", "500", "--word_emb_dim", "64",
                                   "--dump_dir", str(tmp_path / "out"), "--device_metrics", "--bootstrap", "200"])
    out = capsys.readouterr().out
    lines = re.findall(r"^\s+(\S+): (\S+)\s+95% CI \[(\S+), (\S+)\]\s+\(Poisson bootstrap over users, 200 resamples\)$", out, flags=re.M)
    assert {name for name, *_ in lines} == set(metrics) == {"auc", "mrr", "ndcg@5", "ndcg@10"}
    for name, est, lo, hi in lines:
        assert float(est) == pytest.approx(metrics[name], abs=1e-6) and float(lo) < metrics[name] < float(hi), name
