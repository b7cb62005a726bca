"""Host side of the Poisson bootstrap (ebrec/evaluation/bootstrap.py): the weight stream's constants and statistics, the cluster
bootstrap, means / intervals / paired differences, the error cases and the shard-addition rule -- all on the numpy twin
(``device=None``), no GPU."""
import re
from fractions import Fraction
from math import factorial
from pathlib import Path

import numpy as np
import pytest

from ebrec import _hip
from ebrec.evaluation import bootstrap as bs
from ebrec.evaluation import (
    bootstrap_evaluator, bootstrap_means, bootstrap_rank_metrics, paired_bootstrap, poisson_bootstrap_sums, rank_metrics, rank_values,
)

ROOT = Path(__file__).resolve().parents[1]
PMF = np.array([float(Fraction(1, factorial(j))) for j in range(13)]) * float(np.exp(-1.0))


def _exact_thresholds():
    """floor(2^32 * P(W <= j)) for W ~ Poisson(1): the partial sums of 1 / j! exactly, e^-1 bracketed by its alternating series."""
    terms = 40  # 1 / 40! < 2^-150: the bracket is far narrower than the distance of any product to an integer
    lo = sum(Fraction((-1) ** k, factorial(k)) for k in range(terms))
    hi = lo + Fraction(1, factorial(terms))
    lo, hi = min(lo, hi), max(lo, hi)
    out = []
    for j in range(12):
        cdf = sum(Fraction(1, factorial(i)) for i in range(j + 1))
        a, b = (2 ** 32 * cdf * lo).__floor__(), (2 ** 32 * cdf * hi).__floor__()
        assert a == b, "the bracket of e^-1 must decide the floor"
        out.append(a)
    return out


def _header_defines():
    text = re.sub(r"/\*.*?\*/", "", _hip.header_path().read_text(), flags=re.S)  # comments stripped, as the binding's parser does
    return text


def test_threshold_literals_are_the_exact_poisson_cdf():
    exact = _exact_thresholds()
    assert exact == [1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463,
                     4294966817, 4294967252, 4294967292]
    assert bs.THRESHOLDS.dtype == np.uint32 and bs.THRESHOLDS.tolist() == exact
    text = _header_defines()
    macro = re.search(r"#define\s+EBN_BS_THRESHOLDS\b(.*?)\}", text.replace("\\\n", " "), flags=re.S).group(1)
    assert [int(x) for x in re.findall(r"(\d+)u", macro)] == exact
    ints = {k: int(v) for k, v in re.findall(r"#define\s+(EBN_BS_[A-Z_]+)\s+(\d+)\b", text)}
    assert (ints["EBN_BS_MAX_COLS"], ints["EBN_BS_TILE"], ints["EBN_BS_RESAMPLES"], ints["EBN_BS_MAX_WEIGHT"]) == \
        (bs.MAX_COLS, bs.TILE, bs.RESAMPLES, bs.MAX_WEIGHT) == (16, 256, 512, 12)
    # the kernel holds no literals of its own: its table IS the header's macro, its mixer the library's
    kernel = (ROOT / "ebnerd-benchmark_amd" / "csrc" / "ebn_bootstrap.hip").read_text()
    assert re.search(r"kBsC\[EBN_BS_MAX_WEIGHT\]\s*=\s*EBN_BS_THRESHOLDS;", kernel) and "ebn_lowbias32" in kernel
    assert not re.findall(r"\b\d{9,10}u?\b", kernel), "a threshold literal outside the header"
    assert _hip.declared_functions().keys() >= {"ebn_poisson_bootstrap_f64", "ebn_poisson_bootstrap_workspace_bytes"}


def test_lowbias32_matches_the_dropout_stream_mixer():
    from oracle import nrms_numpy as on

    x = np.array([0, 1, 2, 0x9E3779B9, 0xFFFFFFFF, 123456789], dtype=np.uint32)
    assert bs.lowbias32(x).tolist() == [int(on.lowbias32(np.uint32(v))) for v in x]


@pytest.fixture(scope="module")
def stream():
    n, B = 4096, 2048
    return n, B, bs.poisson_weights(np.arange(n, dtype=np.uint32), seed=7, n_resamples=B)


def _z_corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()) * np.sqrt(a.size))


def test_stream_statistics(stream):
    n, B, w = stream
    N = n * B
    assert w.shape == (B, n) and w.dtype == np.uint8 and int(w.max()) <= 12
    for j in range(7):
        p = PMF[j]
        assert abs(float((w == j).mean()) - p) <= 5.0 * np.sqrt(p * (1.0 - p) / N), j
    wf = w.astype(np.float64)
    assert abs(wf.mean() - 1.0) <= 5.0 / np.sqrt(N)
    assert abs(_z_corr(wf[:-1].ravel(), wf[1:].ravel())) <= 5.0  # consecutive resamples
    assert abs(_z_corr(wf[:, :-1].ravel(), wf[:, 1:].ravel())) <= 5.0  # consecutive items
    c = wf - wf.mean(1, keepdims=True)
    c /= np.sqrt((c * c).sum(1, keepdims=True))
    corr = c @ c.T
    np.fill_diagonal(corr, 0.0)
    assert float(np.abs(corr).max()) * np.sqrt(n) <= 6.5
    x = np.random.default_rng(0).random(n) ** 3
    means = (wf @ x) / wf.sum(1)
    ratio = float(means.std(ddof=1) / (x.std(ddof=1) / np.sqrt(n)))
    assert abs(ratio - 1.0) <= 5.0 / np.sqrt(2 * B)


def test_two_seeds_give_independent_weights(stream):
    n, B, w = stream
    other = bs.poisson_weights(np.arange(n, dtype=np.uint32), seed=8, n_resamples=B)
    p = 1.0 - float((PMF ** 2).sum())
    assert abs(p - 0.6915) < 1e-4
    assert abs(float((w != other).mean()) - p) <= 5.0 * np.sqrt(p * (1.0 - p) / (n * B))


def test_blocks_of_resamples_are_rows_of_one_stream(stream):
    n, B, w = stream
    part = bs.poisson_weights(np.arange(n, dtype=np.uint32), seed=7, first_resample=1000, n_resamples=5)
    assert np.array_equal(part, w[1000:1005])


def test_equal_cluster_keys_share_their_weights():
    users = np.repeat(np.arange(100), 5)
    codes = np.unique(users, return_inverse=True)[1].astype(np.uint32)
    w = bs.poisson_weights(codes, seed=3, n_resamples=64).reshape(64, 100, 5)
    assert (w == w[:, :, :1]).all()
    rng = np.random.default_rng(1)
    x = np.repeat(rng.normal(size=100), 5)  # a user's items are equal: 100 independent values, not 500
    rows = bootstrap_means({"x": x}, n_resamples=1000, seed=3, device=None)
    by_user = bootstrap_means({"x": x}, n_resamples=1000, seed=3, clusters=users + 1000, device=None)
    lo, hi = rows.ci()["x"]
    ulo, uhi = by_user.ci()["x"]
    assert uhi - ulo > 1.8 * (hi - lo)  # sqrt(5) = 2.24 in expectation
    assert by_user.std_error["x"] == pytest.approx(x.std() / np.sqrt(100), rel=0.15)


def test_bootstrap_rank_metrics_estimates_are_rank_metrics():
    rng = np.random.default_rng(2)
    ranks = rng.integers(0, 40, 500)
    ranks[rng.random(500) < 0.2] = 0
    counts = rng.integers(40, 60, 500)
    want = rank_metrics(ranks, ks=(5, 10), counts=counts)
    cols = rank_values(ranks, ks=(5, 10), counts=counts)
    assert set(cols) == set(want) | {"ranked"}
    res = bootstrap_means(cols, {k: "ranked" for k in cols if k not in ("ranked", "unranked")}, n_resamples=200, device=None)
    assert set(res.estimate) == set(want)
    for k, v in want.items():
        assert res.estimate[k] == pytest.approx(v, rel=1e-13), k
        lo, hi = res.ci()[k]
        assert lo <= v <= hi, k
    res2 = bootstrap_rank_metrics(ranks, ks=(5, 10), counts=counts, n_resamples=200, device=None)
    assert res2.estimate == res.estimate and all(np.array_equal(res2.replicates[k], res.replicates[k]) for k in want)
    with pytest.raises(ValueError):
        rank_values([1, -1])


def test_paired_bootstrap_of_a_column_with_itself():
    x = np.random.default_rng(3).random(300)
    res = paired_bootstrap({"m": x}, {"m": x}, n_resamples=300, device=None)
    assert res.estimate["m"] == 0.0 and np.all(res.replicates["m"] == 0.0) and res.p_value["m"] == 1.0
    assert res.ci()["m"] == (0.0, 0.0)
    # a shift far beyond the noise: every replicate of the difference stays near it, p is the smallest it can be
    far = paired_bootstrap({"m": x + 1.0}, {"m": x}, n_resamples=300, device=None)
    assert far.estimate["m"] == pytest.approx(1.0) and far.p_value["m"] == pytest.approx(1.0 / 301.0)
    with pytest.raises(ValueError):
        paired_bootstrap({"m": x}, {"other": x}, device=None)


def test_known_answer_quantiles():
    rep = np.arange(101, dtype=np.float64)
    rep_nan = np.concatenate([rep, [np.nan, np.nan]])
    res = bs.BootstrapResult({"v": 40.0}, {"v": rep_nan}, {"v": 2}, 10, 103)
    assert res.ci(0.9)["v"] == pytest.approx((5.0, 95.0))
    assert res.ci(0.9, "basic")["v"] == pytest.approx((2 * 40.0 - 95.0, 2 * 40.0 - 5.0))
    assert res.ci(0.5, "percentile")["v"] == pytest.approx((25.0, 75.0))
    assert res.std_error["v"] == pytest.approx(rep.std(ddof=1))
    for level in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            res.ci(level)
    with pytest.raises(ValueError):
        res.ci(0.9, "bca")


def test_error_cases_and_empty_resamples():
    with pytest.raises(ValueError):
        poisson_bootstrap_sums(np.zeros((2, 0)), device=None)
    with pytest.raises(ValueError):
        bootstrap_means({"a": np.zeros(0)}, device=None)
    with pytest.raises(ValueError, match="'b'"):
        bootstrap_means({"a": np.ones(4), "b": np.array([1.0, np.inf, 0.0, 0.0])}, device=None)
    with pytest.raises(ValueError, match="column 1"):
        poisson_bootstrap_sums(np.array([[1.0, 2.0], [np.nan, 0.0]]), device=None)
    with pytest.raises(ValueError):
        poisson_bootstrap_sums(np.ones(3), n_resamples=0, device=None)
    with pytest.raises(ValueError):
        poisson_bootstrap_sums(np.ones(3), clusters=[1, 2], device=None)
    with pytest.raises(ValueError):
        bootstrap_means({"a": np.ones(3), "b": np.ones(4)}, device=None)

    class NoValues:
        per_impression = {}

    with pytest.raises(ValueError):
        bootstrap_evaluator(NoValues(), device=None)
    # n = 1: the one item's weight is 0 with probability e^-1 per resample; those replicates are NaN, counted, left out
    B = 4000
    one = bootstrap_means({"a": np.array([2.5])}, n_resamples=B, seed=11, device=None)
    w = bs.poisson_weights(np.zeros(1, np.uint32), seed=11, n_resamples=B)[:, 0]
    assert one.n_empty["a"] == int((w == 0).sum()) == int(np.isnan(one.replicates["a"]).sum())
    p = float(np.exp(-1.0))
    assert abs(one.n_empty["a"] / B - p) <= 5.0 * np.sqrt(p * (1.0 - p) / B)
    assert np.all(one.replicates["a"][w > 0] == 2.5) and one.ci()["a"] == (2.5, 2.5)


def test_shards_add_on_the_host_path():
    rng = np.random.default_rng(5)
    n, cut, B = 1000, 377, 50
    x = rng.normal(size=(3, n))
    whole, w_whole = poisson_bootstrap_sums(x, n_resamples=B, seed=9, device=None)
    s0, w0 = poisson_bootstrap_sums(x[:, :cut], n_resamples=B, seed=9, device=None)
    s1, w1 = poisson_bootstrap_sums(x[:, cut:], n_resamples=B, seed=9, first_key=cut, device=None)
    assert np.array_equal(w0 + w1, w_whole)
    np.testing.assert_allclose(s0 + s1, whole, rtol=0, atol=1e-9)
    # and with cluster codes from one dictionary
    codes = rng.integers(0, 50, n).astype(np.uint32)
    whole, w_whole = poisson_bootstrap_sums(x, n_resamples=B, seed=9, keys=codes, device=None)
    s0, w0 = poisson_bootstrap_sums(x[:, :cut], n_resamples=B, seed=9, keys=codes[:cut], device=None)
    s1, w1 = poisson_bootstrap_sums(x[:, cut:], n_resamples=B, seed=9, keys=codes[cut:], device=None)
    assert np.array_equal(w0 + w1, w_whole)
    np.testing.assert_allclose(s0 + s1, whole, rtol=0, atol=1e-9)
    # blocks of resamples are rows of the whole
    s_blk, w_blk = poisson_bootstrap_sums(x, n_resamples=7, seed=9, keys=codes, first_resample=20, device=None)
    assert np.array_equal(w_blk, w_whole[20:27])
    np.testing.assert_allclose(s_blk, whole[20:27], rtol=0, atol=1e-9)


def test_size_query_bounds_its_extents():
    L = _hip.lib()
    q = L.ebn_poisson_bootstrap_workspace_bytes
    assert q(1, 1, 1) == 16 and q(0, 5, 2) == 5 * 3 * 8
    assert q(256 * 512, 10, 4) == 512 * 10 * 5 * 8 and q(256 * 512 + 1, 10, 4) == 257 * 10 * 5 * 8  # two tiles a range: 257 ranges
    assert q(1 << 40, 10, 4) == 0 and q(10, 1 << 31, 4) == 0 and q(10, 10, 17) == 0 and q(10, 10, 0) == 0 and q(-1, 1, 1) == 0
    assert 0 < q((1 << 31) - 257, (1 << 31) - 1, 16) < (1 << 63) - 1
