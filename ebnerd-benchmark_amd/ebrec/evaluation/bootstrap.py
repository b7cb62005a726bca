"""Bootstrap confidence intervals and paired tests for the evaluation metrics: every number ``DeviceMetricEvaluator`` and
``rank_metrics`` report is a mean over impressions (or pairs); this module says how far such a mean, or the difference of two of
them, can be trusted.

    ev = DeviceMetricEvaluator(labels, scores, metrics).evaluate(per_impression=True)
    res = bootstrap_evaluator(ev, n_resamples=2000, clusters=user_ids)
    res.estimate["auc"], res.std_error["auc"], res.ci(0.95)["auc"]
    paired_bootstrap({"auc": auc_nrms}, {"auc": auc_lstur}, clusters=user_ids).p_value["auc"]

A POISSON bootstrap: resample b gives item i an integer weight w(i, b) ~ Poisson(1) instead of drawing n indices, so a resample
is a weighted sum -- no gather, the values are streamed once, and disjoint shards of the items combine by ADDITION.  The weights
come from a counter-based stream (all arithmetic in uint32, ``lowbias32`` the mixer of the dropout stream):

    k   = lowbias32(seed ^ 0x9E3779B9)
    a_i = lowbias32(key_i ^ k)                      key_i = first_key + i, or the item's cluster code
    r_b = lowbias32((b * 0x9E3779B9) ^ ~k)
    u   = lowbias32(a_i + r_b)
    w   = #{ j in 0..11 : u >= THRESHOLDS[j] }      THRESHOLDS[j] = floor(2^32 P(W <= j)), W ~ Poisson(1); so w <= 12

The weight is a function of (seed, key, b) alone.  Items that share a key -- the impressions of one user -- share their weight in
every resample: that is the cluster bootstrap, which EB-NeRD needs because one user contributes many impressions.

Two paths, as in rerank.py.  With a visible GPU the sums come from ``ebn_poisson_bootstrap_f64`` (csrc/ebn_bootstrap.hip: lanes own
resamples, tiles of items go through LDS, partial sums are added in a fixed order); with ``device=None`` or without a GPU they come
from the float64 numpy twin of the same stream in this module, blocked over resamples.  The weights of the two paths are equal bit
for bit, the sums equal within the rounding of their summation orders.  torch is imported only on the device path.

Shards: ``poisson_bootstrap_sums`` of two disjoint item sets, computed with the same seed and GLOBAL keys (``first_key`` = the
shard's first row number, or ``keys`` = cluster codes from one dictionary), add up to the sums and weights of their union."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .device_metrics import _is_tensor, device_available

# EBN_BS_* of include/ebnerd_hip.h
MAX_COLS, TILE, RESAMPLES, MAX_WEIGHT = 16, 256, 512, 12
THRESHOLDS = np.array([1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463,
                       4294966817, 4294967252, 4294967292], dtype=np.uint32)
GOLDEN = 0x9E3779B9
_TWIN_BLOCK = 1 << 22  # (item, resample) pairs the numpy twin draws at a time


# ---- the weight stream ----------------------------------------------------------------------------------------------------------
def lowbias32(x) -> np.ndarray:
    """``ebn_lowbias32`` of csrc/ebn_common.h on a uint32 array (wrapping arithmetic)."""
    x = np.array(x, dtype=np.uint32, ndmin=1)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _stream_key(seed: int) -> np.uint32:
    return lowbias32((int(seed) & 0xFFFFFFFF) ^ GOLDEN)[0]


def item_hashes(keys, seed: int) -> np.ndarray:
    """a_i of the stream for uint32 keys."""
    return lowbias32(np.asarray(keys, dtype=np.uint32) ^ _stream_key(seed))


def resample_hashes(first_resample: int, n_resamples: int, seed: int) -> np.ndarray:
    """r_b of the stream for b = first_resample .. first_resample + n_resamples - 1."""
    b = (np.arange(first_resample, first_resample + n_resamples, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return lowbias32((b * np.uint32(GOLDEN)) ^ ~_stream_key(seed))


def poisson_weights(keys, seed: int = 0, first_resample: int = 0, n_resamples: int = 1) -> np.ndarray:
    """The weights of the stream as a [n_resamples, n_items] uint8 array: w[b, i] for item keys ``keys`` (uint32)."""
    a, r = item_hashes(keys, seed), resample_hashes(first_resample, n_resamples, seed)
    u = lowbias32(a[None, :] + r[:, None])
    return np.searchsorted(THRESHOLDS, u.reshape(-1), side="right").astype(np.uint8).reshape(u.shape)


def _check_resamples(first_resample: int, n_resamples: int):
    if n_resamples < 1:
        raise ValueError(f"n_resamples must be at least 1, got {n_resamples}")
    if first_resample < 0 or first_resample + n_resamples > 2 ** 32:
        raise ValueError("resample numbers must lie in [0, 2^32)")


def _twin_sums(values: np.ndarray, keys: np.ndarray, seed: int, first_resample: int, n_resamples: int):
    """float64 numpy twin of ebn_poisson_bootstrap_f64: values [m, n], keys [n] uint32 -> (sums [B, m], weights [B] int64)."""
    m, n = values.shape
    a = item_hashes(keys, seed)
    sums, weights = np.empty((n_resamples, m)), np.empty(n_resamples, np.int64)
    step = max(1, _TWIN_BLOCK // max(n, 1))
    vt = np.ascontiguousarray(values.T)
    for b0 in range(0, n_resamples, step):
        nb = min(step, n_resamples - b0)
        r = resample_hashes(first_resample + b0, nb, seed)
        u = lowbias32(a[None, :] + r[:, None])
        w = np.searchsorted(THRESHOLDS, u.reshape(-1), side="right").reshape(nb, n)
        weights[b0:b0 + nb] = w.sum(1)
        sums[b0:b0 + nb] = w.astype(np.float64) @ vt
    return sums, weights


# ---- the device call --------------------------------------------------------------------------------------------------------------
def bootstrap_call(values, keys, first_key: int, seed: int, first_resample: int, n_resamples: int, n_items: int | None = None):
    """One ebn_poisson_bootstrap_f64 call on device tensors: values [m, ld] float64 with unit stride along the items (m <= 16; a row
    stride of its own is passed as ld), keys [n] int32 / uint32 bit patterns or None -> (sums [B, m] float64, weights [B] int64)
    device tensors."""
    import torch

    from ebrec import _hip

    m, ld = values.shape[0], values.stride(0) if values.shape[0] > 1 else max(values.shape[1], 1)
    n = values.shape[1] if n_items is None else n_items
    dev = values.device
    sums = torch.empty((n_resamples, m), dtype=torch.float64, device=dev)
    weights = torch.empty(n_resamples, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ws_bytes = int(_hip.lib().ebn_poisson_bootstrap_workspace_bytes(n, n_resamples, m))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        _hip.call("ebn_poisson_bootstrap_f64", _hip.ptr(values), ld, n, m, _hip.ptr(keys), int(first_key) & 0xFFFFFFFF,
                  int(seed) & 0xFFFFFFFF, first_resample, n_resamples, _hip.ptr(sums), _hip.ptr(weights), _hip.ptr(ws), ws.numel(),
                  _hip.stream_handle())
    return sums, weights


def _item_keys(n: int, clusters, keys, first_key: int):
    """uint32 keys of the items, or None for first_key + i"""
    if clusters is not None and keys is not None:
        raise ValueError("give either `clusters` (any ids, made dense here) or `keys` (uint32 codes used as they are), not both")
    if clusters is not None:
        ids = clusters.detach().cpu().numpy() if _is_tensor(clusters) else np.asarray(clusters)
        if ids.shape != (n,):
            raise ValueError(f"clusters must hold one id per item: {ids.shape} against ({n},)")
        return np.unique(ids, return_inverse=True)[1].reshape(-1).astype(np.uint32)
    if keys is not None:
        k = keys.detach().cpu().numpy() if _is_tensor(keys) else np.asarray(keys)
        if k.shape != (n,):
            raise ValueError(f"keys must hold one code per item: {k.shape} against ({n},)")
        return k.astype(np.uint32)
    return None


def _column_name(names, c: int) -> str:
    return f"column {c}" if names is None else f"column {names[c]!r}"


def poisson_bootstrap_sums(values, n_resamples: int = 2000, seed: int = 0, clusters=None, device="cuda", *, keys=None,
                           first_key: int = 0, first_resample: int = 0, names=None):
    """Poisson-bootstrap sums of ``values`` ([m, n] or [n]; numpy array or torch tensor, a float64 device tensor is used in place)
    -> (sums [B, m] float64 = sum_i w(i, b) values[c, i], weights [B] int64 = sum_i w(i, b)) as numpy arrays.

    ``clusters``: any array of n ids (made dense with np.unique); items with equal ids share their weights.  ``keys`` instead: uint32
    codes used as they are, ``first_key``: the key of item 0 when there are neither -- both for shards, whose keys must be global.
    ``first_resample`` numbers the first row, so that a caller may block over resamples.  ``device=None`` or no visible GPU: the
    numpy twin.  Non-finite values raise ValueError naming the column (``names`` for the message), and so does n == 0."""
    tensor = _is_tensor(values)
    v = values if tensor else np.asarray(values)
    if v.ndim == 1:
        v = v.reshape(1, -1)
    if v.ndim != 2:
        raise ValueError(f"values must be [m, n] or [n], got {tuple(v.shape)}")
    m, n = int(v.shape[0]), int(v.shape[1])
    if n == 0 or m == 0:
        raise ValueError("nothing to resample: values holds no items")
    n_resamples, first_resample = int(n_resamples), int(first_resample)
    _check_resamples(first_resample, n_resamples)
    item_keys = _item_keys(n, clusters, keys, first_key)
    if not device_available(device):
        host = v.detach().cpu().numpy() if tensor else v
        host = np.ascontiguousarray(host, dtype=np.float64)
        bad = np.flatnonzero(~np.isfinite(host).all(axis=1))
        if bad.size:
            raise ValueError(f"{_column_name(names, int(bad[0]))} holds a non-finite value: a bootstrap mean of it is undefined")
        k = item_keys if item_keys is not None else (np.arange(n, dtype=np.uint64) + np.uint64(int(first_key) & 0xFFFFFFFF)).astype(np.uint32)
        return _twin_sums(host, k, seed, first_resample, n_resamples)
    import torch

    if tensor:
        dv = v.to(device=device, dtype=torch.float64)
        if dv.stride(1) != 1 or (m > 1 and dv.stride(0) < n):
            dv = dv.contiguous()
    else:
        dv = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(device)
    bad = torch.nonzero(~torch.isfinite(dv).all(dim=1)).reshape(-1)
    if bad.numel():
        raise ValueError(f"{_column_name(names, int(bad[0]))} holds a non-finite value: a bootstrap mean of it is undefined")
    dk = None if item_keys is None else torch.from_numpy(item_keys.view(np.int32)).to(dv.device)
    sums, weights = np.empty((n_resamples, m)), None
    for c0 in range(0, m, MAX_COLS):  # a column's sums do not depend on the columns that share its call
        s, w = bootstrap_call(dv[c0:c0 + MAX_COLS], dk, first_key, seed, first_resample, n_resamples, n)
        sums[:, c0:c0 + MAX_COLS] = s.cpu().numpy()
        weights = w.cpu().numpy() if weights is None else weights
    return sums, weights


# ---- means, intervals, paired differences ----------------------------------------------------------------------------------------
def _check_level(level) -> float:
    level = float(level)
    if not 0.0 < level < 1.0:  # NaN fails both comparisons
        raise ValueError(f"level must lie in (0, 1), got {level}")
    return level


def _interval(replicates: np.ndarray, estimate: float, level: float, method: str):
    valid = replicates[~np.isnan(replicates)]
    if valid.size == 0:
        return float("nan"), float("nan")
    lo, hi = np.quantile(valid, [(1.0 - level) / 2.0, (1.0 + level) / 2.0])
    if method == "percentile":
        return float(lo), float(hi)
    if method == "basic":
        return float(2.0 * estimate - hi), float(2.0 * estimate - lo)
    raise ValueError(f"method must be 'percentile' or 'basic', got {method!r}")


def _std_error(replicates: np.ndarray) -> float:
    valid = replicates[~np.isnan(replicates)]
    return float(np.std(valid, ddof=1)) if valid.size > 1 else float("nan")


@dataclass
class BootstrapResult:
    """``estimate`` {name: the mean on the data}, ``replicates`` {name: [B] float64, NaN where the resample's denominator was 0},
    ``std_error`` {name: standard deviation of the valid replicates}, ``n_empty`` {name: replicates left out}, ``ci()``."""
    estimate: dict
    replicates: dict
    n_empty: dict
    n_items: int
    n_resamples: int
    std_error: dict = field(default_factory=dict)

    def __post_init__(self):
        self.std_error = {k: _std_error(r) for k, r in self.replicates.items()}

    def ci(self, level: float = 0.95, method: str = "percentile") -> dict:
        """{name: (low, high)}.  "percentile": the (1 - level) / 2 and (1 + level) / 2 quantiles of the valid replicates; "basic":
        those quantiles reflected about the estimate, (2 est - q_high, 2 est - q_low)."""
        level = _check_level(level)
        return {k: _interval(r, self.estimate[k], level, method) for k, r in self.replicates.items()}


@dataclass
class PairedBootstrapResult(BootstrapResult):
    """A BootstrapResult of the differences a - b, with ``p_value`` {name: two-sided p of "no difference"}:
    p = (1 + #{b : |d_b - d| >= |d|}) / (B_valid + 1)."""
    p_value: dict = field(default_factory=dict)

    def __post_init__(self):
        super().__post_init__()
        self.p_value = {}
        for k, r in self.replicates.items():
            valid, d = r[~np.isnan(r)], self.estimate[k]
            self.p_value[k] = float((1 + np.count_nonzero(np.abs(valid - d) >= abs(d))) / (valid.size + 1)) if not np.isnan(d) else float("nan")


def _as_column(x, n=None) -> np.ndarray:
    a = x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)
    a = a.reshape(-1).astype(np.float64)
    if n is not None and a.size != n:
        raise ValueError(f"every column must hold one value per item: {a.size} against {n}")
    return a


def _denominator_of(names, denominators) -> dict:
    if denominators is None:
        return {}
    if isinstance(denominators, str):
        return {k: denominators for k in names if k != denominators}
    return dict(denominators)


def _ratio_replicates(columns: dict, denom_of: dict, **kw):
    """{key: [n]} -> ({key: estimate}, {key: [B] replicates}, {key: n_empty}, n, B) for every key that is nobody's denominator"""
    keys = list(columns)
    if not keys:
        raise ValueError("no columns to resample")
    for k, d in denom_of.items():
        if k not in columns or d not in columns:
            raise ValueError(f"denominator {d!r} of {k!r}: both must be columns")
    cols = [_as_column(columns[keys[0]])]
    cols += [_as_column(columns[k], cols[0].size) for k in keys[1:]]
    if cols[0].size == 0:
        raise ValueError("nothing to resample: the columns hold no items")
    values = np.stack(cols)
    sums, weights = poisson_bootstrap_sums(values, names=keys, **kw)
    at = {k: j for j, k in enumerate(keys)}
    used = set(denom_of.values())
    est, rep, empty = {}, {}, {}
    for k in keys:
        if k in used and k not in denom_of:
            continue
        num = sums[:, at[k]]
        if k in denom_of:
            den, total = sums[:, at[denom_of[k]]], float(np.sum(cols[at[denom_of[k]]]))
        else:
            den, total = weights.astype(np.float64), float(cols[0].size)
        zero = den == 0
        rep[k] = np.where(zero, np.nan, num / np.where(zero, 1.0, den))
        empty[k] = int(zero.sum())
        est[k] = float(np.sum(cols[at[k]]) / total) if total != 0 else float("nan")
    return est, rep, empty, cols[0].size, sums.shape[0]


def bootstrap_means(columns: dict, denominators=None, n_resamples: int = 2000, seed: int = 0, clusters=None, device="cuda", **kw):
    """Bootstrap of the means of ``columns`` {name: [n] values}.  A replicate is S_b / W_b (weighted sum over the resample's weight
    sum) or, for a column with a denominator, S_b / D_b with D_b the denominator column's weighted sum -- a mean over a subset, such
    as the ranked pairs only.  ``denominators``: {name: denominator column's name}, or one name for every other column; a column that
    only serves as a denominator is not reported.  Replicates with a zero denominator are NaN, counted in ``n_empty`` and left out of
    the quantiles.  ``clusters`` / ``device`` / ``keys`` / ``first_key`` as in ``poisson_bootstrap_sums``."""
    est, rep, empty, n, B = _ratio_replicates(dict(columns), _denominator_of(list(columns), denominators), n_resamples=n_resamples,
                                              seed=seed, clusters=clusters, device=device, **kw)
    return BootstrapResult(est, rep, empty, n, B)


def paired_bootstrap(columns_a: dict, columns_b: dict, denominators=None, n_resamples: int = 2000, seed: int = 0, clusters=None,
                     device="cuda", **kw):
    """Paired bootstrap of mean(a) - mean(b) for every name of ``columns_a`` (``columns_b`` must hold the same names over the same
    items).  Both sides sit in one call and so take the SAME weights: what the two systems share item by item cancels.  Returns
    the difference's estimate, replicates, std_error, ci() and two-sided ``p_value``."""
    if list(columns_a) != list(columns_b):
        raise ValueError("both sides must hold the same column names in the same order")
    names = list(columns_a)
    merged = {("a", k): v for k, v in columns_a.items()}
    merged.update({("b", k): v for k, v in columns_b.items()})
    denom = _denominator_of(names, denominators)
    denom_of = {(side, k): (side, d) for k, d in denom.items() for side in ("a", "b")}
    est, rep, _, n, B = _ratio_replicates(merged, denom_of, n_resamples=n_resamples, seed=seed, clusters=clusters, device=device, **kw)
    names = [k for k in names if ("a", k) in est]
    d_est = {k: est[("a", k)] - est[("b", k)] for k in names}
    d_rep = {k: rep[("a", k)] - rep[("b", k)] for k in names}  # NaN on either side stays NaN
    d_empty = {k: int(np.isnan(d_rep[k]).sum()) for k in names}
    return PairedBootstrapResult(d_est, d_rep, d_empty, n, B)


def bootstrap_evaluator(evaluator, n_resamples: int = 2000, seed: int = 0, clusters=None, device="cuda", **kw):
    """Bootstrap of a DeviceMetricEvaluator's slot metrics from its ``per_impression`` values (``evaluate(per_impression=True)``
    first; raises when there are none).  ``clusters``: one id per impression, e.g. its user."""
    per = getattr(evaluator, "per_impression", None)
    if not per:
        raise ValueError("the evaluator holds no per-impression values: call evaluate(per_impression=True) on the device path first")
    return bootstrap_means(per, n_resamples=n_resamples, seed=seed, clusters=clusters, device=device, **kw)
