"""The per-impression metrics of metrics_protocols.py on the GPU: `RaggedLists` (flat values + offsets instead of lists of
lists) and `DeviceMetricEvaluator`, a MetricEvaluator whose wrapper metrics -- auc, mrr, ndcg@k, logloss, rmse, accuracy, f1 --
run as ONE launch of ebn_rank_metrics (csrc/ebn_rankmetrics.hip) over all impressions.

The kernel ranks by counting and leaves to the host exactly the lists it cannot decide: those in which two equal scores carry
different labels (mrr / ndcg then depend on the order the host's unstable argsort gives a tie group) and those with a non-finite
score.  They are recomputed with the host wrappers, list by list, and added to the device sums.  With `device=None`, without a
visible GPU, or with labels outside {0, 1}, the whole call goes to MetricEvaluator.  torch is imported only on the device path."""
from __future__ import annotations

from itertools import chain

import numpy as np

from .metrics_protocols import (
    AccuracyScore, AucScore, F1Score, LogLossScore, MetricEvaluator, MrrScore, NdcgScore, RootMeanSquaredError,
)

# EBN_RM_* of include/ebnerd_hip.h
RM_AUC, RM_MRR, RM_NDCG, RM_LOGLOSS, RM_RMSE, RM_ACCURACY, RM_F1 = range(7)
RM_MAX_SLOTS = 16
FLAG_TIE, FLAG_NONFINITE = 1, 2


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


class RaggedLists:
    """Ragged lists as one flat array plus offsets: list l is ``flat[offsets[l]:offsets[l + 1]]``.

    ``RaggedLists.from_lists(lists)`` flattens lists of lists (or of arrays) in one pass; ``RaggedLists(flat, offsets)`` takes
    flat numpy arrays or torch tensors as they are -- a tensor that already lives on the device is used in place by the device
    evaluator, with no round trip through the host."""

    def __init__(self, flat, offsets):
        self.flat = flat if _is_tensor(flat) else np.asarray(flat)
        off = offsets.detach().cpu().numpy() if _is_tensor(offsets) else np.asarray(offsets)
        self.offsets = np.ascontiguousarray(off, dtype=np.int64)
        n = int(self.flat.shape[0]) if self.flat.ndim == 1 else -1
        if (self.offsets.ndim != 1 or self.offsets.size < 1 or n < 0 or self.offsets[0] != 0 or self.offsets[-1] != n
                or np.any(np.diff(self.offsets) < 0)):
            raise ValueError("RaggedLists needs a 1-D `flat` and non-decreasing offsets from 0 to len(flat)")

    @classmethod
    def from_lists(cls, lists, dtype=None) -> "RaggedLists":
        if isinstance(lists, RaggedLists):
            return lists
        lists = lists if hasattr(lists, "__len__") else list(lists)
        offsets = np.zeros(len(lists) + 1, np.int64)
        np.cumsum(np.fromiter((len(x) for x in lists), np.int64, len(lists)), out=offsets[1:])
        total = int(offsets[-1])
        if total and all(isinstance(x, np.ndarray) for x in lists):
            flat = np.concatenate([x.ravel() for x in lists])
            flat = flat if dtype is None else flat.astype(dtype, copy=False)
        else:
            first = next((x[0] for x in lists if len(x)), 0.0)
            flat = np.fromiter(chain.from_iterable(lists), dtype or (type(first) if isinstance(first, np.generic) else np.float64), total)
            if dtype is None and isinstance(first, (bool, int)) and np.array_equal(flat, np.floor(flat)):
                flat = flat.astype(np.int64)  # lists of Python ints (labels); [0, 0.5] stays float64
        return cls(flat, offsets)

    def __len__(self) -> int:
        return self.offsets.size - 1

    @property
    def lengths(self) -> np.ndarray:
        return np.diff(self.offsets)

    def host_flat(self) -> np.ndarray:
        return self.flat.detach().cpu().numpy() if _is_tensor(self.flat) else self.flat

    def to_lists(self) -> list:
        """Plain Python lists (copies: nothing a metric does to them reaches `flat`)."""
        flat, off = self.host_flat().tolist(), self.offsets.tolist()
        return [flat[a:b] for a, b in zip(off[:-1], off[1:])]

    def row(self, l: int) -> list:
        a, b = int(self.offsets[l]), int(self.offsets[l + 1])
        f = self.flat[a:b]
        return (f.detach().cpu().numpy() if _is_tensor(f) else f).tolist()


def tie_ambiguous_and_nonfinite(labels, scores) -> tuple[bool, bool]:
    """The two flag definitions of ebn_rank_metrics for one list, in numpy: (two equal scores carry different labels, the list
    holds a non-finite score)."""
    y, s = np.asarray(labels).ravel() != 0, np.asarray(scores).ravel()
    eq = s[:, None] == s[None, :]
    return bool(np.any(eq & (y[:, None] != y[None, :]))), bool(not np.all(np.isfinite(s)))


def _slot_of(metric):
    """(kind, param) when the metric is EXACTLY one of the seven wrapper classes with a usable parameter, else None."""
    t = type(metric)
    try:
        if t is AucScore:
            return RM_AUC, 0.0
        if t is MrrScore:
            return RM_MRR, 0.0
        if t is NdcgScore:
            k = metric.k
            return (RM_NDCG, float(k)) if isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 1 <= k < 2 ** 53 else None
        if t is LogLossScore:
            return RM_LOGLOSS, 0.0
        if t is RootMeanSquaredError:
            return RM_RMSE, 0.0
        if t in (AccuracyScore, F1Score):
            thr = metric.threshold
            ok = isinstance(thr, (int, float, np.integer, np.floating)) and not isinstance(thr, bool) and np.isfinite(thr)
            return (RM_ACCURACY if t is AccuracyScore else RM_F1, float(thr)) if ok else None
    except AttributeError:
        return None
    return None


def device_available(device) -> bool:
    if device is None:
        return False
    try:
        import torch
    except ImportError:
        return False
    return bool(torch.cuda.is_available())


def _to_device(flat, dtype, device):
    import torch

    if _is_tensor(flat):
        return flat.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(flat)).to(device=device, dtype=dtype)


def device_scores(flat, device):
    """(tensor, score kind): float32 stays float32, everything else is compared as float64."""
    import torch

    is32 = (flat.dtype == torch.float32) if _is_tensor(flat) else (flat.dtype == np.float32)
    return _to_device(flat, torch.float32 if is32 else torch.float64, device), 0 if is32 else 1


def rank_metrics_call(scores, labels, offsets, slots, form: int = 0, per_list: bool = False):
    """One ebn_rank_metrics launch over device tensors.  Returns (sums [n_slots] float64, flags [n_lists] uint8, counters
    [3] int64, per-list values [n_slots, n_lists] float64 or None) as numpy arrays."""
    import torch

    from ebrec import _hip

    dev, n_lists, n_slots = offsets.device, offsets.numel() - 1, len(slots)
    kind = 0 if scores.dtype == torch.float32 else 1
    kinds = torch.tensor([k for k, _ in slots] or [0], dtype=torch.int32, device=dev)
    params = torch.tensor([p for _, p in slots] or [0.0], dtype=torch.float64, device=dev)
    sums = torch.zeros(max(n_slots, 1), dtype=torch.float64, device=dev)
    flags = torch.zeros(max(n_lists, 1), dtype=torch.uint8, device=dev)
    counters = torch.zeros(3, dtype=torch.int64, device=dev)
    values = torch.empty((n_slots, n_lists), dtype=torch.float64, device=dev) if per_list else None
    with torch.cuda.device(dev):
        ws_bytes = int(_hip.lib().ebn_rank_metrics_workspace_bytes(n_lists))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        _hip.call("ebn_rank_metrics", _hip.ptr(scores), kind, _hip.ptr(labels), scores.numel(), _hip.ptr(offsets), n_lists,
                  _hip.ptr(kinds), _hip.ptr(params), n_slots, form, _hip.ptr(sums), _hip.ptr(flags), _hip.ptr(counters),
                  _hip.ptr(values) if per_list and n_slots and n_lists else None, _hip.ptr(ws), ws.numel(), _hip.stream_handle())
    return (sums.cpu().numpy()[:n_slots], flags.cpu().numpy()[:n_lists], counters.cpu().numpy(),
            values.cpu().numpy() if per_list else None)


def list_ranks_call(scores, offsets, form: int = 0):
    """One ebn_list_ranks launch over device tensors: (ranks [n_items] int32, flags [n_lists] uint8) as numpy arrays."""
    import torch

    from ebrec import _hip

    dev, n_lists = offsets.device, offsets.numel() - 1
    kind = 0 if scores.dtype == torch.float32 else 1
    ranks = torch.zeros(max(scores.numel(), 1), dtype=torch.int32, device=dev)
    flags = torch.zeros(max(n_lists, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("ebn_list_ranks", _hip.ptr(scores), kind, scores.numel(), _hip.ptr(offsets), n_lists, form, _hip.ptr(ranks),
                  _hip.ptr(flags), _hip.stream_handle())
    return ranks.cpu().numpy()[:scores.numel()], flags.cpu().numpy()[:n_lists]


class DeviceMetricEvaluator(MetricEvaluator):
    """MetricEvaluator with the wrapper metrics on the GPU: same constructor, ``evaluate()`` returns the evaluator,
    ``.evaluations`` has the same keys in the same order, it prints the same way and rejects non-callable metrics the same way.

    `labels` / `predictions`: lists of lists, or `RaggedLists` (over numpy arrays or torch tensors; device tensors are used in
    place).  Scores given as float32 are compared as float32, anything else as float64.

    * A metric whose type is exactly AucScore, MrrScore, NdcgScore, LogLossScore, RootMeanSquaredError, AccuracyScore or F1Score
      becomes a slot of one ebn_rank_metrics launch.  Any other callable is called with the nested lists, which are built only then.
    * Lists the kernel flags (equal scores with different labels; a non-finite score) are recomputed with the host wrappers and
      added to the sums; `n_host_fallback` counts the lists that needed it for at least one metric.
    * auc / logloss with a one-class list raise the ValueError the host functions raise.
    * Labels outside {0, 1}, ``device=None`` or no visible GPU: the whole call goes to MetricEvaluator, on list inputs.

    Predictions are never mutated and the result equals MetricEvaluator on LIST inputs.  The host evaluator's side effect on
    ndarray inputs -- AccuracyScore / F1Score binarise the arrays in place, so later metrics see 0 / 1 scores -- is NOT reproduced.

    After ``evaluate()``: `sums` {name: sum over impressions} for the slot metrics and `n_impressions`, so that shards combine by
    addition (mean = sum of sums / sum of counts); with ``evaluate(per_impression=True)`` also `per_impression` {name: values}.
    The bootstrap of those values (evaluation/bootstrap.py, ``bootstrap_evaluator``) combines the same way: the `sums` and `weights`
    ``poisson_bootstrap_sums`` gives two disjoint shards of impressions under one seed and GLOBAL keys (``first_key`` = the shard's
    first impression number, or ``keys`` = user codes from one dictionary) add up to those of all impressions."""

    def __init__(self, labels, predictions, metric_functions, device="cuda"):
        super().__init__(labels, predictions, metric_functions)
        self.device = device
        self.sums, self.per_impression = {}, {}
        self.n_impressions = self.n_host_fallback = 0
        self.on_device = False

    def _host(self, L: RaggedLists, P: RaggedLists):
        host = MetricEvaluator(L.to_lists(), P.to_lists(), self.metric_functions).evaluate()
        self.evaluations, self.on_device = host.evaluations, False
        self.sums, self.per_impression, self.n_impressions, self.n_host_fallback = {}, {}, len(L), len(L)
        return self

    def evaluate(self, per_impression: bool = False, form: int = 0):
        L, P = RaggedLists.from_lists(self.labels), RaggedLists.from_lists(self.predictions)
        if len(L) != len(P) or not np.array_equal(L.offsets, P.offsets):
            raise ValueError("labels and predictions are not lists of the same lengths")
        if not device_available(self.device):
            return self._host(L, P)
        import torch

        lab = L.flat
        binary = bool(((lab == 0) | (lab == 1)).all()) if lab.shape[0] else True
        if not binary:
            return self._host(L, P)
        labels = _to_device(lab, torch.uint8, self.device)
        scores, _ = device_scores(P.flat, self.device)
        offsets = torch.from_numpy(L.offsets).to(labels.device)
        n = len(L)
        slots = [(i, _slot_of(m)) for i, m in enumerate(self.metric_functions)]
        dev_slots = [(i, s) for i, s in slots if s is not None]
        sums = np.zeros(len(dev_slots))
        values = np.empty((len(dev_slots), n)) if per_impression else None
        flags, counters = np.zeros(n, np.uint8), np.zeros(3, np.int64)
        for c0 in range(0, max(len(dev_slots), 1), RM_MAX_SLOTS):
            part = [s for _, s in dev_slots[c0:c0 + RM_MAX_SLOTS]]
            if n == 0 or not part:
                break
            s_, flags, counters, v_ = rank_metrics_call(scores, labels, offsets, part, form, per_impression)
            sums[c0:c0 + len(part)] = s_
            if per_impression:
                values[c0:c0 + len(part)] = v_
        two_class = [i for i, (k, _) in dev_slots if k in (RM_AUC, RM_LOGLOSS)]
        if two_class and counters[0] > 0:
            self._raise_one_class(L, P, self.metric_functions[two_class[0]])
        # the lists the kernel left to the host
        redo_all = np.flatnonzero(flags & FLAG_NONFINITE)
        redo_ranked = np.flatnonzero((flags & FLAG_TIE) != 0) if any(k in (RM_MRR, RM_NDCG) for _, (k, _) in dev_slots) else redo_all[:0]
        redo = np.union1d(redo_all, redo_ranked)
        nonfinite = set(redo_all.tolist())
        for l in redo.tolist():
            y, p = [L.row(l)], [P.row(l)]
            for j, (i, (k, _)) in enumerate(dev_slots):
                if l in nonfinite or k in (RM_MRR, RM_NDCG):
                    v = self.metric_functions[i].calculate(y, p)
                    sums[j] += v
                    if per_impression:
                        values[j, l] = v
        self.n_impressions, self.n_host_fallback, self.on_device = n, int(redo.size), True
        self.flags, self.counters = flags, counters
        self.sums, self.per_impression, results = {}, {}, {}
        nested = None
        at = {i: j for j, (i, _) in enumerate(dev_slots)}
        for i, metric in enumerate(self.metric_functions):
            if i in at:
                total = float(sums[at[i]])
                self.sums[metric.name] = total
                results[metric.name] = total / n if n else float("nan")
                if per_impression:
                    self.per_impression[metric.name] = values[at[i]]
            else:
                if nested is None:
                    nested = (L.to_lists(), P.to_lists())
                results[metric.name] = metric(*nested)
        self.evaluations = results
        return self

    @staticmethod
    def _raise_one_class(L, P, metric):
        y = L.host_flat() != 0
        pos = np.concatenate(([0], np.cumsum(y)))[L.offsets]
        n_pos, n_all = np.diff(pos), L.lengths
        l = int(np.flatnonzero((n_pos == 0) | (n_pos == n_all))[0])
        metric.calculate([L.row(l)], [P.row(l)])  # raises the host's own error
        raise ValueError("Only one class present in y_true.")
