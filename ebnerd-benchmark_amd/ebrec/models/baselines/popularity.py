"""Popularity baselines: what a news-recommendation result is read against.

    index = PopularityIndex.from_behaviors(df_train, events="clicks")            # per-article sorted click times
    pop = RecentPopularity(index, [timedelta(hours=1), timedelta(hours=6), timedelta(days=1)])
    scores = pop.predict(df_validation)                                          # RaggedLists aligned with article_ids_inview
    DeviceMetricEvaluator(labels, scores, [AucScore(), MrrScore()]).evaluate()

``RecentPopularity`` is the time-aware baseline: for every in-view article of an impression at time t and every window w,

    counts[w, i] = #{ events e of the article : t - max_age_w <= e < t - min_age }

The interval is half-open at the top: with ``min_age = 0`` an event at the impression's own time is NOT counted, so an index built
from the very impressions that are evaluated does not leak their clicks into their scores (``Freshness`` is closed at both ends: an
article published at the impression's instant may be shown).  ``predict`` orders by the first window and breaks its ties by the
second, and so on (``lexicographic_scores``); lists in which a clicked and an unclicked article still tie take the evaluator's host
path for mrr / ndcg, so several windows are also the way to thin such ties out.

``ArticleFeatureBaseline`` and ``InviewEstimateBaseline`` are the four lookups of the reference's
examples/baseline/ebnerd_feat_baselines.py (total_pageviews / total_inviews / total_read_time of the articles frame, and the in-view
frequency of the evaluated frame).  They count over the whole dataset and so see every impression's future.

Two paths, as in evaluation/bootstrap.py.  With a visible GPU the counts come from ``ebn_window_counts_i32``
(csrc/ebn_popularity.hip: one lane per item, nested binary searches over the row's sorted times, all compares int64).
``device=None`` or no GPU runs ``window_counts_host``, the numpy twin.  Times are datetime-like (compared as int64 microseconds,
timezone-aware values as UTC; ages are timedeltas) or plain integral numbers (ages in the same unit); the two kinds do not mix.
numpy / pandas on the host; torch is imported only on the device path."""
from __future__ import annotations

import datetime

import numpy as np
import pandas as pd

from ebrec.evaluation.device_metrics import RaggedLists, _is_tensor, device_available
from ebrec.evaluation.freshness import _age_key, _time_keys
from ebrec.utils._constants import (
    DEFAULT_ARTICLE_ID_COL, DEFAULT_CLICKED_ARTICLES_COL, DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_HISTORY_IMPRESSION_TIMESTAMP_COL,
    DEFAULT_IMPRESSION_TIMESTAMP_COL, DEFAULT_INVIEW_ARTICLES_COL,
)

# EBN_WC_* of include/ebnerd_hip.h
MAX_WINDOWS = 8
UNBOUNDED = 2 ** 63 - 1
_I64_MIN = -2 ** 63


# ---- times and ages ----------------------------------------------------------------------------------------------------------
def _int_time_keys(values, what):
    """_time_keys with int64 keys in both kinds -> (kind | None, keys [n] int64, missing [n] bool); numbers must be integral"""
    kind, keys, missing = _time_keys(values, what)
    if kind != "number":
        return kind, keys.astype(np.int64, copy=False), missing
    arr = values.to_numpy() if isinstance(values, (pd.Series, pd.Index)) else np.asarray(values)
    if arr.dtype.kind in "iu":  # exact past 2^53, which the float64 keys are not
        if arr.dtype.kind == "u" and arr.size and int(arr.max()) > UNBOUNDED:
            raise TypeError(f"{what} do not fit int64")
        return kind, arr.astype(np.int64).ravel(), missing
    ok = keys[~missing]
    if not np.all(np.isfinite(ok)) or np.any(ok != np.floor(ok)) or np.any(np.abs(ok) >= 2.0 ** 63):
        raise TypeError(f"{what} are numbers that are not integral-valued: scale the times to an integer unit")
    out = np.zeros(len(keys), np.int64)
    out[~missing] = ok.astype(np.int64)
    return kind, out, missing


def _int_age(age, kind, name):
    """an age as a non-negative int in key units; ``None`` -> UNBOUNDED"""
    if age is None:
        return UNBOUNDED
    if kind is None:  # no time to tell the kind by: the age tells it
        kind = "datetime" if isinstance(age, (datetime.timedelta, np.timedelta64)) else "number"
    if kind == "number" and isinstance(age, (int, np.integer)) and not isinstance(age, (bool, np.bool_)):
        key = int(age)
    else:
        key = _age_key(age, kind, name)
        if key != int(key):
            raise TypeError(f"{name} = {age!r} is not integral-valued: scale the times to an integer unit")
        key = int(key)
    if key < 0:
        raise ValueError(f"ages must not be negative, got {name} = {age!r}")
    if key >= UNBOUNDED:
        raise ValueError(f"{name} = {age!r} does not fit the int64 time axis; None is the unbounded window")
    return key


def _frame(df):
    return df.to_pandas() if hasattr(df, "to_pandas") else df


def _explode(lists):
    """lists of ids (a pandas column, a list of lists / arrays; None counts as empty) -> (flat ids, offsets int64)"""
    arrs = [np.asarray([] if x is None else x).ravel() for x in lists]
    offsets = np.zeros(len(arrs) + 1, np.int64)
    np.cumsum([a.size for a in arrs], out=offsets[1:])
    full = [a for a in arrs if a.size]
    return (np.concatenate(full) if full else np.zeros(0, np.int64)), offsets


def _ragged_ids(ids):
    if isinstance(ids, RaggedLists):
        return ids.host_flat(), ids.offsets
    return _explode(ids)


def _rows_of(sorted_ids, ids) -> np.ndarray:
    """int32 positions of a flat array of ids in ``sorted_ids``, -1 for unknown ids (DeviceLookup.rows_of: one searchsorted)"""
    flat = np.asarray(ids).ravel()
    n = len(sorted_ids)
    if flat.size == 0 or n == 0:
        return np.full(flat.size, -1, np.int32)
    a, b = sorted_ids.dtype.kind, flat.dtype.kind
    if not ((a in "iu" and b in "iu") or (a == b and a in "US")):
        row = {k: r for r, k in enumerate(sorted_ids.tolist())}
        return np.fromiter((row.get(i, -1) for i in flat.tolist()), np.int32, flat.size)
    pos = np.minimum(np.searchsorted(sorted_ids, flat), n - 1)
    return np.where(sorted_ids[pos] == flat, pos, -1).astype(np.int32)


def _inview(behaviors, time_col=None):
    """a behaviours frame -> (flat in-view ids, offsets, the impression times column or None)"""
    df = _frame(behaviors)
    if DEFAULT_INVIEW_ARTICLES_COL not in df.columns:
        raise ValueError(f"the behaviours frame lacks the column '{DEFAULT_INVIEW_ARTICLES_COL}'")
    if time_col is not None and time_col not in df.columns:
        raise ValueError(f"the behaviours frame lacks the column '{time_col}' with the impression times")
    flat, offsets = _explode(df[DEFAULT_INVIEW_ARTICLES_COL])
    return flat, offsets, (None if time_col is None else df[time_col].reset_index(drop=True))


# ---- the numpy twin ----------------------------------------------------------------------------------------------------------
def _sat_sub(t, age: int):
    """t - age for int64 t and an int age >= 0, saturating at INT64_MIN"""
    age = int(age)
    with np.errstate(over="ignore"):
        return np.where(t < _I64_MIN + age, np.int64(_I64_MIN), t - np.int64(age))


def rank_keys(event_times, row_offsets):
    """(the distinct event times ascending, one composite key per event): the key is ``row * (U + 1) + rank`` with ``rank`` the
    event time's position among the U distinct times, so the keys ascend over the whole event array and a bound x becomes
    ``row * (U + 1) + #{distinct times < x}`` -- any int64 time, no ``row * span + time`` that would have to fit 64 bits."""
    ev, off = np.asarray(event_times, np.int64), np.asarray(row_offsets, np.int64)
    uniq = np.unique(ev)
    if (len(off) - 1) * (len(uniq) + 1) >= 2 ** 63:
        raise ValueError("rows x distinct event times does not fit int64")
    rows = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    return uniq, rows * np.int64(len(uniq) + 1) + np.searchsorted(uniq, ev)


def window_counts_host(event_times, row_offsets, item_rows, list_offsets, list_times, max_ages, min_age=0, keys=None) -> np.ndarray:
    """numpy twin of ebn_window_counts_i32 (same contract, include/ebnerd_hip.h) -> counts [W, n_items] int32.  Vectorised: one
    np.searchsorted over the composite keys of ``rank_keys`` per window end (``keys``: a cached result of it)."""
    ev, off = np.asarray(event_times, np.int64), np.asarray(row_offsets, np.int64)
    rows, loff, lt = np.asarray(item_rows, np.int64), np.asarray(list_offsets, np.int64), np.asarray(list_times, np.int64)
    ages = [int(a) for a in max_ages]
    if not 1 <= len(ages) <= MAX_WINDOWS or min(ages) < 0 or int(min_age) < 0:
        raise ValueError(f"1 to {MAX_WINDOWS} windows of non-negative ages and a non-negative min_age")
    n, n_rows = rows.size, off.size - 1
    out = np.zeros((len(ages), n), np.int32)
    if n == 0:
        return out
    if loff.size < 2 or loff[0] != 0 or loff[-1] < n or np.any(np.diff(loff) < 0):
        raise ValueError("list_offsets must ascend from 0 to at least n_items")
    uniq, comp = rank_keys(ev, off) if keys is None else keys
    known = (rows >= 0) & (rows < n_rows)
    t = np.repeat(lt, np.diff(loff))[:n][known]
    base = rows[known] * np.int64(len(uniq) + 1)
    p_hi = np.searchsorted(comp, base + np.searchsorted(uniq, _sat_sub(t, min_age)))
    for w, age in enumerate(ages):
        lo = base if age == UNBOUNDED else base + np.searchsorted(uniq, _sat_sub(t, age))
        out[w, known] = np.maximum(p_hi - np.searchsorted(comp, lo), 0)
    return out


# ---- the index ---------------------------------------------------------------------------------------------------------------
class PopularityIndex:
    """Per-article sorted event times.  ``article_ids`` [n_events] and ``times`` [n_events] (datetime-like or integral numbers, no
    nulls): `ids` are the sorted distinct article ids, the events of ``ids[r]`` are
    ``event_times[row_offsets[r]:row_offsets[r + 1]]`` ascending (int64; microseconds for datetimes).  Built with one stable
    lexsort; uploaded at the first device call."""

    def __init__(self, article_ids, times):
        ids = np.asarray(article_ids).ravel()
        kind, keys, missing = _int_time_keys(times, "event times")
        if len(keys) != ids.size:
            raise ValueError(f"{ids.size} article ids but {len(keys)} times")
        if missing.any():
            raise ValueError(f"{int(missing.sum())} events have no time (first at position {int(np.flatnonzero(missing)[0])})")
        self._build(ids, kind, keys)

    def _build(self, ids, kind, keys):
        if ids.size and ids.dtype.kind not in "iuUS":
            raise TypeError(f"PopularityIndex needs ids that are all strings or all integers, got dtype {ids.dtype}")
        self.kind = kind if ids.size else None  # no event, no kind: the query times and the ages tell it
        self.ids, inverse = np.unique(ids, return_inverse=True)
        order = np.lexsort((keys, inverse))  # by row, then by time; stable
        self.event_times = np.ascontiguousarray(keys[order], dtype=np.int64)
        self.row_offsets = np.zeros(len(self.ids) + 1, np.int64)
        np.cumsum(np.bincount(inverse.ravel(), minlength=len(self.ids)), out=self.row_offsets[1:])
        self._host_keys, self._dev = None, {}

    @classmethod
    def from_behaviors(cls, df, events: str = "clicks", time_col: str = DEFAULT_IMPRESSION_TIMESTAMP_COL) -> "PopularityIndex":
        """one event per clicked (``events="clicks"``) or shown (``"inviews"``) article of every impression, at its time"""
        if events not in ("clicks", "inviews"):
            raise ValueError(f"events must be 'clicks' or 'inviews', got {events!r}")
        return cls._from_lists(_frame(df), DEFAULT_CLICKED_ARTICLES_COL if events == "clicks" else DEFAULT_INVIEW_ARTICLES_COL, time_col)

    @classmethod
    def from_history(cls, df) -> "PopularityIndex":
        """one event per article of every user's click history, at its time"""
        return cls._from_lists(_frame(df), DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_HISTORY_IMPRESSION_TIMESTAMP_COL, per_item_times=True)

    @classmethod
    def _from_lists(cls, df, id_col, time_col, per_item_times=False):
        for col in (id_col, time_col):
            if col not in df.columns:
                raise ValueError(f"the frame lacks the column '{col}'")
        ids, offsets = _explode(df[id_col])
        if per_item_times:
            times, t_offsets = _explode(df[time_col])
            if not np.array_equal(offsets, t_offsets):
                raise ValueError(f"'{id_col}' and '{time_col}' are not lists of the same lengths")
        else:
            kind, keys, missing = _int_time_keys(df[time_col], "impression times")
            lengths = np.diff(offsets)
            if (missing & (lengths > 0)).any():
                raise ValueError(f"{int((missing & (lengths > 0)).sum())} impressions with events have no time")
            times = np.repeat(keys.astype("datetime64[us]") if kind == "datetime" else keys, lengths)
        return cls(ids, times)

    @classmethod
    def concat(cls, *indexes) -> "PopularityIndex":
        """the events of several indexes (clicks of the behaviours and of the histories, say) in one"""
        kinds = {ix.kind for ix in indexes if ix.kind is not None and ix.n_events}
        if len(kinds) > 1:
            raise TypeError("the indexes hold datetimes and plain numbers: the two kinds do not mix")
        full = [ix for ix in indexes if ix.n_events]
        out = cls.__new__(cls)
        out._build(np.concatenate([np.repeat(ix.ids, np.diff(ix.row_offsets)) for ix in full]) if full else np.zeros(0, np.int64),
                   kinds.pop() if kinds else None, np.concatenate([ix.event_times for ix in full]) if full else np.zeros(0, np.int64))
        return out

    @property
    def n_events(self) -> int:
        return int(self.event_times.size)

    def __len__(self) -> int:
        return len(self.ids)

    def rows_of(self, ids) -> np.ndarray:
        """int32 rows of a flat array of article ids, -1 where the article has no event (as DeviceLookup.rows_of)"""
        return _rows_of(self.ids, ids)

    def host_keys(self):
        if self._host_keys is None:
            self._host_keys = rank_keys(self.event_times, self.row_offsets)
        return self._host_keys

    def device_tensors(self, device):
        """(event_times, row_offsets) int64 tensors on ``device``, uploaded once"""
        import torch

        dev = torch.device(device)
        dev = torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev
        if dev not in self._dev:
            self._dev[dev] = (torch.from_numpy(self.event_times).to(dev), torch.from_numpy(self.row_offsets).to(dev))
        return self._dev[dev]


def window_counts_call(event_times, row_offsets, item_rows, list_offsets, list_times, max_ages, min_age=0):
    """One ebn_window_counts_i32 launch over device tensors (int64 / int64 / int32 / int64 / int64) -> counts [W, n_items] int32 on
    the device."""
    import torch

    from ebrec import _hip

    ages = [int(a) for a in max_ages]
    n, W = item_rows.numel(), len(ages)
    counts = torch.empty((W, n), dtype=torch.int32, device=item_rows.device)
    with torch.cuda.device(item_rows.device):
        _hip.call("ebn_window_counts_i32", _hip.ptr(event_times), _hip.ptr(row_offsets), row_offsets.numel() - 1, _hip.ptr(item_rows), n,
                  _hip.ptr(list_offsets), _hip.ptr(list_times), list_offsets.numel() - 1, W, *(ages + [0] * (MAX_WINDOWS - W)),
                  int(min_age), _hip.ptr(counts), n, _hip.stream_handle())
    return counts


class WindowCounts:
    """``counts`` [W, n_items] int32 (a device tensor on the device path, a numpy array on the host path) of the items of the
    lists ``offsets`` [n_lists + 1]."""

    def __init__(self, counts, offsets):
        self.counts, self.offsets = counts, offsets

    def host(self) -> np.ndarray:
        return self.counts.cpu().numpy() if _is_tensor(self.counts) else self.counts


class RecentPopularity:
    """Trailing-window popularity over a ``PopularityIndex``.  ``windows``: 1 to 8 max-ages (or a single one), each a timedelta, a
    number in the unit of the index's times, or ``None`` for "since the first event"; ``min_age``: the youngest event counted
    (0: up to, not including, the impression's own time)."""

    def __init__(self, index: PopularityIndex, windows, min_age=0, device="cuda", time_col: str = DEFAULT_IMPRESSION_TIMESTAMP_COL):
        if windows is None or isinstance(windows, (datetime.timedelta, np.timedelta64, int, float, np.integer, np.floating)):
            windows = [windows]
        windows = list(windows)
        if not 1 <= len(windows) <= MAX_WINDOWS:
            raise ValueError(f"1 to {MAX_WINDOWS} windows, got {len(windows)}")
        self.index, self.windows, self.min_age, self.device, self.time_col = index, windows, min_age, device, time_col
        self._ages(index.kind)  # a wrong age is found here when the index tells the kind

    def _ages(self, kind):
        return [_int_age(w, kind, f"windows[{j}]") for j, w in enumerate(self.windows)], _int_age(self.min_age, kind, "min_age")

    def counts(self, behaviors_or_ids, times=None) -> WindowCounts:
        """``counts(behaviors)``: a frame with ``article_ids_inview`` and ``impression_time``; ``counts(ids, times)``: a RaggedLists
        or lists of lists of article ids and one time per list."""
        if times is None:
            flat, offsets, times = _inview(behaviors_or_ids, self.time_col)
        else:
            flat, offsets = _ragged_ids(behaviors_or_ids)
        t_kind, t, missing = _int_time_keys(times, "impression times")
        if len(t) != len(offsets) - 1:
            raise ValueError(f"{len(offsets) - 1} lists but {len(t)} times")
        if missing.any():
            raise ValueError(f"{int(missing.sum())} impressions have no time (first at row {int(np.flatnonzero(missing)[0])})")
        kind = self.index.kind if self.index.kind is not None else t_kind
        if t_kind is not None and kind is not None and t_kind != kind:
            raise TypeError(f"the impression times are {t_kind}s, the event times {kind}s: the two kinds do not mix")
        max_ages, min_age = self._ages(kind)
        rows = self.index.rows_of(flat)
        t = np.ascontiguousarray(t, dtype=np.int64)
        if not device_available(self.device) or rows.size == 0:
            host = window_counts_host(self.index.event_times, self.index.row_offsets, rows, offsets, t, max_ages, min_age,
                                      keys=self.index.host_keys() if rows.size else None)
            if device_available(self.device):
                import torch

                return WindowCounts(torch.from_numpy(host).to(self.device), offsets)
            return WindowCounts(host, offsets)
        import torch

        ev, off = self.index.device_tensors(self.device)
        dev = ev.device
        counts = window_counts_call(ev, off, torch.from_numpy(rows).to(dev), torch.from_numpy(offsets).to(dev),
                                    torch.from_numpy(t).to(dev), max_ages, min_age)
        return WindowCounts(counts, offsets)

    def predict(self, behaviors_or_ids, times=None) -> RaggedLists:
        """float64 scores aligned with the in-view lists: ``lexicographic_scores`` of the counts"""
        c = self.counts(behaviors_or_ids, times)
        return RaggedLists(lexicographic_scores(c.counts), c.offsets)


def lexicographic_scores(counts):
    """counts [W, n] non-negative integers (numpy or a torch tensor) -> [n] float64
    ``((c_0 (m_1 + 1) + c_1) (m_2 + 1) + c_2) ...`` with m_w the maximum of window w: ordered by window 0, ties broken by window 1,
    and so on.  Exact: raises ValueError when the product of the (m_w + 1) reaches 2^53.  Plain array arithmetic, on the device for
    a device tensor."""
    tensor = _is_tensor(counts)
    if counts.ndim != 2 or counts.shape[0] < 1:
        raise ValueError("counts must be [n_windows, n_items]")
    if tensor:
        import torch

        c = counts.to(torch.float64)
        tops = [int(v) for v in counts.max(dim=1).values.tolist()] if counts.shape[1] else [0] * counts.shape[0]
        low = int(counts.min()) if counts.numel() else 0
    else:
        counts = np.asarray(counts)
        if counts.dtype.kind not in "iu":
            raise TypeError(f"counts must be integers, got dtype {counts.dtype}")
        c = counts.astype(np.float64)
        tops = [int(v) for v in counts.max(axis=1)] if counts.shape[1] else [0] * counts.shape[0]
        low = int(counts.min()) if counts.size else 0
    if low < 0:
        raise ValueError("counts must not be negative")
    span = 1
    for m in tops:
        span *= m + 1
    if span >= 2 ** 53:
        raise ValueError(f"the windows' maxima {tops} span {span} >= 2^53 distinct scores: not exact in float64; use fewer windows")
    s = c[0].clone() if tensor else c[0].copy()
    for w in range(1, len(tops)):
        s = s * float(tops[w] + 1) + c[w]
    return s


# ---- the reference script's lookups --------------------------------------------------------------------------------------------
class ArticleFeatureBaseline:
    """Scores every in-view article by a numeric column of the articles frame (``total_pageviews`` / ``total_inviews`` /
    ``total_read_time``); unknown ids and nulls score 0.  A gather over ``rows_of``."""

    def __init__(self, articles, column: str):
        df = _frame(articles)
        for col in (DEFAULT_ARTICLE_ID_COL, column):
            if col not in df.columns:
                raise ValueError(f"the articles frame lacks the column '{col}'")
        ids = df[DEFAULT_ARTICLE_ID_COL].to_numpy()
        values = np.nan_to_num(pd.to_numeric(df[column]).to_numpy(dtype=np.float64, na_value=np.nan), nan=0.0)
        order = np.argsort(ids, kind="stable")
        self.column, self.ids, self.values = column, ids[order], values[order]

    def rows_of(self, ids) -> np.ndarray:
        return _rows_of(self.ids, ids)

    def predict(self, behaviors_or_ids) -> RaggedLists:
        if isinstance(behaviors_or_ids, RaggedLists) or not hasattr(_frame(behaviors_or_ids), "columns"):
            flat, offsets = _ragged_ids(behaviors_or_ids)
        else:
            flat, offsets, _ = _inview(behaviors_or_ids)
        rows = self.rows_of(flat)
        scores = np.where(rows >= 0, self.values[np.maximum(rows, 0)] if len(self.values) else 0.0, 0.0)
        return RaggedLists(scores.astype(np.float64), offsets)


class InviewEstimateBaseline:
    """Scores every in-view article by how often it is in view over the given frame (the reference's ``inview_dict_estimate``)."""

    def predict(self, behaviors_or_ids) -> RaggedLists:
        if isinstance(behaviors_or_ids, RaggedLists) or not hasattr(_frame(behaviors_or_ids), "columns"):
            flat, offsets = _ragged_ids(behaviors_or_ids)
        else:
            flat, offsets, _ = _inview(behaviors_or_ids)
        _, inverse, freq = np.unique(flat, return_inverse=True, return_counts=True)
        return RaggedLists(freq[inverse.ravel()].astype(np.float64), offsets)
