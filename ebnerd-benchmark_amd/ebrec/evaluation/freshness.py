"""Freshness windows for ``model.recommend(..., window=Freshness(...))``: which candidates an impression may be offered, by
the article's publish time and the impression's time.

    fresh = Freshness(articles, max_age=datetime.timedelta(days=2))       # an articles frame, or {article_id: publish time}
    ids = model.recommend(loader, candidate_ids, top_n=5, window=fresh)   # loader.X keeps ``impression_time``

An article published at ``p`` is admissible for an impression at ``t`` iff  t - max_age <= p <= t - min_age  (``max_age=None``: no
lower end), so never an article from the impression's future.  With the candidates sorted by publish time that set is ONE range
[lo, hi) of candidate positions, which is what ``ebn_topk_score_window_f32`` takes per user (include/ebnerd_hip.h): ``windows``
returns the sorting permutation and the two ends.

Times are either datetime-like (anything pandas reads as datetimes; compared as ``datetime64[us]`` integers, timezone-aware
values as UTC; ages are ``datetime.timedelta`` / ``np.timedelta64`` / ``pd.Timedelta``) or plain numbers (compared as float64;
ages are numbers in the same unit).  The two kinds do not mix.  numpy / pandas only: nothing here needs torch or a GPU.
"""
from __future__ import annotations

import datetime

import numpy as np
import pandas as pd

from ebrec.utils._constants import (
    DEFAULT_ARTICLE_ID_COL, DEFAULT_ARTICLE_PUBLISHED_TIMESTAMP_COL, DEFAULT_IMPRESSION_TIMESTAMP_COL,
)

MAX_CANDIDATES = 2 ** 31 - 1  # positions are int32


def _time_keys(values, what):
    """-> (kind "datetime" | "number" | None for nothing to tell it by, keys [n] int64 microseconds | float64, missing [n] bool)"""
    if isinstance(values, (pd.Series, pd.Index, np.ndarray)):
        s = pd.Series(values).reset_index(drop=True)
    else:
        values = list(values)
        s = pd.Series(values, dtype=None if values else object)
    if s.dtype == object:
        s = s.infer_objects()
    if s.dtype == object and s.isna().all():
        return None, np.zeros(len(s), np.int64), np.ones(len(s), bool)
    if pd.api.types.is_datetime64_any_dtype(s.dtype):
        if getattr(s.dt, "tz", None) is not None:
            s = s.dt.tz_convert("UTC").dt.tz_localize(None)
        t = s.to_numpy().astype("datetime64[us]")
        return "datetime", t.view(np.int64), np.isnat(t)
    if pd.api.types.is_numeric_dtype(s.dtype) and not pd.api.types.is_bool_dtype(s.dtype):
        t = s.to_numpy(dtype=np.float64, na_value=np.nan)
        return "number", t, np.isnan(t)
    raise TypeError(f"{what} must be datetime-like or plain numbers, got dtype {s.dtype}")


def _age_key(age, kind, name):
    """an age in the unit of the keys of ``kind``; the plain number 0 is no age in either kind"""
    if isinstance(age, (datetime.timedelta, np.timedelta64)):  # pd.Timedelta is a datetime.timedelta
        if kind == "number":
            raise TypeError(f"{name} is a timedelta but the times are plain numbers: give it in their unit")
        us = pd.Timedelta(age).value // 1000  # .value: nanoseconds
        return int(us)
    if isinstance(age, (bool, np.bool_)) or not isinstance(age, (int, float, np.integer, np.floating)):
        raise TypeError(f"{name} must be a timedelta or a plain number, got {type(age).__name__}")
    if kind == "datetime" and age != 0:
        raise TypeError(f"{name} is a plain number but the times are datetimes: give a timedelta")
    return int(age) if kind == "datetime" else float(age)


class Freshness:
    """``published``: {article_id: publish time} or an articles frame with the columns ``article_id`` and ``published_time``.
    ``max_age`` / ``min_age``: the oldest and the youngest an article may be at the impression (``None``: any age; 0: up to the
    impression itself).  ``time_col``: the column of the eval loader's frame (``loader.X``) that holds the impression times."""

    def __init__(self, published, max_age=None, min_age=0, time_col: str = DEFAULT_IMPRESSION_TIMESTAMP_COL):
        if hasattr(published, "to_pandas"):
            published = published.to_pandas()
        if isinstance(published, pd.DataFrame):
            for col in (DEFAULT_ARTICLE_ID_COL, DEFAULT_ARTICLE_PUBLISHED_TIMESTAMP_COL):
                if col not in published.columns:
                    raise ValueError(f"the articles frame lacks the column '{col}'")
            ids, times = published[DEFAULT_ARTICLE_ID_COL].tolist(), published[DEFAULT_ARTICLE_PUBLISHED_TIMESTAMP_COL].reset_index(drop=True)
        elif isinstance(published, dict):
            ids, times = list(published), list(published.values())
        else:
            raise TypeError(f"published must be an {{article_id: time}} dict or an articles frame, got {type(published).__name__}")
        self.kind, self._key, self._missing = _time_keys(times, "publish times")
        self._row = {a: i for i, a in enumerate(ids)}
        self.max_age, self.min_age, self.time_col = max_age, min_age, time_col
        self._ages(self.kind)  # a wrong age is found here when the publish times tell the kind

    def _ages(self, kind):
        """(max_age | None, min_age) in key units"""
        lo = None if self.max_age is None else _age_key(self.max_age, kind, "max_age")
        hi = _age_key(self.min_age, kind, "min_age")
        if hi < 0 or (lo is not None and lo < 0):
            raise ValueError(f"ages must not be negative, got max_age = {self.max_age!r}, min_age = {self.min_age!r}")
        if lo is not None and hi > lo:
            raise ValueError(f"min_age = {self.min_age!r} is larger than max_age = {self.max_age!r}: no article is admissible")
        return lo, hi

    def impression_times(self, loader):
        """the impression times of an eval loader, one per row of ``loader.X`` (row r is in batch r // batch_size)"""
        X = getattr(loader, "X", None)
        if X is None or self.time_col not in getattr(X, "columns", ()):
            raise ValueError(f"the loader's frame lacks the column '{self.time_col}' with the impression times: keep it on the "
                             "behaviours frame the loader is built from, or name the column with time_col=")
        return X[self.time_col]

    def windows(self, candidate_ids, impression_times):
        """-> (order [M] int64, lo [n] int32, hi [n] int32): ``order`` is the stable argsort of the candidates' publish times (ties
        keep their order in ``candidate_ids``); impression i may be offered exactly the candidates ``order[lo[i]:hi[i]]``."""
        cand = np.asarray(candidate_ids).reshape(-1)
        if len(cand) > MAX_CANDIDATES:
            raise ValueError(f"at most {MAX_CANDIDATES} candidates (int32 positions), got {len(cand)}")
        keys = cand.tolist()
        rows = np.fromiter((self._row.get(k, -1) for k in keys), dtype=np.int64, count=len(keys))
        bad = rows < 0
        bad[~bad] = self._missing[rows[~bad]]
        if bad.any():
            missing = list(dict.fromkeys(cand[bad].tolist()))
            more = f" and {len(missing) - 5} more" if len(missing) > 5 else ""
            raise ValueError(f"candidate ids without a publish time: {missing[:5]}{more}")
        t_kind, t, t_missing = _time_keys(impression_times, "impression times")
        if t_missing.any():
            raise ValueError(f"{int(t_missing.sum())} impressions have no time (first at row {int(np.flatnonzero(t_missing)[0])})")
        kind = self.kind if len(cand) else t_kind
        if t_kind is not None and kind is not None and t_kind != kind:
            raise TypeError(f"the impression times are {t_kind}s, the publish times {kind}s: the two kinds do not mix")
        max_age, min_age = self._ages(kind)
        pub = self._key[rows]
        order = np.argsort(pub, kind="stable").astype(np.int64)
        sorted_pub = pub[order]
        t = t.astype(sorted_pub.dtype, copy=False)
        lo = np.zeros(len(t), np.int64) if max_age is None else np.searchsorted(sorted_pub, t - max_age, "left")
        hi = np.searchsorted(sorted_pub, t - min_age, "right")
        return order, lo.astype(np.int32), hi.astype(np.int32)
