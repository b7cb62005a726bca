"""Content-similarity baselines: "recommend what looks like what this user read", from the document vectors alone.

    lookup = DeviceLookup(articles_dict, vector_keys=("document_vector",))
    cs = ContentSimilarity(lookup, "document_vector", mode="centroid", history_weights="exponential", lambda_factor=0.9)
    scores = cs.predict(df_validation, history=df_history)                       # RaggedLists aligned with article_ids_inview
    DeviceMetricEvaluator(labels, scores, [AucScore(), MrrScore()]).evaluate()

Over the unit rows T of the vector table, for a user's history h_1 .. h_H (oldest first) with weights w_j and a candidate c:

    centroid   p = sum_j w_j T[h_j],  score = p . T[c] / ||p||     the cosine between the weighted mean of what they read and c
    nearest    score = max_j w_j (T[h_j] . T[c])                   the candidate's closest history article (item-kNN, k = 1)

A user's history is the same for all of their impressions: histories are kept PER USER and every impression points at one by an
index (``list_hist``; -1: no history).  With ``history=`` one history per distinct user is built; the centroid profile is computed
once per user and read by every impression of that user.  ``fill`` is the score of what cannot be scored: an unknown candidate, or
a user without a single known history article.

Two paths, as in popularity.py.  With a visible GPU the scores come from csrc/ebn_content.hip (``ebn_cs_profiles_f32`` +
``ebn_cs_centroid_scores_f32``, or one ``ebn_cs_nearest_scores_f32``; contract in include/ebnerd_hip.h).  ``device=None`` or no GPU
runs the numpy twins ``content_profiles_host`` / ``content_centroid_scores_host`` / ``content_nearest_scores_host``: the same
contract, float64 accumulation, chunked.  numpy / pandas on the host; torch is imported only on the device path."""
from __future__ import annotations

import numpy as np

from ebrec.evaluation.beyond_accuracy import DeviceLookup
from ebrec.evaluation.device_metrics import RaggedLists, device_available
from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_USER_COL

from ._topn import DenseSession, TopN
from .popularity import _explode, _frame, _ragged_ids

MAX_D = 1024  # EBN_CS_MAX_D of include/ebnerd_hip.h
_CHUNK_FLOATS = 1 << 24  # float64 elements a twin materialises at a time (128 MiB)


# ---- the numpy twins -----------------------------------------------------------------------------------------------------------
def unit_rows_host(table) -> np.ndarray:
    """rows / ||row|| in float64 (a zero row stays zero), rounded to float32: what ebn_ba_unit_rows_f32 leaves on the device"""
    t = np.asarray(table, np.float64)
    norm = np.sqrt(np.einsum("ij,ij->i", t, t))
    return (t / np.where(norm > 0, norm, 1.0)[:, None]).astype(np.float32)


def _operands(table, rows, offsets, what):
    table = np.asarray(table)
    if table.ndim != 2:
        raise ValueError("table must be [n_rows, D]")
    rows, offsets = np.asarray(rows, np.int64).ravel(), np.asarray(offsets, np.int64).ravel()
    if offsets.size < 1 or offsets[0] != 0 or offsets[-1] > rows.size or np.any(np.diff(offsets) < 0):
        raise ValueError(f"{what} offsets must ascend from 0 to at most the number of entries")
    return table, rows, offsets


def _present_entries(n_rows, hist_rows, hist_weights, hist_offsets):
    """the present entries of every history, compacted -> (rows, weights float64, offsets [n_hists + 1])"""
    n = int(hist_offsets[-1])
    rows = hist_rows[:n]
    w = np.ones(n) if hist_weights is None else np.asarray(hist_weights, np.float64).ravel()[:n]
    ok = (rows >= 0) & (rows < n_rows)
    off = np.zeros(hist_offsets.size, np.int64)
    off[1:] = np.cumsum(ok)[hist_offsets[1:] - 1] if n else 0
    off[1:][hist_offsets[1:] == 0] = 0
    return rows[ok], w[ok], off


def _list_histories(list_hist, n_lists, n_hists):
    """history index per list, -1 where it is outside [0, n_hists)"""
    u = np.arange(n_lists, dtype=np.int64) if list_hist is None else np.asarray(list_hist, np.int64).ravel()
    if u.size != n_lists:
        raise ValueError(f"{n_lists} lists but {u.size} history indices")
    return np.where((u >= 0) & (u < n_hists), u, -1)


def content_profiles_host(table, hist_rows, hist_weights, hist_offsets) -> np.ndarray:
    """numpy twin of ebn_cs_profiles_f32 -> [n_hists, D] float64 unit profiles (float64 accumulation over the table's values; a
    zero row where no entry is present or the sum's norm is 0)."""
    table, hist_rows, hist_offsets = _operands(table, hist_rows, hist_offsets, "history")
    n_rows, D = table.shape
    rows, w, off = _present_entries(n_rows, hist_rows, hist_weights, hist_offsets)
    p = np.zeros((hist_offsets.size - 1, D))
    owner = np.repeat(np.arange(hist_offsets.size - 1, dtype=np.int64), np.diff(off))
    step = max(1, _CHUNK_FLOATS // max(D, 1))
    for a in range(0, rows.size, step):
        seg = owner[a:a + step]
        starts = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
        p[seg[starts]] += np.add.reduceat(table[rows[a:a + step]].astype(np.float64) * w[a:a + step, None], starts, axis=0)
    norm = np.sqrt(np.einsum("ij,ij->i", p, p))
    return np.where(norm[:, None] > 0, p / np.where(norm > 0, norm, 1.0)[:, None], 0.0)


def content_centroid_scores_host(table, profiles, list_hist, cand_rows, cand_offsets) -> np.ndarray:
    """numpy twin of ebn_cs_centroid_scores_f32 -> [n_items] float64"""
    table, cand_rows, cand_offsets = _operands(table, cand_rows, cand_offsets, "candidate")
    profiles = np.asarray(profiles)
    n_rows, D = table.shape
    n = int(cand_offsets[-1])
    u = np.repeat(_list_histories(list_hist, cand_offsets.size - 1, profiles.shape[0]), np.diff(cand_offsets))
    rows = cand_rows[:n]
    ok = np.flatnonzero((rows >= 0) & (rows < n_rows) & (u >= 0))
    out = np.zeros(cand_rows.size)
    step = max(1, _CHUNK_FLOATS // (2 * max(D, 1)))
    for a in range(0, ok.size, step):
        i = ok[a:a + step]
        out[i] = np.einsum("ij,ij->i", table[rows[i]].astype(np.float64), profiles[u[i]].astype(np.float64))
    return out


def content_nearest_scores_host(table, hist_rows, hist_weights, hist_offsets, list_hist, cand_rows, cand_offsets) -> np.ndarray:
    """numpy twin of ebn_cs_nearest_scores_f32 -> [n_items] float64: (item, present entry) pairs in blocks, float64 dots, a
    segmented max per item"""
    table, hist_rows, hist_offsets = _operands(table, hist_rows, hist_offsets, "history")
    _, cand_rows, cand_offsets = _operands(table, cand_rows, cand_offsets, "candidate")
    n_rows, D = table.shape
    h_rows, h_w, h_off = _present_entries(n_rows, hist_rows, hist_weights, hist_offsets)
    n = int(cand_offsets[-1])
    u = np.repeat(_list_histories(list_hist, cand_offsets.size - 1, hist_offsets.size - 1), np.diff(cand_offsets))
    rows = cand_rows[:n]
    first = np.where(u >= 0, h_off[np.maximum(u, 0)], 0)
    count = np.where((rows >= 0) & (rows < n_rows) & (u >= 0), h_off[np.maximum(u, 0) + 1] - first, 0)
    out = np.zeros(cand_rows.size)
    items = np.flatnonzero(count > 0)
    ends = np.cumsum(count[items])
    budget = max(1, _CHUNK_FLOATS // (2 * max(D, 1)))
    a = 0
    while a < items.size:
        done = int(ends[a - 1]) if a else 0
        b = max(a + 1, int(np.searchsorted(ends, done + budget, side="right")))
        i, c = items[a:b], count[items[a:b]]
        starts = np.cumsum(c) - c
        entry = np.arange(int(c.sum()), dtype=np.int64) - np.repeat(starts, c) + np.repeat(first[i], c)
        dots = np.einsum("ij,ij->i", table[np.repeat(rows[i], c)].astype(np.float64), table[h_rows[entry]].astype(np.float64))
        out[i] = np.maximum.reduceat(h_w[entry] * dots, starts)
        a = b
    return out


# ---- history weights -----------------------------------------------------------------------------------------------------------
def history_weight_values(kind, offsets, lambda_factor: float = 0.9):
    """float64 weights of the slots of histories ``offsets`` (oldest first), or None for ``kind=None``.  "linear" / "exponential"
    are utils/_decay.py's weights with ``ascending=True`` per history length, computed from every slot's distance to its
    history's end; a callable ``n -> n weights`` is called once per distinct length.  Negative, NaN or infinite weights raise."""
    if kind is None:
        return None
    offsets = np.asarray(offsets, np.int64)
    lengths = np.diff(offsets)
    n = int(offsets[-1])
    size = np.repeat(lengths, lengths)
    dist = np.repeat(offsets[1:], lengths) - 1 - np.arange(n, dtype=np.int64)  # 0 for the most recent click
    if callable(kind):
        w = np.zeros(n)
        for m in np.unique(lengths[lengths > 0]).tolist():
            values = np.asarray(kind(m), np.float64).ravel()
            if values.size != m:
                raise ValueError(f"history_weights({m}) returned {values.size} weights")
            at = size == m
            w[at] = values[m - 1 - dist[at]]
    elif kind == "linear":
        w = (size - dist) / np.maximum(size, 1)
    elif kind == "exponential":
        powers = np.array([float(lambda_factor) ** d for d in range(int(lengths.max()) if lengths.size else 0)], np.float64)
        w = powers[dist] if n else np.zeros(0)
    else:
        raise ValueError(f"history_weights must be None, 'linear', 'exponential' or a callable, got {kind!r}")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("history weights must be finite and not negative")
    return w


def _keep_last(flat, offsets, size):
    """each list's last ``size`` entries"""
    lengths = np.diff(offsets)
    keep = np.repeat(offsets[1:], lengths) - np.arange(int(offsets[-1]), dtype=np.int64) <= size
    out = np.zeros(offsets.size, np.int64)
    np.cumsum(np.minimum(lengths, size), out=out[1:])
    return flat[keep], out


def history_operands(rows_of, histories, history_size, history_weights, lambda_factor):
    """ids of histories -> (rows int32 by ``rows_of``, offsets int64, weights float32 | None): each history cut to its last
    ``history_size`` entries, weighted by ``history_weight_values``"""
    flat, offsets = _ragged_ids(histories)
    if history_size is not None:
        flat, offsets = _keep_last(flat, offsets, history_size)
    w = history_weight_values(history_weights, offsets, lambda_factor)
    return rows_of(flat), np.ascontiguousarray(offsets, dtype=np.int64), (None if w is None else w.astype(np.float32))


def join_frames(behaviors, history):
    """frames -> (candidates (flat ids, offsets), histories (flat ids, offsets), list_hist | None, users | None): with ``history`` one
    history per distinct user, ``users[h]`` the user of history h and ``list_hist`` the join on ``user_id``; without it the
    behaviours frame's own ``article_id_fixed`` per impression (list_hist and users None)"""
    df = _frame(behaviors)
    if DEFAULT_INVIEW_ARTICLES_COL not in df.columns:
        raise ValueError(f"the behaviours frame lacks the column '{DEFAULT_INVIEW_ARTICLES_COL}'")
    cand = _explode(df[DEFAULT_INVIEW_ARTICLES_COL])
    if history is None:
        if DEFAULT_HISTORY_ARTICLE_ID_COL not in df.columns:
            raise ValueError(f"the behaviours frame lacks the column '{DEFAULT_HISTORY_ARTICLE_ID_COL}': pass history=")
        return cand, _explode(df[DEFAULT_HISTORY_ARTICLE_ID_COL]), None, None
    hf = _frame(history)
    for frame, col in ((df, DEFAULT_USER_COL), (hf, DEFAULT_USER_COL), (hf, DEFAULT_HISTORY_ARTICLE_ID_COL)):
        if col not in frame.columns:
            raise ValueError(f"a frame lacks the column '{col}'")
    users, first = np.unique(hf[DEFAULT_USER_COL].to_numpy(), return_index=True)  # one history per distinct user
    hist = _explode(hf[DEFAULT_HISTORY_ARTICLE_ID_COL].iloc[first])
    asked = df[DEFAULT_USER_COL].to_numpy()
    if users.size == 0:
        return cand, hist, np.full(asked.size, -1, np.int32), users
    pos = np.minimum(np.searchsorted(users, asked), users.size - 1)
    return cand, hist, np.where(users[pos] == asked, pos, -1).astype(np.int32), users


# ---- the class -----------------------------------------------------------------------------------------------------------------
class ContentSimilarity(TopN):
    """Centroid or nearest-history scores over a vector key of a ``DeviceLookup`` (or of a plain ``lookup_dict``, which is
    wrapped).  ``history_weights``: None (all 1), "linear", "exponential" (with ``lambda_factor``) or a callable
    ``n -> n weights, oldest first``; ``history_size``: keep each history's last n entries; ``fill``: the score of an unknown
    candidate and of every candidate of a user without a known history article."""

    def __init__(self, lookup, key: str, mode: str = "centroid", history_weights=None, lambda_factor: float = 0.9, history_size=None,
                 fill: float = 0.0, device="cuda"):
        if mode not in ("centroid", "nearest"):
            raise ValueError(f"mode must be 'centroid' or 'nearest', got {mode!r}")
        if not (history_weights is None or callable(history_weights) or history_weights in ("linear", "exponential")):
            raise ValueError(f"history_weights must be None, 'linear', 'exponential' or a callable, got {history_weights!r}")
        if history_size is not None and (isinstance(history_size, bool) or int(history_size) != history_size or history_size < 1):
            raise ValueError(f"history_size must be a positive integer or None, got {history_size!r}")
        if not isinstance(lookup, DeviceLookup):
            lookup = DeviceLookup(lookup, vector_keys=(key,), device=device)
        if key not in lookup.vector_keys:
            raise ValueError(f"'{key}' is not among the lookup's vector keys {lookup.vector_keys}")
        self.lookup, self.key, self.mode, self.history_weights, self.lambda_factor = lookup, key, mode, history_weights, float(lambda_factor)
        self.history_size, self.fill, self.device = (None if history_size is None else int(history_size)), float(fill), device
        self._host_unit = None
        D = self.lookup.host_table(key).shape[1]
        if D > MAX_D:
            raise ValueError(f"'{key}' has {D} columns; the content kernels take at most {MAX_D}")

    # -- operands
    def _on_device(self) -> bool:
        return device_available(self.device) and self.lookup.device is not None and self.lookup.host_table(self.key).size > 0

    def host_unit_table(self) -> np.ndarray:
        if self._host_unit is None:
            self._host_unit = unit_rows_host(self.lookup.host_table(self.key))
        return self._host_unit

    def _histories(self, histories):
        """ids of histories -> (rows int32, offsets int64, weights float32 | None)"""
        return history_operands(self.lookup.rows_of, histories, self.history_size, self.history_weights, self.lambda_factor)

    def _frames(self, behaviors, history):
        """frames -> (candidates (flat ids, offsets), histories (flat ids, offsets), list_hist | None)"""
        return join_frames(behaviors, history)[:3]

    # -- public
    def profiles(self, histories):
        """[n_hists, D] float32 unit profiles of histories (a RaggedLists or lists of lists of article ids): the decay-weighted
        mean direction of each; a zero row for a history without a known article.  A device tensor on the device path."""
        rows, offsets, w = self._histories(histories)
        return self._profiles(rows, offsets, w)

    def _profiles(self, rows, offsets, w):
        if not self._on_device():
            return content_profiles_host(self.host_unit_table(), rows, w, offsets).astype(np.float32)
        import torch

        from ebrec import _hip

        table = self.lookup.device_table(self.key)
        dev = table.device
        n_hists = offsets.size - 1
        out = torch.empty((n_hists, table.shape[1]), dtype=torch.float32, device=dev)
        rows_d, off_d = torch.from_numpy(rows).to(dev), torch.from_numpy(offsets).to(dev)
        w_d = None if w is None else torch.from_numpy(w).to(dev)
        with torch.cuda.device(dev):
            _hip.call("ebn_cs_profiles_f32", _hip.ptr(table), table.shape[0], table.shape[1], table.stride(0), _hip.ptr(rows_d),
                      _hip.ptr(w_d), _hip.ptr(off_d), n_hists, rows_d.numel(), _hip.ptr(out), out.stride(0), _hip.stream_handle())
        return out

    # -- recommend / rank_targets (TopN, _topn.py), centroid mode: the unit profiles against the unit table through the existing
    # dense top-k and target-rank launches; a history without a known article has a zero profile and gets an empty list
    def _topn_ids(self):
        return self.lookup.ids

    def _topn_rows_of(self, ids):
        return self.lookup.rows_of(ids)

    def _topn_session(self, histories):
        if self.mode != "centroid":
            raise NotImplementedError("recommend / rank_targets are not implemented for ContentSimilarity(mode='nearest'): only the "
                                      "centroid profile is a dense user vector the top-k launches take")
        table = self.lookup.device_table(self.key) if self._on_device() else self.host_unit_table()
        return DenseSession(self.profiles(histories), table)

    def predict(self, candidates, histories=None, list_hist=None, *, history=None) -> RaggedLists:
        """float64 scores aligned with the candidate lists.  ``predict(behaviors, history=history_frame)``: joined on ``user_id``;
        ``predict(behaviors)``: the frame carries ``article_id_fixed`` per impression; ``predict(candidates, histories,
        list_hist=None)``: RaggedLists or lists of lists of ids, ``list_hist[l]`` the history of list l (default: l itself)."""
        if histories is None:
            if not hasattr(_frame(candidates), "columns"):
                raise ValueError("predict(candidates, histories) needs the histories; predict(behaviors) a frame")
            cand, histories, list_hist = self._frames(candidates, history)
            histories = RaggedLists(*histories)
        else:
            if history is not None:
                raise ValueError("pass either histories or history=, not both")
            cand = _ragged_ids(candidates)
        c_rows, c_off = self.lookup.rows_of(cand[0]), np.ascontiguousarray(cand[1], dtype=np.int64)
        h_rows, h_off, w = self._histories(histories)
        n_lists, n_hists = c_off.size - 1, h_off.size - 1
        if list_hist is None:
            if n_lists != n_hists:
                raise ValueError(f"{n_lists} lists but {n_hists} histories: pass list_hist")
        else:
            list_hist = np.asarray(list_hist).ravel()
            if list_hist.size != n_lists:
                raise ValueError(f"{n_lists} lists but {list_hist.size} history indices")
            list_hist = np.where((list_hist >= 0) & (list_hist < n_hists), list_hist, -1).astype(np.int32)
        if not self._on_device():
            unit = self.host_unit_table()
            if self.mode == "centroid":
                p = content_profiles_host(unit, h_rows, w, h_off).astype(np.float32)
                flat = content_centroid_scores_host(unit, p, list_hist, c_rows, c_off)
            else:
                flat = content_nearest_scores_host(unit, h_rows, w, h_off, list_hist, c_rows, c_off)
            if self.fill != 0.0:
                flat[self._unscorable(c_rows, c_off, h_rows, h_off, list_hist)] = self.fill
            if device_available(self.device) and self.lookup.device is not None:
                import torch

                return RaggedLists(torch.from_numpy(flat).to(self.device), c_off)
            return RaggedLists(flat, c_off)
        import torch

        flat = self._device_scores(c_rows, c_off, h_rows, h_off, w, list_hist).to(torch.float64)
        if self.fill != 0.0:  # the kernels leave 0 there
            flat[torch.from_numpy(self._unscorable(c_rows, c_off, h_rows, h_off, list_hist)).to(flat.device)] = self.fill
        return RaggedLists(flat, c_off)

    @staticmethod
    def _unscorable(c_rows, c_off, h_rows, h_off, list_hist) -> np.ndarray:
        """[n_items] bool: an unknown candidate, or a list whose history holds no known article"""
        known = np.zeros(h_rows.size + 1, np.int64)
        np.cumsum(h_rows >= 0, out=known[1:])
        has = known[h_off[1:]] > known[h_off[:-1]]
        u = np.arange(c_off.size - 1) if list_hist is None else list_hist.astype(np.int64)
        scorable = np.append(has, False)[u]  # -1 picks the appended False
        return (c_rows < 0) | ~np.repeat(scorable, np.diff(c_off))

    def _device_scores(self, c_rows, c_off, h_rows, h_off, w, list_hist):
        import torch

        from ebrec import _hip

        table = self.lookup.device_table(self.key)
        dev = table.device
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        c_rows_d, c_off_d, h_rows_d, h_off_d, w_d, lh_d = up(c_rows), up(c_off), up(h_rows), up(h_off), up(w), up(list_hist)
        n_lists, n_hists, n_items = c_off.size - 1, h_off.size - 1, c_rows.size
        scores = torch.empty(n_items, dtype=torch.float32, device=dev)
        shape = (_hip.ptr(table), table.shape[0], table.shape[1], table.stride(0))
        with torch.cuda.device(dev):
            if self.mode == "centroid":
                prof = torch.empty((n_hists, table.shape[1]), dtype=torch.float32, device=dev)
                _hip.call("ebn_cs_profiles_f32", *shape, _hip.ptr(h_rows_d), _hip.ptr(w_d), _hip.ptr(h_off_d), n_hists, h_rows.size,
                          _hip.ptr(prof), table.shape[1], _hip.stream_handle())
                _hip.call("ebn_cs_centroid_scores_f32", *shape, _hip.ptr(prof), n_hists, table.shape[1], _hip.ptr(lh_d), _hip.ptr(c_rows_d),
                          _hip.ptr(c_off_d), n_lists, n_items, _hip.ptr(scores), _hip.stream_handle())
            else:
                _hip.call("ebn_cs_nearest_scores_f32", *shape, _hip.ptr(h_rows_d), _hip.ptr(w_d), _hip.ptr(h_off_d), n_hists, h_rows.size,
                          _hip.ptr(lh_d), _hip.ptr(c_rows_d), _hip.ptr(c_off_d), n_lists, n_items, _hip.ptr(scores), _hip.stream_handle())
        return scores
