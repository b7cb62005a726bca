"""Batch producers of the NRMS / NRMSDocVec path: same constructor arguments and the same
``len(loader)`` / ``loader[idx] -> ((his, pred), y)`` protocol as the reference's
``NRMSDataLoader`` / ``NRMSDataLoaderPretransform`` (dataloader.py:19-180), without polars or
TensorFlow (a ``tf.keras.utils.Sequence`` is only "something with __len__ and __getitem__").

Shapes (dataloader.py:83-119):
  train mode   his (B, H, T)        pred (B, C, T)        y (B, C)          -- every in-view list has C ids
  eval mode    his (sum C_i, H, T)  pred (sum C_i, 1, T)  y (sum C_i, 1)    -- history repeated per candidate
with T = len(article_dict value): token ids (int64) for NRMS, a document vector (float) for DocVec.
Unknown / null / padded article ids map to row 0 of the lookup matrix (dataloader.py:43; Appendix B).

Article ids are mapped to lookup-matrix rows ONCE in ``__post_init__`` into padded int32 index arrays
(both loader classes: the per-batch polars transform of ``NRMSDataLoader`` (dataloader.py:68-81) exists
for memory reasons that do not apply to an index array), so ``__getitem__`` is two numpy gathers.
``compact_eval_batch`` additionally hands the scorer un-repeated histories (§8f row 1).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ebrec.utils._constants import DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_LABELS_COL, DEFAULT_USER_COL
from ebrec.utils._frames import list_column, to_pandas
from ebrec.utils._python import create_lookup_objects, repeat_by_list_values_from_matrix


def _map_ids(cells, mapping: dict) -> tuple[np.ndarray, np.ndarray]:
    """Ragged article ids (the cells of a list-valued column: lists, tuples, numpy arrays; None = a null list) -> (flat lookup
    rows int32, offsets); unknown / null ids -> row 0.  A null cell counts as ONE null id (polars explodes null -> null), like
    ``as_list``.  Integer columns take a vectorised path (one concatenate + one binary search over the sorted article ids:
    the reference's per-row polars transform and ``to_list()`` were where its loader time went); anything
    else (None inside a list, mixed types) falls back to the per-element dictionary lookup."""
    cells = list(cells)
    lens = np.fromiter((1 if c is None or isinstance(c, float) else len(c) for c in cells), dtype=np.int64, count=len(cells))
    offsets = np.concatenate(([0], np.cumsum(lens)))
    total = int(offsets[-1])
    if total and mapping:
        try:
            null = np.array([np.iinfo(np.int64).min], dtype=np.int64)
            flat_ids = np.concatenate([null if (c is None or isinstance(c, float)) else np.asarray(c) for c in cells])
        except ValueError:
            flat_ids = None
        if flat_ids is not None and flat_ids.dtype.kind in "iu" and flat_ids.size == total:
            keys = np.fromiter(mapping.keys(), dtype=np.int64, count=len(mapping))
            rows = np.fromiter(mapping.values(), dtype=np.int32, count=len(mapping))
            order = np.argsort(keys, kind="stable")
            keys, rows = keys[order], rows[order]
            flat_ids = flat_ids.astype(np.int64, copy=False)
            pos = np.minimum(np.searchsorted(keys, flat_ids), len(keys) - 1)
            return np.where(keys[pos] == flat_ids, rows[pos], 0).astype(np.int32), offsets
    get = mapping.get
    flat = np.fromiter((get(a, 0) for c in cells for a in ([None] if (c is None or isinstance(c, float)) else
                                                          (c.tolist() if isinstance(c, np.ndarray) else c))),
                       dtype=np.int32, count=total)
    return flat, offsets


@dataclass
class NewsrecDataLoader:
    """Base loader (reference dataloader.py:19-63)."""

    behaviors: object
    history_column: str
    article_dict: dict
    unknown_representation: str
    eval_mode: bool = False
    batch_size: int = 32
    inview_col: str = DEFAULT_INVIEW_ARTICLES_COL
    labels_col: str = DEFAULT_LABELS_COL
    user_col: str = DEFAULT_USER_COL
    kwargs: dict = None

    def __post_init__(self):
        self.lookup_article_index, self.lookup_article_matrix = create_lookup_objects(
            self.article_dict, unknown_representation=self.unknown_representation)
        self.unknown_index = [0]
        self.X, self.y = self.load_data()
        if self.kwargs is not None:
            self.set_kwargs(self.kwargs)

    def __len__(self) -> int:
        return int(np.ceil(len(self.X) / float(self.batch_size)))

    def __getitem__(self, idx):
        raise ValueError("Function '__getitem__' needs to be implemented.")

    def load_data(self):
        """X = behaviors without the labels column plus ``n_samples`` (in-view length); y = the labels."""
        df = to_pandas(self.behaviors)
        y = list_column(df, self.labels_col)
        X = df.drop(columns=[self.labels_col]).reset_index(drop=True)
        X["n_samples"] = [len(l) for l in list_column(X, self.inview_col)]
        return X, y

    def set_kwargs(self, kwargs: dict):
        for key, value in kwargs.items():
            setattr(self, key, value)


@dataclass
class NRMSDataLoader(NewsrecDataLoader):
    """reference dataloader.py:66-119."""

    def __post_init__(self):
        super().__post_init__()
        self._his_flat, self._his_off = _map_ids(self.X[self.history_column].tolist(), self.lookup_article_index)
        self._inv_flat, self._inv_off = _map_ids(self.X[self.inview_col].tolist(), self.lookup_article_index)
        self._y_flat = np.concatenate([np.asarray(l, dtype=np.int64) for l in self.y]) if len(self.y) else np.zeros(0, np.int64)
        hl = np.diff(self._his_off)
        if len(hl) and hl.min() != hl.max():
            raise ValueError("history lists must all have the same length (truncate_history with a padding value)")
        self._H = int(hl[0]) if len(hl) else 0

    # ---- ragged helpers --------------------------------------------------------------------
    def _rows(self, idx):
        lo = idx * self.batch_size
        return lo, min(lo + self.batch_size, len(self.X))

    def _history_rows(self, lo, hi) -> np.ndarray:
        return self._his_flat[self._his_off[lo]: self._his_off[hi]].reshape(hi - lo, self._H)

    def __getitem__(self, idx):
        """his_input_title (samples, history_size, T), pred_input_title (samples, npratio+1, T), batch_y."""
        lo, hi = self._rows(idx)
        his_idx = self._history_rows(lo, hi)
        inv = self._inv_flat[self._inv_off[lo]: self._inv_off[hi]]
        ylab = self._y_flat[self._inv_off[lo]: self._inv_off[hi]]
        if self.eval_mode:
            repeats = np.diff(self._inv_off[lo: hi + 1])
            batch_y = ylab.reshape(-1, 1)
            his_input_title = repeat_by_list_values_from_matrix(his_idx, matrix=self.lookup_article_matrix, repeats=repeats)
            pred_input_title = self.lookup_article_matrix[inv][:, None, :]
        else:
            lens = np.diff(self._inv_off[lo: hi + 1])
            if len(lens) and lens.min() != lens.max():
                raise ValueError("train mode needs equal-length in-view lists (sampling_strategy_wu2019); use eval_mode=True")
            C = int(lens[0]) if len(lens) else 0
            batch_y = ylab.reshape(hi - lo, C)
            his_input_title = self.lookup_article_matrix[his_idx]
            pred_input_title = self.lookup_article_matrix[inv.reshape(hi - lo, C)]
        return (his_input_title, pred_input_title), batch_y

    def index_batch(self, idx):
        """Train batch as article-row numbers of ``lookup_article_matrix`` -- ((his (B,H), pred (B,C)) int32, y (B,C)):
        what a model that keeps the matrix in HBM needs per step (device-side batch assembly)."""
        lo, hi = self._rows(idx)
        lens = np.diff(self._inv_off[lo: hi + 1])
        if len(lens) and lens.min() != lens.max():
            raise ValueError("train mode needs equal-length in-view lists (sampling_strategy_wu2019)")
        C = int(lens[0]) if len(lens) else 0
        sl = slice(self._inv_off[lo], self._inv_off[hi])
        return (self._history_rows(lo, hi), self._inv_flat[sl].reshape(hi - lo, C)), self._y_flat[sl].reshape(hi - lo, C)

    def index_eval_batch(self, idx):
        """Eval batch as article-row numbers of ``lookup_article_matrix``: (his (b,H) int32, cand (sum C_i,) int32,
        impression_of_row (sum C_i,) int32, y (sum C_i, 1)) -- what a scorer that has encoded every article of the
        matrix ONCE needs per batch."""
        lo, hi = self._rows(idx)
        sl = slice(self._inv_off[lo], self._inv_off[hi])
        repeats = np.diff(self._inv_off[lo: hi + 1])
        rows = np.repeat(np.arange(hi - lo, dtype=np.int32), repeats)
        return self._history_rows(lo, hi), self._inv_flat[sl], rows, self._y_flat[sl].reshape(-1, 1)

    def compact_eval_batch(self, idx):
        """Eval batch WITHOUT the per-candidate repetition of the history: (his (b,H,T), pred (sum C_i, T),
        impression_of_row (sum C_i,), y (sum C_i, 1)).  Scores are identical to the repeated layout."""
        lo, hi = self._rows(idx)
        inv = self._inv_flat[self._inv_off[lo]: self._inv_off[hi]]
        repeats = np.diff(self._inv_off[lo: hi + 1])
        rows = np.repeat(np.arange(hi - lo, dtype=np.int32), repeats)
        y = self._y_flat[self._inv_off[lo]: self._inv_off[hi]].reshape(-1, 1)
        return self.lookup_article_matrix[self._history_rows(lo, hi)], self.lookup_article_matrix[inv], rows, y


@dataclass
class NRMSDataLoaderPretransform(NRMSDataLoader):
    """reference dataloader.py:122-180: the whole frame is mapped up front (which NRMSDataLoader here
    does as well -- the class is kept so ``--nrms_loader NRMSDataLoaderPretransform`` keeps working)."""


@dataclass
class LSTURDataLoader(NRMSDataLoader):
    """reference dataloader.py:183-263 ("NPA and LSTUR shares the same DataLoader"): the NRMS batches plus the user index of
    every impression, ``user_id_mapping[user_id]`` (``unknown_user_value`` for users not in the mapping).

      train mode   ((user_indexes (B,1), his (B,H,T), pred (B,C,T)), y (B,C))
      eval mode    ((user_indexes (sum C_i,1), his (sum C_i,H,T), pred (sum C_i,1,T)), y (sum C_i,1))  -- user and history
                   repeated once per candidate
    """

    user_id_mapping: dict = None
    unknown_user_value: int = 0

    def __post_init__(self):
        super().__post_init__()
        mapping = self.user_id_mapping or {}
        get, unk = mapping.get, int(self.unknown_user_value)
        users = self.X[self.user_col].tolist() if len(self.X) else []
        self._users = np.fromiter((get(u, unk) for u in users), dtype=np.int64, count=len(users))

    def _user_rows(self, lo, hi) -> np.ndarray:
        return self._users[lo:hi]

    def __getitem__(self, idx):
        (his, pred), y = super().__getitem__(idx)
        lo, hi = self._rows(idx)
        users = self._user_rows(lo, hi)
        if self.eval_mode:
            users = np.repeat(users, np.diff(self._inv_off[lo: hi + 1]))
        return (users.reshape(-1, 1), his, pred), y

    def index_batch(self, idx):
        """Train batch as user indexes + article-row numbers: ((user (B,), his (B,H), pred (B,C)), y (B,C))."""
        (his, pred), y = super().index_batch(idx)
        lo, hi = self._rows(idx)
        return (self._user_rows(lo, hi), his, pred), y

    def compact_eval_batch(self, idx):
        """Eval batch without the per-candidate repetition: (user (b,), his (b,H,T), pred (sum C_i, T), impression_of_row
        (sum C_i,), y (sum C_i, 1))."""
        lo, hi = self._rows(idx)
        return (self._user_rows(lo, hi),) + tuple(super().compact_eval_batch(idx))

    def user_index_eval_batch(self, idx):
        """``index_eval_batch`` with the batch's user indexes in front: (user (b,), his (b,H) int32, cand (sum C_i,) int32,
        impression_of_row (sum C_i,) int32, y (sum C_i, 1)) -- what a scorer that has encoded every article of the matrix once
        needs per batch when the user encoder also takes the user id."""
        lo, hi = self._rows(idx)
        return (self._user_rows(lo, hi),) + tuple(self.index_eval_batch(idx))


@dataclass
class NAMLDataLoader(NewsrecDataLoader):
    """reference dataloader.py:266-419: the title, body, category and subcategory of every article of the history and of the
    in-view list.  ``category_mapping`` / ``subcategory_mapping`` are keyed by ARTICLE id (as the reference applies them);
    articles they do not name, and null ids, take ``unknown_category_value`` / ``unknown_subcategory_value``.  Bodies are looked
    up in their own ``create_lookup_objects`` matrix of ``body_mapping`` (unknown articles: row 0).

      train mode   ((his_title (B,H,T), his_body (B,H,Tb), his_vert (B,H,1), his_subvert (B,H,1),
                     pred_title (B,C,T), pred_body (B,C,Tb), pred_vert (B,C,1), pred_subvert (B,C,1)), y (B,C))
      eval mode    the same with every history repeated once per candidate and pred_* of shape (sum C_i, 1, .), y (sum C_i, 1)

    Deliberate difference: the reference raises on ``eval_mode=True``; here eval mode is the layout its scorer takes (one
    candidate per row), so that ``model.scorer.predict`` has a loader to run on.  ``compact_eval_batch`` hands the scorer the
    histories once per impression instead.
    """

    unknown_category_value: int = 0
    unknown_subcategory_value: int = 0
    body_mapping: dict = None
    category_mapping: dict = None
    subcategory_mapping: dict = None

    def __post_init__(self):
        self.lookup_article_index_body, self.lookup_article_matrix_body = create_lookup_objects(
            self.body_mapping, unknown_representation=self.unknown_representation)
        super().__post_init__()
        his_cells = self.X[self.history_column].tolist() if len(self.X) else []
        inv_cells = self.X[self.inview_col].tolist() if len(self.X) else []
        self._his_flat, self._his_off = _map_ids(his_cells, self.lookup_article_index)
        self._inv_flat, self._inv_off = _map_ids(inv_cells, self.lookup_article_index)
        self._hisb_flat, _ = _map_ids(his_cells, self.lookup_article_index_body)
        self._invb_flat, _ = _map_ids(inv_cells, self.lookup_article_index_body)
        self._his_cat = [self._categories(his_cells, m, u) for m, u in ((self.category_mapping, self.unknown_category_value),
                                                                        (self.subcategory_mapping, self.unknown_subcategory_value))]
        self._inv_cat = [self._categories(inv_cells, m, u) for m, u in ((self.category_mapping, self.unknown_category_value),
                                                                        (self.subcategory_mapping, self.unknown_subcategory_value))]
        self._y_flat = np.concatenate([np.asarray(l, dtype=np.int64) for l in self.y]) if len(self.y) else np.zeros(0, np.int64)
        hl = np.diff(self._his_off)
        if len(hl) and hl.min() != hl.max():
            raise ValueError("history lists must all have the same length (truncate_history with a padding value)")
        self._H = int(hl[0]) if len(hl) else 0

    @staticmethod
    def _categories(cells, mapping: dict, unknown: int) -> np.ndarray:
        """article id -> category (int64) over the ragged cells; unknown / null ids -> `unknown`."""
        shifted = {k: i + 1 for i, k in enumerate(mapping or {})}  # _map_ids sends unknown ids to 0: look up 1-based positions
        values = np.concatenate([[int(unknown)], np.fromiter((int(v) for v in (mapping or {}).values()), dtype=np.int64,
                                                             count=len(mapping or {}))])
        pos, _ = _map_ids(cells, shifted)
        return values[pos]

    def _rows(self, idx):
        lo = idx * self.batch_size
        return lo, min(lo + self.batch_size, len(self.X))

    def _history(self, lo, hi):
        """(title rows, body rows, vert, subvert) of the histories of impressions lo..hi, each (hi-lo, H)."""
        sl = slice(self._his_off[lo], self._his_off[hi])
        shape = (hi - lo, self._H)
        return (self._his_flat[sl].reshape(shape), self._hisb_flat[sl].reshape(shape), self._his_cat[0][sl].reshape(shape),
                self._his_cat[1][sl].reshape(shape))

    def _inview(self, lo, hi):
        sl = slice(self._inv_off[lo], self._inv_off[hi])
        return self._inv_flat[sl], self._invb_flat[sl], self._inv_cat[0][sl], self._inv_cat[1][sl], self._y_flat[sl]

    def __getitem__(self, idx):
        lo, hi = self._rows(idx)
        ht, hb, hv, hs = self._history(lo, hi)
        it, ib, iv, is_, ylab = self._inview(lo, hi)
        lens = np.diff(self._inv_off[lo: hi + 1])
        tm, bm = self.lookup_article_matrix, self.lookup_article_matrix_body
        if self.eval_mode:
            rep = lambda a: np.repeat(a, lens, axis=0)
            his = (tm[rep(ht)], bm[rep(hb)], rep(hv)[:, :, None], rep(hs)[:, :, None])
            pred = (tm[it][:, None, :], bm[ib][:, None, :], iv.reshape(-1, 1, 1), is_.reshape(-1, 1, 1))
            return his + pred, ylab.reshape(-1, 1)
        if len(lens) and lens.min() != lens.max():
            raise ValueError("train mode needs equal-length in-view lists (sampling_strategy_wu2019); use eval_mode=True")
        C = int(lens[0]) if len(lens) else 0
        shape = (hi - lo, C)
        his = (tm[ht], bm[hb], hv[:, :, None], hs[:, :, None])
        pred = (tm[it.reshape(shape)], bm[ib.reshape(shape)], iv.reshape(shape)[:, :, None], is_.reshape(shape)[:, :, None])
        return his + pred, ylab.reshape(shape)

    def compact_eval_batch(self, idx):
        """Eval batch without the per-candidate repetition of the history: (his_title (b,H,T), his_body (b,H,Tb),
        his_vert (b,H,1), his_subvert (b,H,1), cand_title (n,T), cand_body (n,Tb), cand_vert (n,), cand_subvert (n,),
        impression_of_row (n,), y (n, 1)), n = sum C_i.  Scores are identical to the repeated layout."""
        lo, hi = self._rows(idx)
        ht, hb, hv, hs = self._history(lo, hi)
        it, ib, iv, is_, ylab = self._inview(lo, hi)
        rows = np.repeat(np.arange(hi - lo, dtype=np.int32), np.diff(self._inv_off[lo: hi + 1]))
        tm, bm = self.lookup_article_matrix, self.lookup_article_matrix_body
        return (tm[ht], bm[hb], hv[:, :, None], hs[:, :, None], tm[it], bm[ib], iv, is_, rows, ylab.reshape(-1, 1))

    # ---- article catalogue: every distinct (title row, body row, vert, subvert) of the frame, for a scorer that encodes it once --
    def _build_catalogue(self):
        cols = [np.concatenate([h, i]).astype(np.int64) for h, i in ((self._his_flat, self._inv_flat), (self._hisb_flat, self._invb_flat),
                                                                     (self._his_cat[0], self._inv_cat[0]),
                                                                     (self._his_cat[1], self._inv_cat[1]))]
        # one int64 key per id: the four values are functions of the article id, so distinct keys <= known articles + the unknown row
        key = cols[0] * int(self.lookup_article_matrix_body.shape[0]) + cols[1]
        for c in cols[2:]:  # category values may be any integers: their dense positions go into the key
            values, pos = np.unique(c, return_inverse=True)
            key = key * max(len(values), 1) + pos.reshape(-1)
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        self._catalogue = tuple(c[first] for c in cols[:2]) + tuple(c[first] for c in cols[2:])
        inv = inv.reshape(-1).astype(np.int32)
        self._his_cidx, self._inv_cidx = inv[: len(self._his_flat)], inv[len(self._his_flat):]

    def article_catalogue(self):
        """The distinct articles of the histories and in-view lists as four aligned arrays (title rows of ``lookup_article_matrix``,
        body rows of ``lookup_article_matrix_body``, vert, subvert), each (n_catalogue,) -- no duplicate rows.  Built on first use."""
        if getattr(self, "_catalogue", None) is None:
            self._build_catalogue()
        return self._catalogue

    def index_eval_batch(self, idx):
        """Eval batch as row numbers of ``article_catalogue()``: (his (b,H) int32, cand (sum C_i,) int32, impression_of_row
        (sum C_i,) int32, y (sum C_i, 1)) -- indexing the catalogue's arrays with them gives ``compact_eval_batch``."""
        self.article_catalogue()
        lo, hi = self._rows(idx)
        sl = slice(self._inv_off[lo], self._inv_off[hi])
        rows = np.repeat(np.arange(hi - lo, dtype=np.int32), np.diff(self._inv_off[lo: hi + 1]))
        his = self._his_cidx[self._his_off[lo]: self._his_off[hi]].reshape(hi - lo, self._H)
        return his, self._inv_cidx[sl], rows, self._y_flat[sl].reshape(-1, 1)
