"""Implicit-feedback ALS baseline (Hu, Koren, Volinsky 2008): latent-factor collaborative filtering, the "does the model beat matrix
factorisation?" row of a baseline table.

    als = ImplicitALS(factors=64, regularization=0.01, alpha=40.0, iterations=15).fit(df_history_train)
    scores = als.predict(df_validation, history=df_history)                      # RaggedLists aligned with article_ids_inview
    DeviceMetricEvaluator(labels, scores, [AucScore(), MrrScore()]).evaluate()
    ids, cosines = als.similar_items(article_id, n=10)

MODEL.  Users u and items i have factors x_u, y_i in R^F.  Preference p_ui = 1 for an observed pair and 0 otherwise; confidence
c_ui = 1 + a_ui with a_ui = 0 for an unobserved pair.  The objective is

    L = sum over ALL pairs (u, i) of c_ui (p_ui - x_u . y_i)^2 + reg (||X||_F^2 + ||Y||_F^2)

with plain ``reg`` (as the ``implicit`` package does: not scaled by the row length).  One half-sweep solves every row of one side
against the fixed other side Y:

    A_u = Y^T Y + reg I + sum_{k in row u} a_k y_k y_k^T,     b_u = sum_k (1 + a_k) y_k,     x_u = A_u^{-1} b_u

A sweep solves the users first, then the items.  ``a_ui`` is ``alpha`` times the summed weights of the item's occurrences in the
user's sequence; the weight of an occurrence is 1 without ``history_weights`` (``a_ui = alpha * count``), else the decay weight of
content.py.  ``history_size`` and ``history_weights`` cut and weigh the training sequences exactly as they cut and weigh the
histories of ``predict``.  The item factors start as ``default_rng(seed).standard_normal((n_items, F)).astype(float32) * 0.01`` on
the host: both paths start from the same bits.
FOLD-IN.  ``predict`` needs no user ids: a history becomes one CSR row (duplicates combined, ``a = alpha *`` summed weight), ONE
half-sweep against the item factors gives its factor row, and the score of a candidate is the row's dot product with the
candidate's factors.  ``fill`` is the score of what cannot be scored, exactly where ``ContentSimilarity`` puts it.

Two paths, as in covisit.py.  With a visible GPU the (user, item) keys are sorted and reduced in torch, the Gram matrix comes from
``ebn_gemm_f32_ws`` (transA = 1), the rows from ``ebn_als_partials_f32`` (only rows longer than ``split_len`` entries, cut into
parts of at most ``split_len``) and ``ebn_als_solve_f32`` (csrc/ebn_als.hip; contract in include/ebnerd_hip.h), the scores from
``ebn_cs_centroid_scores_f32`` with the solved rows as profiles.  The kernels use the entries as given -- a repeated column counts
twice -- so this layer combines duplicates before every call.  ``device=None`` or no GPU runs the numpy twins ``als_partials_host``
/ ``als_solve_host`` / ``als_scores_host`` / ``als_loss_host``: the same contracts in float64 on the float32 operands, rounded once
to float32 where the kernel stores float32, including the NaN row on a pivot that is not > 0.  A NaN row raises FloatingPointError.
numpy / pandas on the host; torch is imported only on the device path."""
from __future__ import annotations

import numpy as np

from ebrec.evaluation.device_metrics import RaggedLists, device_available
from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL

from ._topn import DenseSession, TopN
from .content import ContentSimilarity, _keep_last, content_centroid_scores_host, history_weight_values
from .popularity import _explode, _frame, _ragged_ids, _rows_of

MAX_F = 128        # EBN_ALS_MAX_F of include/ebnerd_hip.h
SPLIT_LEN = 4096   # entries of a row above which it is cut into parts
_CHUNK_FLOATS = 1 << 22  # float64 elements a twin materialises at a time (32 MiB)


# ---- the numpy twins -----------------------------------------------------------------------------------------------------------
def _fixed(fixed):
    fixed = np.asarray(fixed)
    if fixed.ndim != 2 or fixed.shape[1] < 1:
        raise ValueError("fixed must be [n_fixed, F] with F >= 1")
    return fixed


def _sums_host(fixed, cols, conf, begin, end):
    """per range r the float64 sums (sum a_k y_k y_k^T [F, F], sum (1 + a_k) y_k [F], present entries) over the entries
    [begin[r], end[r]) clamped to [0, nnz] whose column lies in [0, n_fixed)"""
    n_fixed, F = fixed.shape
    cols, conf = np.asarray(cols, np.int64).ravel(), np.asarray(conf).astype(np.float64).ravel()
    nnz = cols.size
    begin, end = np.clip(np.asarray(begin, np.int64).ravel(), 0, nnz), np.clip(np.asarray(end, np.int64).ravel(), 0, nnz)
    n = begin.size
    length = np.maximum(end - begin, 0)
    A, b, present = np.zeros((n, F, F)), np.zeros((n, F)), np.zeros(n, np.int64)
    starts = np.cumsum(length) - length
    owner = np.repeat(np.arange(n, dtype=np.int64), length)
    entry = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(starts, length) + np.repeat(begin, length)
    ok = (cols[entry] >= 0) & (cols[entry] < n_fixed)
    owner, entry = owner[ok], entry[ok]
    np.add.at(present, owner, 1)
    step = max(1, _CHUNK_FLOATS // (F * F))
    for a in range(0, entry.size, step):
        seg, e = owner[a:a + step], entry[a:a + step]
        y, w = fixed[cols[e]].astype(np.float64), conf[e]
        first = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
        A[seg[first]] += np.add.reduceat((w[:, None] * y)[:, :, None] * y[:, None, :], first, axis=0)
        b[seg[first]] += np.add.reduceat((1.0 + w)[:, None] * y, first, axis=0)
    return A, b, present


def als_partials_host(fixed, cols, conf, part_begin, part_end) -> np.ndarray:
    """numpy twin of ebn_als_partials_f32 -> [n_parts, F (F + 1)] float32: per part the full symmetric sum a_k y_k y_k^T (row-major)
    followed by the F sums (1 + a_k) y_k; float64 accumulation, rounded once"""
    fixed = _fixed(fixed)
    A, b, _ = _sums_host(fixed, cols, conf, part_begin, part_end)
    return np.concatenate([A.reshape(A.shape[0], -1), b], axis=1).astype(np.float32)


def _cholesky_solve_host(A, b):
    """batched right-looking Cholesky + the two triangular solves in float64 -> (x [n, F], bad [n]): ``bad`` where a pivot was not
    > 0 (NaN included), as the kernel flags it"""
    n, F = b.shape
    L = np.array(A, np.float64)
    bad = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for k in range(F):
            p = L[:, k, k]
            bad |= ~(p > 0)
            d = np.sqrt(p)
            L[:, k, k] = d
            L[:, k + 1:, k] /= d[:, None]
            L[:, k + 1:, k + 1:] -= L[:, k + 1:, k, None] * L[:, None, k + 1:, k]
        z = np.array(b, np.float64)
        for k in range(F):
            z[:, k] /= L[:, k, k]
            z[:, k + 1:] -= L[:, k + 1:, k] * z[:, k, None]
        for k in range(F - 1, -1, -1):
            z[:, k] /= L[:, k, k]
            z[:, :k] -= L[:, k, :k] * z[:, k, None]
    return z, bad


def als_solve_host(fixed, gram, indptr, cols, conf, reg, row_parts=None, partials=None) -> np.ndarray:
    """numpy twin of ebn_als_solve_f32 -> [n_solve, F] float32: float64 sums over the float32 operands, a float64 Cholesky, rounded
    once.  Exact +0 for a row without a present entry, a NaN row where a pivot is not > 0.  ``reg`` is used as the float32 the
    kernel receives; only the lower triangle of ``gram`` (and of the partials) is read."""
    fixed = _fixed(fixed)
    F = fixed.shape[1]
    reg = float(np.float32(reg))
    if not (np.isfinite(reg) and reg > 0):
        raise ValueError(f"reg must be finite and > 0, got {reg!r}")
    g = np.asarray(gram).astype(np.float64)[:F, :F]
    g = np.tril(g) + np.tril(g, -1).T
    indptr = np.asarray(indptr, np.int64).ravel()
    n = indptr.size - 1
    out = np.zeros((n, F), np.float32)
    n_parts = 0 if partials is None else int(np.asarray(partials).shape[0])
    p0 = p1 = np.zeros(n, np.int64)
    if row_parts is not None and n_parts > 0:
        rp = np.clip(np.asarray(row_parts, np.int64).ravel(), 0, n_parts)
        p0, p1 = rp[:-1], rp[1:]
    step = max(1, _CHUNK_FLOATS // (F * F))
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        split = p0[lo:hi] < p1[lo:hi]
        begin = np.where(split, 0, indptr[lo:hi])
        A, b, present = _sums_host(fixed, cols, conf, begin, np.where(split, 0, indptr[lo + 1:hi + 1]))
        for r in np.flatnonzero(split):
            part = np.asarray(partials)[p0[lo + r]:p1[lo + r]].astype(np.float64)
            S = part[:, :F * F].sum(axis=0).reshape(F, F)
            A[r], b[r] = np.tril(S) + np.tril(S, -1).T, part[:, F * F:].sum(axis=0)
        live = np.flatnonzero(split | (present > 0))
        if live.size == 0:
            continue
        x, bad = _cholesky_solve_host(A[live] + g + reg * np.eye(F), b[live])
        x[bad] = np.nan
        out[lo + live] = x.astype(np.float32)
    return out


def als_scores_host(item_factors, rows, list_hist, cand_rows, cand_offsets) -> np.ndarray:
    """numpy twin of the scoring launch (ebn_cs_centroid_scores_f32 with the solved rows as profiles) -> [n_items] float64:
    ``rows[u(l)] . item_factors[cand_rows[i]]`` for item i of list l, 0 for an unknown candidate or a list without a row"""
    return content_centroid_scores_host(item_factors, rows, list_hist, cand_rows, cand_offsets)


def als_loss_host(user_factors, item_factors, indptr, cols, conf, reg) -> float:
    """L = sum over ALL pairs c_ui (p_ui - x_u . y_i)^2 + reg (||X||^2 + ||Y||^2) in float64, for the observed pairs of the CSR
    (duplicates combined; a column outside the items is skipped).  The all-pairs term comes from the Gram identity
    sum_ui (x_u . y_i)^2 = <X^T X, Y^T Y>: an n_users x n_items matrix never exists."""
    X, Y = np.asarray(user_factors).astype(np.float64), np.asarray(item_factors).astype(np.float64)
    indptr, cols = np.asarray(indptr, np.int64).ravel(), np.asarray(cols, np.int64).ravel()
    a = np.asarray(conf).astype(np.float64).ravel()
    total = float(np.sum((X.T @ X) * (Y.T @ Y)))
    users = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    ok = (cols >= 0) & (cols < Y.shape[0])
    step = max(1, _CHUNK_FLOATS // max(X.shape[1], 1))
    for k in range(0, cols.size, step):
        m = ok[k:k + step]
        s = np.einsum("ij,ij->i", X[users[k:k + step][m]], Y[cols[k:k + step][m]])
        total += float(np.sum((1.0 + a[k:k + step][m]) * (1.0 - s) ** 2 - s * s))
    return total + float(np.float32(reg)) * (float(np.sum(X * X)) + float(np.sum(Y * Y)))


# ---- CSR building ----------------------------------------------------------------------------------------------------------------
def _combine_host(owner, rows, weights, n_owners, n_items, alpha):
    """(owner, item row >= 0, float64 weight) triples -> CSR over the owners with duplicates combined:
    (indptr int64, cols int32 ascending per row, conf float32 = alpha * summed weight)"""
    key = owner.astype(np.int64) * max(n_items, 1) + rows.astype(np.int64)
    order = np.argsort(key, kind="stable")
    key, w = key[order], weights[order]
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if key.size else np.zeros(0, np.int64)
    sums = np.add.reduceat(w, first) if key.size else np.zeros(0)
    key = key[first]
    indptr = np.searchsorted(key // max(n_items, 1), np.arange(n_owners + 1, dtype=np.int64)).astype(np.int64)
    return indptr, (key % max(n_items, 1)).astype(np.int32), (alpha * sums).astype(np.float32)


def _combine_device(owner, rows, weights, n_owners, n_items, alpha, dev):
    """``_combine_host`` in torch: composite keys sorted (stable), the weights reduced per run of equal keys, as covisit.py's
    ``_runs_device`` counts runs"""
    import torch

    key = torch.from_numpy(owner.astype(np.int64) * max(n_items, 1) + rows.astype(np.int64)).to(dev)
    key, order = torch.sort(key, stable=True)
    w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).to(dev)[order]
    key, counts = torch.unique_consecutive(key, return_counts=True)
    sums = torch.segment_reduce(w, "sum", lengths=counts) if w.numel() else w
    owner_of = torch.div(key, max(n_items, 1), rounding_mode="floor")
    indptr = torch.searchsorted(owner_of, torch.arange(n_owners + 1, dtype=torch.int64, device=dev))
    return indptr, (key - owner_of * max(n_items, 1)).to(torch.int32), (alpha * sums).to(torch.float32)


def _transpose_host(indptr, cols, conf, n_cols):
    """CSR [n_rows, n_cols] -> the CSR of its transpose (columns ascending per row)"""
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    order = np.argsort(cols.astype(np.int64) * max(indptr.size - 1, 1) + rows, kind="stable")
    t_indptr = np.searchsorted(cols[order], np.arange(n_cols + 1)).astype(np.int64)
    return t_indptr, rows[order].astype(np.int32), conf[order]


def _transpose_device(indptr, cols, conf, n_cols):
    import torch

    n_rows = indptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n_rows, device=cols.device), indptr[1:] - indptr[:-1])
    key, order = torch.sort(cols.long() * max(n_rows, 1) + rows)
    t_indptr = torch.searchsorted(cols.long()[order].contiguous(), torch.arange(n_cols + 1, dtype=torch.int64, device=cols.device))
    return t_indptr, rows[order].to(torch.int32), conf[order].contiguous()


def split_parts(indptr, split_len):
    """the part tables of the rows longer than ``split_len`` entries -> (row_parts [n_rows + 1], part_begin, part_end) int64, or
    None when no row is that long: row r owns the parts [row_parts[r], row_parts[r + 1]), each of at most ``split_len`` entries"""
    indptr = np.asarray(indptr, np.int64)
    length = np.diff(indptr)
    n_of = np.where(length > split_len, -(-length // split_len), 0)
    if not n_of.any():
        return None
    row_parts = np.zeros(indptr.size, np.int64)
    np.cumsum(n_of, out=row_parts[1:])
    owner = np.repeat(np.arange(length.size, dtype=np.int64), n_of)
    j = np.arange(int(row_parts[-1]), dtype=np.int64) - row_parts[owner]
    begin = indptr[owner] + j * split_len
    return row_parts, begin, np.minimum(begin + split_len, indptr[owner + 1])


class _Side:
    """one CSR orientation with its part tables; numpy arrays on the host path, device tensors on the device path"""

    def __init__(self, indptr, cols, conf, split_len):
        self.indptr, self.cols, self.conf = indptr, cols, conf
        self.on_device = not isinstance(indptr, np.ndarray)
        parts = split_parts(indptr.cpu().numpy() if self.on_device else indptr, split_len)  # the one small download
        self.row_parts = self.part_begin = self.part_end = None
        if parts is not None:
            if self.on_device:
                import torch

                parts = tuple(torch.from_numpy(p).to(indptr.device) for p in parts)
            self.row_parts, self.part_begin, self.part_end = parts

    def host(self):
        parts = (self.indptr, self.cols, self.conf)
        return tuple(p.cpu().numpy() for p in parts) if self.on_device else parts


# ---- the launches ----------------------------------------------------------------------------------------------------------------
def gram_call(fixed):
    """fixed^T fixed [F, F] float32 through ebn_gemm_f32_ws (transA = 1) on the factors' device"""
    import ctypes

    import torch

    from ebrec import _hip

    n, F = fixed.shape
    gram = torch.empty((F, F), dtype=torch.float32, device=fixed.device)
    with torch.cuda.device(fixed.device):
        ws = torch.empty(max(int(_hip.lib().ebn_gemm_workspace_floats(F, F, n)), 1), dtype=torch.float32, device=fixed.device)
        _hip.call("ebn_gemm_f32_ws", 1, 0, F, F, n, ctypes.c_float(1.0), _hip.ptr(fixed), fixed.stride(0), _hip.ptr(fixed), fixed.stride(0),
                  ctypes.c_float(0.0), _hip.ptr(gram), F, _hip.ptr(ws), ws.numel(), _hip.stream_handle())
    return gram


def solve_call(fixed, gram, side, reg):
    """one half-sweep over device tensors: ebn_als_partials_f32 when ``side`` has long rows, then ebn_als_solve_f32 -> [n_solve, F]
    float32 on the device"""
    import ctypes

    import torch

    from ebrec import _hip

    n_fixed, F = fixed.shape
    n_solve, nnz = side.indptr.numel() - 1, side.cols.numel()
    out = torch.empty((n_solve, F), dtype=torch.float32, device=fixed.device)
    partials, n_parts = None, 0
    with torch.cuda.device(fixed.device):
        if side.row_parts is not None:
            n_parts = side.part_begin.numel()
            partials = torch.empty(n_parts * F * (F + 1), dtype=torch.float32, device=fixed.device)
            _hip.call("ebn_als_partials_f32", _hip.ptr(fixed), n_fixed, F, fixed.stride(0), _hip.ptr(side.cols), _hip.ptr(side.conf), nnz,
                      _hip.ptr(side.part_begin), _hip.ptr(side.part_end), n_parts, _hip.ptr(partials), _hip.stream_handle())
        _hip.call("ebn_als_solve_f32", _hip.ptr(fixed), n_fixed, F, fixed.stride(0), _hip.ptr(gram), gram.stride(0), _hip.ptr(side.indptr),
                  _hip.ptr(side.cols), _hip.ptr(side.conf), n_solve, nnz, ctypes.c_float(reg), _hip.ptr(side.row_parts), _hip.ptr(partials),
                  n_parts, _hip.ptr(out), out.stride(0), _hip.stream_handle())
    return out


def _solve_host(fixed, side, reg):
    gram = (fixed.astype(np.float64).T @ fixed.astype(np.float64)).astype(np.float32)  # float32: what the GEMM stores
    partials = None if side.row_parts is None else als_partials_host(fixed, side.cols, side.conf, side.part_begin, side.part_end)
    return als_solve_host(fixed, gram, side.indptr, side.cols, side.conf, reg, side.row_parts, partials)


# ---- the class -----------------------------------------------------------------------------------------------------------------
class ImplicitALS(TopN):
    """Implicit-feedback ALS.  ``factors``: F, 1 to 128; ``regularization``: reg > 0; ``alpha``: the confidence of one (unit-weight)
    occurrence; ``iterations``: sweeps (users, then items); ``seed``: of the initial item factors; ``history_weights`` /
    ``lambda_factor`` / ``history_size`` / ``fill``: as in ``ContentSimilarity``; ``split_len``: rows with more entries are cut into
    parts of at most this many; ``compute_loss``: append the float64 loss to ``losses`` after every half-sweep (host arithmetic on
    downloaded factors).  After ``fit``: ``item_factors`` / ``user_factors`` float32 (device tensors on the device path),
    ``article_ids`` (sorted, numpy), ``losses`` (float64 array)."""

    def __init__(self, factors: int = 64, regularization: float = 0.01, alpha: float = 40.0, iterations: int = 15, seed: int = 0,
                 history_weights=None, lambda_factor: float = 0.9, history_size=None, fill: float = 0.0, device="cuda",
                 split_len: int = SPLIT_LEN, compute_loss: bool = False):
        for name, v, lo in (("factors", factors, 1), ("iterations", iterations, 0), ("split_len", split_len, 1)):
            if isinstance(v, (bool, np.bool_)) or int(v) != v or int(v) < lo:
                raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
        if int(factors) > MAX_F:
            raise ValueError(f"factors must be at most {MAX_F}, got {factors!r}")
        reg32 = float(np.float32(regularization))
        if not (np.isfinite(reg32) and reg32 > 0):
            raise ValueError(f"regularization must be finite and > 0 (as a float32), got {regularization!r}")
        if not (np.isfinite(alpha) and alpha >= 0):
            raise ValueError(f"alpha must be finite and >= 0, got {alpha!r}")
        if not (history_weights is None or callable(history_weights) or history_weights in ("linear", "exponential")):
            raise ValueError(f"history_weights must be None, 'linear', 'exponential' or a callable, got {history_weights!r}")
        if history_size is not None and (isinstance(history_size, bool) or int(history_size) != history_size or history_size < 1):
            raise ValueError(f"history_size must be a positive integer or None, got {history_size!r}")
        self.factors, self.regularization, self.alpha, self.iterations = int(factors), float(regularization), float(alpha), int(iterations)
        self.seed, self.history_weights, self.lambda_factor = seed, history_weights, float(lambda_factor)
        self.history_size, self.fill, self.device = (None if history_size is None else int(history_size)), float(fill), device
        self.split_len, self.compute_loss = int(split_len), bool(compute_loss)
        self.article_ids = self.item_factors = self.user_factors = None
        self.losses = np.zeros(0)
        self._gram = self._sides = None

    # -- operands
    def _weighted(self, flat, offsets):
        """history_size and history_weights applied to ragged ids -> (flat ids, offsets int64, float64 weights)"""
        flat, offsets = np.asarray(flat).ravel(), np.ascontiguousarray(offsets, dtype=np.int64)
        if self.history_size is not None:
            flat, offsets = _keep_last(flat, offsets, self.history_size)
        w = history_weight_values(self.history_weights, offsets, self.lambda_factor)
        return flat, offsets, (np.ones(flat.size) if w is None else w)

    def _csr(self, rows, offsets, w, dev):
        """ragged item rows (-1: unknown, dropped) with weights -> the CSR of the sequences, duplicates combined"""
        owner = np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))
        n = int(offsets[-1])
        ok = rows[:n] >= 0
        args = (owner[ok], rows[:n][ok], w[:n][ok], offsets.size - 1, len(self.article_ids), self.alpha)
        return _combine_host(*args) if dev is None else _combine_device(*args, dev)

    def _on_device(self) -> bool:
        return device_available(self.device) and self.article_ids is not None and len(self.article_ids) > 0

    def _check(self, solved, what):
        finite = bool(np.isfinite(solved).all()) if isinstance(solved, np.ndarray) else bool(solved.isfinite().all())
        if not finite:
            raise FloatingPointError(f"ImplicitALS: a Cholesky pivot of the {what} systems was not positive (or a factor overflowed): "
                                     f"regularization={self.regularization!r} is too small for these confidences")
        return solved

    def _half_sweep(self, fixed, side, what):
        if side.on_device:
            return self._check(solve_call(fixed, gram_call(fixed), side, self.regularization), what)
        return self._check(_solve_host(fixed, side, self.regularization), what)

    # -- fit
    def fit(self, sequences, init_item_factors=None) -> "ImplicitALS":
        """``fit(history_frame)``: one user per row of its ``article_id_fixed``; ``fit(sequences)``: a RaggedLists or lists of lists
        of article ids, oldest first.  ``init_item_factors`` [n_items, F] (rows in the order of the sorted distinct ids) replaces the
        seeded start.  Returns self."""
        df = sequences if isinstance(sequences, RaggedLists) else _frame(sequences)
        if hasattr(df, "columns"):
            if DEFAULT_HISTORY_ARTICLE_ID_COL not in df.columns:
                raise ValueError(f"the frame lacks the column '{DEFAULT_HISTORY_ARTICLE_ID_COL}'")
            flat, off = _explode(df[DEFAULT_HISTORY_ARTICLE_ID_COL])
        else:
            flat, off = _ragged_ids(df)
        flat = np.asarray(flat).ravel()
        if flat.size and flat.dtype.kind not in "iuUS":
            raise TypeError(f"ImplicitALS needs ids that are all strings or all integers, got dtype {flat.dtype}")
        flat, off, w = self._weighted(flat, off)
        self.article_ids = np.unique(flat)
        n_items, n_users, F = self.article_ids.size, off.size - 1, self.factors
        if init_item_factors is None:
            Y = (np.random.default_rng(self.seed).standard_normal((n_items, F)).astype(np.float32) * np.float32(0.01)).astype(np.float32)
        else:
            Y = np.ascontiguousarray(init_item_factors, dtype=np.float32)
            if Y.shape != (n_items, F):
                raise ValueError(f"init_item_factors must be [{n_items}, {F}], got {Y.shape}")
        dev = None
        if self._on_device():
            import torch

            dev = torch.device(self.device)
            Y = torch.from_numpy(Y).to(dev)
        indptr, cols, conf = self._csr(_rows_of(self.article_ids, flat), off, w, dev)
        users = _Side(indptr, cols, conf, self.split_len)
        items = _Side(*(_transpose_host if dev is None else _transpose_device)(indptr, cols, conf, n_items), self.split_len)
        X = np.zeros((n_users, F), np.float32) if dev is None else torch.zeros((n_users, F), dtype=torch.float32, device=dev)
        losses = []
        for _ in range(self.iterations):
            X = self._half_sweep(Y, users, "user")
            if self.compute_loss:
                losses.append(self._loss(X, Y, users))
            Y = self._half_sweep(X, items, "item")
            if self.compute_loss:
                losses.append(self._loss(X, Y, users))
        self.user_factors, self.item_factors, self.losses, self._gram = X, Y, np.asarray(losses, np.float64), None
        self._sides = (users, items)
        return self

    def _loss(self, X, Y, users) -> float:
        host = lambda t: t if isinstance(t, np.ndarray) else t.cpu().numpy()
        return als_loss_host(host(X), host(Y), *users.host(), self.regularization)

    @classmethod
    def from_factors(cls, article_ids, item_factors, **kw) -> "ImplicitALS":
        """a fitted model from given item factors [n_items, F] (no user factors): ``predict`` and ``similar_items`` work.  ``article_ids``
        in any order, without repeats; ``factors`` is taken from the matrix."""
        ids = np.asarray(article_ids).ravel()
        Y = np.asarray(item_factors, np.float32)
        if Y.ndim != 2 or Y.shape[0] != ids.size or np.unique(ids).size != ids.size:
            raise ValueError("item_factors must be [n_items, F] with one row per distinct article id")
        kw.pop("factors", None)
        self = cls(factors=Y.shape[1], **kw)
        order = np.argsort(ids, kind="stable")
        self.article_ids, Y = ids[order], np.ascontiguousarray(Y[order])
        if self._on_device():
            import torch

            Y = torch.from_numpy(Y).to(self.device)
        self.item_factors = Y
        return self

    def _fitted(self):
        if self.item_factors is None:
            raise RuntimeError("ImplicitALS.fit has not been called")
        return self.item_factors

    def rows_of(self, ids) -> np.ndarray:
        """int32 factor rows of a flat array of article ids, -1 for an article the training sequences did not hold"""
        self._fitted()
        return _rows_of(self.article_ids, ids)

    # -- public
    def fold_in(self, histories):
        """[n_hists, F] float32 factor rows of histories (a RaggedLists or lists of lists of article ids): one half-sweep against
        the item factors; a zero row for a history without a known article.  A device tensor on the device path."""
        flat, offsets, w = self._weighted(*_ragged_ids(histories))
        return self._fold_in(self.rows_of(flat), offsets, w)

    def _fold_in(self, h_rows, h_off, w):
        Y = self._fitted()
        dev = None if isinstance(Y, np.ndarray) else Y.device
        side = _Side(*self._csr(h_rows, h_off, w, dev), self.split_len)
        if dev is None:
            return self._check(_solve_host(Y, side, self.regularization), "fold-in")
        if self._gram is None:
            self._gram = gram_call(Y)
        return self._check(solve_call(Y, self._gram, side, self.regularization), "fold-in")

    # -- recommend / rank_targets (TopN, _topn.py): the fold-in rows against the item factors through the existing dense top-k and
    # target-rank launches; a history without a known article folds into a zero row and gets an empty list
    def _topn_ids(self):
        self._fitted()
        return self.article_ids

    def _topn_rows_of(self, ids):
        return self.rows_of(ids)

    def _topn_session(self, histories):
        return DenseSession(self.fold_in(histories), self._fitted())

    def predict(self, candidates, histories=None, list_hist=None, *, history=None) -> RaggedLists:
        """float64 scores aligned with the candidate lists; the three call forms of ``ContentSimilarity.predict``:
        ``predict(behaviors, history=history_frame)`` joined on ``user_id``, ``predict(behaviors)`` with ``article_id_fixed`` per
        impression, ``predict(candidates, histories, list_hist=None)`` over RaggedLists or lists of lists of ids."""
        Y = self._fitted()
        if histories is None:
            if not hasattr(_frame(candidates), "columns"):
                raise ValueError("predict(candidates, histories) needs the histories; predict(behaviors) a frame")
            cand, histories, list_hist = ContentSimilarity._frames(self, candidates, history)  # the join; reads nothing of self
            histories = RaggedLists(*histories)
        else:
            if history is not None:
                raise ValueError("pass either histories or history=, not both")
            cand = _ragged_ids(candidates)
        c_rows, c_off = self.rows_of(cand[0]), np.ascontiguousarray(cand[1], dtype=np.int64)
        h_flat, h_off, w = self._weighted(*_ragged_ids(histories))
        h_rows = self.rows_of(h_flat)
        n_lists, n_hists = c_off.size - 1, h_off.size - 1
        if list_hist is None:
            if n_lists != n_hists:
                raise ValueError(f"{n_lists} lists but {n_hists} histories: pass list_hist")
        else:
            list_hist = np.asarray(list_hist).ravel()
            if list_hist.size != n_lists:
                raise ValueError(f"{n_lists} lists but {list_hist.size} history indices")
            list_hist = np.where((list_hist >= 0) & (list_hist < n_hists), list_hist, -1).astype(np.int32)
        rows = self._fold_in(h_rows, h_off, w)
        on_device = not isinstance(Y, np.ndarray)
        if on_device:
            import torch

            from ebrec import _hip

            dev = Y.device
            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            c_rows_d, c_off_d, lh_d = up(c_rows), up(c_off), up(list_hist)
            scores = torch.empty(c_rows.size, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _hip.call("ebn_cs_centroid_scores_f32", _hip.ptr(Y), Y.shape[0], Y.shape[1], Y.stride(0), _hip.ptr(rows), n_hists, rows.stride(0),
                          _hip.ptr(lh_d), _hip.ptr(c_rows_d), _hip.ptr(c_off_d), n_lists, c_rows.size, _hip.ptr(scores), _hip.stream_handle())
            flat = scores.to(torch.float64)
        else:
            flat = als_scores_host(Y, rows, list_hist, c_rows, c_off)
        if self.fill != 0.0:  # the kernel and the twin leave 0 there
            at = ContentSimilarity._unscorable(c_rows, c_off, h_rows, h_off, list_hist)
            if on_device:
                flat[torch.from_numpy(at).to(flat.device)] = self.fill
            else:
                flat[at] = self.fill
        if not on_device and device_available(self.device):
            import torch

            flat = torch.from_numpy(flat).to(self.device)
        return RaggedLists(flat, c_off)

    def similar_items(self, article_id, n: int = 10):
        """(article ids, cosines) of the ``n`` items whose factors point most nearly the way the article's do (the article itself
        left out), ties by the smaller id.  Host side, float64; KeyError for an article the training sequences did not hold."""
        Y = self._fitted()
        r = int(self.rows_of(np.asarray([article_id]))[0])
        if r < 0:
            raise KeyError(article_id)
        Y = (Y if isinstance(Y, np.ndarray) else Y.cpu().numpy()).astype(np.float64)
        norm = np.sqrt(np.einsum("ij,ij->i", Y, Y))
        unit = Y / np.where(norm > 0, norm, 1.0)[:, None]
        cos = unit @ unit[r]
        others = np.flatnonzero(np.arange(Y.shape[0]) != r)
        order = others[np.lexsort((others, -cos[others]))][:max(int(n), 0)]  # the ids ascend with the rows
        return self.article_ids[order], cos[order]
