"""EASE^R baseline (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", WWW 2019): the item-to-item ridge regression in
closed form, the "does the model beat a linear item model?" row of a baseline table.

    ease = EASE(regularization=500.0).fit(df_history_train)
    scores = ease.predict(df_validation, history=df_history)                     # RaggedLists aligned with article_ids_inview
    DeviceMetricEvaluator(labels, scores, [AucScore(), MrrScore()]).evaluate()
    ids, weights = ease.similar_items(article_id, n=10)

MODEL.  X [users, n] is binary: X[u, i] = 1 when item i occurs in user u's training sequence (after the ``history_size`` cut) at
least once.  G = X^T X holds the co-click counts (the item counts on its diagonal), A = G + reg I, P = A^{-1}, and

    B[i, j] = -P[i, j] / P[j, j]   (i != j),        B[j, j] = 0

is the minimiser of ||X - X B||_F^2 + reg ||B||_F^2 under diag(B) = 0.  The score of candidate c for a history h_1 .. h_m with
weights w is sum_j w_j B[h_j, c] (x^T B: B is not symmetric); every weight is 1 without ``history_weights``, else the decay weight
of content.py.  A repeated history entry counts twice.  With more distinct articles than ``max_items`` the ``max_items`` most-clicked
are kept (by the number of sequences that hold them, ties to the smaller id); the rest are unknown articles, scored ``fill``
exactly where ``ContentSimilarity`` puts it.

Two paths, as in als.py.  With a visible GPU the (user, item) keys are sorted and reduced in torch, and csrc/ebn_ease.hip (contract
in include/ebnerd_hip.h) does the rest: ``ebn_ease_gram_i32`` (integer atomics), ``ebn_ease_system_f32``, ``ebn_ease_invert_f32`` (a
blocked Cholesky inverse on the exact-fp32 GEMM, the system padded with an identity tail to a multiple of 4 rows so that the GEMMs
use their vector loads), ``ebn_ease_weights_f32`` in place, ``ebn_ease_scores_f32`` per ``predict``.  ``device=None`` or no GPU
runs the numpy twins ``ease_gram_host`` / ``ease_system_host`` / ``ease_invert_host`` / ``ease_weights_host`` / ``ease_scores_host``:
the same contracts in float64 on the float32 / integer operands, rounded once to float32 where the kernel stores float32.  A pivot
that is not > 0 raises FloatingPointError on both paths, a co-click count above 2^24 OverflowError.
TOP-N.  ``recommend`` / ``rank_targets`` (``TopN``, _topn.py) are the second outlet: each impression's best ``top_n`` of ALL fitted
articles, and the full-catalogue rank of its clicked article, under history exclusion and freshness windows.  B is dense, so every
article has a score for a user with at least one known history article (negative ones included), and a user without one gets an
empty list.  On the device they run ``ebn_ease_topk_f32`` / ``ebn_ease_target_rank_f32`` (csrc/ebn_ease_topk.hip): a history's score
row is the sum of its rows of B, kept in registers.  The numpy twins ``ease_topk_host`` / ``ease_target_rank_host`` do the same
float32 chain in history order, vectorised over the columns, and are bit-equal to the kernels.  That chain is not the summation
order of ``ebn_ease_scores_f32``: ``return_scores`` and ``predict`` agree to rounding, not in bits.
Not here: weighted X, catalogues above 32768 items, several GPUs, a max mode.  numpy / pandas on the host; torch is imported only on
the device path."""
from __future__ import annotations

import numpy as np

from ebrec.evaluation.device_metrics import RaggedLists, device_available
from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL

from ._topn import TopN
from .als import _combine_device, _combine_host
from .content import ContentSimilarity, _keep_last, _list_histories, _present_entries, history_operands
from .popularity import _explode, _frame, _ragged_ids, _rows_of

MAX_ITEMS = 32768          # EBN_EASE_MAX_ITEMS of include/ebnerd_hip.h
MAX_EXACT_COUNT = 1 << 24  # counts above it are not exact in float32
_CHUNK_FLOATS = 1 << 22    # float64 elements a twin materialises at a time (32 MiB)


# ---- the numpy twins -----------------------------------------------------------------------------------------------------------
def ease_gram_host(indptr, cols, n_items) -> np.ndarray:
    """numpy twin of ebn_ease_gram_i32 -> [n_items, n_items] int32, the LOWER triangle (zeros above it): 1 for every pair of
    positions p >= q of a row whose columns lie in [0, n_items), at [max, min] of the two columns.  Entries as given: a column that
    occurs x times in a row adds x (x + 1) / 2 to its diagonal element."""
    indptr, cols = np.asarray(indptr, np.int64).ravel(), np.asarray(cols, np.int64).ravel()
    n_items, n_users = int(n_items), indptr.size - 1
    ptr = np.clip(indptr, 0, cols.size)
    G = np.zeros((n_items, n_items), np.float64)
    step = max(1, _CHUNK_FLOATS // max(n_items, 1))
    for lo in range(0, n_users, step):
        hi = min(n_users, lo + step)
        length = np.maximum(ptr[lo + 1:hi + 1] - ptr[lo:hi], 0)
        owner = np.repeat(np.arange(hi - lo, dtype=np.int64), length)
        entry = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(np.cumsum(length) - length, length) + np.repeat(ptr[lo:hi], length)
        c = cols[entry]
        ok = (c >= 0) & (c < n_items)
        X = np.zeros((hi - lo, n_items))
        np.add.at(X, (owner[ok], c[ok]), 1.0)
        G += np.tril(X.T @ X, -1) + np.diag((X * (X + 1.0) / 2.0).sum(axis=0))  # exact: integers far below 2^53
    return G.astype(np.int64).astype(np.int32)


def ease_system_host(G, reg) -> np.ndarray:
    """numpy twin of ebn_ease_system_f32 -> A [n, n] float32: the lower triangle of G mirrored, ``reg`` (as the float32 the kernel
    receives) added on the diagonal in one rounding.  OverflowError for a count above 2^24."""
    G = np.asarray(G)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError("G must be [n, n]")
    low = np.tril(G).astype(np.float64)
    if low.size and low.max() > MAX_EXACT_COUNT:
        raise OverflowError(f"a co-click count exceeds 2^24 ({int(low.max())}): not exact in float32")
    A = (low + np.tril(low, -1).T).astype(np.float32).astype(np.float64)
    A[np.diag_indices_from(A)] += float(np.float32(reg))
    return A.astype(np.float32)


def _first_bad_pivot(A) -> int:
    """index + 1 of the first Cholesky pivot of the float64 matrix that is not > 0 (NaN included), 0 when there is none"""
    L = np.array(A, np.float64)
    with np.errstate(all="ignore"):
        for k in range(L.shape[0]):
            p = L[k, k]
            if not p > 0:
                return k + 1
            col = L[k + 1:, k] / np.sqrt(p)
            L[k + 1:, k + 1:] -= col[:, None] * col[None, :]
    return 0


def ease_invert_host(A):
    """numpy twin of ebn_ease_invert_f32 -> (P [n, n] float32, info): the float64 inverse of the symmetric matrix the LOWER triangle
    of the float32 A spells, symmetrised and rounded once; info = 0, or k + 1 for the first pivot (index k) that is not > 0 -- P is
    NaN-filled then."""
    A = np.asarray(A)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("A must be [n, n]")
    low = np.tril(A).astype(np.float64)
    S = low + np.tril(low, -1).T
    if S.size == 0:
        return np.zeros((0, 0), np.float32), 0
    try:
        if not np.isfinite(S).all():
            raise np.linalg.LinAlgError
        np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        info = _first_bad_pivot(S)
        if info:
            return np.full(S.shape, np.nan, np.float32), info
    P = np.linalg.inv(S)
    return ((P + P.T) * 0.5).astype(np.float32), 0


def ease_weights_host(P) -> np.ndarray:
    """numpy twin of ebn_ease_weights_f32 -> B [n, n] float32: -(P[i, j] / P[j, j]) in float64 on the float32 operands, rounded
    once; exact +0 on the diagonal"""
    P = np.asarray(P).astype(np.float64)
    if P.ndim != 2 or P.shape[0] != P.shape[1]:
        raise ValueError("P must be [n, n]")
    with np.errstate(all="ignore"):
        B = -(P / np.diag(P)[None, :])
    B[np.diag_indices_from(B)] = 0.0
    return B.astype(np.float32)


def ease_scores_host(B, hist_rows, hist_weights, hist_offsets, list_hist, cand_rows, cand_offsets) -> np.ndarray:
    """numpy twin of ebn_ease_scores_f32 -> [n_items] float64: sum over the present entries j of the item's history of
    w_j * B[hist_rows[j], c]; 0 for an absent candidate, a history index outside the histories or a history without a present
    entry"""
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != B.shape[1]:
        raise ValueError("B must be [n, n]")
    n_rows = B.shape[0]
    hist_rows, hist_offsets = np.asarray(hist_rows, np.int64).ravel(), np.asarray(hist_offsets, np.int64).ravel()
    cand_rows, cand_offsets = np.asarray(cand_rows, np.int64).ravel(), np.asarray(cand_offsets, np.int64).ravel()
    h_rows, h_w, h_off = _present_entries(n_rows, hist_rows, hist_weights, hist_offsets)
    n = int(cand_offsets[-1])
    u = np.repeat(_list_histories(list_hist, cand_offsets.size - 1, hist_offsets.size - 1), np.diff(cand_offsets))
    rows = cand_rows[:n]
    first = np.where(u >= 0, h_off[np.maximum(u, 0)], 0)
    count = np.where((rows >= 0) & (rows < n_rows) & (u >= 0), h_off[np.maximum(u, 0) + 1] - first, 0)
    out = np.zeros(cand_rows.size)
    items = np.flatnonzero(count > 0)
    ends = np.cumsum(count[items])
    a = 0
    while a < items.size:
        done = int(ends[a - 1]) if a else 0
        b = max(a + 1, int(np.searchsorted(ends, done + _CHUNK_FLOATS, side="right")))
        i, c = items[a:b], count[items[a:b]]
        starts = np.cumsum(c) - c
        entry = np.arange(int(c.sum()), dtype=np.int64) - np.repeat(starts, c) + np.repeat(first[i], c)
        out[i] = np.add.reduceat(h_w[entry] * B[h_rows[entry], np.repeat(rows[i], c)].astype(np.float64), starts)
        a = b
    return out


# ---- top-N over the whole catalogue: the numpy twins of ebn_ease_topk_f32 / ebn_ease_target_rank_f32 -----------------------------
MAX_TOP_K, MAX_EXCLUDE = 64, 256  # limits of include/ebnerd_hip.h


def ease_chain_host(B, rows, weights):
    """one history's scores over the whole catalogue in the kernel's arithmetic -> (scored: bool, score [n_rows] float32): the
    present entries in history order, the first product stored, the later ones added; every product and every add rounds once to
    float32, vectorised over the columns"""
    n_rows = B.shape[0]
    score, scored = np.zeros(n_rows, np.float32), False
    with np.errstate(all="ignore"):
        for j, h in enumerate(np.asarray(rows).tolist()):
            if not 0 <= h < n_rows:
                continue
            p = B[h, :n_rows] if weights is None else np.float32(weights[j]) * B[h, :n_rows]
            score = (score + p if scored else p).astype(np.float32)
            scored = True
    return scored, score


def ease_chains_host(B, hist_rows, hist_weights, hist_offsets) -> list:
    """[(scored, score [n_rows] float32)] per history: the part of the twins that depends on neither the candidates nor the windows
    nor the exclusion lists (``chains=`` of both twins takes it, so that several calls share it)"""
    B = np.asarray(B, np.float32)
    hist_rows, hist_offsets = np.asarray(hist_rows, np.int64).ravel(), np.asarray(hist_offsets, np.int64).ravel()
    w_all = None if hist_weights is None else np.asarray(hist_weights, np.float32).ravel()
    out = []
    for h in range(hist_offsets.size - 1):
        a, b = (min(max(int(v), 0), hist_rows.size) for v in (hist_offsets[h], hist_offsets[h + 1]))
        out.append(ease_chain_host(B, hist_rows[a:b], None if w_all is None else w_all[a:b]))
    return out


def _ease_walk_host(B, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, window, exclude, chains=None):
    """per user: (admissible columns, their positions, the float32 scores of all columns, flags)"""
    B = np.asarray(B, np.float32)
    if B.ndim != 2 or B.shape[1] < B.shape[0]:
        raise ValueError("B must be [n, ld] with ld >= n")
    n_rows = B.shape[0]
    hist_rows, hist_offsets = np.asarray(hist_rows, np.int64).ravel(), np.asarray(hist_offsets, np.int64).ravel()
    w_all = None if hist_weights is None else np.asarray(hist_weights, np.float32).ravel()
    n_hists = hist_offsets.size - 1
    pos_of = np.arange(n_rows, dtype=np.int64) if cand_pos is None else np.asarray(cand_pos, np.int64).ravel()
    if pos_of.size != n_rows or (cand_pos is None and M != n_rows):
        raise ValueError(f"cand_pos must hold one position per catalogue row ({n_rows}); without it M == n_rows")
    flags = np.zeros(2, np.int32)
    beyond, none = bool((pos_of >= M).any()), (False, np.zeros(n_rows, np.float32))
    memo = {}
    for u in range(int(n_users)):
        h = u if user_hist is None else int(user_hist[u])
        scored, score = none
        if 0 <= h < n_hists:
            if chains is not None:
                scored, score = chains[h]
            else:
                if h not in memo:
                    if len(memo) >= 64:
                        memo.clear()
                    a, b = (min(max(int(v), 0), hist_rows.size) for v in (hist_offsets[h], hist_offsets[h + 1]))
                    memo[h] = ease_chain_host(B, hist_rows[a:b], None if w_all is None else w_all[a:b])
                scored, score = memo[h]
        lo, hi = 0, int(M)
        if window is not None:
            lo, hi = max(int(window[u][0]), 0), min(int(window[u][1]), int(M))
            if lo >= hi:
                lo = hi = 0
        if scored and beyond:
            flags[0] = 1
        adm = np.full(n_rows, scored) & (pos_of >= lo) & (pos_of < hi)
        if exclude is not None:
            ex = np.asarray(exclude[u], np.int64).ravel()
            adm[ex[(ex >= 0) & (ex < n_rows)]] = False
        if (adm & np.isnan(score)).any():
            flags[1] = 1
        adm &= ~np.isnan(score)
        cols = np.flatnonzero(adm)
        yield u, cols, pos_of[cols], score, flags


def ease_topk_host(B, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, window, exclude, k, chains=None):
    """numpy twin of ebn_ease_topk_f32, bit-equal to it -> (pos [U, k] int32, score [U, k] float32, flags [2] int32)"""
    if not 1 <= int(k) <= MAX_TOP_K:
        raise ValueError(f"k must lie in [1, {MAX_TOP_K}], got {k}")
    out_pos, out_score = np.full((int(n_users), int(k)), -1, np.int32), np.full((int(n_users), int(k)), -np.inf, np.float32)
    flags = np.zeros(2, np.int32)
    for u, cols, pos, score, flags in _ease_walk_host(B, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, window,
                                                      exclude, chains):
        s = score[cols]
        best = np.lexsort((pos, -s))[:int(k)]  # score descending, then position ascending
        out_pos[u, :best.size], out_score[u, :best.size] = pos[best], s[best]
    return out_pos, out_score, flags


def ease_target_rank_host(B, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, target_pos, window, exclude,
                          chains=None):
    """numpy twin of ebn_ease_target_rank_f32 -> (rank [U] int32, count [U] int32, score [U] float32, flags [2] int32)"""
    target_pos = np.asarray(target_pos, np.int64).ravel()
    U = int(n_users)
    rank, count, t_out = np.zeros(U, np.int32), np.zeros(U, np.int32), np.full(U, -np.inf, np.float32)
    flags, oob_target = np.zeros(2, np.int32), bool((target_pos[:U] >= M).any())
    for u, cols, pos, score, flags in _ease_walk_host(B, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, window,
                                                      exclude, chains):
        count[u] = cols.size
        at = np.flatnonzero(pos == target_pos[u]) if 0 <= target_pos[u] < M else np.zeros(0, np.int64)
        if at.size:
            s, t = score[cols], score[cols[at[0]]]
            rank[u] = 1 + int(((s > t) | ((s == t) & (pos < target_pos[u]))).sum())
            t_out[u] = t
    if oob_target:
        flags[0] = 1
    return rank, count, t_out, flags


# ---- the launches ----------------------------------------------------------------------------------------------------------------
def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


def gram_call(indptr, cols, n_items):
    """ebn_ease_gram_i32 over device tensors -> G [n_items, ld] int32 on the device (ld = n_items rounded up to 4); only its lower
    triangle is defined"""
    import torch

    from ebrec import _hip

    G = torch.empty((n_items, _pad4(n_items)), dtype=torch.int32, device=indptr.device)
    with torch.cuda.device(indptr.device):
        _hip.call("ebn_ease_gram_i32", _hip.ptr(indptr), _hip.ptr(cols), indptr.numel() - 1, cols.numel(), n_items, _hip.ptr(G), G.stride(0),
                  _hip.stream_handle())
    return G


def weights_call(G, n, reg):
    """system, inverse and weights over the device Gram matrix -> (B [n, n] float32 view at a row stride of n rounded up to 4,
    status [2] int32 on the device: the 2^24 flag and the inverse's info).  The system carries an identity tail up to that stride:
    the inverse of diag(A, I) is diag(P, I)."""
    import ctypes

    import torch

    from ebrec import _hip

    dev, m = G.device, _pad4(n)
    A = torch.zeros((m, m), dtype=torch.float32, device=dev)
    if m > n:
        A.diagonal()[n:] = 1.0
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _hip.stream_handle()
        _hip.call("ebn_ease_system_f32", _hip.ptr(G), G.stride(0), n, ctypes.c_float(reg), _hip.ptr(A), m, _hip.ptr(status), st)
        floats = int(_hip.lib().ebn_ease_workspace_floats(m))
        work = torch.empty(max(floats, 1), dtype=torch.float32, device=dev)
        _hip.call("ebn_ease_invert_f32", _hip.ptr(A), m, m, _hip.ptr(work), floats, ctypes.c_void_p(status.data_ptr() + 4), st)
        _hip.call("ebn_ease_weights_f32", _hip.ptr(A), m, n, _hip.ptr(A), m, st)
    return A[:n, :n], status


def scores_call(B, hist_rows, hist_weights, hist_offsets, list_hist, cand_rows, cand_offsets):
    """One ebn_ease_scores_f32 launch over device tensors -> scores [n_items] float32 on the device (``hist_weights`` / ``list_hist``
    may be None)"""
    import torch

    from ebrec import _hip

    scores = torch.empty(cand_rows.numel(), dtype=torch.float32, device=cand_rows.device)
    with torch.cuda.device(cand_rows.device):
        _hip.call("ebn_ease_scores_f32", _hip.ptr(B), B.shape[0], B.stride(0), _hip.ptr(hist_rows), _hip.ptr(hist_weights), _hip.ptr(hist_offsets),
                  hist_offsets.numel() - 1, hist_rows.numel(), _hip.ptr(list_hist), _hip.ptr(cand_rows), _hip.ptr(cand_offsets),
                  cand_offsets.numel() - 1, cand_rows.numel(), _hip.ptr(scores), _hip.stream_handle())
    return scores


def _ease_operands(B, hist_rows, hist_weights, hist_offsets, user_hist, cand_pos, M):
    from ebrec import _hip

    n_rows = B.shape[0]
    if B.dim() != 2 or B.stride(1) != 1 or B.stride(0) < n_rows:
        raise ValueError("B must be a [n, n] float32 tensor with unit column stride")
    M = n_rows if cand_pos is None else int(M)
    return (_hip.ptr(B), n_rows, max(B.stride(0), n_rows), _hip.ptr(hist_rows), _hip.ptr(hist_weights),
            _hip.ptr(hist_offsets), hist_offsets.numel() - 1, hist_rows.numel(), _hip.ptr(user_hist), _hip.ptr(cand_pos), M), n_rows


def _check_device_args(U, window, exclude, target_pos=None):
    import torch

    for name, t, shape in (("window", window, (U, 2)), ("exclude", exclude, None), ("target_pos", target_pos, (U,))):
        if t is None:
            continue
        if t.dtype != torch.int32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape) or \
                (shape is None and (t.dim() != 2 or t.shape[0] != U)):
            raise ValueError(f"{name} must be a contiguous int32 tensor with one row per user ({U}), got {tuple(t.shape)} {t.dtype}")


def topk_call(B, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, window, exclude, k, flags, n_splits: int = 0):
    """One ebn_ease_topk_f32 launch over device tensors (``hist_weights`` / ``user_hist`` / ``cand_pos`` / ``window`` [U, 2] /
    ``exclude`` [U, X] may be None; B at any row stride) -> (pos [U, k] int32, score [U, k] float32); ``flags`` [2] int32
    accumulates."""
    import torch

    from ebrec import _hip

    U, dev = int(n_users), B.device
    _check_device_args(U, window, exclude)
    ops, n_rows = _ease_operands(B, hist_rows, hist_weights, hist_offsets, user_hist, cand_pos, M)
    pos = torch.empty(U, k, dtype=torch.int32, device=dev)
    score = torch.empty(U, k, dtype=torch.float32, device=dev)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_ease_topk_auto_splits(U, n_rows))
    ws = torch.empty(max(int(lib.ebn_ease_topk_workspace_bytes(U, k, max(splits, 1))), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("ebn_ease_topk_f32", *ops, _hip.ptr(window), _hip.ptr(exclude), 0 if exclude is None else exclude.shape[1], int(k), splits,
                  _hip.ptr(pos), _hip.ptr(score), _hip.ptr(flags), _hip.ptr(ws), ws.numel(), U, _hip.stream_handle())
    return pos, score


def rank_call(B, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, target_pos, window, exclude, flags,
              n_splits: int = 0):
    """One ebn_ease_target_rank_f32 launch over device tensors: ``target_pos`` [U] int32 candidate positions (< 0: none) -> (rank [U]
    int32: 1-based place in ``topk_call``'s order, 0 = not ranked; count [U] int32: the user's admissible columns; score [U]
    float32: the target's score, -inf where rank is 0); ``flags`` accumulates."""
    import torch

    from ebrec import _hip

    U, dev = int(n_users), B.device
    _check_device_args(U, window, exclude, target_pos)
    ops, n_rows = _ease_operands(B, hist_rows, hist_weights, hist_offsets, user_hist, cand_pos, M)
    rank = torch.empty(U, dtype=torch.int32, device=dev)
    count = torch.empty(U, dtype=torch.int32, device=dev)
    score = torch.empty(U, dtype=torch.float32, device=dev)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_ease_topk_auto_splits(U, n_rows))
    ws = torch.empty(max(int(lib.ebn_ease_target_rank_workspace_bytes(U, max(splits, 1), 0 if cand_pos is None else int(M))), 16),
                     dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("ebn_ease_target_rank_f32", *ops, _hip.ptr(target_pos), _hip.ptr(window), _hip.ptr(exclude),
                  0 if exclude is None else exclude.shape[1], splits, _hip.ptr(rank), _hip.ptr(count), _hip.ptr(score), _hip.ptr(flags),
                  _hip.ptr(ws), ws.numel(), U, _hip.stream_handle())
    return rank, count, score


class EaseSession:
    """what ``TopN`` drives (see _topn.py): the histories of one ``recommend`` / ``rank_targets`` call against B; device tensors and
    the two kernels when B lives on the device, the float32 twins otherwise"""

    def __init__(self, B, h_rows, h_off, w, on_device: bool):
        self.on_device, self.B, self.n_rows = on_device, B, int(B.shape[0])
        self.cand_pos, self.M = None, self.n_rows
        self.device = B.device if on_device else None
        if on_device:
            import torch

            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            self.hist = (up(h_rows.astype(np.int32)), up(w), up(np.ascontiguousarray(h_off, dtype=np.int64)))
        else:
            self.hist = (h_rows, w, np.ascontiguousarray(h_off, dtype=np.int64))

    def candidates(self, cand_rows):
        """position -> row becomes the kernels' row -> position (-1: no candidate); the identity is passed as None"""
        rows = np.asarray(cand_rows, np.int64)
        self.M = rows.size
        if rows.size == self.n_rows and np.array_equal(rows, np.arange(self.n_rows)):
            self.cand_pos = None
            return
        pos = np.full(self.n_rows, -1, np.int32)
        pos[rows] = np.arange(rows.size, dtype=np.int32)
        self.cand_pos = pos
        if self.on_device:
            import torch

            self.cand_pos = torch.from_numpy(pos).to(self.device)

    def _up(self, a):
        import torch

        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    def topk(self, hist_idx, window, exclude, k, flags):
        U = len(hist_idx)
        if not self.on_device:
            pos, score, f = ease_topk_host(self.B, *self.hist, hist_idx, U, self.cand_pos, self.M, window, exclude, k)
            flags |= f
            return pos, score
        return topk_call(self.B, *self.hist, self._up(hist_idx), U, self.cand_pos, self.M, self._up(window), self._up(exclude), k, flags)

    def rank(self, hist_idx, target_pos, window, exclude, flags):
        U = len(hist_idx)
        if not self.on_device:
            rank, count, score, f = ease_target_rank_host(self.B, *self.hist, hist_idx, U, self.cand_pos, self.M, target_pos, window, exclude)
            flags |= f
            return rank, count, score
        return rank_call(self.B, *self.hist, self._up(hist_idx), U, self.cand_pos, self.M, self._up(target_pos), self._up(window),
                         self._up(exclude), flags)


# ---- the class -----------------------------------------------------------------------------------------------------------------
class EASE(TopN):
    """EASE^R.  ``regularization``: reg > 0 (as a float32); ``max_items``: the most-clicked articles kept, at most 32768;
    ``history_size`` / ``history_weights`` / ``lambda_factor`` / ``fill``: as in ``ContentSimilarity`` (``history_size`` also cuts the
    training sequences; the training matrix is binary whatever the weights).  After ``fit``: ``article_ids`` (sorted, numpy),
    ``item_counts`` (int64: the sequences that hold the article) and ``weights`` = B [n, n] float32 (a device tensor on the device
    path)."""

    def __init__(self, regularization: float = 500.0, max_items: int = 16384, history_size=None, history_weights=None,
                 lambda_factor: float = 0.9, fill: float = 0.0, device="cuda"):
        reg32 = float(np.float32(regularization))
        if not (np.isfinite(reg32) and reg32 > 0):
            raise ValueError(f"regularization must be finite and > 0 (as a float32), got {regularization!r}")
        if isinstance(max_items, (bool, np.bool_)) or int(max_items) != max_items or not 1 <= int(max_items) <= MAX_ITEMS:
            raise ValueError(f"max_items must be an integer in [1, {MAX_ITEMS}], got {max_items!r}")
        if not (history_weights is None or callable(history_weights) or history_weights in ("linear", "exponential")):
            raise ValueError(f"history_weights must be None, 'linear', 'exponential' or a callable, got {history_weights!r}")
        if history_size is not None and (isinstance(history_size, bool) or int(history_size) != history_size or history_size < 1):
            raise ValueError(f"history_size must be a positive integer or None, got {history_size!r}")
        self.regularization, self.max_items = float(regularization), int(max_items)
        self.history_weights, self.lambda_factor = history_weights, float(lambda_factor)
        self.history_size, self.fill, self.device = (None if history_size is None else int(history_size)), float(fill), device
        self.article_ids = self.item_counts = self.weights = None

    # -- fit
    def fit(self, sequences) -> "EASE":
        """``fit(history_frame)``: one user per row of its ``article_id_fixed``; ``fit(sequences)``: a RaggedLists or lists of lists
        of article ids.  Returns self."""
        df = sequences if isinstance(sequences, RaggedLists) else _frame(sequences)
        if hasattr(df, "columns"):
            if DEFAULT_HISTORY_ARTICLE_ID_COL not in df.columns:
                raise ValueError(f"the frame lacks the column '{DEFAULT_HISTORY_ARTICLE_ID_COL}'")
            flat, off = _explode(df[DEFAULT_HISTORY_ARTICLE_ID_COL])
        else:
            flat, off = _ragged_ids(df)
        flat, off = np.asarray(flat).ravel(), np.ascontiguousarray(off, dtype=np.int64)
        if flat.size and flat.dtype.kind not in "iuUS":
            raise TypeError(f"EASE needs ids that are all strings or all integers, got dtype {flat.dtype}")
        if self.history_size is not None:
            flat, off = _keep_last(flat, off, self.history_size)
        n_users = off.size - 1
        owner = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(off))
        all_ids = np.unique(flat)
        # the sequences that hold each article (duplicates count once), then the max_items most-clicked, ties to the smaller id
        pairs = np.unique(owner * max(all_ids.size, 1) + _rows_of(all_ids, flat).astype(np.int64))
        counts = np.bincount(pairs % max(all_ids.size, 1), minlength=all_ids.size).astype(np.int64)
        keep = np.sort(np.lexsort((np.arange(all_ids.size), -counts))[:self.max_items])
        self.article_ids, self.item_counts = all_ids[keep], counts[keep]
        n = self.article_ids.size
        rows = _rows_of(self.article_ids, flat)
        ok = rows >= 0
        args = (owner[ok], rows[ok], np.ones(int(ok.sum())), n_users, n, 1.0)  # the CSR of X: columns ascending and distinct
        reg = float(np.float32(self.regularization))
        if device_available(self.device) and n > 0:
            import torch

            indptr, cols, _ = _combine_device(*args, torch.device(self.device))
            G = gram_call(indptr, cols, n)
            B, status = weights_call(G, n, reg)
            over, info = (int(v) for v in status.cpu().numpy())
        else:
            indptr, cols, _ = _combine_host(*args)
            G = ease_gram_host(indptr, cols, n)
            over = int(G.size > 0 and int(G.max()) > MAX_EXACT_COUNT)
            P, info = (None, 0) if over else ease_invert_host(ease_system_host(G, reg))
            B = None if over else ease_weights_host(P)
        if over:
            raise OverflowError("EASE: a co-click count exceeds 2^24 and is not exact in float32")
        if info:
            raise FloatingPointError(f"EASE: pivot {info - 1} of the Cholesky factorisation was not positive: "
                                     f"regularization={self.regularization!r} is too small for these counts")
        self.weights = B
        return self

    @classmethod
    def from_weights(cls, article_ids, B, **kw) -> "EASE":
        """a fitted model from a given matrix B [n, n] (rows and columns in the order of ``article_ids``: any order, no repeats):
        ``predict``, ``recommend``, ``rank_targets`` and ``similar_items`` work; ``item_counts`` stays None"""
        ids = np.asarray(article_ids).ravel()
        B = np.asarray(B.cpu().numpy() if hasattr(B, "cpu") else B, np.float32)
        if B.ndim != 2 or B.shape != (ids.size, ids.size) or np.unique(ids).size != ids.size:
            raise ValueError("B must be [n, n] with one row and one column per distinct article id")
        if ids.size > MAX_ITEMS:
            raise ValueError(f"at most {MAX_ITEMS} articles, got {ids.size}")
        self = cls(**kw)
        order = np.argsort(ids, kind="stable")
        self.article_ids, B = ids[order], np.ascontiguousarray(B[np.ix_(order, order)])
        if device_available(self.device) and ids.size:
            import torch

            B = torch.from_numpy(B).to(self.device)
        self.weights = B
        return self

    def _fitted(self):
        if self.weights is None:
            raise RuntimeError("EASE.fit has not been called")
        return self.weights

    def host_weights(self) -> np.ndarray:
        """B as a contiguous float32 numpy array"""
        B = self._fitted()
        return B if isinstance(B, np.ndarray) else B.cpu().numpy()

    def rows_of(self, ids) -> np.ndarray:
        """int32 rows of B of a flat array of article ids, -1 for an article that was not kept"""
        self._fitted()
        return _rows_of(self.article_ids, ids)

    def _histories(self, histories):
        """ids of histories -> (rows int32, offsets int64, weights float32 | None)"""
        return history_operands(self.rows_of, histories, self.history_size, self.history_weights, self.lambda_factor)

    # -- recommend / rank_targets (TopN, _topn.py): ebn_ease_topk_f32 / ebn_ease_target_rank_f32 over B.  Every article has a score
    # for a user with a known history article; a user without one gets an empty list and rank 0
    def _topn_ids(self):
        self._fitted()
        return self.article_ids

    def _topn_rows_of(self, ids):
        return self.rows_of(ids)

    def _topn_session(self, histories):
        B = self._fitted()
        h_rows, h_off, w = self._histories(histories)
        on_device = not isinstance(B, np.ndarray) and device_available(self.device)
        return EaseSession(B if on_device else self.host_weights(), h_rows, h_off, w, on_device)

    # -- public
    def predict(self, candidates, histories=None, list_hist=None, *, history=None) -> RaggedLists:
        """float64 scores aligned with the candidate lists; the three call forms of ``ContentSimilarity.predict``:
        ``predict(behaviors, history=history_frame)`` joined on ``user_id``, ``predict(behaviors)`` with ``article_id_fixed`` per
        impression, ``predict(candidates, histories, list_hist=None)`` over RaggedLists or lists of lists of ids."""
        B = self._fitted()
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
        on_device = not isinstance(B, np.ndarray) and device_available(self.device)
        if on_device:
            import torch

            dev = B.device
            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            flat = scores_call(B, up(h_rows), up(w), up(h_off), up(list_hist), up(c_rows), up(c_off)).to(torch.float64)
        else:
            flat = ease_scores_host(self.host_weights(), h_rows, w, h_off, list_hist, c_rows, c_off)
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
        """(article ids, weights) of the ``n`` largest B[article, :] -- what a click on the article speaks for most (the article
        itself left out) -- ties by the smaller id.  Host side; KeyError for an article that was not kept."""
        B = self._fitted()
        r = int(self.rows_of(np.asarray([article_id]))[0])
        if r < 0:
            raise KeyError(article_id)
        row = (B[r] if isinstance(B, np.ndarray) else B[r].cpu().numpy()).astype(np.float64)
        others = np.flatnonzero(np.arange(row.size) != r)
        order = others[np.lexsort((others, -row[others]))][:max(int(n), 0)]  # the ids ascend with the rows
        return self.article_ids[order], row[order].astype(np.float32)
