"""Co-visitation baseline: "recommend what other readers of the same articles went on to read" -- item-to-item collaborative
filtering over the users' click sequences, the one baseline here that uses the behaviour of OTHER users.

    cv = CoVisitation(max_gap=3, symmetric=True, similarity="cosine", mode="sum").fit(df_history_train)
    scores = cv.predict(df_validation, history=df_history_validation)           # RaggedLists aligned with article_ids_inview
    DeviceMetricEvaluator(labels, scores, [AucScore(), MrrScore()]).evaluate()
    cv.neighbours(article_id, n=10)                                              # what followed this article most

COUNTS.  Over every sequence (oldest first) and every pair of positions i < j <= i + max_gap inside it whose articles are known and
differ, ``C[later, earlier] += 1`` (and ``C[earlier, later] += 1`` with ``symmetric``).  The matrix row is the article clicked
later, the column the one clicked before it: row c answers "after which articles was c read".
SIMILARITY.  With d_row[c] = sum_h C[c, h] and d_col[h] = sum_c C[c, h]:

    "count"        C[c, h]
    "cosine"       C[c, h] / sqrt(d_row[c] d_col[h])
    "conditional"  C[c, h] / d_col[h]                      the share of what followed h that was c

computed in float64 and rounded once to float32.
SCORES.  For a candidate c and a user's history h_1 .. h_H with weights w_j: ``sum_j w_j S[c, h_j]`` (mode "sum") or
``max_j w_j S[c, h_j]`` ("max") over the known history articles; an article that occurs twice counts twice.  ``fill`` is the
score of what cannot be scored, exactly where ``ContentSimilarity`` puts it: an unknown candidate, or a user without a single known
history article.  Histories, their weights, ``history_size`` and ``list_hist`` are those of content.py, whose helpers this module
uses.

TOP-N.  ``recommend`` / ``rank_targets`` (``TopN``, _topn.py) are the second outlet: each impression's best ``top_n`` of ALL fitted
articles, and the full-catalogue rank of its clicked article, under history exclusion and freshness windows.  Only articles that
were co-visited with at least one history article can be listed -- "never co-visited" is not "score 0" -- while a listed article may
have a negative score.  On the device they run ``ebn_cv_topk_f32`` / ``ebn_cv_target_rank_f32`` (csrc/ebn_covisit_topk.hip) over the
TRANSPOSED matrix (``CoVisitMatrix.transpose``, built at the first use); the numpy twins ``covisit_topk_host`` /
``covisit_target_rank_host`` do the same float32 arithmetic in the same history order and are bit-equal to the kernels.

Two paths, as in content.py.  With a visible GPU the pair keys come from ``ebn_cv_pair_keys_i64`` and the scores from
``ebn_cv_scores_f32`` (csrc/ebn_covisit.hip; contract in include/ebnerd_hip.h); between them torch sorts the keys, counts the
runs of equal ones and finds the row starts.  The sequences are cut into blocks whose keys stay within ``max_keys`` (never inside
a sequence) and the blocks' (key, count) runs are merged.  ``device=None`` or no GPU runs the numpy twins ``covisit_pair_keys_host``
/ ``covisit_matrix_host`` / ``covisit_values_host`` / ``covisit_scores_host``: the same contracts, float64 where values are involved.
numpy / pandas on the host; torch is imported only on the device path."""
from __future__ import annotations

import numpy as np

from ebrec.evaluation.device_metrics import RaggedLists, device_available
from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL

from ._topn import TopN
from .content import ContentSimilarity, _keep_last, _list_histories, _present_entries, history_weight_values
from .popularity import _explode, _frame, _ragged_ids, _rows_of

MAX_GAP = 64           # EBN_CV_MAX_GAP of include/ebnerd_hip.h
NO_PAIR = 2 ** 63 - 1  # EBN_CV_NO_PAIR
MAX_COUNT = 2 ** 31 - 1
SIMILARITIES = ("count", "cosine", "conditional")
MODES = ("sum", "max")
_CHUNK_PAIRS = 1 << 23  # (item, history entry) pairs covisit_scores_host materialises at a time


# ---- the numpy twins -----------------------------------------------------------------------------------------------------------
def _sequences(seq_rows, seq_offsets):
    rows, off = np.asarray(seq_rows, np.int64).ravel(), np.asarray(seq_offsets, np.int64).ravel()
    if off.size < 1 or off[0] != 0 or off[-1] > rows.size or np.any(np.diff(off) < 0):
        raise ValueError("sequence offsets must ascend from 0 to at most the number of entries")
    return rows, off


def _gap(max_gap, n_rows):
    if isinstance(max_gap, (bool, np.bool_)) or int(max_gap) != max_gap or not 1 <= int(max_gap) <= MAX_GAP:
        raise ValueError(f"max_gap must be an integer in [1, {MAX_GAP}], got {max_gap!r}")
    if not 0 <= int(n_rows) <= MAX_COUNT:
        raise ValueError(f"n_rows must lie in [0, 2^31 - 1], got {n_rows!r}")
    return int(max_gap), int(n_rows)


def covisit_pair_keys_host(seq_rows, seq_offsets, n_rows, max_gap, symmetric) -> np.ndarray:
    """numpy twin of ebn_cv_pair_keys_i64 -> keys [n_entries * K] int64, K = 2 max_gap with ``symmetric`` else max_gap"""
    rows, off = _sequences(seq_rows, seq_offsets)
    G, n_rows = _gap(max_gap, n_rows)
    n, K = rows.size, (2 * G if symmetric else G)
    keys = np.full((n, K), NO_PAIR, np.int64)
    end = np.zeros(n, np.int64)  # the end of the entry's sequence; 0: the entry belongs to none
    end[:int(off[-1])] = np.repeat(off[1:], np.diff(off))
    known = (rows >= 0) & (rows < n_rows)
    for g in range(1, min(G, n - 1) + 1):
        i = np.arange(n - g, dtype=np.int64)
        j = i + g
        ok = (j < end[i]) & known[i] & known[j] & (rows[i] != rows[j])
        i, j = i[ok], j[ok]
        keys[i, g - 1] = rows[j] * n_rows + rows[i]
        if symmetric:
            keys[i, G + g - 1] = rows[i] * n_rows + rows[j]
    return keys.ravel()


def sequence_blocks(seq_offsets, keys_per_entry: int, max_keys) -> list:
    """cuts [0, n_seqs] into blocks of whole sequences whose entries x ``keys_per_entry`` stay within ``max_keys``; a single
    sequence past the budget forms a block of its own -> the block boundaries [0, ..., n_seqs]"""
    off = np.asarray(seq_offsets, np.int64)
    n_seqs = off.size - 1
    if max_keys is None:
        return [0, n_seqs]
    if isinstance(max_keys, (bool, np.bool_)) or int(max_keys) != max_keys or int(max_keys) < 1:
        raise ValueError(f"max_keys must be a positive integer or None, got {max_keys!r}")
    budget = int(max_keys) // keys_per_entry  # entries of a block; 0: every sequence with an entry is a block of its own
    cut = [0]
    while cut[-1] < n_seqs:
        a = cut[-1]
        b = int(np.searchsorted(off, off[a] + budget, side="right")) - 1  # the last boundary within the budget
        cut.append(min(max(b, a + 1), n_seqs))
    return cut


def _merge_host(parts):
    """[(ascending distinct keys, counts int64)] -> one (ascending distinct keys, counts int64)"""
    parts = [p for p in parts if p[0].size]
    if not parts:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if len(parts) == 1:
        return parts[0]
    keys, cnt = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    order = np.argsort(keys, kind="stable")
    keys, cnt = keys[order], cnt[order]
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    return keys[starts], np.add.reduceat(cnt, starts)


def _csr_host(keys, cnt, n_rows):
    if cnt.size and int(cnt.max()) > MAX_COUNT:
        raise OverflowError(f"a pair was counted {int(cnt.max())} times: more than an int32 holds")
    row_of = keys // n_rows if n_rows else keys
    indptr = np.searchsorted(row_of, np.arange(n_rows + 1, dtype=np.int64)).astype(np.int64)
    return indptr, (keys % n_rows if n_rows else keys).astype(np.int32), cnt.astype(np.int32)


def covisit_matrix_host(seq_rows, seq_offsets, n_rows, max_gap, symmetric, max_keys=None):
    """the co-visitation counts as CSR -> (indptr [n_rows + 1] int64, cols int32 strictly ascending per row, counts int32):
    ``covisit_pair_keys_host`` per block of sequences (``max_keys``: as on the device path; None: one block), the sentinels
    dropped, equal keys counted, the blocks merged.  A count above 2^31 - 1 raises OverflowError."""
    rows, off = _sequences(seq_rows, seq_offsets)
    G, n_rows = _gap(max_gap, n_rows)
    cut = sequence_blocks(off, 2 * G if symmetric else G, max_keys)
    parts = []
    for a, b in zip(cut[:-1], cut[1:]):
        keys = covisit_pair_keys_host(rows[off[a]:off[b]], off[a:b + 1] - off[a], n_rows, G, symmetric)
        uniq, cnt = np.unique(keys[keys != NO_PAIR], return_counts=True)
        parts.append((uniq, cnt.astype(np.int64)))
    return _csr_host(*_merge_host(parts), n_rows)


def covisit_values_host(indptr, cols, counts, similarity) -> np.ndarray:
    """the similarity of every stored pair -> float32 [nnz] (float64 arithmetic, rounded once)"""
    if similarity not in SIMILARITIES:
        raise ValueError(f"similarity must be one of {SIMILARITIES}, got {similarity!r}")
    indptr, cols = np.asarray(indptr, np.int64), np.asarray(cols, np.int64)
    C = np.asarray(counts).astype(np.float64)
    n_rows = indptr.size - 1
    if similarity == "count" or C.size == 0:
        return C.astype(np.float32)
    row_of = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(indptr))
    d_col = np.bincount(cols, weights=C, minlength=n_rows)  # sums of integers below 2^53: exact in any order
    if similarity == "conditional":
        return (C / d_col[cols]).astype(np.float32)
    d_row = np.bincount(row_of, weights=C, minlength=n_rows)
    return (C / np.sqrt(d_row[row_of] * d_col[cols])).astype(np.float32)


def covisit_scores_host(indptr, cols, vals, hist_rows, hist_weights, hist_offsets, list_hist, cand_rows, cand_offsets, mode) -> np.ndarray:
    """numpy twin of ebn_cv_scores_f32 -> [n_items] float64: the (item, present entry) pairs in blocks, S[c, h] by one searchsorted
    over the composite keys ``row * n_rows + column`` of the matrix, a segmented float64 sum or max per item.  ``mode``: 0 / "sum"
    or 1 / "max"."""
    mode = {"sum": 0, "max": 1}.get(mode, mode)
    if mode not in (0, 1):
        raise ValueError(f"mode must be 0 / 'sum' or 1 / 'max', got {mode!r}")
    indptr, cols = np.asarray(indptr, np.int64).ravel(), np.asarray(cols, np.int64).ravel()
    vals = np.asarray(vals).astype(np.float64).ravel()
    n_rows = indptr.size - 1
    hist_rows, hist_offsets = _sequences(hist_rows, hist_offsets)
    cand_rows, cand_offsets = _sequences(cand_rows, cand_offsets)
    comp = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(indptr)) * n_rows + cols  # ascending: CSR with ascending columns
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
        b = max(a + 1, int(np.searchsorted(ends, done + _CHUNK_PAIRS, side="right")))
        i, c = items[a:b], count[items[a:b]]
        starts = np.cumsum(c) - c
        entry = np.arange(int(c.sum()), dtype=np.int64) - np.repeat(starts, c) + np.repeat(first[i], c)
        key = np.repeat(rows[i], c) * n_rows + h_rows[entry]
        pos = np.minimum(np.searchsorted(comp, key), max(comp.size - 1, 0))
        s = np.where(comp[pos] == key, vals[pos], 0.0) if comp.size else np.zeros(key.size)
        out[i] = (np.maximum if mode == 1 else np.add).reduceat(h_w[entry] * s, starts)
        a = b
    return out


# ---- top-N over the whole catalogue: the numpy twins of ebn_cv_topk_f32 / ebn_cv_target_rank_f32 ---------------------------------
MAX_TOP_K, MAX_EXCLUDE, NO_POSITION = 64, 256, 2 ** 31 - 1  # limits of include/ebnerd_hip.h; the position of an empty list slot


def covisit_transpose_host(indptr, cols, vals):
    """the transpose of a square CSR matrix with ascending columns -> (t_indptr int64, t_cols int32 ascending per row, t_vals):
    row h of the result holds every row c with a stored entry (c, h), and its value"""
    indptr, cols, vals = np.asarray(indptr, np.int64).ravel(), np.asarray(cols).ravel(), np.asarray(vals).ravel()
    n = indptr.size - 1
    row_of = np.repeat(np.arange(n, dtype=np.int32), np.diff(indptr))
    order = np.argsort(cols, kind="stable")  # stable: the rows of one column stay ascending
    t_indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(cols, minlength=n)[:n], out=t_indptr[1:])
    return t_indptr, row_of[order], vals[order]


def covisit_transpose_device(indptr, cols, vals):
    """``covisit_transpose_host`` in torch on the matrix's device"""
    import torch

    n = indptr.numel() - 1
    row_of = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=cols.device), indptr[1:] - indptr[:-1])
    key, order = torch.sort(cols.long(), stable=True)
    t_indptr = torch.zeros(n + 1, dtype=torch.int64, device=cols.device)
    t_indptr[1:] = torch.cumsum(torch.bincount(key, minlength=n)[:n], 0)
    return t_indptr, row_of[order].contiguous(), vals[order].contiguous()


def _chain_host(t_indptr, t_cols, t_vals, rows, weights, mode):
    """one user's scores over the whole catalogue in the kernel's arithmetic -> (touched [n_rows] bool, score [n_rows] float32):
    the history entries in order, vectorised over the rows of each; every product and every add rounds once to float32"""
    n_rows, nnz = t_indptr.size - 1, t_cols.size
    touched, score = np.zeros(n_rows, bool), np.zeros(n_rows, np.float32)
    with np.errstate(all="ignore"):
        for j, h in enumerate(np.asarray(rows).tolist()):
            if not 0 <= h < n_rows:
                continue
            a, b = (min(max(int(v), 0), nnz) for v in (t_indptr[h], t_indptr[h + 1]))
            if a >= b:
                continue
            c = t_cols[a:b]
            p = (np.float32(1.0) if weights is None else np.float32(weights[j])) * t_vals[a:b].astype(np.float32)
            old = score[c]
            later = np.where((p > old) | np.isnan(p), p, old) if mode == 1 else old + p
            score[c] = np.where(touched[c], later, p).astype(np.float32)
            touched[c] = True
    return touched, score


def covisit_chains_host(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, mode) -> list:
    """[(touched [n_rows] bool, score [n_rows] float32)] per history: the part of the twins that depends on neither the candidates
    nor the windows nor the exclusion lists (``chains=`` of both twins takes it, so that several calls share it)"""
    mode = {"sum": 0, "max": 1}.get(mode, mode)
    if mode not in (0, 1):
        raise ValueError(f"mode must be 0 / 'sum' or 1 / 'max', got {mode!r}")
    t_indptr, t_cols = np.asarray(t_indptr, np.int64).ravel(), np.asarray(t_cols, np.int64).ravel()
    t_vals = np.asarray(t_vals, np.float32).ravel()
    hist_rows, hist_offsets = np.asarray(hist_rows, np.int64).ravel(), np.asarray(hist_offsets, np.int64).ravel()
    out = []
    for h in range(hist_offsets.size - 1):
        a, b = (min(max(int(v), 0), hist_rows.size) for v in (hist_offsets[h], hist_offsets[h + 1]))
        w = None if hist_weights is None else np.asarray(hist_weights, np.float32).ravel()[a:b]
        out.append(_chain_host(t_indptr, t_cols, t_vals, hist_rows[a:b], w, mode))
    return out


def _walk_host(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, window, exclude, mode,
               chains=None):
    """per user: (admissible rows, their positions, the float32 scores of all rows), and the two flags at the end"""
    if chains is None:
        chains = covisit_chains_host(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, mode)
    n_rows, n_hists = np.asarray(t_indptr).size - 1, len(chains)
    pos_of = np.arange(n_rows, dtype=np.int64) if cand_pos is None else np.asarray(cand_pos, np.int64).ravel()
    if pos_of.size != n_rows or (cand_pos is None and M != n_rows):
        raise ValueError(f"cand_pos must hold one position per catalogue row ({n_rows}); without it M == n_rows")
    flags = np.zeros(2, np.int32)
    for u in range(int(n_users)):
        h = u if user_hist is None else int(user_hist[u])
        touched, score = np.zeros(n_rows, bool), np.zeros(n_rows, np.float32)
        if 0 <= h < n_hists:
            touched, score = chains[h]
        lo, hi = 0, int(M)
        if window is not None:
            lo, hi = max(int(window[u][0]), 0), min(int(window[u][1]), int(M))
            if lo >= hi:
                lo = hi = 0
        if (touched & (pos_of >= M)).any():
            flags[0] = 1
        adm = touched & (pos_of >= lo) & (pos_of < hi)
        if exclude is not None:
            ex = np.asarray(exclude[u], np.int64).ravel()
            adm[ex[(ex >= 0) & (ex < n_rows)]] = False
        if (adm & np.isnan(score)).any():
            flags[1] = 1
        adm &= ~np.isnan(score)
        rows = np.flatnonzero(adm)
        yield u, rows, pos_of[rows], score, flags


def covisit_topk_host(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, window, exclude,
                      k, mode, chains=None):
    """numpy twin of ebn_cv_topk_f32, bit-equal to it -> (pos [U, k] int32, score [U, k] float32, flags [2] int32)"""
    if not 1 <= int(k) <= MAX_TOP_K:
        raise ValueError(f"k must lie in [1, {MAX_TOP_K}], got {k}")
    out_pos, out_score = np.full((int(n_users), int(k)), -1, np.int32), np.full((int(n_users), int(k)), -np.inf, np.float32)
    flags = np.zeros(2, np.int32)
    for u, rows, pos, score, flags in _walk_host(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos,
                                                 M, window, exclude, mode, chains):
        s = score[rows]
        best = np.lexsort((pos, -s))[:int(k)]  # score descending, then position ascending
        out_pos[u, :best.size], out_score[u, :best.size] = pos[best], s[best]
    return out_pos, out_score, flags


def covisit_target_rank_host(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, target_pos,
                             window, exclude, mode, chains=None):
    """numpy twin of ebn_cv_target_rank_f32 -> (rank [U] int32, count [U] int32, score [U] float32, flags [2] int32)"""
    target_pos = np.asarray(target_pos, np.int64).ravel()
    U = int(n_users)
    rank, count, t_out = np.zeros(U, np.int32), np.zeros(U, np.int32), np.full(U, -np.inf, np.float32)
    flags, oob_target = np.zeros(2, np.int32), bool((target_pos[:U] >= M).any())
    for u, rows, pos, score, flags in _walk_host(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos,
                                                 M, window, exclude, mode, chains):
        count[u] = rows.size
        at = np.flatnonzero(pos == target_pos[u]) if 0 <= target_pos[u] < M else np.zeros(0, np.int64)
        if at.size:
            s, t = score[rows], score[rows[at[0]]]
            rank[u] = 1 + int(((s > t) | ((s == t) & (pos < target_pos[u]))).sum())
            t_out[u] = t
    if oob_target:
        flags[0] = 1
    return rank, count, t_out, flags


# ---- the matrix ----------------------------------------------------------------------------------------------------------------
class CoVisitMatrix:
    """``article_ids`` (sorted, numpy) name the rows and columns; ``indptr`` int64 [n_rows + 1], ``cols`` int32, ``counts`` int32 and
    ``vals`` float32 are CSR: device tensors on the device path, numpy arrays on the host path (``host()`` gives numpy either way)."""

    def __init__(self, article_ids, indptr, cols, counts, vals):
        self.article_ids, self.indptr, self.cols, self.counts, self.vals = article_ids, indptr, cols, counts, vals
        self._host = self._transpose = self._transpose_host = None

    def transpose(self):
        """(t_indptr, t_cols, t_vals): the transposed CSR the catalogue kernels walk, where the matrix lives (device tensors on the
        device path); built at the first use and kept"""
        if self._transpose is None:
            build = covisit_transpose_device if self.on_device else covisit_transpose_host
            self._transpose = build(self.indptr, self.cols, self.vals)
        return self._transpose

    def transpose_host(self):
        """the same as numpy arrays, downloaded (or built) once"""
        if self._transpose_host is None:
            t = self.transpose()
            self._transpose_host = tuple(p.cpu().numpy() for p in t) if self.on_device else t
        return self._transpose_host

    @property
    def on_device(self) -> bool:
        return not isinstance(self.indptr, np.ndarray)

    @property
    def n_rows(self) -> int:
        return len(self.article_ids)

    @property
    def nnz(self) -> int:
        return int(self.cols.shape[0])

    def host(self):
        """(indptr, cols, counts, vals) as numpy arrays, downloaded once"""
        if self._host is None:
            parts = (self.indptr, self.cols, self.counts, self.vals)
            self._host = tuple(p.cpu().numpy() for p in parts) if self.on_device else parts
        return self._host


def pair_keys_call(seq_rows, seq_offsets, n_rows, max_gap, symmetric):
    """One ebn_cv_pair_keys_i64 launch over device tensors (int32 rows, int64 offsets) -> keys [n_entries * K] int64 on the device"""
    import torch

    from ebrec import _hip

    n, K = seq_rows.numel(), (2 * int(max_gap) if symmetric else int(max_gap))
    keys = torch.empty(n * K, dtype=torch.int64, device=seq_rows.device)
    with torch.cuda.device(seq_rows.device):
        _hip.call("ebn_cv_pair_keys_i64", _hip.ptr(seq_rows), _hip.ptr(seq_offsets), seq_offsets.numel() - 1, n, int(n_rows), int(max_gap),
                  1 if symmetric else 0, _hip.ptr(keys), _hip.stream_handle())
    return keys


def _runs_device(keys):
    """keys (any order, with sentinels) -> (ascending distinct keys, counts int64)"""
    import torch

    keys = torch.sort(keys).values
    n_valid = int(torch.searchsorted(keys, torch.tensor([NO_PAIR], dtype=torch.int64, device=keys.device)))
    return torch.unique_consecutive(keys[:n_valid], return_counts=True)


def covisit_matrix_device(seq_rows, seq_offsets, n_rows, max_gap, symmetric, max_keys=2 ** 27, device="cuda"):
    """the device build of ``covisit_matrix_host`` -> (indptr int64, cols int32, counts int32) tensors: per block of sequences one
    ebn_cv_pair_keys_i64 launch, torch.sort, the sentinels cut off, unique_consecutive with counts; the blocks' runs concatenated,
    sorted by key and reduced again; rows and columns are ``// n_rows`` and ``% n_rows``, indptr one searchsorted."""
    import torch

    rows, off = _sequences(seq_rows, seq_offsets)
    G, n_rows = _gap(max_gap, n_rows)
    dev = torch.device(device)
    cut = sequence_blocks(off, 2 * G if symmetric else G, max_keys)
    rows_d = torch.from_numpy(rows.astype(np.int32)).to(dev)
    parts = []
    for a, b in zip(cut[:-1], cut[1:]):
        if off[b] == off[a]:
            continue
        off_d = torch.from_numpy(off[a:b + 1] - off[a]).to(dev)
        parts.append(_runs_device(pair_keys_call(rows_d[int(off[a]):int(off[b])], off_d, n_rows, G, symmetric)))
    if not parts:
        keys, cnt = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
    elif len(parts) == 1:
        keys, cnt = parts[0]
    else:
        keys, order = torch.sort(torch.cat([p[0] for p in parts]))
        keys, inverse = torch.unique_consecutive(keys, return_inverse=True)
        cnt = torch.zeros(keys.numel(), dtype=torch.int64, device=dev).index_add_(0, inverse, torch.cat([p[1] for p in parts])[order])
    if cnt.numel() and int(cnt.max()) > MAX_COUNT:
        raise OverflowError(f"a pair was counted {int(cnt.max())} times: more than an int32 holds")
    row_of = torch.div(keys, max(n_rows, 1), rounding_mode="floor")
    indptr = torch.searchsorted(row_of, torch.arange(n_rows + 1, dtype=torch.int64, device=dev))
    return indptr, (keys - row_of * max(n_rows, 1)).to(torch.int32), cnt.to(torch.int32)


def covisit_values_device(indptr, cols, counts, similarity):
    """``covisit_values_host`` in torch on the matrix's device: float64 arithmetic, rounded once to float32"""
    import torch

    if similarity not in SIMILARITIES:
        raise ValueError(f"similarity must be one of {SIMILARITIES}, got {similarity!r}")
    C = counts.to(torch.float64)
    n_rows = indptr.numel() - 1
    if similarity == "count" or C.numel() == 0:
        return C.to(torch.float32)
    c = cols.long()
    d_col = torch.zeros(n_rows, dtype=torch.int64, device=C.device).index_add_(0, c, counts.long()).to(torch.float64)
    if similarity == "conditional":
        return (C / d_col[c]).to(torch.float32)
    row_of = torch.repeat_interleave(torch.arange(n_rows, device=C.device), indptr[1:] - indptr[:-1])
    d_row = torch.zeros(n_rows, dtype=torch.int64, device=C.device).index_add_(0, row_of, counts.long()).to(torch.float64)
    return (C / torch.sqrt(d_row[row_of] * d_col[c])).to(torch.float32)


def scores_call(indptr, cols, vals, hist_rows, hist_weights, hist_offsets, list_hist, cand_rows, cand_offsets, mode):
    """One ebn_cv_scores_f32 launch over device tensors -> scores [n_items] float32 on the device (``hist_weights`` / ``list_hist``
    may be None)"""
    import torch

    from ebrec import _hip

    scores = torch.empty(cand_rows.numel(), dtype=torch.float32, device=cand_rows.device)
    with torch.cuda.device(cand_rows.device):
        _hip.call("ebn_cv_scores_f32", _hip.ptr(indptr), _hip.ptr(cols), _hip.ptr(vals), indptr.numel() - 1, cols.numel(), _hip.ptr(hist_rows),
                  _hip.ptr(hist_weights), _hip.ptr(hist_offsets), hist_offsets.numel() - 1, hist_rows.numel(), _hip.ptr(list_hist),
                  _hip.ptr(cand_rows), _hip.ptr(cand_offsets), cand_offsets.numel() - 1, cand_rows.numel(), int(mode), _hip.ptr(scores),
                  _hip.stream_handle())
    return scores


def _cv_operands(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, user_hist, cand_pos, M):
    from ebrec import _hip

    n_rows = t_indptr.numel() - 1
    M = n_rows if cand_pos is None else int(M)
    return (_hip.ptr(t_indptr), _hip.ptr(t_cols), _hip.ptr(t_vals), n_rows, t_cols.numel(), _hip.ptr(hist_rows), _hip.ptr(hist_weights),
            _hip.ptr(hist_offsets), hist_offsets.numel() - 1, hist_rows.numel(), _hip.ptr(user_hist), _hip.ptr(cand_pos), M), n_rows


def _check_device_args(U, window, exclude, target_pos=None):
    import torch

    for name, t, shape in (("window", window, (U, 2)), ("exclude", exclude, None), ("target_pos", target_pos, (U,))):
        if t is None:
            continue
        if t.dtype != torch.int32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape) or \
                (shape is None and (t.dim() != 2 or t.shape[0] != U)):
            raise ValueError(f"{name} must be a contiguous int32 tensor with one row per user ({U}), got {tuple(t.shape)} {t.dtype}")


def topk_call(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, window, exclude, k, mode,
              flags, n_splits: int = 0):
    """One ebn_cv_topk_f32 launch over device tensors (``hist_weights`` / ``user_hist`` / ``cand_pos`` / ``window`` [U, 2] /
    ``exclude`` [U, X] may be None) -> (pos [U, k] int32, score [U, k] float32); ``flags`` [2] int32 accumulates."""
    import torch

    from ebrec import _hip

    U, dev = int(n_users), t_indptr.device
    _check_device_args(U, window, exclude)
    ops, n_rows = _cv_operands(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, user_hist, cand_pos, M)
    pos = torch.empty(U, k, dtype=torch.int32, device=dev)
    score = torch.empty(U, k, dtype=torch.float32, device=dev)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_cv_topk_auto_splits(U, n_rows))
    ws = torch.empty(max(int(lib.ebn_cv_topk_workspace_bytes(U, k, max(splits, 1))), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("ebn_cv_topk_f32", *ops, _hip.ptr(window), _hip.ptr(exclude), 0 if exclude is None else exclude.shape[1], int(k), int(mode),
                  splits, _hip.ptr(pos), _hip.ptr(score), _hip.ptr(flags), _hip.ptr(ws), ws.numel(), U, _hip.stream_handle())
    return pos, score


def target_rank_call(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, user_hist, n_users, cand_pos, M, target_pos, window,
                     exclude, mode, flags, n_splits: int = 0):
    """One ebn_cv_target_rank_f32 launch over device tensors: ``target_pos`` [U] int32 candidate positions (< 0: none) -> (rank [U]
    int32: 1-based place in ``topk_call``'s order, 0 = not ranked; count [U] int32: the user's admissible rows; score [U] float32:
    the target's score, -inf where rank is 0); ``flags`` accumulates."""
    import torch

    from ebrec import _hip

    U, dev = int(n_users), t_indptr.device
    _check_device_args(U, window, exclude, target_pos)
    ops, n_rows = _cv_operands(t_indptr, t_cols, t_vals, hist_rows, hist_weights, hist_offsets, user_hist, cand_pos, M)
    rank = torch.empty(U, dtype=torch.int32, device=dev)
    count = torch.empty(U, dtype=torch.int32, device=dev)
    score = torch.empty(U, dtype=torch.float32, device=dev)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_cv_topk_auto_splits(U, n_rows))
    ws = torch.empty(max(int(lib.ebn_cv_target_rank_workspace_bytes(U, max(splits, 1), 0 if cand_pos is None else int(M))), 16),
                     dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("ebn_cv_target_rank_f32", *ops, _hip.ptr(target_pos), _hip.ptr(window), _hip.ptr(exclude),
                  0 if exclude is None else exclude.shape[1], int(mode), splits, _hip.ptr(rank), _hip.ptr(count), _hip.ptr(score),
                  _hip.ptr(flags), _hip.ptr(ws), ws.numel(), U, _hip.stream_handle())
    return rank, count, score


class _CoVisitSession:
    """what ``TopN`` drives (see _topn.py): the histories of one ``recommend`` / ``rank_targets`` call against the transposed matrix;
    device tensors and the two kernels when the matrix lives on the device, the float32 twins otherwise"""

    def __init__(self, matrix: CoVisitMatrix, h_rows, h_off, w, mode: int, on_device: bool):
        self.on_device, self.mode, self.n_rows = on_device, mode, matrix.n_rows
        self.cand_pos, self.M = None, matrix.n_rows
        if on_device:
            import torch

            self.device = matrix.indptr.device
            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            self.t = matrix.transpose()
            self.hist = (up(h_rows.astype(np.int32)), up(w), up(np.ascontiguousarray(h_off, dtype=np.int64)))
        else:
            self.t = matrix.transpose_host()
            self.hist = (h_rows, w, np.ascontiguousarray(h_off, dtype=np.int64))
            self.chains = covisit_chains_host(*self.t, *self.hist, mode)  # once for every batch of the call

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
            pos, score, f = covisit_topk_host(*self.t, *self.hist, hist_idx, U, self.cand_pos, self.M, window, exclude, k, self.mode,
                                              self.chains)
            flags |= f
            return pos, score
        return topk_call(*self.t, *self.hist, self._up(hist_idx), U, self.cand_pos, self.M, self._up(window), self._up(exclude), k,
                         self.mode, flags)

    def rank(self, hist_idx, target_pos, window, exclude, flags):
        U = len(hist_idx)
        if not self.on_device:
            rank, count, score, f = covisit_target_rank_host(*self.t, *self.hist, hist_idx, U, self.cand_pos, self.M, target_pos, window,
                                                             exclude, self.mode, self.chains)
            flags |= f
            return rank, count, score
        return target_rank_call(*self.t, *self.hist, self._up(hist_idx), U, self.cand_pos, self.M, self._up(target_pos), self._up(window),
                                self._up(exclude), self.mode, flags)


# ---- the class -----------------------------------------------------------------------------------------------------------------
class CoVisitation(TopN):
    """Item-to-item co-visitation scores.  ``max_gap``: how many later clicks of a sequence an article is paired with (1 to 64);
    ``symmetric``: count every pair in both directions; ``similarity``: "count", "cosine" or "conditional"; ``mode``: "sum" or
    "max" over the history; ``history_weights`` / ``lambda_factor`` / ``history_size`` / ``fill``: as in ``ContentSimilarity``;
    ``max_keys``: the pair keys one block of the device build may hold (8 bytes each)."""

    def __init__(self, max_gap: int = 3, symmetric: bool = True, similarity: str = "cosine", mode: str = "sum", history_weights=None,
                 lambda_factor: float = 0.9, history_size=None, fill: float = 0.0, device="cuda", max_keys=2 ** 27):
        _gap(max_gap, 0)
        if similarity not in SIMILARITIES:
            raise ValueError(f"similarity must be one of {SIMILARITIES}, got {similarity!r}")
        if mode not in MODES:
            raise ValueError(f"mode must be 'sum' or 'max', got {mode!r}")
        if not (history_weights is None or callable(history_weights) or history_weights in ("linear", "exponential")):
            raise ValueError(f"history_weights must be None, 'linear', 'exponential' or a callable, got {history_weights!r}")
        if history_size is not None and (isinstance(history_size, bool) or int(history_size) != history_size or history_size < 1):
            raise ValueError(f"history_size must be a positive integer or None, got {history_size!r}")
        sequence_blocks(np.zeros(1, np.int64), 1, max_keys)  # validates max_keys
        self.max_gap, self.symmetric, self.similarity, self.mode = int(max_gap), bool(symmetric), similarity, mode
        self.history_weights, self.lambda_factor = history_weights, float(lambda_factor)
        self.history_size, self.fill, self.device = (None if history_size is None else int(history_size)), float(fill), device
        self.max_keys = None if max_keys is None else int(max_keys)
        self.matrix = None

    # -- fit
    def fit(self, sequences) -> "CoVisitation":
        """``fit(history_frame)``: one sequence per row of its ``article_id_fixed``; ``fit(sequences)``: a RaggedLists or lists of
        lists of article ids, oldest first.  Returns self."""
        df = sequences if isinstance(sequences, RaggedLists) else _frame(sequences)
        if hasattr(df, "columns"):
            if DEFAULT_HISTORY_ARTICLE_ID_COL not in df.columns:
                raise ValueError(f"the frame lacks the column '{DEFAULT_HISTORY_ARTICLE_ID_COL}'")
            flat, off = _explode(df[DEFAULT_HISTORY_ARTICLE_ID_COL])
        else:
            flat, off = _ragged_ids(df)
        flat, off = np.asarray(flat).ravel(), np.ascontiguousarray(off, dtype=np.int64)
        if flat.size and flat.dtype.kind not in "iuUS":
            raise TypeError(f"CoVisitation needs ids that are all strings or all integers, got dtype {flat.dtype}")
        ids = np.unique(flat)
        rows = _rows_of(ids, flat)
        if device_available(self.device) and ids.size:
            indptr, cols, counts = covisit_matrix_device(rows, off, ids.size, self.max_gap, self.symmetric, self.max_keys, self.device)
            vals = covisit_values_device(indptr, cols, counts, self.similarity)
        else:
            indptr, cols, counts = covisit_matrix_host(rows, off, ids.size, self.max_gap, self.symmetric, self.max_keys)
            vals = covisit_values_host(indptr, cols, counts, self.similarity)
        self.matrix = CoVisitMatrix(ids, indptr, cols, counts, vals)
        return self

    def _fitted(self) -> CoVisitMatrix:
        if self.matrix is None:
            raise RuntimeError("CoVisitation.fit has not been called")
        return self.matrix

    def rows_of(self, ids) -> np.ndarray:
        """int32 matrix rows of a flat array of article ids, -1 for an article no sequence held"""
        return _rows_of(self._fitted().article_ids, ids)

    def _histories(self, histories):
        """ids of histories -> (rows int32, offsets int64, weights float32 | None): ContentSimilarity._histories over this matrix"""
        flat, offsets = _ragged_ids(histories)
        if self.history_size is not None:
            flat, offsets = _keep_last(flat, offsets, self.history_size)
        w = history_weight_values(self.history_weights, offsets, self.lambda_factor)
        return self.rows_of(flat), np.ascontiguousarray(offsets, dtype=np.int64), (None if w is None else w.astype(np.float32))

    # -- recommend / rank_targets (TopN, _topn.py): ebn_cv_topk_f32 / ebn_cv_target_rank_f32 over the transposed matrix.  A row no
    # history article was ever co-visited with is never listed; a row with a negative score is
    def _topn_ids(self):
        return self._fitted().article_ids

    def _topn_rows_of(self, ids):
        return self.rows_of(ids)

    def _topn_session(self, histories):
        m = self._fitted()
        h_rows, h_off, w = self._histories(histories)
        return _CoVisitSession(m, h_rows, h_off, w, MODES.index(self.mode), m.on_device and device_available(self.device))

    # -- public
    def predict(self, candidates, histories=None, list_hist=None, *, history=None) -> RaggedLists:
        """float64 scores aligned with the candidate lists; the three call forms of ``ContentSimilarity.predict``:
        ``predict(behaviors, history=history_frame)`` joined on ``user_id``, ``predict(behaviors)`` with ``article_id_fixed`` per
        impression, ``predict(candidates, histories, list_hist=None)`` over RaggedLists or lists of lists of ids."""
        m = self._fitted()
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
        mode = MODES.index(self.mode)
        on_device = m.on_device and device_available(self.device)
        if on_device:
            import torch

            dev = m.indptr.device
            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            flat = scores_call(m.indptr, m.cols, m.vals, up(h_rows), up(w), up(h_off), up(list_hist), up(c_rows), up(c_off), mode).to(torch.float64)
        else:
            flat = covisit_scores_host(*m.host()[:2], m.host()[3], h_rows, w, h_off, list_hist, c_rows, c_off, mode)
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

    def neighbours(self, article_id, n: int = 10):
        """(article ids, values) of the ``n`` largest values of the article's matrix row -- after which articles it was read most
        (with ``symmetric``: and before which) -- ties by the smaller id.  Host side; KeyError for an article no sequence held."""
        m = self._fitted()
        r = int(self.rows_of(np.asarray([article_id]))[0])
        if r < 0:
            raise KeyError(article_id)
        indptr, cols, _, vals = m.host()
        c, v = cols[indptr[r]:indptr[r + 1]], vals[indptr[r]:indptr[r + 1]]
        order = np.lexsort((c, -v.astype(np.float64)))[:max(int(n), 0)]  # the ids ascend with the columns
        return m.article_ids[c[order]], v[order]
