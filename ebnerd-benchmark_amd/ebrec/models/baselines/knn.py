"""History-kNN baseline: "find the readers whose click sequences look most like this one, and recommend what they read" --
neighbourhood collaborative filtering over WHOLE click sequences (S-KNN / V-SKNN: Jannach & Ludewig 2017, Ludewig & Jannach 2018),
beside the item-to-item ``CoVisitation`` and the latent ``ImplicitALS``.

    knn = HistoryKNN(k=100, sample_size=1000, similarity="cosine", history_weights="linear").fit(df_history_train)
    scores = knn.predict(df_validation, history=df_history)                      # RaggedLists aligned with article_ids_inview
    seqs, sims = knn.neighbours(histories)                                       # [n_hists, k] input rows of the fitted sequences
    knn.index                                                                    # postings + sets, .article_ids, .sequence_of, .keys

FITTED DATA.  The training sequences are ordered by recency (a frame with ``impression_time_fixed``: the sequence's last time; a
frame without it: row order; lists: ``recency=`` or input order; ties by input order) and numbered: sequence id ``s`` ascends from
the oldest to the most recent; ``index.sequence_of[s]`` is its input row, ``index.keys[s]`` its key (the frame's ``user_id``).  Two
CSR structures are built once: POSTINGS (per article row the distinct sequences that hold it, ascending) and SETS (per sequence its
distinct rows, ascending).
QUERY.  A history's items are its distinct known articles; an item takes the weight of its LAST occurrence and the items keep the
order of those occurrences.  Weights, ``history_size`` and ``list_hist`` are those of content.py.
NEIGHBOURS.  Of all sequences that share an item with the query (never the user's own one, ``exclude_self``) the ``sample_size``
most recent are the candidates; ``sim = sum of the weights of the shared items`` ("dot"), times ``1 / sqrt(|set(s)|)`` ("cosine"; the
query's own norm is the same for all candidates and left out); the best ``k`` by sim, then by recency, are the neighbours.
SCORES.  ``score(c) = idf(c) * sum of the sims of the neighbours that hold c``, ``idf(c) = log(n_seqs / df(c))`` with ``idf=True``, else
1.  ``fill`` is the score of what cannot be scored, exactly where ``CoVisitation`` puts it: an unknown candidate, or a user without
a single known history article.

Two paths, as in covisit.py.  With a visible GPU the neighbours come from ``ebn_knn_neighbours_f32`` and the scores from
``ebn_knn_scores_f32`` (csrc/ebn_knn.hip; contract in include/ebnerd_hip.h): one launch over the histories, one over the items; the
index is built by torch (composite int64 keys, sort, unique_consecutive, searchsorted) in blocks of at most ``max_keys`` keys.
``device=None`` or no GPU runs the numpy twins ``knn_index_host`` / ``knn_neighbours_host`` (float32 adds in item order: bit-equal to
the kernel) / ``knn_scores_host`` (float64).  numpy / pandas on the host; torch is imported only on the device path.

TOP-N.  ``recommend`` / ``rank_targets`` (``TopN``, _topn.py) are the second outlet: each impression's best ``top_n`` of ALL fitted
articles, and the full-catalogue rank of its clicked article, under history exclusion and freshness windows; ``exclude_self`` holds
as in ``predict`` (frames joined on ``user_id`` match on that key, the list form takes ``history_keys=``).  Only an article some
neighbour read has a score: a history without neighbours gets an empty list and rank 0.  The neighbour search runs ONCE per call;
on the device the lists and ranks come from ``ebn_knn_topk_f32`` / ``ebn_knn_target_rank_f32`` (csrc/ebn_knn_topk.hip), which walk
the neighbours' sets instead of searching them.  The numpy twins ``knn_topk_host`` / ``knn_target_rank_host`` add the sims in float32
in neighbour-list order, vectorised over the rows of one neighbour, and are bit-equal to the kernels.  That chain is not the
summation order of ``ebn_knn_scores_f32``: ``return_scores`` and ``predict`` agree to rounding, not in bits."""
from __future__ import annotations

import numpy as np

from ebrec.evaluation.device_metrics import RaggedLists, device_available
from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_HISTORY_IMPRESSION_TIMESTAMP_COL, DEFAULT_USER_COL

from ._topn import TopN
from .content import ContentSimilarity, _list_histories, history_operands, join_frames
from .covisit import _sequences
from .popularity import _explode, _frame, _ragged_ids, _rows_of

MAX_K, MAX_SAMPLE = 512, 4096  # EBN_KNN_MAX_K / EBN_KNN_MAX_SAMPLE of include/ebnerd_hip.h
MAX_DIM = 2 ** 31 - 1
SIMILARITIES = ("dot", "cosine")
_CHUNK_PAIRS = 1 << 23  # (item, neighbour) pairs knn_scores_host materialises at a time
MAX_TOP_K, MAX_EXCLUDE = 64, 256  # limits of the top-N kernels (include/ebnerd_hip.h)


def _limits(k, sample_size):
    for name, v in (("k", k), ("sample_size", sample_size)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an integer, got {v!r}")
    if not 1 <= sample_size <= MAX_SAMPLE:
        raise ValueError(f"sample_size must lie in [1, {MAX_SAMPLE}], got {sample_size}")
    if not 1 <= k <= min(MAX_K, sample_size):
        raise ValueError(f"k must lie in [1, min({MAX_K}, sample_size)], got {k} with sample_size {sample_size}")
    return int(k), int(sample_size)


def _max_keys(max_keys):
    if max_keys is None:
        return None
    if isinstance(max_keys, (bool, np.bool_)) or int(max_keys) != max_keys or int(max_keys) < 2:
        raise ValueError(f"max_keys must be an integer of at least 2 or None, got {max_keys!r}")
    return int(max_keys)


# ---- the numpy twins -----------------------------------------------------------------------------------------------------------
def _csr_of_keys(keys, n_major, n_minor):
    """ascending distinct composite keys ``major * n_minor + minor`` -> (indptr [n_major + 1] int64, minors int32)"""
    major = keys // max(n_minor, 1)
    indptr = np.searchsorted(major, np.arange(n_major + 1, dtype=np.int64)).astype(np.int64)
    return indptr, (keys - major * max(n_minor, 1)).astype(np.int32)


def knn_index_host(seq_rows, seq_offsets, n_rows, max_keys=None):
    """the two CSR structures of sequences (rows outside [0, n_rows) are skipped) -> (p_indptr [n_rows + 1] int64, p_seqs int32,
    s_indptr [n_seqs + 1] int64, s_items int32): composite keys ``row * n_seqs + seq`` and ``seq * n_rows + row`` per block of at most
    ``max_keys // 2`` entries, np.unique, the blocks' keys merged by another np.unique"""
    rows, off = _sequences(seq_rows, seq_offsets)
    n_rows, n_seqs, n = int(n_rows), off.size - 1, int(off[-1])
    if not (0 <= n_rows <= MAX_DIM and n_seqs <= MAX_DIM):
        raise ValueError("n_rows and the number of sequences must lie in [0, 2^31 - 1]")
    seq_of = np.repeat(np.arange(n_seqs, dtype=np.int64), np.diff(off))
    step = n if _max_keys(max_keys) is None else max(1, int(max_keys) // 2)
    pk, sk = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for a in range(0, n, max(step, 1)):
        r, s = rows[a:a + step], seq_of[a:a + step]
        ok = (r >= 0) & (r < n_rows)
        pk.append(np.unique(r[ok] * n_seqs + s[ok]))
        sk.append(np.unique(s[ok] * n_rows + r[ok]))
    return _csr_of_keys(np.unique(np.concatenate(pk)), n_rows, n_seqs) + _csr_of_keys(np.unique(np.concatenate(sk)), n_seqs, n_rows)


def knn_seq_scale_host(s_indptr) -> np.ndarray:
    """1 / sqrt(|set(s)|) in float64, rounded once to float32; 0 for an empty sequence (it is nobody's candidate)"""
    n = np.diff(np.asarray(s_indptr, np.int64)).astype(np.float64)
    return np.where(n > 0, 1.0 / np.sqrt(np.maximum(n, 1.0)), 0.0).astype(np.float32)


def knn_idf_host(p_indptr, n_seqs) -> np.ndarray:
    """log(n_seqs / df) in float64, rounded once to float32; 0 for a row no sequence holds"""
    df = np.diff(np.asarray(p_indptr, np.int64)).astype(np.float64)
    return np.where(df > 0, np.log(float(n_seqs) / np.maximum(df, 1.0)), 0.0).astype(np.float32)


def query_items(rows, weights, n_rows):
    """one history's entries -> (item rows, float32 weights) in the kernel's order: the distinct present rows by the position of
    their LAST occurrence, each with that occurrence's weight (``weights`` None: ones)"""
    rows = np.asarray(rows, np.int64).ravel()
    at = np.flatnonzero((rows >= 0) & (rows < n_rows))
    if at.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    _, first_rev = np.unique(rows[at][::-1], return_index=True)
    last = np.sort(at[at.size - 1 - first_rev])
    w = np.ones(last.size, np.float32) if weights is None else np.asarray(weights, np.float32).ravel()[last]
    return rows[last], w


def knn_neighbours_host(p_indptr, p_seqs, n_seqs, seq_scale, hist_rows, hist_weights, hist_offsets, hist_self, sample_size, k, tails=True):
    """numpy twin of ebn_knn_neighbours_f32, bit-equal to it -> (seq [n_hists, k] int32, sim [n_hists, k] float32; -1 / -inf past the
    last candidate).  Per history: the items in order, every add in float32; ``tails=False`` reads whole posting rows instead of
    their last ``sample_size + 1`` entries (the same result: the tail argument of include/ebnerd_hip.h)."""
    k, S = _limits(k, sample_size)
    p_indptr, p_seqs = np.asarray(p_indptr, np.int64).ravel(), np.asarray(p_seqs, np.int64).ravel()
    n_rows, nnz, n_seqs = p_indptr.size - 1, p_seqs.size, int(n_seqs)
    hist_rows, hist_offsets = np.asarray(hist_rows, np.int64).ravel(), np.asarray(hist_offsets, np.int64).ravel()
    w_all = None if hist_weights is None else np.asarray(hist_weights, np.float32).ravel()
    scale = None if seq_scale is None else np.asarray(seq_scale, np.float32).ravel()
    n_hists = hist_offsets.size - 1
    out_seq, out_sim = np.full((n_hists, k), -1, np.int32), np.full((n_hists, k), -np.inf, np.float32)
    with np.errstate(all="ignore"):
        for u in range(n_hists):
            a, b = (min(max(int(v), 0), hist_rows.size) for v in (hist_offsets[u], hist_offsets[u + 1]))
            items, w = query_items(hist_rows[a:b], None if w_all is None else w_all[a:b], n_rows)
            segs = []
            for r in items.tolist():
                lo, hi = (min(max(int(v), 0), nnz) for v in (p_indptr[r], p_indptr[r + 1]))
                segs.append(p_seqs[max(lo, hi - (S + 1)) if tails else lo:max(hi, lo)])
            if not segs:
                continue
            ids = np.unique(np.concatenate(segs))
            ids = ids[(ids >= 0) & (ids < n_seqs)]
            acc, touched = np.zeros(ids.size, np.float32), np.zeros(ids.size, bool)
            for seg, wv in zip(segs, w):
                seg = seg[(seg >= 0) & (seg < n_seqs)]
                loc = np.searchsorted(ids, seg)
                acc[loc] = np.where(touched[loc], acc[loc] + wv, wv)  # float32 + float32: one rounding
                touched[loc] = True
            if hist_self is not None:
                keep = ids != int(hist_self[u])
                ids, acc = ids[keep], acc[keep]
            ids, acc = ids[-S:], acc[-S:]  # the most recent sample_size of the union
            sim = acc if scale is None else acc * scale[ids]
            best = np.lexsort((-ids, -sim.astype(np.float64)))[:k]  # sim descending, then id descending
            out_seq[u, :best.size], out_sim[u, :best.size] = ids[best], sim[best]
    return out_seq, out_sim


def knn_scores_host(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim, list_hist, cand_rows, cand_offsets) -> np.ndarray:
    """numpy twin of ebn_knn_scores_f32 -> [n_items] float64: the (item, neighbour) pairs in blocks, membership by one searchsorted
    over the composite keys ``seq * n_rows + row`` of the sets, a float64 sum per item, one multiply by ``item_scale``"""
    s_items, s_indptr = _sequences(s_items, s_indptr)
    n_seqs, n_rows = s_indptr.size - 1, int(n_rows)
    nbr_seq, nbr_sim = np.asarray(nbr_seq, np.int64), np.asarray(nbr_sim).astype(np.float64)
    if nbr_seq.ndim != 2 or nbr_seq.shape != nbr_sim.shape:
        raise ValueError("nbr_seq and nbr_sim must be [n_hists, k]")
    n_hists, k = nbr_seq.shape
    cand_rows, cand_offsets = _sequences(cand_rows, cand_offsets)
    comp = np.repeat(np.arange(n_seqs, dtype=np.int64), np.diff(s_indptr)) * n_rows + s_items[:int(s_indptr[-1])]
    n = int(cand_offsets[-1])
    u = np.repeat(_list_histories(list_hist, cand_offsets.size - 1, n_hists), np.diff(cand_offsets))
    rows = cand_rows[:n]
    out = np.zeros(cand_rows.size)
    items = np.flatnonzero((rows >= 0) & (rows < n_rows) & (u >= 0))
    step = max(1, _CHUNK_PAIRS // max(k, 1))
    for a in range(0, items.size if comp.size else 0, step):
        i = items[a:a + step]
        seq, sim = nbr_seq[u[i]], nbr_sim[u[i]]
        valid = (seq >= 0) & (seq < n_seqs)
        key = np.where(valid, seq, 0) * n_rows + rows[i][:, None]
        pos = np.minimum(np.searchsorted(comp, key), comp.size - 1)
        total = np.where(valid & (comp[pos] == key), sim, 0.0).sum(axis=1)
        out[i] = total if item_scale is None else total * np.asarray(item_scale).astype(np.float64)[rows[i]]
    return out


# ---- top-N over the whole catalogue: the numpy twins of ebn_knn_topk_f32 / ebn_knn_target_rank_f32 -------------------------------
def knn_chains_host(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim) -> list:
    """[(touched [n_rows] bool, score [n_rows] float32)] per neighbour row in the kernels' arithmetic: the slots in list order,
    vectorised over the rows of one neighbour's set; the first touching neighbour assigns its sim, every later one adds it with one
    float32 rounding; one float32 multiply by ``item_scale`` closes.  The part of both twins that depends on neither the candidates
    nor the windows nor the exclusion lists (``chains=`` takes it, so that several calls share it)."""
    s_indptr, s_items = np.asarray(s_indptr, np.int64).ravel(), np.asarray(s_items, np.int64).ravel()
    n_seqs, nnz, n_rows = s_indptr.size - 1, s_items.size, int(n_rows)
    nbr_seq, nbr_sim = np.asarray(nbr_seq, np.int64), np.asarray(nbr_sim, np.float32)
    if nbr_seq.ndim != 2 or nbr_seq.shape != nbr_sim.shape or not 1 <= nbr_seq.shape[1] <= MAX_K:
        raise ValueError(f"nbr_seq and nbr_sim must be [n_hists, k] with 1 <= k <= {MAX_K}")
    scale = None if item_scale is None else np.asarray(item_scale, np.float32).ravel()
    out = []
    with np.errstate(all="ignore"):
        for seqs, sims in zip(nbr_seq, nbr_sim):
            touched, acc = np.zeros(n_rows, bool), np.zeros(n_rows, np.float32)
            for s, sim in zip(seqs.tolist(), sims):
                if not 0 <= s < n_seqs:
                    continue
                a, b = (min(max(int(v), 0), nnz) for v in (s_indptr[s], s_indptr[s + 1]))
                c = s_items[a:b]
                c = c[(c >= 0) & (c < n_rows)]
                acc[c] = np.where(touched[c], acc[c] + sim, sim)  # float32 + float32: one rounding
                touched[c] = True
            out.append((touched, acc if scale is None else acc * scale))
    return out


def _topn_walk_host(chains, n_rows, user_hist, n_users, cand_pos, M, window, exclude):
    """per user: (admissible rows, their positions, the float32 scores of all rows), and the two flags at the end"""
    n_hists = len(chains)
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


def knn_topk_host(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim, user_hist, n_users, cand_pos, M, window, exclude, k, chains=None):
    """numpy twin of ebn_knn_topk_f32, bit-equal to it -> (pos [U, k] int32, score [U, k] float32, flags [2] int32)"""
    if not 1 <= int(k) <= MAX_TOP_K:
        raise ValueError(f"k must lie in [1, {MAX_TOP_K}], got {k}")
    if chains is None:
        chains = knn_chains_host(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim)
    out_pos, out_score = np.full((int(n_users), int(k)), -1, np.int32), np.full((int(n_users), int(k)), -np.inf, np.float32)
    flags = np.zeros(2, np.int32)
    for u, rows, pos, score, flags in _topn_walk_host(chains, int(n_rows), user_hist, n_users, cand_pos, M, window, exclude):
        s = score[rows]
        best = np.lexsort((pos, -s))[:int(k)]  # score descending, then position ascending
        out_pos[u, :best.size], out_score[u, :best.size] = pos[best], s[best]
    return out_pos, out_score, flags


def knn_target_rank_host(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim, user_hist, n_users, cand_pos, M, target_pos, window, exclude,
                         chains=None):
    """numpy twin of ebn_knn_target_rank_f32 -> (rank [U] int32, count [U] int32, score [U] float32, flags [2] int32)"""
    if chains is None:
        chains = knn_chains_host(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim)
    target_pos = np.asarray(target_pos, np.int64).ravel()
    U = int(n_users)
    rank, count, t_out = np.zeros(U, np.int32), np.zeros(U, np.int32), np.full(U, -np.inf, np.float32)
    flags, oob_target = np.zeros(2, np.int32), bool((target_pos[:U] >= M).any())
    for u, rows, pos, score, flags in _topn_walk_host(chains, int(n_rows), user_hist, n_users, cand_pos, M, window, exclude):
        count[u] = rows.size
        at = np.flatnonzero(pos == target_pos[u]) if 0 <= target_pos[u] < M else np.zeros(0, np.int64)
        if at.size:
            s, t = score[rows], score[rows[at[0]]]
            rank[u] = 1 + int(((s > t) | ((s == t) & (pos < target_pos[u]))).sum())
            t_out[u] = t
    if oob_target:
        flags[0] = 1
    return rank, count, t_out, flags


# ---- the index -----------------------------------------------------------------------------------------------------------------
class KNNIndex:
    """``article_ids`` (sorted, numpy) name the rows; ``p_indptr`` int64 / ``p_seqs`` int32 are the postings, ``s_indptr`` int64 /
    ``s_items`` int32 the sets, ``seq_scale`` / ``item_scale`` float32 or None: device tensors on the device path, numpy arrays on the
    host path (``host()`` gives numpy either way).  ``sequence_of`` [n_seqs] int64 (numpy): the input row of sequence id s;
    ``keys`` [n_seqs] (numpy) or None: the key of sequence id s."""

    def __init__(self, article_ids, p_indptr, p_seqs, s_indptr, s_items, seq_scale, item_scale, sequence_of, keys):
        self.article_ids, self.p_indptr, self.p_seqs, self.s_indptr, self.s_items = article_ids, p_indptr, p_seqs, s_indptr, s_items
        self.seq_scale, self.item_scale, self.sequence_of, self.keys = seq_scale, item_scale, sequence_of, keys
        self._host = None

    @property
    def on_device(self) -> bool:
        return not isinstance(self.p_indptr, np.ndarray)

    @property
    def n_rows(self) -> int:
        return len(self.article_ids)

    @property
    def n_seqs(self) -> int:
        return len(self.sequence_of)

    def host(self):
        """(p_indptr, p_seqs, s_indptr, s_items, seq_scale, item_scale) as numpy arrays (None stays None), downloaded once"""
        if self._host is None:
            parts = (self.p_indptr, self.p_seqs, self.s_indptr, self.s_items, self.seq_scale, self.item_scale)
            self._host = tuple(p if p is None or isinstance(p, np.ndarray) else p.cpu().numpy() for p in parts)
        return self._host


def _unique_keys_device(parts):
    import torch

    keys = parts[0] if len(parts) == 1 else torch.unique_consecutive(torch.sort(torch.cat(parts)).values)
    return keys


def knn_index_device(seq_rows, seq_offsets, n_rows, max_keys=2 ** 27, device="cuda"):
    """the device build of ``knn_index_host`` -> the same four arrays as tensors: per block of at most ``max_keys // 2`` uploaded
    entries the two composite int64 keys, torch.sort and unique_consecutive; the blocks' keys concatenated, sorted and reduced
    again; indptr one searchsorted each"""
    import torch

    rows, off = _sequences(seq_rows, seq_offsets)
    n_rows, n_seqs, n = int(n_rows), off.size - 1, int(off[-1])
    if not (0 <= n_rows <= MAX_DIM and n_seqs <= MAX_DIM):
        raise ValueError("n_rows and the number of sequences must lie in [0, 2^31 - 1]")
    dev = torch.device(device)
    rows_d = torch.from_numpy(np.ascontiguousarray(rows[:n])).to(dev)
    seq_of = torch.repeat_interleave(torch.arange(n_seqs, dtype=torch.int64, device=dev), torch.from_numpy(np.diff(off)).to(dev))
    step = max(n, 1) if _max_keys(max_keys) is None else max(1, int(max_keys) // 2)
    pk, sk = [], []
    for a in range(0, n, step):
        r, s = rows_d[a:a + step], seq_of[a:a + step]
        ok = (r >= 0) & (r < n_rows)
        r, s = r[ok], s[ok]
        pk.append(torch.unique_consecutive(torch.sort(r * n_seqs + s).values))
        sk.append(torch.unique_consecutive(torch.sort(s * n_rows + r).values))
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    out = []
    for keys, n_major, n_minor in ((_unique_keys_device(pk) if pk else empty, n_rows, n_seqs),
                                   (_unique_keys_device(sk) if sk else empty, n_seqs, n_rows)):
        major = torch.div(keys, max(n_minor, 1), rounding_mode="floor")
        out += [torch.searchsorted(major, torch.arange(n_major + 1, dtype=torch.int64, device=dev)),
                (keys - major * max(n_minor, 1)).to(torch.int32)]
    return tuple(out)


def neighbours_call(p_indptr, p_seqs, n_seqs, seq_scale, hist_rows, hist_weights, hist_offsets, hist_self, sample_size, k):
    """One ebn_knn_neighbours_f32 launch over device tensors (``seq_scale`` / ``hist_weights`` / ``hist_self`` may be None) ->
    (seq [n_hists, k] int32, sim [n_hists, k] float32) on the device"""
    import torch

    from ebrec import _hip

    n_hists, dev = hist_offsets.numel() - 1, hist_offsets.device
    seq = torch.empty(n_hists, int(k), dtype=torch.int32, device=dev)
    sim = torch.empty(n_hists, int(k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _hip.call("ebn_knn_neighbours_f32", _hip.ptr(p_indptr), _hip.ptr(p_seqs), p_indptr.numel() - 1, p_seqs.numel(), int(n_seqs),
                  _hip.ptr(seq_scale), _hip.ptr(hist_rows), _hip.ptr(hist_weights), _hip.ptr(hist_offsets), n_hists, hist_rows.numel(),
                  _hip.ptr(hist_self), int(sample_size), int(k), _hip.ptr(seq), _hip.ptr(sim), _hip.stream_handle())
    return seq, sim


def scores_call(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim, list_hist, cand_rows, cand_offsets):
    """One ebn_knn_scores_f32 launch over device tensors (``item_scale`` / ``list_hist`` may be None) -> scores [n_items] float32"""
    import torch

    from ebrec import _hip

    scores = torch.empty(cand_rows.numel(), dtype=torch.float32, device=cand_rows.device)
    with torch.cuda.device(cand_rows.device):
        _hip.call("ebn_knn_scores_f32", _hip.ptr(s_indptr), _hip.ptr(s_items), s_indptr.numel() - 1, s_items.numel(), int(n_rows),
                  _hip.ptr(item_scale), _hip.ptr(nbr_seq), _hip.ptr(nbr_sim), nbr_seq.shape[0], nbr_seq.shape[1], _hip.ptr(list_hist),
                  _hip.ptr(cand_rows), _hip.ptr(cand_offsets), cand_offsets.numel() - 1, cand_rows.numel(), _hip.ptr(scores),
                  _hip.stream_handle())
    return scores


def _topn_operands(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim, user_hist, cand_pos, M):
    from ebrec import _hip

    n_rows = int(n_rows)
    M = n_rows if cand_pos is None else int(M)
    return (_hip.ptr(s_indptr), _hip.ptr(s_items), s_indptr.numel() - 1, s_items.numel(), n_rows, _hip.ptr(item_scale), _hip.ptr(nbr_seq),
            _hip.ptr(nbr_sim), nbr_seq.shape[0], nbr_seq.shape[1], _hip.ptr(user_hist), _hip.ptr(cand_pos), M)


def _check_topn_args(U, nbr_seq, nbr_sim, window, exclude, target_pos=None):
    import torch

    if nbr_seq.dim() != 2 or nbr_seq.shape != nbr_sim.shape or nbr_seq.dtype != torch.int32 or nbr_sim.dtype != torch.float32 or \
            not (nbr_seq.is_contiguous() and nbr_sim.is_contiguous()):
        raise ValueError("nbr_seq int32 and nbr_sim float32 must be contiguous [n_hists, k] tensors")
    for name, t, shape in (("window", window, (U, 2)), ("exclude", exclude, None), ("target_pos", target_pos, (U,))):
        if t is None:
            continue
        if t.dtype != torch.int32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape) or \
                (shape is None and (t.dim() != 2 or t.shape[0] != U)):
            raise ValueError(f"{name} must be a contiguous int32 tensor with one row per user ({U}), got {tuple(t.shape)} {t.dtype}")


def topk_call(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim, user_hist, n_users, cand_pos, M, window, exclude, k, flags,
              n_splits: int = 0):
    """One ebn_knn_topk_f32 launch over device tensors (``item_scale`` / ``user_hist`` / ``cand_pos`` / ``window`` [U, 2] /
    ``exclude`` [U, X] may be None) -> (pos [U, k] int32, score [U, k] float32); ``flags`` [2] int32 accumulates."""
    import torch

    from ebrec import _hip

    U, dev = int(n_users), s_indptr.device
    _check_topn_args(U, nbr_seq, nbr_sim, window, exclude)
    ops = _topn_operands(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim, user_hist, cand_pos, M)
    pos = torch.empty(U, k, dtype=torch.int32, device=dev)
    score = torch.empty(U, k, dtype=torch.float32, device=dev)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_knn_topk_auto_splits(U, int(n_rows)))
    ws = torch.empty(max(int(lib.ebn_knn_topk_workspace_bytes(U, k, max(splits, 1))), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("ebn_knn_topk_f32", *ops, _hip.ptr(window), _hip.ptr(exclude), 0 if exclude is None else exclude.shape[1], int(k), splits,
                  _hip.ptr(pos), _hip.ptr(score), _hip.ptr(flags), _hip.ptr(ws), ws.numel(), U, _hip.stream_handle())
    return pos, score


def target_rank_call(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim, user_hist, n_users, cand_pos, M, target_pos, window, exclude,
                     flags, n_splits: int = 0):
    """One ebn_knn_target_rank_f32 launch over device tensors: ``target_pos`` [U] int32 candidate positions (< 0: none) -> (rank [U]
    int32: 1-based place in ``topk_call``'s order, 0 = not ranked; count [U] int32: the user's admissible rows; score [U] float32:
    the target's score, -inf where rank is 0); ``flags`` accumulates."""
    import torch

    from ebrec import _hip

    U, dev = int(n_users), s_indptr.device
    _check_topn_args(U, nbr_seq, nbr_sim, window, exclude, target_pos)
    ops = _topn_operands(s_indptr, s_items, n_rows, item_scale, nbr_seq, nbr_sim, user_hist, cand_pos, M)
    rank = torch.empty(U, dtype=torch.int32, device=dev)
    count = torch.empty(U, dtype=torch.int32, device=dev)
    score = torch.empty(U, dtype=torch.float32, device=dev)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_knn_topk_auto_splits(U, int(n_rows)))
    ws = torch.empty(max(int(lib.ebn_knn_target_rank_workspace_bytes(U, max(splits, 1), 0 if cand_pos is None else int(M))), 16),
                     dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("ebn_knn_target_rank_f32", *ops, _hip.ptr(target_pos), _hip.ptr(window), _hip.ptr(exclude),
                  0 if exclude is None else exclude.shape[1], splits, _hip.ptr(rank), _hip.ptr(count), _hip.ptr(score), _hip.ptr(flags),
                  _hip.ptr(ws), ws.numel(), U, _hip.stream_handle())
    return rank, count, score


class KnnSession:
    """what ``TopN`` drives (see _topn.py): the histories of one ``recommend`` / ``rank_targets`` call.  The neighbour search has run
    ONCE over them (``nbr_seq`` / ``nbr_sim`` [n_hists, k]: device tensors -> the two kernels, numpy arrays -> the float32 twins);
    every batch launch passes ``user_hist = hist_idx``."""

    def __init__(self, index: "KNNIndex", nbr_seq, nbr_sim):
        self.on_device = not isinstance(nbr_seq, np.ndarray)
        self.n_rows, self.seq, self.sim = index.n_rows, nbr_seq, nbr_sim
        self.cand_pos, self.M, self.device = None, index.n_rows, None
        if self.on_device:
            self.device = nbr_seq.device
            self.sets = (index.s_indptr, index.s_items, index.n_rows, index.item_scale)
        else:
            _, _, s_indptr, s_items, _, item_scale = index.host()
            self.sets = (s_indptr, s_items, index.n_rows, item_scale)
            self.chains = knn_chains_host(*self.sets, nbr_seq, nbr_sim)  # once for every batch of the call

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
            pos, score, f = knn_topk_host(*self.sets, self.seq, self.sim, hist_idx, U, self.cand_pos, self.M, window, exclude, k, self.chains)
            flags |= f
            return pos, score
        return topk_call(*self.sets, self.seq, self.sim, self._up(hist_idx), U, self.cand_pos, self.M, self._up(window), self._up(exclude), k,
                         flags)

    def rank(self, hist_idx, target_pos, window, exclude, flags):
        U = len(hist_idx)
        if not self.on_device:
            rank, count, score, f = knn_target_rank_host(*self.sets, self.seq, self.sim, hist_idx, U, self.cand_pos, self.M, target_pos, window,
                                                         exclude, self.chains)
            flags |= f
            return rank, count, score
        return target_rank_call(*self.sets, self.seq, self.sim, self._up(hist_idx), U, self.cand_pos, self.M, self._up(target_pos),
                                self._up(window), self._up(exclude), flags)


# ---- the class -----------------------------------------------------------------------------------------------------------------
class HistoryKNN(TopN):
    """Sequence-neighbourhood scores.  ``k``: the neighbours of a history (1 to 512, at most ``sample_size``); ``sample_size``: the most
    recent sequences sharing an article with it that are compared at all (1 to 4096); ``similarity``: "dot" or "cosine";
    ``history_weights`` / ``lambda_factor`` / ``history_size`` / ``fill``: as in ``ContentSimilarity``; ``idf``: weigh an article's
    score by log(n_seqs / df); ``exclude_self``: never use the fitted sequence whose key equals the history's key; ``max_keys``: the
    composite keys one block of the device build may hold (8 bytes each)."""

    def __init__(self, k: int = 100, sample_size: int = 1000, similarity: str = "cosine", history_weights="linear", lambda_factor: float = 0.9,
                 history_size=None, idf: bool = False, exclude_self: bool = True, fill: float = 0.0, device="cuda", max_keys=2 ** 27):
        self.k, self.sample_size = _limits(k, sample_size)
        if similarity not in SIMILARITIES:
            raise ValueError(f"similarity must be one of {SIMILARITIES}, got {similarity!r}")
        if not (history_weights is None or callable(history_weights) or history_weights in ("linear", "exponential")):
            raise ValueError(f"history_weights must be None, 'linear', 'exponential' or a callable, got {history_weights!r}")
        if history_size is not None and (isinstance(history_size, bool) or int(history_size) != history_size or history_size < 1):
            raise ValueError(f"history_size must be a positive integer or None, got {history_size!r}")
        for name, flag in (("idf", idf), ("exclude_self", exclude_self)):
            if not isinstance(flag, (bool, np.bool_)):
                raise TypeError(f"{name} must be a bool, got {flag!r}")
        self.similarity, self.history_weights, self.lambda_factor = similarity, history_weights, float(lambda_factor)
        self.history_size, self.idf, self.exclude_self = (None if history_size is None else int(history_size)), bool(idf), bool(exclude_self)
        self.fill, self.device, self.max_keys = float(fill), device, _max_keys(max_keys)
        self.index = None

    # -- fit
    def fit(self, sequences, keys=None, recency=None) -> "HistoryKNN":
        """``fit(history_frame)``: one sequence per row of its ``article_id_fixed``, keyed by ``user_id``, ordered by the last of
        ``impression_time_fixed`` where the frame has that column; ``fit(sequences)``: a RaggedLists or lists of lists of article
        ids, oldest first.  ``keys=``: one key per sequence (what ``exclude_self`` matches); ``recency=``: one sortable value per
        sequence, larger = more recent.  Returns self."""
        df = sequences if isinstance(sequences, RaggedLists) else _frame(sequences)
        if hasattr(df, "columns"):
            if DEFAULT_HISTORY_ARTICLE_ID_COL not in df.columns:
                raise ValueError(f"the frame lacks the column '{DEFAULT_HISTORY_ARTICLE_ID_COL}'")
            flat, off = _explode(df[DEFAULT_HISTORY_ARTICLE_ID_COL])
            if keys is None and DEFAULT_USER_COL in df.columns:
                keys = df[DEFAULT_USER_COL].to_numpy()
            if recency is None and DEFAULT_HISTORY_IMPRESSION_TIMESTAMP_COL in df.columns:
                times = [np.asarray([] if t is None else t).ravel() for t in df[DEFAULT_HISTORY_IMPRESSION_TIMESTAMP_COL]]
                last = [t[-1:].astype("datetime64[ns]").astype(np.int64) for t in times]
                recency = np.array([int(t[0]) if t.size else np.iinfo(np.int64).min for t in last], np.int64)
        else:
            flat, off = _ragged_ids(df)
        flat, off = np.asarray(flat).ravel(), np.ascontiguousarray(off, dtype=np.int64)
        if flat.size and flat.dtype.kind not in "iuUS":
            raise TypeError(f"HistoryKNN needs ids that are all strings or all integers, got dtype {flat.dtype}")
        n_seqs = off.size - 1
        for name, v in (("keys", keys), ("recency", recency)):
            if v is not None and np.asarray(v).ravel().size != n_seqs:
                raise ValueError(f"{n_seqs} sequences but {np.asarray(v).ravel().size} {name}")
        order = np.arange(n_seqs, dtype=np.int64) if recency is None else np.argsort(np.asarray(recency).ravel(), kind="stable").astype(np.int64)
        lengths = np.diff(off)[order]
        new_off = np.zeros(n_seqs + 1, np.int64)
        np.cumsum(lengths, out=new_off[1:])
        take = np.repeat(off[:-1][order] - new_off[:-1], lengths) + np.arange(int(new_off[-1]), dtype=np.int64)
        ids = np.unique(flat)
        rows = _rows_of(ids, flat[:int(off[-1])][take] if take.size else flat[:0])
        on_device = device_available(self.device) and ids.size > 0
        if on_device:
            import torch

            p_indptr, p_seqs, s_indptr, s_items = knn_index_device(rows, new_off, ids.size, self.max_keys, self.device)
            up = lambda a: torch.from_numpy(a).to(p_indptr.device)
        else:
            p_indptr, p_seqs, s_indptr, s_items = knn_index_host(rows, new_off, ids.size, self.max_keys)
            up = lambda a: a
        host_ptr = lambda t: t if isinstance(t, np.ndarray) else t.cpu().numpy()
        seq_scale = up(knn_seq_scale_host(host_ptr(s_indptr))) if self.similarity == "cosine" else None
        item_scale = up(knn_idf_host(host_ptr(p_indptr), n_seqs)) if self.idf else None
        self.index = KNNIndex(ids, p_indptr, p_seqs, s_indptr, s_items, seq_scale, item_scale, order,
                              None if keys is None else np.asarray(keys).ravel()[order])
        return self

    def _fitted(self) -> KNNIndex:
        if self.index is None:
            raise RuntimeError("HistoryKNN.fit has not been called")
        return self.index

    def rows_of(self, ids) -> np.ndarray:
        """int32 index rows of a flat array of article ids, -1 for an article no sequence held"""
        return _rows_of(self._fitted().article_ids, ids)

    def _histories(self, histories):
        """ids of histories -> (rows int32, offsets int64, weights float32 | None): content.py's handling over this index"""
        return history_operands(self.rows_of, histories, self.history_size, self.history_weights, self.lambda_factor)

    def _self_of(self, history_keys, n_hists):
        """the fitted sequence id whose key equals each history's key (the most recent one of several), -1 for none; None when
        nothing is to be excluded"""
        ix = self._fitted()
        if not self.exclude_self or history_keys is None or ix.keys is None:
            return None
        asked = np.asarray(history_keys).ravel()
        if asked.size != n_hists:
            raise ValueError(f"{n_hists} histories but {asked.size} history keys")
        out = np.full(n_hists, -1, np.int32)
        if ix.keys.size == 0 or n_hists == 0:
            return out
        a, b = ix.keys.dtype.kind, asked.dtype.kind
        if (a in "iu" and b in "iu") or (a == b and a in "US"):
            order = np.argsort(ix.keys, kind="stable")  # equal keys keep ascending ids: side="right" finds the most recent
            ks = ix.keys[order]
            pos = np.searchsorted(ks, asked, side="right") - 1
            hit = (pos >= 0) & (ks[np.maximum(pos, 0)] == asked)
            out[hit] = order[pos[hit]]
        else:
            seq_of_key = {key: s for s, key in enumerate(ix.keys.tolist())}
            out[:] = [seq_of_key.get(key, -1) for key in asked.tolist()]
        return out

    def _neighbours(self, h_rows, h_off, w, hist_self):
        """(seq, sim) of prepared histories: device tensors on the device path"""
        ix = self._fitted()
        if ix.on_device and device_available(self.device):
            import torch

            dev = ix.p_indptr.device
            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            return neighbours_call(ix.p_indptr, ix.p_seqs, ix.n_seqs, ix.seq_scale, up(h_rows), up(w), up(h_off), up(hist_self),
                                   self.sample_size, self.k)
        p_indptr, p_seqs, _, _, seq_scale, _ = ix.host()
        return knn_neighbours_host(p_indptr, p_seqs, ix.n_seqs, seq_scale, h_rows, w, h_off, hist_self, self.sample_size, self.k)

    # -- recommend / rank_targets (TopN, _topn.py): ebn_knn_topk_f32 / ebn_knn_target_rank_f32 over the sets.  Only an article some
    # neighbour read has a score; a history without neighbours gets an empty list and rank 0
    def _topn_ids(self):
        return self._fitted().article_ids

    def _topn_rows_of(self, ids):
        return self.rows_of(ids)

    def _topn_session(self, histories, history_keys=None):
        ix = self._fitted()
        h_rows, h_off, w = self._histories(histories)
        seq, sim = self._neighbours(h_rows, h_off, w, self._self_of(history_keys, h_off.size - 1))
        return KnnSession(ix, seq, sim)

    # -- public
    def neighbours(self, histories, history_keys=None):
        """(rows [n_hists, k] int64, sims [n_hists, k] float32): each history's neighbours as INPUT-ROW indices of the fitted
        sequences (``index.sequence_of`` applied; -1 / -inf past the last neighbour), best first.  ``history_keys``: what
        ``exclude_self`` matches.  Device tensors on the device path, numpy arrays otherwise."""
        ix = self._fitted()
        h_rows, h_off, w = self._histories(histories)
        seq, sim = self._neighbours(h_rows, h_off, w, self._self_of(history_keys, h_off.size - 1))
        if isinstance(seq, np.ndarray):
            return np.where(seq >= 0, np.append(ix.sequence_of, -1)[seq], -1).astype(np.int64), sim
        import torch

        table = torch.from_numpy(np.append(ix.sequence_of, -1)).to(seq.device)
        return table[seq.long()], sim  # -1 picks the appended -1

    def predict(self, candidates, histories=None, list_hist=None, *, history=None, history_keys=None) -> RaggedLists:
        """float64 scores aligned with the candidate lists; the three call forms of ``ContentSimilarity.predict``:
        ``predict(behaviors, history=history_frame)`` joined on ``user_id`` (which is also what ``exclude_self`` matches),
        ``predict(behaviors)`` with ``article_id_fixed`` per impression, ``predict(candidates, histories, list_hist=None,
        history_keys=None)`` over RaggedLists or lists of lists of ids."""
        ix = self._fitted()
        if histories is None:
            df = _frame(candidates)
            if not hasattr(df, "columns"):
                raise ValueError("predict(candidates, histories) needs the histories; predict(behaviors) a frame")
            if history_keys is not None:
                raise ValueError("history_keys= belongs to predict(candidates, histories); the frames are joined on user_id")
            cand, histories, list_hist, users = join_frames(candidates, history)
            histories = RaggedLists(*histories)
            if users is not None:
                history_keys = users  # the user of every history the join kept
            elif DEFAULT_USER_COL in df.columns:
                history_keys = df[DEFAULT_USER_COL].to_numpy()  # a history per impression: its row's user
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
        seq, sim = self._neighbours(h_rows, h_off, w, self._self_of(history_keys, n_hists))
        on_device = not isinstance(seq, np.ndarray)
        if on_device:
            import torch

            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(seq.device)
            flat = scores_call(ix.s_indptr, ix.s_items, ix.n_rows, ix.item_scale, seq, sim, up(list_hist), up(c_rows), up(c_off)).to(torch.float64)
        else:
            _, _, s_indptr, s_items, _, item_scale = ix.host()
            flat = knn_scores_host(s_indptr, s_items, ix.n_rows, item_scale, seq, sim, list_hist, c_rows, c_off)
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
