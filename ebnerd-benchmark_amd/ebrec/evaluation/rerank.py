"""Greedy re-ranking of a relevance pool: MMR trades a list's relevance against its IntralistDiversity, Calibrated (second half
of this module) against the KL divergence between a target label distribution and the list's -- what Distribution reports.

Maximal-Marginal-Relevance (MMR).

Per list there is a pool of P <= 64 (id, score) entries.  An entry is ABSENT when its id is no key of the lookup or its score is
not finite.  With u_i the unit vector of entry i and d(i, j) = clip(1 - u_i . u_j, 0, 2) -- the distance IntralistDiversity
averages --

    round 0:      pick the present entry with the largest score
    round t >= 1: pick, among the present entries not yet picked, the largest  lam * score_i + (1 - lam) * min over picked j of d(i, j)

larger objective first, equal objectives to the smaller pool index; the rounds end after ``top_n`` picks or when nothing is
left.  ``lam = 1`` is the relevance order of the pool, ``lam = 0`` looks at the distances alone (after the first pick).

Two paths, as in beyond_accuracy.py.  With a `DeviceLookup` that holds the key the pools go through ``ebn_mmr_rerank_f32``
(csrc/ebn_rerank.hip: the unit rows gathered into LDS, an exact-fp32 MFMA Gram matrix per pool, one wave running the rounds);
with a plain dict (or a DeviceLookup with ``device=None``) they run in float64 numpy, list by list.  torch is imported only on
the device path.  ``model.recommend(..., rerank=MMR(...))`` runs the same kernel on the model's own top-``pool``.

Determinantal point process (DPP), fast greedy MAP inference (Chen, Zhang, Zhou, NeurIPS 2018).

The same pools, absent entries and distance.  MMR scores a pick against its NEAREST earlier pick; DPP scores the whole list through
log det of its similarity matrix, so an entry inside the span of three earlier picks is penalised though it is close to none.

    S(i, j) = 1 - d(i, j) / 2       (1 + cos) / 2 for unit vectors: positive semi-definite, in [0, 1]; the diagonal as computed
                                    (1 for a unit vector, 1/2 for a zero vector)
    state per entry: d2_i, the conditional variance of i given the picks (initially S(i, i)), and a Cholesky row c_i;  EPS = 1e-4
    round t = 0, 1, ...: pick, among the present entries not yet picked, the largest  lam * score_i + (1 - lam) * log(max(d2_i, EPS))
    after picking j: if d2_j <= EPS the pick is degenerate (already spanned): c_i[t] = 0 and nothing else changes; otherwise
        e_i = (S(j, i) - sum_{s<t} c_j[s] c_i[s]) / sqrt(d2_j),   c_i[t] = e_i,   d2_i -= e_i * e_i

larger objective first, equal objectives to the smaller pool index; the rounds end after ``top_n`` picks or when nothing is left.
lam * score_i is the marginal gain of lam * sum score + (1 - lam) * log det S_Y, so ``lam = 1`` is the relevance order of the pool.
A pool whose rank is below ``top_n`` still fills its list: spanned entries are clamped at EPS, not dropped, and then order by
score.  The two paths are MMR's: ``ebn_dpp_rerank_f32`` (csrc/ebn_dpp.hip: the same Gram stage, then one wave per pool running an
incremental Cholesky with its rows in LDS) or float64 numpy; ``model.recommend(..., rerank=DPP(...))`` runs the kernel on the
model's own top-``pool``."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ebrec.evaluation.beyond_accuracy import DeviceLookup, label_lookup
from ebrec.evaluation.utils import check_key_in_all_nested_dicts

MAX_POOL, MAX_TOP_N = 64, 64  # limits of ebn_mmr_rerank_f32, ebn_dpp_rerank_f32 and ebn_calibrated_rerank_f32 (include/ebnerd_hip.h)
MAX_LABELS, MAX_HISTORY = 128, 256  # limits of ebn_calibrated_rerank_f32 / ebn_label_target_f32


@dataclass(frozen=True)
class MMR:
    """``model.recommend(..., rerank=MMR(lookup, key, lam, pool))``: re-rank each impression's ``pool`` most relevant candidates
    by MMR over the unit vectors ``lookup`` (a DeviceLookup) holds under ``key``.  ``pool`` must lie in [top_n, 64]."""
    lookup: DeviceLookup
    key: str
    lam: float = 0.7
    pool: int = 50


@dataclass(frozen=True)
class DPP:
    """``model.recommend(..., rerank=DPP(lookup, key, lam, pool))``: re-rank each impression's ``pool`` most relevant candidates
    by greedy DPP MAP inference over the unit vectors ``lookup`` (a DeviceLookup) holds under ``key``.  ``pool`` must lie in
    [top_n, 64]."""
    lookup: DeviceLookup
    key: str
    lam: float = 0.7
    pool: int = 50


DPP_EPS = 1e-4  # the clamp of a conditional variance (ebn_dpp_rerank_f32)


def check_lam(lam) -> float:
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:  # NaN fails both comparisons
        raise ValueError(f"lam must lie in [0, 1], got {lam}")
    return lam


def _is_vector_key(lookup_dict, key: str) -> bool:
    if isinstance(lookup_dict, DeviceLookup):
        if key in lookup_dict.vector_keys:
            return True
        if key in lookup_dict.scalar_keys:
            return False
    check_key_in_all_nested_dicts(lookup_dict, key)
    first = next(iter(lookup_dict.values()), None)
    return first is None or np.ndim(first[key]) == 1


def _pool_select(entry: str, unit, pool_rows, pool_rel, k: int, lam: float, flags, want_obj: bool):
    import torch

    from ebrec import _hip

    U, P = pool_rows.shape
    sel = torch.empty(U, k, dtype=torch.int32, device=pool_rows.device)
    obj = torch.empty(U, k, dtype=torch.float32, device=pool_rows.device) if want_obj else None
    with torch.cuda.device(pool_rows.device):
        _hip.call(entry, _hip.ptr(unit), unit.shape[0], unit.shape[1], _hip.ptr(pool_rows), _hip.ptr(pool_rel), P, k,
                  float(lam), _hip.ptr(sel), _hip.ptr(obj), _hip.ptr(flags), U, _hip.stream_handle())
    return sel, obj


def mmr_select(unit, pool_rows, pool_rel, k: int, lam: float, flags, want_obj: bool = False):
    """One ebn_mmr_rerank_f32 call on device tensors: unit [n_rows, D] float32, pool_rows [U, P] int32, pool_rel [U, P] float32
    -> (sel [U, k] int32 pool indices, -1 in empty slots; obj [U, k] float32 or None).  ``flags`` [2] int32 accumulates."""
    return _pool_select("ebn_mmr_rerank_f32", unit, pool_rows, pool_rel, k, lam, flags, want_obj)


def dpp_select(unit, pool_rows, pool_rel, k: int, lam: float, flags, want_obj: bool = False):
    """One ebn_dpp_rerank_f32 call on device tensors, with the operands and results of ``mmr_select``."""
    return _pool_select("ebn_dpp_rerank_f32", unit, pool_rows, pool_rel, k, lam, flags, want_obj)


def _unit_distances(vectors: np.ndarray) -> np.ndarray:
    """float64 [P, P] distances of the vectors as stored (normalised here, a zero row stays zero; a NaN dot product gives 0)"""
    norm = np.sqrt((vectors * vectors).sum(1, keepdims=True))
    unit = vectors / np.where(norm == 0, 1.0, norm)
    with np.errstate(invalid="ignore"):
        dist = np.clip(1.0 - unit @ unit.T, 0.0, 2.0)
    return np.where(np.isnan(dist), 0.0, dist)


def _host_select(vectors: np.ndarray, present: np.ndarray, rel: np.ndarray, k: int, lam: float) -> list:
    """pool indices of one list, float64: vectors [P, D] as stored (normalised here, a zero row stays zero)"""
    dist = _unit_distances(vectors)
    left = present.copy()
    mind = np.full(len(rel), np.inf)
    picks = []
    for t in range(k):
        if not left.any():
            break
        safe = np.where(left, rel, 0.0)  # an absent entry's relevance may be anything
        obj = safe if t == 0 else lam * safe + (1.0 - lam) * mind
        best = int(np.argmax(np.where(left, obj, -np.inf)))  # the first of equal objectives: the smaller pool index
        picks.append(best)
        left[best] = False
        mind = np.minimum(mind, dist[best])
    return picks


def _host_dpp_select(vectors: np.ndarray, present: np.ndarray, rel: np.ndarray, k: int, lam: float) -> list:
    """pool indices of one list, float64, by the DPP recurrence of the module docstring: vectors [P, D] as stored"""
    S = 1.0 - 0.5 * _unit_distances(vectors)
    P = len(rel)
    left = present.copy()
    d2 = np.diag(S).copy()
    chol = np.zeros((P, k))
    picks = []
    for t in range(k):
        if not left.any():
            break
        obj = lam * np.where(left, rel, 0.0) + (1.0 - lam) * np.log(np.maximum(d2, DPP_EPS))
        best = int(np.argmax(np.where(left, obj, -np.inf)))  # the first of equal objectives: the smaller pool index
        picks.append(best)
        left[best] = False
        if d2[best] > DPP_EPS:  # else a degenerate pick: slot t stays zero
            e = (S[best] - chol[:, :t] @ chol[best, :t]) / np.sqrt(d2[best])
            chol[:, t] = e
            d2 = d2 - e * e
    return picks


def mmr_rerank(ids, scores, lookup_dict, lookup_key: str, top_n: int, lam: float = 0.7, return_scores: bool = False, fill_id=-1):
    """ids [n, P] with their scores [n, P] -> ids [n, top_n]: the MMR order of each pool (module docstring), lists left shorter
    than ``top_n`` padded with ``fill_id``.  An id that is no key of ``lookup_dict`` and an entry whose score is not finite are
    absent.  ``return_scores``: also the given score of each kept entry [n, top_n] (-inf in the padding), in selection order --
    which is NOT monotone: a later pick may carry a higher score than an earlier one's successor would have.
    ValueError: ``lam`` outside [0, 1], P > 64, ``top_n`` outside [1, 64], ``lookup_key`` not a vector key, and, on the device
    path, a vector width that is no multiple of 4."""
    return _rerank_by_vectors(mmr_select, _host_select, ids, scores, lookup_dict, lookup_key, top_n, lam, return_scores, fill_id)


def dpp_rerank(ids, scores, lookup_dict, lookup_key: str, top_n: int, lam: float = 0.7, return_scores: bool = False, fill_id=-1):
    """ids [n, P] with their scores [n, P] -> ids [n, top_n]: the greedy DPP order of each pool (module docstring), with the
    arguments, absent entries, padding, ``return_scores`` (the given score of each kept entry, in selection order: NOT monotone)
    and ValueErrors of ``mmr_rerank``."""
    return _rerank_by_vectors(dpp_select, _host_dpp_select, ids, scores, lookup_dict, lookup_key, top_n, lam, return_scores, fill_id)


def _rerank_by_vectors(device_select, host_select, ids, scores, lookup_dict, lookup_key, top_n, lam, return_scores, fill_id):
    """the body of ``mmr_rerank`` and ``dpp_rerank``: the checks, the two paths (``device_select``: mmr_select or dpp_select,
    ``host_select``: their float64 twins) and the padding"""
    lam = check_lam(lam)
    ids = np.asarray(ids)
    scores = np.asarray(scores)
    if scores.dtype.kind != "f":
        scores = scores.astype(np.float64)
    if ids.ndim != 2 or scores.shape != ids.shape:
        raise ValueError(f"ids and scores must be [n, P] arrays of one shape, got {ids.shape} and {scores.shape}")
    n, P = ids.shape
    if P > MAX_POOL:
        raise ValueError(f"pools of at most {MAX_POOL} entries are supported, got P = {P}")
    if not 1 <= int(top_n) <= MAX_TOP_N:
        raise ValueError(f"top_n must lie in [1, {MAX_TOP_N}], got {top_n}")
    top_n = int(top_n)
    if not _is_vector_key(lookup_dict, lookup_key):
        raise ValueError(f"'{lookup_key}' is not a vector key of the lookup")
    fill = np.asarray(fill_id) if ids.dtype.kind in "US" else np.asarray(fill_id, dtype=ids.dtype)  # a string filler is not cut short
    if n == 0 or P == 0:
        out = np.full((n, top_n), fill)
        return (out, np.full((n, top_n), -np.inf, scores.dtype)) if return_scores else out

    if isinstance(lookup_dict, DeviceLookup) and lookup_dict.holds(lookup_key) and len(lookup_dict):
        import torch

        unit = lookup_dict.device_table(lookup_key)
        if unit.shape[1] == 0 or unit.shape[1] % 4:
            raise ValueError(f"the device path needs a vector width that is a positive multiple of 4, '{lookup_key}' has {unit.shape[1]}")
        rows = torch.from_numpy(lookup_dict.rows_of(ids).reshape(n, P)).to(unit.device)
        rel = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(unit.device)
        flags = torch.zeros(2, dtype=torch.int32, device=unit.device)
        sel = device_select(unit, rows, rel, top_n, lam, flags)[0].cpu().numpy().astype(np.int64)
    else:
        sel = np.full((n, top_n), -1, np.int64)
        rel64 = scores.astype(np.float64)
        for r in range(n):
            keys = ids[r].tolist()
            present = np.fromiter((key in lookup_dict for key in keys), bool, P) & np.isfinite(rel64[r])
            if not present.any():
                continue
            D = len(lookup_dict[keys[int(np.argmax(present))]][lookup_key])
            vectors = np.zeros((P, D))
            for i in np.flatnonzero(present):
                vectors[i] = lookup_dict[keys[i]][lookup_key]
            picks = host_select(vectors, present, rel64[r], top_n, lam)
            sel[r, :len(picks)] = picks
    kept = np.maximum(sel, 0)
    out = np.where(sel >= 0, np.take_along_axis(ids, kept, 1), fill)
    if return_scores:
        return out, np.where(sel >= 0, np.take_along_axis(scores, kept, 1), -np.inf).astype(scores.dtype)
    return out


# ------------------------------------------------------------------------------------------------ calibrated re-ranking
# Steck, "Calibrated Recommendations" (RecSys 2018).  Every item has a LABEL ROW over the C labels of an attribute (the sorted
# distinct labels of the lookup): one-hot for a single label, 1 / n on each of the n distinct labels of a list, zeros for None or an
# empty list.  Per list there is a pool of P <= 64 (id, score) entries -- absent as above -- and a target distribution p [C]: the
# weighted mean label row of the user's click history, or one given mix for everybody.  With S the sum of the picked label rows,
# n their number, q~ = (1 - alpha) S / n + alpha p and KL = sum over c with p_c > 0 of p_c log(p_c / q~_c),
#
#     every round: pick, among the present entries not yet picked, the largest  lam * score_i - (1 - lam) * KL(picks + {i})
#
# larger objective first, equal objectives to the smaller pool index; ``lam = 1`` is the relevance order, an all-zero target (an
# empty history) leaves lam * score.  A DeviceLookup that holds the key as a LABEL key runs ebn_label_target_f32 and
# ebn_calibrated_rerank_f32 (csrc/ebn_calibrate.hip: one wave per list, the pool's label rows in LDS); a plain dict, or a
# DeviceLookup with ``device=None``, runs in float64 numpy list by list.
@dataclass(frozen=True)
class Calibrated:
    """``model.recommend(..., rerank=Calibrated(lookup, key, lam, pool, alpha, target, history_weights))``: re-rank each
    impression's ``pool`` most relevant candidates so that the list's distribution over the labels ``lookup`` (a DeviceLookup)
    holds under the label key ``key`` stays close to ``target``: "history" (the impression's own click history, each slot weighted
    by ``history_weights`` [H], e.g. ebrec.utils._decay weights; default all ones), a {label: weight} dict, or a [C] array aligned
    to ``lookup.label_vocabulary(key)``.  ``pool`` must lie in [top_n, 64], ``alpha`` in (0, 1)."""
    lookup: DeviceLookup
    key: str
    lam: float = 0.7
    pool: int = 50
    alpha: float = 0.01
    target: object = "history"
    history_weights: object = None


def check_alpha(alpha) -> float:
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:  # NaN fails both comparisons
        raise ValueError(f"alpha must lie in (0, 1), got {alpha}")
    return alpha


def given_target(target, vocabulary: list) -> np.ndarray:
    """A {label: weight} dict, a [C] array or an [n, C] array -> float64 of the same shape, every row normalised to sum 1 (a
    row of zeros stays).  ValueError: a label outside the vocabulary, a wrong width, a negative or non-finite weight."""
    C = len(vocabulary)
    if isinstance(target, dict):
        column = {label: c for c, label in enumerate(vocabulary)}
        unknown = [label for label in target if label not in column]
        if unknown:
            raise ValueError(f"target labels outside the lookup's vocabulary: {unknown[:5]}")
        p = np.zeros(C)
        for label, weight in target.items():
            p[column[label]] = float(weight)
    else:
        p = np.array(target, dtype=np.float64)
        if p.ndim not in (1, 2) or p.shape[-1] != C:
            raise ValueError(f"a target array must be [C] or [n, C] with C = {C} labels, got shape {p.shape}")
    if not np.isfinite(p).all() or (p < 0).any():
        raise ValueError("target weights must be finite and not negative")
    total = p.sum(-1, keepdims=True)
    return p / np.where(total == 0, 1.0, total)


def check_history_weights(weights):
    """None, or a float64 [H] array of finite, non-negative weights with 1 <= H <= 256"""
    if weights is None:
        return None
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or not 1 <= w.size <= MAX_HISTORY or not np.isfinite(w).all() or (w < 0).any():
        raise ValueError(f"history_weights must be 1 to {MAX_HISTORY} finite weights >= 0, one per history slot")
    return w


def _history_rows(lookup: DeviceLookup, histories) -> np.ndarray:
    """[n, H] int32 rows of the lookup's tables, -1 for an id that is no key and behind the end of a ragged list"""
    if isinstance(histories, np.ndarray) and histories.ndim == 2 and histories.dtype != object:
        return lookup.rows_of(histories).reshape(histories.shape)
    flat, off = lookup.map_lists(histories)
    n = len(off) - 1
    length = np.diff(off)
    rows = np.full((n, int(length.max()) if n else 0), -1, np.int32)
    rows[np.repeat(np.arange(n), length), np.arange(len(flat)) - np.repeat(off[:-1], length)] = flat
    return rows


def label_target(W, hist_rows, weights, flags):
    """One ebn_label_target_f32 call on device tensors: W [n_rows, C] float32, hist_rows [U, H] int32, weights [H] float32 or
    None -> target [U, C] float32.  ``flags`` [2] int32 accumulates."""
    import torch

    from ebrec import _hip

    U, H = hist_rows.shape
    target = torch.empty(U, W.shape[1], dtype=torch.float32, device=hist_rows.device)
    with torch.cuda.device(hist_rows.device):
        _hip.call("ebn_label_target_f32", _hip.ptr(W), W.shape[0], W.shape[1], _hip.ptr(hist_rows), H, _hip.ptr(weights),
                  _hip.ptr(target), _hip.ptr(flags), U, _hip.stream_handle())
    return target


def calibrated_select(W, pool_rows, pool_rel, target, k: int, lam: float, alpha: float, flags, want_obj: bool = False):
    """One ebn_calibrated_rerank_f32 call on device tensors: W [n_rows, C] float32, pool_rows [U, P] int32, pool_rel [U, P]
    float32, target [U, C] or [C] (one row for all) float32 -> (sel [U, k] int32 pool indices, -1 in empty slots; obj [U, k]
    float32 or None).  ``flags`` [2] int32 accumulates."""
    import torch

    from ebrec import _hip

    U, P = pool_rows.shape
    C = W.shape[1]
    sel = torch.empty(U, k, dtype=torch.int32, device=pool_rows.device)
    obj = torch.empty(U, k, dtype=torch.float32, device=pool_rows.device) if want_obj else None
    with torch.cuda.device(pool_rows.device):
        _hip.call("ebn_calibrated_rerank_f32", _hip.ptr(W), W.shape[0], C, _hip.ptr(pool_rows), _hip.ptr(pool_rel), P, _hip.ptr(target),
                  C if target.dim() == 2 else 0, k, float(lam), float(alpha), _hip.ptr(sel), _hip.ptr(obj), _hip.ptr(flags), U,
                  _hip.stream_handle())
    return sel, obj


def _on_device(lookup_dict, lookup_key: str) -> bool:
    return isinstance(lookup_dict, DeviceLookup) and lookup_dict.holds(lookup_key) and len(lookup_dict) > 0


def _check_label_key(lookup_dict, lookup_key: str) -> DeviceLookup:
    if isinstance(lookup_dict, DeviceLookup) and lookup_key not in lookup_dict.label_keys:
        raise ValueError(f"'{lookup_key}' is not a label key of the lookup")
    return label_lookup(lookup_dict, lookup_key)


def _device_limits(lookup: DeviceLookup, lookup_key: str, H: int = 0):
    C = len(lookup.label_vocabulary(lookup_key))
    if not 1 <= C <= MAX_LABELS:
        raise ValueError(f"the device path supports 1 to {MAX_LABELS} labels, '{lookup_key}' has {C}")
    if H > MAX_HISTORY:
        raise ValueError(f"the device path supports histories of at most {MAX_HISTORY} articles, got {H}")


def _slot_weights(weights, H: int):
    if weights is not None and len(weights) < H:
        raise ValueError(f"history_weights has {len(weights)} entries, the longest history {H}")
    return None if weights is None else weights[:H]


def history_distribution(histories, lookup_dict, lookup_key: str, weights=None):
    """(p [n, C] float64, vocabulary): p[u] = sum_h w_h row(histories[u][h]) / sum_h w_h over the history ids that are keys of
    the lookup, with row() the label row of module comment above and ``weights`` one weight per history SLOT (default all
    ones); no valid id, or a weight sum of 0, gives a zero row.  ``histories`` is an [n, H] id array or ragged lists.  float64
    numpy on the host path, ebn_label_target_f32 (float32 sums) with a DeviceLookup that holds the key."""
    lookup = _check_label_key(lookup_dict, lookup_key)
    weights = check_history_weights(weights)
    vocabulary = lookup.label_vocabulary(lookup_key)
    rows = _history_rows(lookup, histories)
    n, H = rows.shape
    weights = _slot_weights(weights, H)
    if n == 0 or H == 0 or not vocabulary:
        return np.zeros((n, len(vocabulary))), vocabulary
    if _on_device(lookup_dict, lookup_key):
        import torch

        _device_limits(lookup, lookup_key, H)
        W = lookup.device_table(lookup_key)
        w = None if weights is None else torch.from_numpy(weights.astype(np.float32)).to(W.device)
        flags = torch.zeros(2, dtype=torch.int32, device=W.device)
        return label_target(W, torch.from_numpy(rows).to(W.device), w, flags).cpu().numpy().astype(np.float64), vocabulary
    W = lookup._label_table(lookup_key)[1]
    w = np.where(rows >= 0, 1.0 if weights is None else weights[None, :], 0.0)  # [n, H]
    total = np.einsum("nh,nhc->nc", w, W[np.maximum(rows, 0)])
    wsum = w.sum(1, keepdims=True)
    return np.where(wsum > 0, total / np.where(wsum > 0, wsum, 1.0), 0.0), vocabulary


def _host_calibrated_select(rows_w: np.ndarray, present: np.ndarray, rel: np.ndarray, p: np.ndarray, k: int, lam: float, alpha: float) -> list:
    """pool indices of one list, float64: rows_w [P, C] the label rows (anything where absent), p [C] the target"""
    left = present.copy()
    S = np.zeros_like(p)
    pos = p > 0
    picks = []
    for t in range(k):
        if not left.any():
            break
        q = (1.0 - alpha) * (S[None, :] + rows_w) / (t + 1) + alpha * p[None, :]
        kl = (p[pos] * np.log(p[pos] / q[:, pos])).sum(1)
        obj = lam * np.where(left, rel, 0.0) - (1.0 - lam) * kl
        best = int(np.argmax(np.where(left, obj, -np.inf)))  # the first of equal objectives: the smaller pool index
        picks.append(best)
        left[best] = False
        S = S + rows_w[best]
    return picks


def calibrated_rerank(ids, scores, lookup_dict, lookup_key: str, top_n: int, target="history", histories=None, history_weights=None,
                      lam: float = 0.7, alpha: float = 0.01, return_scores: bool = False, fill_id=-1):
    """ids [n, P] with their scores [n, P] -> ids [n, top_n]: the calibrated order of each pool (comment above), lists left
    shorter than ``top_n`` padded with ``fill_id``.  An id that is no key of ``lookup_dict`` and an entry whose score is not
    finite are absent.  ``target``: "history" (then ``histories`` [n, H] ids or n ragged lists, ids that are no keys ignored,
    each slot weighted by ``history_weights`` [H]), a {label: weight} dict, a [C] array aligned to the label vocabulary, or an
    [n, C] array; given targets are normalised in float64.  ``return_scores``: also the given score of each kept entry
    [n, top_n] (-inf in the padding), in selection order, which is NOT monotone.
    ValueError: ``lam`` outside [0, 1], ``alpha`` outside (0, 1), P > 64, ``top_n`` outside [1, 64], ``lookup_key`` not a label
    key of a DeviceLookup, target="history" without ``histories``, and, on the device path, more than 128 labels or histories
    longer than 256."""
    lam, alpha = check_lam(lam), check_alpha(alpha)
    ids = np.asarray(ids)
    scores = np.asarray(scores)
    if scores.dtype.kind != "f":
        scores = scores.astype(np.float64)
    if ids.ndim != 2 or scores.shape != ids.shape:
        raise ValueError(f"ids and scores must be [n, P] arrays of one shape, got {ids.shape} and {scores.shape}")
    n, P = ids.shape
    if P > MAX_POOL:
        raise ValueError(f"pools of at most {MAX_POOL} entries are supported, got P = {P}")
    if not 1 <= int(top_n) <= MAX_TOP_N:
        raise ValueError(f"top_n must lie in [1, {MAX_TOP_N}], got {top_n}")
    top_n = int(top_n)
    lookup = _check_label_key(lookup_dict, lookup_key)
    vocabulary = lookup.label_vocabulary(lookup_key)
    from_history = isinstance(target, str)
    if from_history:
        if target != "history":
            raise ValueError(f"target must be 'history', a {{label: weight}} dict or an array, got {target!r}")
        if histories is None:
            raise ValueError("target='history' needs the click histories (histories=...)")
        if len(histories) != n:
            raise ValueError(f"{len(histories)} histories for {n} lists")
        history_weights = check_history_weights(history_weights)
    else:
        given = given_target(target, vocabulary)
        if given.ndim == 2 and len(given) != n:
            raise ValueError(f"{len(given)} target rows for {n} lists")
    device = _on_device(lookup_dict, lookup_key)
    if device:  # the kernels' limits, found before anything is uploaded
        hist = _history_rows(lookup, histories) if from_history else np.empty((n, 0), np.int32)
        _device_limits(lookup, lookup_key, hist.shape[1])
    fill = np.asarray(fill_id) if ids.dtype.kind in "US" else np.asarray(fill_id, dtype=ids.dtype)  # a string filler is not cut short
    if n == 0 or P == 0:
        out = np.full((n, top_n), fill)
        return (out, np.full((n, top_n), -np.inf, scores.dtype)) if return_scores else out

    if device:
        import torch

        W = lookup.device_table(lookup_key)
        flags = torch.zeros(2, dtype=torch.int32, device=W.device)
        if from_history:
            w = _slot_weights(history_weights, hist.shape[1])
            if hist.shape[1] == 0:
                p = torch.zeros(len(vocabulary), dtype=torch.float32, device=W.device)
            else:
                p = label_target(W, torch.from_numpy(hist).to(W.device),
                                 None if w is None else torch.from_numpy(w.astype(np.float32)).to(W.device), flags)
        else:
            p = torch.from_numpy(given.astype(np.float32)).to(W.device)
        rows = torch.from_numpy(lookup.rows_of(ids).reshape(n, P)).to(W.device)
        rel = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(W.device)
        sel = calibrated_select(W, rows, rel, p, top_n, lam, alpha, flags)[0].cpu().numpy().astype(np.int64)
    else:
        p = history_distribution(histories, lookup, lookup_key, history_weights)[0] if from_history else given
        W = lookup._label_table(lookup_key)[1]
        rows = lookup.rows_of(ids).reshape(n, P)
        sel = np.full((n, top_n), -1, np.int64)
        rel64 = scores.astype(np.float64)
        for r in range(n):
            present = (rows[r] >= 0) & np.isfinite(rel64[r])
            picks = _host_calibrated_select(W[np.maximum(rows[r], 0)], present, rel64[r], p[r] if p.ndim == 2 else p, top_n, lam, alpha)
            sel[r, :len(picks)] = picks
    kept = np.maximum(sel, 0)
    out = np.where(sel >= 0, np.take_along_axis(ids, kept, 1), fill)
    if return_scores:
        return out, np.where(sel >= 0, np.take_along_axis(scores, kept, 1), -np.inf).astype(scores.dtype)
    return out
