"""Greedy Maximal-Marginal-Relevance (MMR) re-ranking: trade a list's relevance against its IntralistDiversity.

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
the device path.  ``model.recommend(..., rerank=MMR(...))`` runs the same kernel on the model's own top-``pool``."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ebrec.evaluation.beyond_accuracy import DeviceLookup
from ebrec.evaluation.utils import check_key_in_all_nested_dicts

MAX_POOL, MAX_TOP_N = 64, 64  # limits of ebn_mmr_rerank_f32 (include/ebnerd_hip.h)


@dataclass(frozen=True)
class MMR:
    """``model.recommend(..., rerank=MMR(lookup, key, lam, pool))``: re-rank each impression's ``pool`` most relevant candidates
    by MMR over the unit vectors ``lookup`` (a DeviceLookup) holds under ``key``.  ``pool`` must lie in [top_n, 64]."""
    lookup: DeviceLookup
    key: str
    lam: float = 0.7
    pool: int = 50


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


def mmr_select(unit, pool_rows, pool_rel, k: int, lam: float, flags, want_obj: bool = False):
    """One ebn_mmr_rerank_f32 call on device tensors: unit [n_rows, D] float32, pool_rows [U, P] int32, pool_rel [U, P] float32
    -> (sel [U, k] int32 pool indices, -1 in empty slots; obj [U, k] float32 or None).  ``flags`` [2] int32 accumulates."""
    import torch

    from ebrec import _hip

    U, P = pool_rows.shape
    sel = torch.empty(U, k, dtype=torch.int32, device=pool_rows.device)
    obj = torch.empty(U, k, dtype=torch.float32, device=pool_rows.device) if want_obj else None
    with torch.cuda.device(pool_rows.device):
        _hip.call("ebn_mmr_rerank_f32", _hip.ptr(unit), unit.shape[0], unit.shape[1], _hip.ptr(pool_rows), _hip.ptr(pool_rel), P, k,
                  float(lam), _hip.ptr(sel), _hip.ptr(obj), _hip.ptr(flags), U, _hip.stream_handle())
    return sel, obj


def _host_select(vectors: np.ndarray, present: np.ndarray, rel: np.ndarray, k: int, lam: float) -> list:
    """pool indices of one list, float64: vectors [P, D] as stored (normalised here, a zero row stays zero)"""
    norm = np.sqrt((vectors * vectors).sum(1, keepdims=True))
    unit = vectors / np.where(norm == 0, 1.0, norm)
    with np.errstate(invalid="ignore"):
        dist = np.clip(1.0 - unit @ unit.T, 0.0, 2.0)
    dist = np.where(np.isnan(dist), 0.0, dist)
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


def mmr_rerank(ids, scores, lookup_dict, lookup_key: str, top_n: int, lam: float = 0.7, return_scores: bool = False, fill_id=-1):
    """ids [n, P] with their scores [n, P] -> ids [n, top_n]: the MMR order of each pool (module docstring), lists left shorter
    than ``top_n`` padded with ``fill_id``.  An id that is no key of ``lookup_dict`` and an entry whose score is not finite are
    absent.  ``return_scores``: also the given score of each kept entry [n, top_n] (-inf in the padding), in selection order --
    which is NOT monotone: a later pick may carry a higher score than an earlier one's successor would have.
    ValueError: ``lam`` outside [0, 1], P > 64, ``top_n`` outside [1, 64], ``lookup_key`` not a vector key, and, on the device
    path, a vector width that is no multiple of 4."""
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
        sel = mmr_select(unit, rows, rel, top_n, lam, flags)[0].cpu().numpy().astype(np.int64)
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
            picks = _host_select(vectors, present, rel64[r], top_n, lam)
            sel[r, :len(picks)] = picks
    kept = np.maximum(sel, 0)
    out = np.where(sel >= 0, np.take_along_axis(ids, kept, 1), fill)
    if return_scores:
        return out, np.where(sel >= 0, np.take_along_axis(scores, kept, 1), -np.inf).astype(scores.dtype)
    return out
