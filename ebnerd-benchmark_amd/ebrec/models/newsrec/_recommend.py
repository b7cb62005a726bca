"""Top-N recommendation lists from a trained model: every impression of an eval loader against ONE shared candidate list
(the reference's beyond-accuracy workflow, examples/beyond_accuracy/make_beyond_accuracy.ipynb, cell "Your Model").

    ids = model.recommend(loader, candidate_ids, top_n=5)                    # [n_impressions, 5] article ids
    IntralistDiversity()(ids, lookup_dict=DeviceLookup(articles, ["emb"]), lookup_key="emb")

All cacheable models score as act(user . news): the catalogue is encoded once, a batch costs its user vectors, and
``ebn_topk_score_f32`` scores a tile of users against the streamed candidates keeping only each user's best ``top_n`` -- the
[users, candidates] score matrix is never materialised.  A model takes part by offering three hooks:

    _recommend_loader_method                 what an eval loader must offer (the name of a method)
    _recommend_index(loader)              -> {article id: row of news_all}  (host only: arguments are checked before the device works)
    _recommend_cache(loader)              -> (cache, news_all [n_rows, F] device tensor)
    _user_vectors_cached(cache, loader, i) -> (user [b, F] device tensor, his_rows [b, H] rows of news_all)

``rerank=MMR(lookup, key, lam, pool)`` (ebrec/evaluation/rerank.py) diversifies the lists: the same launch keeps each user's best
``pool``, their positions are mapped to rows of the lookup's unit table on the device, and ``ebn_mmr_rerank_f32`` picks ``top_n`` of
them greedily by lam * score + (1 - lam) * (distance to the nearest item already picked).
"""
from __future__ import annotations

import numpy as np
import torch

from ebrec import _hip
from ebrec.evaluation.rerank import MAX_POOL, MMR, check_lam, mmr_select

MAX_TOP_N, MAX_EXCLUDE = 64, 256  # limits of ebn_topk_score_f32 (include/ebnerd_hip.h)


def candidate_rows(row_of_id: dict, candidate_ids=None):
    """(ids [M], rows [M] int32) of the candidate list.  ``None``: every article of the index, in row order -- row 0, the
    unknown / padding article, is no key of the index and so never a candidate.  Ids that are not in the index raise."""
    if candidate_ids is None:
        items = sorted(row_of_id.items(), key=lambda kv: kv[1])
        return np.asarray([k for k, _ in items]), np.asarray([r for _, r in items], dtype=np.int32)
    ids = np.asarray(candidate_ids).reshape(-1)
    keys = ids.tolist()
    missing = [k for k in dict.fromkeys(keys) if k not in row_of_id]
    if missing:
        more = f" and {len(missing) - 5} more" if len(missing) > 5 else ""
        raise ValueError(f"candidate ids not in the loader's article index: {missing[:5]}{more}")
    return ids, np.fromiter((row_of_id[k] for k in keys), dtype=np.int32, count=len(keys))


def _check(model, loader, top_n, scores):
    if scores not in ("sigmoid", "raw"):
        raise ValueError(f"scores must be 'sigmoid' or 'raw', got {scores!r}")
    if not 1 <= int(top_n) <= MAX_TOP_N:
        raise ValueError(f"top_n must lie in [1, {MAX_TOP_N}], got {top_n}")
    if not hasattr(model, "_user_vectors_cached"):
        raise NotImplementedError(f"{type(model).__name__} has no catalogue to rank against")
    if not getattr(loader, "eval_mode", False):
        raise ValueError("recommend needs an eval-mode loader (eval_mode=True): one row per impression")
    need = model._recommend_loader_method
    if not hasattr(loader, need):
        raise ValueError(f"{type(loader).__name__} lacks {need}(), which {type(model).__name__}'s cached scoring path needs")


def _check_rerank(rerank, top_n, cand_ids):
    """Host side of ``rerank=``: -> (pool, lookup rows [M] int32 of the candidates).  Everything that can be wrong with the
    arguments is found here, before the device works."""
    if not isinstance(rerank, MMR):
        raise ValueError(f"rerank must be None or an MMR(lookup, key, lam, pool), got {type(rerank).__name__}")
    check_lam(rerank.lam)
    pool = int(rerank.pool)
    if not top_n <= pool <= MAX_POOL:
        raise ValueError(f"the MMR pool must lie in [top_n, {MAX_POOL}] = [{top_n}, {MAX_POOL}], got {pool}")
    lookup, key = rerank.lookup, rerank.key
    if not (hasattr(lookup, "holds") and lookup.holds(key) and key in lookup.vector_keys):
        raise ValueError(f"MMR needs a DeviceLookup that holds '{key}' as a vector key")
    rows = lookup.rows_of(cand_ids)
    if (rows < 0).any():
        missing = list(dict.fromkeys(np.asarray(cand_ids)[rows < 0].tolist()))
        more = f" and {len(missing) - 5} more" if len(missing) > 5 else ""
        raise ValueError(f"candidate ids without a '{key}' vector in the MMR lookup: {missing[:5]}{more}")
    D = lookup.host_table(key).shape[1]
    if D == 0 or D % 4:
        raise ValueError(f"MMR needs a vector width that is a positive multiple of 4, '{key}' has {D}")
    return min(pool, len(rows)), rows


def topk(users: torch.Tensor, news_all: torch.Tensor, cand_rows, exclude, k: int, sigmoid: bool, flags: torch.Tensor, n_splits: int = 0):
    """One ebn_topk_score_f32 call on device tensors -> (pos [U, k] int32, score [U, k] float32); ``flags`` accumulates."""
    U, F = users.shape
    n_rows = news_all.shape[0]
    M = n_rows if cand_rows is None else cand_rows.shape[0]
    X = 0 if exclude is None else exclude.shape[1]
    pos = torch.empty(U, k, dtype=torch.int32, device=users.device)
    score = torch.empty(U, k, dtype=torch.float32, device=users.device)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_topk_auto_splits(U, M))
    ws_bytes = int(lib.ebn_topk_workspace_bytes(U, k, max(splits, 1)))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=users.device)
    _hip.call("ebn_topk_score_f32", _hip.ptr(users), _hip.ptr(news_all), n_rows, _hip.ptr(cand_rows), M, _hip.ptr(exclude), X, k,
              1 if sigmoid else 0, splits, _hip.ptr(pos), _hip.ptr(score), _hip.ptr(flags), _hip.ptr(ws), ws.numel(), U, F,
              _hip.stream_handle())
    return pos, score


def recommend(model, loader, candidate_ids=None, top_n=10, exclude_history=True, return_scores=False, scores="sigmoid", fill_id=-1,
              users_per_call=65536, rerank=None):
    """ids [n_impressions, top_n] of the loader's article ids: each impression's ``top_n`` best of ``candidate_ids`` (``None``:
    every article of the loader's index) by the model's score, best first, ties by position in ``candidate_ids``.
    ``exclude_history`` drops the articles of the impression's own history; a list left shorter than ``top_n`` is padded with
    ``fill_id`` (score -inf).  ``return_scores``: also the scores [n_impressions, top_n] float32 ('sigmoid': what
    ``scorer.predict`` gives for the pair, 'raw': the dot product).  The catalogue cache is built for the current weights and
    dropped on return.
    ``rerank=MMR(lookup, key, lam=0.7, pool=50)``: each list is the greedy MMR order of the impression's ``pool`` best candidates
    (``pool`` in [top_n, 64], clamped to the number of candidates; every candidate id must have a ``key`` vector in ``lookup``)
    with the score chosen by ``scores`` as the relevance; ``lam = 1`` gives the plain lists.  The returned scores are then still
    the MODEL's score of each kept item, in selection order: they are NOT monotone along a list."""
    _check(model, loader, top_n, scores)
    top_n = int(top_n)
    cand_ids, rows = candidate_rows(model._recommend_index(loader), candidate_ids)
    if top_n > len(rows):
        raise ValueError(f"top_n = {top_n} is larger than the number of candidates ({len(rows)})")
    if rerank is not None:
        pool, lookup_rows = _check_rerank(rerank, top_n, cand_ids)
    cache, news_all = model._recommend_cache(loader)
    news_all = news_all.contiguous()
    device = news_all.device
    cand_d = torch.from_numpy(rows).to(device)
    flags = torch.zeros(2, dtype=torch.int32, device=device)
    if rerank is not None:
        unit = rerank.lookup.device_table(rerank.key)
        row_of_pos = torch.from_numpy(lookup_rows).to(device)  # candidate position -> row of the lookup's table
    pos_out, score_out, users, his, pending = [], [], [], [], 0

    def flush():
        nonlocal pending
        if not users:
            return
        u = torch.cat(users).contiguous()
        ex = torch.cat(his).contiguous() if exclude_history else None
        if rerank is None:
            p, s = topk(u, news_all, cand_d, ex, top_n, scores == "sigmoid", flags)
        else:  # the pool, its rows in the lookup's table (-1 stays -1), the greedy picks, and the picks' positions and scores
            pp, ps = topk(u, news_all, cand_d, ex, pool, scores == "sigmoid", flags)
            pool_rows = torch.where(pp >= 0, row_of_pos[pp.clamp(min=0).long()], pp).contiguous()
            sel, _ = mmr_select(unit.to(device), pool_rows, ps, top_n, rerank.lam, flags)
            kept = sel.clamp(min=0).long()
            p = torch.where(sel >= 0, pp.gather(1, kept), sel)
            s = torch.where(sel >= 0, ps.gather(1, kept), torch.full_like(ps[:, :1], float("-inf")))
        pos_out.append(p)
        score_out.append(s)
        users.clear()
        his.clear()
        pending = 0

    for i in range(len(loader)):
        user, his_rows = model._user_vectors_cached(cache, loader, i)
        if exclude_history:
            h = torch.as_tensor(np.ascontiguousarray(his_rows, dtype=np.int32)).to(device)
            if h.shape[1] > MAX_EXCLUDE:
                raise ValueError(f"exclude_history supports histories of at most {MAX_EXCLUDE} articles, got {h.shape[1]}")
            if his and his[0].shape[1] != h.shape[1]:
                flush()
            his.append(h)
        users.append(user)
        pending += user.shape[0]
        if pending >= users_per_call:
            flush()
    flush()
    if not pos_out:
        ids = np.full((0, top_n), fill_id, dtype=np.asarray(cand_ids).dtype if len(cand_ids) else np.int64)
        return (ids, np.zeros((0, top_n), np.float32)) if return_scores else ids
    pos = torch.cat(pos_out).cpu().numpy().astype(np.int64)
    row_bad, nan_seen = (int(v) for v in flags.cpu().tolist())
    if row_bad:
        raise IndexError("candidate row out of range for the encoded catalogue")
    if nan_seen:
        raise FloatingPointError("NaN scores: the model's user or news vectors are not finite")
    ids = np.where(pos >= 0, cand_ids[np.maximum(pos, 0)], np.asarray(fill_id, dtype=cand_ids.dtype))
    if return_scores:
        return ids, torch.cat(score_out).cpu().numpy()
    return ids
