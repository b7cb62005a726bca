"""Top-N recommendation lists from a trained model: every impression of an eval loader against ONE shared candidate list
(the reference's beyond-accuracy workflow, examples/beyond_accuracy/make_beyond_accuracy.ipynb, cell "Your Model").

    ids = model.recommend(loader, candidate_ids, top_n=5)                    # [n_impressions, 5] article ids
    IntralistDiversity()(ids, lookup_dict=DeviceLookup(articles, ["emb"]), lookup_key="emb")

Most cacheable models score as act(user . news): the catalogue is encoded once, a batch costs its user vectors, and
``ebn_topk_score_f32`` scores a tile of users against the streamed candidates keeping only each user's best ``top_n`` -- the
[users, candidates] score matrix is never materialised.  A model takes part by offering three hooks:

    _recommend_loader_method                 what an eval loader must offer (the name of a method)
    _recommend_index(loader)              -> {article id: row of news_all}  (host only: arguments are checked before the device works)
    _recommend_cache(loader)              -> (cache, news_all [n_rows, F] device tensor)
    _user_vectors_cached(cache, loader, i) -> (user [b, F] device tensor, his_rows [b, H] rows of news_all)

and, where act(user . news) is not its score, a fourth that replaces the scoring launch (everything around it stays this module's):

    _recommend_topk(cache, users, cand_rows, exclude, k, sigmoid, flags) -> (pos [U, k] int32, score [U, k] float32)

with ``users`` the concatenated first results of ``_user_vectors_cached`` (whatever the model packs into a row) and the contract of
``ebn_topk_score_f32`` for everything else.  ``_recommend_cache`` then returns, in place of ``news_all``, any device tensor with one
leading row per catalogue row.  NPA is the one such model: its news vector depends on the user, a row is ``user_vec | Qn`` and the
launch is ``ebn_npa_topk_score_f32`` (``npa_topk`` below, ``NPAModel.recommend_pairwise``).  Such a model offers the windowed form of
its launch (see ``window=`` below) as one more hook, passed to the body both entries share (``_recommend``):

    _recommend_topk_window(cache, users, cand_rows, window, exclude, k, sigmoid, flags) -> (pos [U, k] int32, score [U, k] float32)

NPA's is ``ebn_npa_topk_score_window_f32`` (``npa_topk_window`` below) behind ``NPAModel.recommend_pairwise_windowed``.

``rerank=MMR(lookup, key, lam, pool)`` (ebrec/evaluation/rerank.py) diversifies the lists: the same launch keeps each user's best
``pool``, their positions are mapped to rows of the lookup's unit table on the device, and ``ebn_mmr_rerank_f32`` picks ``top_n`` of
them greedily by lam * score + (1 - lam) * (distance to the nearest item already picked).
``rerank=DPP(lookup, key, lam, pool)`` takes the same path into ``ebn_dpp_rerank_f32``: greedy DPP MAP inference, each pick by
lam * score + (1 - lam) * log(conditional variance of the item given the items already picked).
``rerank=Calibrated(lookup, key, lam, pool, alpha, target, history_weights)`` calibrates them instead: the pool is formed the same
way, ``ebn_label_target_f32`` turns the batch's history rows (mapped to the lookup's rows through one host-built int32 map) into
each user's target label distribution, and ``ebn_calibrated_rerank_f32`` picks ``top_n`` greedily by
lam * score - (1 - lam) * KL(target || the list's label distribution).

``window=Freshness(published, max_age, min_age)`` (ebrec/evaluation/freshness.py) restricts every impression to the candidates
published inside its own time window: the candidates are sorted by publish time, which makes an impression's admissible set one
range [lo, hi) of positions, the users of a launch are sorted by ``lo``, and ``ebn_topk_score_window_f32`` lets a 128-user
workgroup walk only the candidate tiles its users' ranges meet (``topk_window`` below).

``rank_targets(model, loader, targets=None, candidate_ids=None, ...)`` is the accuracy side of the same lists: where the article an
impression clicked stands among ALL candidates, under the same exclusion and freshness rules.  It shares this module's host path
with ``recommend`` (checks, candidate rows, windows, cache, batching, the sort by ``lo``, the flags) and launches
``ebn_target_rank_f32`` (``target_rank`` below): the same GEMM with a count in place of the selection, 12 bytes per pair.
``ebrec.evaluation.rank_metrics`` turns the ranks into hit-rate@k, MRR and nDCG@k.  A model with a scoring launch of its own offers
its counting form as a fifth hook, passed to the same body (``_rank_targets``):

    _rank_launch(cache, users, cand_rows, target_pos, window, exclude, sigmoid, flags) -> (rank [U], count [U], score [U])

NPA's is ``ebn_npa_target_rank_f32`` (``npa_target_rank`` below) behind ``NPAModel.rank_targets_pairwise``; it takes windows, and the
lists its windowed ranks refer to are those of ``NPAModel.recommend_pairwise_windowed``.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ebrec import _hip
from ebrec.evaluation.freshness import Freshness
from ebrec.evaluation.rerank import (
    DPP, MAX_HISTORY, MAX_LABELS, MAX_POOL, MMR, Calibrated, calibrated_select, check_alpha, check_history_weights, check_lam,
    dpp_select, given_target, label_target, mmr_select,
)

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
    if not isinstance(rerank, (MMR, DPP, Calibrated)):
        raise ValueError("rerank must be None or an MMR(lookup, key, lam, pool), a DPP(lookup, key, lam, pool) or a Calibrated(lookup, key, ...), "
                         f"got {type(rerank).__name__}")
    check_lam(rerank.lam)
    pool = int(rerank.pool)
    if not top_n <= pool <= MAX_POOL:
        raise ValueError(f"the {type(rerank).__name__} pool must lie in [top_n, {MAX_POOL}] = [{top_n}, {MAX_POOL}], got {pool}")
    lookup, key = rerank.lookup, rerank.key
    if isinstance(rerank, Calibrated):
        return min(pool, len(cand_ids)), _check_calibrated(rerank, cand_ids)
    name = type(rerank).__name__  # MMR or DPP: one contract
    if not (hasattr(lookup, "holds") and lookup.holds(key) and key in lookup.vector_keys):
        raise ValueError(f"{name} needs a DeviceLookup that holds '{key}' as a vector key")
    rows = lookup.rows_of(cand_ids)
    if (rows < 0).any():
        missing = list(dict.fromkeys(np.asarray(cand_ids)[rows < 0].tolist()))
        more = f" and {len(missing) - 5} more" if len(missing) > 5 else ""
        raise ValueError(f"candidate ids without a '{key}' vector in the {name} lookup: {missing[:5]}{more}")
    D = lookup.host_table(key).shape[1]
    if D == 0 or D % 4:
        raise ValueError(f"{name} needs a vector width that is a positive multiple of 4, '{key}' has {D}")
    return min(pool, len(rows)), rows


def _check_calibrated(rerank: Calibrated, cand_ids):
    """-> lookup rows [M] int32 of the candidates; the rest of what can be wrong with a Calibrated(...)"""
    lookup, key = rerank.lookup, rerank.key
    check_alpha(rerank.alpha)
    if not (hasattr(lookup, "holds") and lookup.holds(key) and key in lookup.label_keys):
        raise ValueError(f"Calibrated needs a DeviceLookup that holds '{key}' as a label key")
    C = len(lookup.label_vocabulary(key))
    if not 1 <= C <= MAX_LABELS:
        raise ValueError(f"Calibrated supports 1 to {MAX_LABELS} labels, '{key}' has {C}")
    if isinstance(rerank.target, str):
        if rerank.target != "history":
            raise ValueError(f"the Calibrated target must be 'history', a {{label: weight}} dict or a [C] array, got {rerank.target!r}")
        check_history_weights(rerank.history_weights)
    elif given_target(rerank.target, lookup.label_vocabulary(key)).ndim != 1:
        raise ValueError("a given Calibrated target is ONE distribution for every impression: a {label: weight} dict or a [C] array")
    rows = lookup.rows_of(cand_ids)
    if (rows < 0).any():
        missing = list(dict.fromkeys(np.asarray(cand_ids)[rows < 0].tolist()))
        more = f" and {len(missing) - 5} more" if len(missing) > 5 else ""
        raise ValueError(f"candidate ids without a '{key}' label row in the Calibrated lookup: {missing[:5]}{more}")
    return rows


def _history_row_map(row_of_id: dict, lookup, n_news_rows: int) -> np.ndarray:
    """[n_news_rows] int32: row of the encoded catalogue -> row of the lookup's tables, -1 for the padding row 0, for rows no
    article id points at and for articles the lookup lacks"""
    out = np.full(n_news_rows, -1, np.int32)
    if row_of_id:
        ids = np.asarray(list(row_of_id))
        rows = np.fromiter(row_of_id.values(), dtype=np.int64, count=len(row_of_id))
        keep = (rows > 0) & (rows < n_news_rows)
        out[rows[keep]] = lookup.rows_of(ids[keep])
    return out


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


def topk_window(users: torch.Tensor, news_all: torch.Tensor, cand_rows, window: torch.Tensor, exclude, k: int, sigmoid: bool,
                flags: torch.Tensor, n_splits: int = 0):
    """One ebn_topk_score_window_f32 call on device tensors: ``topk`` with window [U, 2] int32, user u may only receive the
    candidate positions window[u, 0] <= c < window[u, 1] -> (pos [U, k] int32, score [U, k] float32); ``flags`` accumulates.
    Cheapest with the users sorted by window[:, 0]: a workgroup of 128 users skips the candidate tiles none of their windows meets."""
    U, F = users.shape
    n_rows = news_all.shape[0]
    M = n_rows if cand_rows is None else cand_rows.shape[0]
    X = 0 if exclude is None else exclude.shape[1]
    if window.shape != (U, 2) or window.dtype != torch.int32 or not window.is_contiguous():
        raise ValueError(f"window must be a contiguous [{U}, 2] int32 tensor, got {tuple(window.shape)} {window.dtype}")
    pos = torch.empty(U, k, dtype=torch.int32, device=users.device)
    score = torch.empty(U, k, dtype=torch.float32, device=users.device)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_topk_auto_splits(U, M))
    ws_bytes = int(lib.ebn_topk_workspace_bytes(U, k, max(splits, 1)))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=users.device)
    _hip.call("ebn_topk_score_window_f32", _hip.ptr(users), _hip.ptr(news_all), n_rows, _hip.ptr(cand_rows), M, _hip.ptr(window),
              _hip.ptr(exclude), X, k, 1 if sigmoid else 0, splits, _hip.ptr(pos), _hip.ptr(score), _hip.ptr(flags), _hip.ptr(ws),
              ws.numel(), U, F, _hip.stream_handle())
    return pos, score


def npa_topk(users: torch.Tensor, Q: torch.Tensor, Ua_all: torch.Tensor, Vd_all: torch.Tensor, cand_rows, exclude, k: int, sigmoid: bool,
             flags: torch.Tensor, n_splits: int = 0):
    """One ebn_npa_topk_score_f32 call on device tensors (users [U, F], Q [U, A], Ua_all [n_rows, L, A], Vd_all [n_rows, L, F])
    -> (pos [U, k] int32, score [U, k] float32); ``flags`` accumulates."""
    U, F = users.shape
    n_rows, L, A = Ua_all.shape
    M = n_rows if cand_rows is None else cand_rows.shape[0]
    X = 0 if exclude is None else exclude.shape[1]
    pos = torch.empty(U, k, dtype=torch.int32, device=users.device)
    score = torch.empty(U, k, dtype=torch.float32, device=users.device)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_npa_topk_auto_splits(U, M, L))
    ws_bytes = int(lib.ebn_topk_workspace_bytes(U, k, max(splits, 1)))  # the partial lists are ebn_topk_score_f32's
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=users.device)
    _hip.call("ebn_npa_topk_score_f32", _hip.ptr(users), _hip.ptr(Q), _hip.ptr(Ua_all), _hip.ptr(Vd_all), n_rows, _hip.ptr(cand_rows), M,
              _hip.ptr(exclude), X, k, 1 if sigmoid else 0, splits, _hip.ptr(pos), _hip.ptr(score), _hip.ptr(flags), _hip.ptr(ws),
              ws.numel(), U, L, F, A, _hip.stream_handle())
    return pos, score


def npa_topk_window(users: torch.Tensor, Q: torch.Tensor, Ua_all: torch.Tensor, Vd_all: torch.Tensor, cand_rows, window: torch.Tensor,
                    exclude, k: int, sigmoid: bool, flags: torch.Tensor, n_splits: int = 0):
    """One ebn_npa_topk_score_window_f32 call on device tensors: ``npa_topk`` with window [U, 2] int32, user u may only receive the
    candidate positions window[u, 0] <= c < window[u, 1] -> (pos [U, k] int32, score [U, k] float32); ``flags`` accumulates.
    Cheapest with the users sorted by window[:, 0]: a workgroup of 128 users skips the candidate steps none of their windows meets."""
    U, F = users.shape
    n_rows, L, A = Ua_all.shape
    M = n_rows if cand_rows is None else cand_rows.shape[0]
    X = 0 if exclude is None else exclude.shape[1]
    if window.shape != (U, 2) or window.dtype != torch.int32 or not window.is_contiguous():
        raise ValueError(f"window must be a contiguous [{U}, 2] int32 tensor, got {tuple(window.shape)} {window.dtype}")
    pos = torch.empty(U, k, dtype=torch.int32, device=users.device)
    score = torch.empty(U, k, dtype=torch.float32, device=users.device)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_npa_topk_auto_splits(U, M, L))
    ws_bytes = int(lib.ebn_topk_workspace_bytes(U, k, max(splits, 1)))  # the partial lists are ebn_topk_score_f32's
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=users.device)
    _hip.call("ebn_npa_topk_score_window_f32", _hip.ptr(users), _hip.ptr(Q), _hip.ptr(Ua_all), _hip.ptr(Vd_all), n_rows, _hip.ptr(cand_rows),
              M, _hip.ptr(window), _hip.ptr(exclude), X, k, 1 if sigmoid else 0, splits, _hip.ptr(pos), _hip.ptr(score), _hip.ptr(flags),
              _hip.ptr(ws), ws.numel(), U, L, F, A, _hip.stream_handle())
    return pos, score


def target_rank(users: torch.Tensor, news_all: torch.Tensor, cand_rows, target_pos: torch.Tensor, window, exclude, sigmoid: bool,
                flags: torch.Tensor, n_splits: int = 0):
    """One ebn_target_rank_f32 call on device tensors: target_pos [U] int32 positions in the candidate list (< 0: none), window
    [U, 2] int32 or None -> (rank [U] int32: 1-based place of the target in ``topk``'s order, 0 = not ranked; count [U] int32:
    the user's admissible candidates; score [U] float32: the target's score, -inf where rank is 0); ``flags`` accumulates."""
    U, F = users.shape
    n_rows = news_all.shape[0]
    M = n_rows if cand_rows is None else cand_rows.shape[0]
    X = 0 if exclude is None else exclude.shape[1]
    if target_pos.shape != (U,) or target_pos.dtype != torch.int32 or not target_pos.is_contiguous():
        raise ValueError(f"target_pos must be a contiguous [{U}] int32 tensor, got {tuple(target_pos.shape)} {target_pos.dtype}")
    if window is not None and (window.shape != (U, 2) or window.dtype != torch.int32 or not window.is_contiguous()):
        raise ValueError(f"window must be a contiguous [{U}, 2] int32 tensor, got {tuple(window.shape)} {window.dtype}")
    rank = torch.empty(U, dtype=torch.int32, device=users.device)
    count = torch.empty(U, dtype=torch.int32, device=users.device)
    score = torch.empty(U, dtype=torch.float32, device=users.device)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_topk_auto_splits(U, M))
    ws_bytes = int(lib.ebn_target_rank_workspace_bytes(U, max(splits, 1)))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=users.device)
    _hip.call("ebn_target_rank_f32", _hip.ptr(users), _hip.ptr(news_all), n_rows, _hip.ptr(cand_rows), M, _hip.ptr(target_pos),
              _hip.ptr(window), _hip.ptr(exclude), X, 1 if sigmoid else 0, splits, _hip.ptr(rank), _hip.ptr(count), _hip.ptr(score),
              _hip.ptr(flags), _hip.ptr(ws), ws.numel(), U, F, _hip.stream_handle())
    return rank, count, score


def npa_target_rank(users: torch.Tensor, Q: torch.Tensor, Ua_all: torch.Tensor, Vd_all: torch.Tensor, cand_rows, target_pos: torch.Tensor,
                    window, exclude, sigmoid: bool, flags: torch.Tensor, n_splits: int = 0):
    """One ebn_npa_target_rank_f32 call on device tensors: the operands of ``npa_topk``, target_pos and window as for ``target_rank``
    -> (rank [U] int32: 1-based place of the target in ``npa_topk``'s order, 0 = not ranked; count [U] int32; score [U] float32:
    the target's score, -inf where rank is 0); ``flags`` accumulates."""
    U, F = users.shape
    n_rows, L, A = Ua_all.shape
    M = n_rows if cand_rows is None else cand_rows.shape[0]
    X = 0 if exclude is None else exclude.shape[1]
    if target_pos.shape != (U,) or target_pos.dtype != torch.int32 or not target_pos.is_contiguous():
        raise ValueError(f"target_pos must be a contiguous [{U}] int32 tensor, got {tuple(target_pos.shape)} {target_pos.dtype}")
    if window is not None and (window.shape != (U, 2) or window.dtype != torch.int32 or not window.is_contiguous()):
        raise ValueError(f"window must be a contiguous [{U}, 2] int32 tensor, got {tuple(window.shape)} {window.dtype}")
    rank = torch.empty(U, dtype=torch.int32, device=users.device)
    count = torch.empty(U, dtype=torch.int32, device=users.device)
    score = torch.empty(U, dtype=torch.float32, device=users.device)
    lib = _hip.lib()
    splits = n_splits if n_splits > 0 else int(lib.ebn_npa_topk_auto_splits(U, M, L))
    ws_bytes = int(lib.ebn_npa_target_rank_workspace_bytes(U, max(splits, 1)))  # one range needs it too: the target scores
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=users.device)
    _hip.call("ebn_npa_target_rank_f32", _hip.ptr(users), _hip.ptr(Q), _hip.ptr(Ua_all), _hip.ptr(Vd_all), n_rows, _hip.ptr(cand_rows), M,
              _hip.ptr(target_pos), _hip.ptr(window), _hip.ptr(exclude), X, 1 if sigmoid else 0, splits, _hip.ptr(rank), _hip.ptr(count),
              _hip.ptr(score), _hip.ptr(flags), _hip.ptr(ws), ws.numel(), U, L, F, A, _hip.stream_handle())
    return rank, count, score


def _check_window(model, window):
    if window is not None:
        if getattr(model, "_recommend_topk", None) is not None:
            raise NotImplementedError(f"window= is not supported for {type(model).__name__}: its scoring launch has no windowed form")
        if not isinstance(window, Freshness):
            raise ValueError(f"window must be None or a Freshness(published, max_age, min_age), got {type(window).__name__}")


def _by_publish_time(window, loader, cand_ids, rows):
    """the candidates by publish time -- positions, lookup rows and the final id mapping alike -- and the impressions' ranges
    [n_impressions, 2] int32 in loader order"""
    order, win_lo, win_hi = window.windows(cand_ids, window.impression_times(loader))
    return cand_ids[order], rows[order], np.ascontiguousarray(np.stack([win_lo, win_hi], 1), dtype=np.int32)


def _launch_batches(model, cache, loader, device, need_his, exclude_history, win_all, users_per_call, run, check_history=None,
                    repeat=None):
    """The loop both ``recommend`` and ``rank_targets`` run over the loader's batches: user vectors (and history rows, and windows)
    are collected until ``users_per_call`` impressions are pending, then launched together.  ``repeat(first, n)`` (or None) gives,
    for the n impressions from loader row ``first`` on, a device index [P] of the impressions the launch's rows stand for (an
    impression may be taken several times, or not at all).  With windows the rows of a launch are sorted by ``lo`` (stable), so
    that neighbours share their candidate tiles.  ``run(users, his, window, first, perm)`` (``perm``: the sort, or None) -> a tuple
    of tensors with one leading entry per row; they come back in the order the rows had before the sort.  -> the list of those
    tuples, one per launch."""
    outs, users, his, wins, pending, first = [], [], [], [], 0, 0

    def flush():
        nonlocal pending, first
        if not users:
            return
        u = torch.cat(users).contiguous()
        hh = torch.cat(his).contiguous() if need_his else None
        wd = torch.from_numpy(np.concatenate(wins)).to(device) if win_all is not None else None
        n = u.shape[0]
        if repeat is not None:
            idx = repeat(first, n)
            u = u[idx].contiguous()
            hh = hh[idx].contiguous() if need_his else None
            wd = wd[idx].contiguous() if wd is not None else None
        perm = None
        if wd is not None:  # users, histories and windows sorted by lo (stable): neighbours share their candidate tiles
            perm = torch.argsort(wd[:, 0], stable=True)
            u, wd = u[perm].contiguous(), wd[perm].contiguous()
            hh = hh[perm].contiguous() if need_his else None
        out = run(u, hh, wd, first, perm)
        if perm is not None:  # back to loader order
            out = tuple(torch.empty_like(t).index_copy_(0, perm, t) for t in out)
        outs.append(out)
        users.clear()
        his.clear()
        wins.clear()
        pending = 0
        first += n

    for i in range(len(loader)):
        user, his_rows = model._user_vectors_cached(cache, loader, i)
        if need_his:
            h = torch.as_tensor(np.ascontiguousarray(his_rows, dtype=np.int32)).to(device)
            if exclude_history and h.shape[1] > MAX_EXCLUDE:
                raise ValueError(f"exclude_history supports histories of at most {MAX_EXCLUDE} articles, got {h.shape[1]}")
            if check_history is not None:
                check_history(h)
            if his and his[0].shape[1] != h.shape[1]:
                flush()
            his.append(h)
        if win_all is not None:
            w = win_all[i * loader.batch_size: i * loader.batch_size + user.shape[0]]
            if len(w) != user.shape[0]:
                raise ValueError(f"batch {i} has {user.shape[0]} impressions, the loader's frame holds {len(w)} rows for it")
            wins.append(w)
        users.append(user)
        pending += user.shape[0]
        if pending >= users_per_call:
            flush()
    flush()
    return outs


def _raise_flags(flags):
    row_bad, nan_seen = (int(v) for v in flags.cpu().tolist())
    if row_bad:
        raise IndexError("candidate row out of range for the encoded catalogue")
    if nan_seen:
        raise FloatingPointError("NaN scores: the model's user or news vectors are not finite")


def recommend(model, loader, candidate_ids=None, top_n=10, exclude_history=True, return_scores=False, scores="sigmoid", fill_id=-1,
              users_per_call=65536, rerank=None, window=None):
    """ids [n_impressions, top_n] of the loader's article ids: each impression's ``top_n`` best of ``candidate_ids`` (``None``:
    every article of the loader's index) by the model's score, best first, ties by position in ``candidate_ids``.
    ``exclude_history`` drops the articles of the impression's own history; a list left shorter than ``top_n`` is padded with
    ``fill_id`` (score -inf).  ``return_scores``: also the scores [n_impressions, top_n] float32 ('sigmoid': what
    ``scorer.predict`` gives for the pair, 'raw': the dot product).  The catalogue cache is built for the current weights and
    dropped on return.
    ``rerank=MMR(lookup, key, lam=0.7, pool=50)``: each list is the greedy MMR order of the impression's ``pool`` best candidates
    (``pool`` in [top_n, 64], clamped to the number of candidates; every candidate id must have a ``key`` vector in ``lookup``)
    with the score chosen by ``scores`` as the relevance; ``lam = 1`` gives the plain lists.  The returned scores are then still
    the MODEL's score of each kept item, in selection order: they are NOT monotone along a list.
    ``rerank=DPP(lookup, key, lam=0.7, pool=50)``: the same pool, lookup and scores, each list in greedy DPP order
    (ebrec/evaluation/rerank.py): lam * score + (1 - lam) * log(conditional variance given the items already picked), which
    penalises an item spanned by several earlier picks even when it is close to none of them; ``lam = 1`` gives the plain lists.
    ``rerank=Calibrated(lookup, key, lam=0.7, pool=50, alpha=0.01, target="history", history_weights=None)``: each list is the
    greedy calibrated order of the same pool (ebrec/evaluation/rerank.py): lam * score - (1 - lam) * KL(target || list) over the
    labels ``lookup`` holds under the label key ``key``.  The target is the label distribution of the impression's own history --
    needed even with ``exclude_history=False``; ``history_weights`` [H] weighs the loader's history slots -- or one given
    {label: weight} dict / [C] array for everybody.  Scores as for MMR.
    ``window=Freshness(published, max_age=None, min_age=0, time_col="impression_time")``: an impression at time t (its row of
    ``loader.X[time_col]``) is only offered the candidates published in [t - max_age, t - min_age]; every candidate needs a publish
    time.  The tie rule then reads: equal scores go to the OLDER article, then to the earlier position in ``candidate_ids``.  A
    window holding fewer than ``top_n`` candidates gives a list padded with ``fill_id``; ``rerank=`` works on top unchanged (its
    pool is the window's best, a history target is not touched by the window).  Not for models with a scoring launch of their
    own (NPA: ``NPAModel.recommend_pairwise_windowed``)."""
    _check_window(model, window)
    return _recommend(model, loader, candidate_ids, top_n, exclude_history, return_scores, scores, fill_id, users_per_call, rerank, window)


def _recommend(model, loader, candidate_ids=None, top_n=10, exclude_history=True, return_scores=False, scores="sigmoid", fill_id=-1,
               users_per_call=65536, rerank=None, window=None, model_window_launch=None):
    """The body of ``recommend``.  ``model_window_launch(cache, users, cand_rows, window, exclude, k, sigmoid, flags)`` -> (pos, score)
    is the windowed form of the model's own scoring launch (``NPAModel._recommend_topk_window``), or None: ``topk_window`` over
    act(user . news)."""
    if window is not None and not isinstance(window, Freshness):
        raise ValueError(f"window must be None or a Freshness(published, max_age, min_age), got {type(window).__name__}")
    _check(model, loader, top_n, scores)
    top_n = int(top_n)
    index = model._recommend_index(loader)
    cand_ids, rows = candidate_rows(index, candidate_ids)
    if top_n > len(rows):
        raise ValueError(f"top_n = {top_n} is larger than the number of candidates ({len(rows)})")
    win_all = None
    if window is not None:  # the candidates by publish time from here on
        cand_ids, rows, win_all = _by_publish_time(window, loader, cand_ids, rows)
    if rerank is not None:
        pool, lookup_rows = _check_rerank(rerank, top_n, cand_ids)
    cache, news_all = model._recommend_cache(loader)
    news_all = news_all.contiguous()
    device = news_all.device
    cand_d = torch.from_numpy(rows).to(device)
    flags = torch.zeros(2, dtype=torch.int32, device=device)
    calibrated = isinstance(rerank, Calibrated)
    from_history = calibrated and isinstance(rerank.target, str)
    if rerank is not None:
        unit = rerank.lookup.device_table(rerank.key).to(device)  # MMR, DPP: the unit rows; Calibrated: the label table
        row_of_pos = torch.from_numpy(lookup_rows).to(device)  # candidate position -> row of the lookup's table
    if from_history:
        lookup_row_of_news = torch.from_numpy(_history_row_map(index, rerank.lookup, news_all.shape[0])).to(device)
        slot_w = check_history_weights(rerank.history_weights)
    elif calibrated:
        shared = torch.from_numpy(given_target(rerank.target, rerank.lookup.label_vocabulary(rerank.key)).astype(np.float32)).to(device)
    need_his = exclude_history or from_history
    sigmoid = scores == "sigmoid"
    model_topk = getattr(model, "_recommend_topk", None)  # the scoring launch: the model's own, or act(user . news)
    if window is not None and model_window_launch is not None:
        launch = lambda u, ex, k, w: model_window_launch(cache, u, cand_d, w, ex, k, sigmoid, flags)
    elif window is not None:
        launch = lambda u, ex, k, w: topk_window(u, news_all, cand_d, w, ex, k, sigmoid, flags)
    elif model_topk is None:
        launch = lambda u, ex, k, w: topk(u, news_all, cand_d, ex, k, sigmoid, flags)
    else:
        launch = lambda u, ex, k, w: model_topk(cache, u, cand_d, ex, k, sigmoid, flags)

    def run(u, hh, wd, first, perm):
        ex = hh if exclude_history else None
        if rerank is None:
            return launch(u, ex, top_n, wd)
        # the pool, its rows in the lookup's table (-1 stays -1), the greedy picks, and the picks' positions and scores
        pp, ps = launch(u, ex, pool, wd)
        pool_rows = torch.where(pp >= 0, row_of_pos[pp.clamp(min=0).long()], pp).contiguous()
        if not calibrated:
            select = dpp_select if isinstance(rerank, DPP) else mmr_select
            sel, _ = select(unit, pool_rows, ps, top_n, rerank.lam, flags)
        else:
            if from_history:  # history rows of the catalogue -> rows of the label table (outside the catalogue: the padding)
                inside = (hh >= 0) & (hh < lookup_row_of_news.shape[0])
                hist_rows = torch.where(inside, lookup_row_of_news[hh.clamp(0, lookup_row_of_news.shape[0] - 1).long()],
                                        torch.full_like(hh, -1)).contiguous()
                w = None if slot_w is None else torch.from_numpy(slot_w.astype(np.float32)).to(device)
                target = label_target(unit, hist_rows, w, flags)
            else:
                target = shared
            sel, _ = calibrated_select(unit, pool_rows, ps, target, top_n, rerank.lam, rerank.alpha, flags)
        kept = sel.clamp(min=0).long()
        p = torch.where(sel >= 0, pp.gather(1, kept), sel)
        s = torch.where(sel >= 0, ps.gather(1, kept), torch.full_like(ps[:, :1], float("-inf")))
        return p, s

    def check_history(h):
        if from_history and not 1 <= h.shape[1] <= MAX_HISTORY:
            raise ValueError(f"a history target supports histories of 1 to {MAX_HISTORY} articles, got {h.shape[1]}")
        if from_history and slot_w is not None and len(slot_w) != h.shape[1]:
            raise ValueError(f"history_weights has {len(slot_w)} entries, the loader's histories {h.shape[1]} slots")

    outs = _launch_batches(model, cache, loader, device, need_his, exclude_history, win_all, users_per_call, run, check_history)
    pos_out, score_out = [o[0] for o in outs], [o[1] for o in outs]
    if not pos_out:
        ids = np.full((0, top_n), fill_id, dtype=np.asarray(cand_ids).dtype if len(cand_ids) else np.int64)
        return (ids, np.zeros((0, top_n), np.float32)) if return_scores else ids
    pos = torch.cat(pos_out).cpu().numpy().astype(np.int64)
    _raise_flags(flags)
    ids = np.where(pos >= 0, cand_ids[np.maximum(pos, 0)], np.asarray(fill_id, dtype=cand_ids.dtype))
    if return_scores:
        return ids, torch.cat(score_out).cpu().numpy()
    return ids


@dataclass
class TargetRanks:
    """One entry per (impression, target) pair, in loader order: ``impression`` the row of ``loader.X``, ``target_id`` the
    article, ``rank`` its 1-based place among the impression's admissible candidates in ``recommend``'s order (0: not ranked --
    no candidate, outside the window, excluded), ``count`` the number of those candidates, ``score`` its score (-inf where
    ``rank`` is 0).  ``ebrec.evaluation.rank_metrics(ranks.rank, counts=ranks.count)`` gives the metrics."""
    impression: np.ndarray
    target_id: np.ndarray
    rank: np.ndarray
    count: np.ndarray
    score: np.ndarray

    def __len__(self):
        return len(self.rank)


def _target_pairs(loader, targets):
    """(impression [P] int64, target id [P]) in loader order.  ``None``: every in-view article labelled 1 in ``loader.y``."""
    n = len(loader.X)
    if targets is None:
        inview = loader.X[loader.inview_col].tolist() if n else []
        per_row = [[a for a, l in zip(ids, labels) if l == 1] for ids, labels in zip(inview, loader.y)]
    else:
        per_row = [np.asarray(t).reshape(-1).tolist() for t in targets]
        if len(per_row) != n:
            raise ValueError(f"targets must hold one id or one list of ids per impression: the loader has {n} rows, got {len(per_row)}")
    imp = np.repeat(np.arange(n, dtype=np.int64), [len(t) for t in per_row])
    flat = [a for t in per_row for a in t]
    return imp, (np.asarray(flat) if flat else np.zeros(0, np.int64))


def rank_targets(model, loader, targets=None, candidate_ids=None, exclude_history=True, window=None, scores="sigmoid",
                 users_per_call=65536) -> TargetRanks:
    """Where each impression's target article stands among ALL of ``candidate_ids`` (``None``: every article of the loader's
    index) by the model's score: the unsampled counterpart of the in-view metrics, under ``recommend``'s rules.  ``rank`` r <= k
    holds exactly when ``recommend(loader, candidate_ids, top_n=k, ...)`` with the same ``exclude_history`` and ``window`` has the
    target at index r - 1, and ``score`` is that slot's score.
    ``targets=None``: every in-view article labelled 1 in ``loader.y`` -- an impression with two clicks gives two pairs; else one
    id or a list of ids per impression.  A target that is not in the candidate list (or not in the loader's article index) is
    no error: its pair comes back with rank 0, as does a target the impression's history excludes or its window does not hold.
    A target id that occurs twice in ``candidate_ids`` is its first occurrence (under ``window=``: the first after the sort by
    publish time).  Not for models with a scoring launch of their own (NPA)."""
    if getattr(model, "_recommend_topk", None) is not None:
        raise NotImplementedError(f"rank_targets is not supported for {type(model).__name__}: its scoring launch has no counting form")
    _check_window(model, window)
    return _rank_targets(model, loader, targets, candidate_ids, exclude_history, window, scores, users_per_call)


def _rank_targets(model, loader, targets=None, candidate_ids=None, exclude_history=True, window=None, scores="sigmoid",
                  users_per_call=65536, model_launch=None) -> TargetRanks:
    """The body of ``rank_targets``.  ``model_launch(cache, users, cand_rows, target_pos, window, exclude, sigmoid, flags)`` ->
    (rank, count, score) is the model's own counting launch (``NPAModel._rank_launch``), or None: ``target_rank`` over act(user . news)."""
    if window is not None and not isinstance(window, Freshness):
        raise ValueError(f"window must be None or a Freshness(published, max_age, min_age), got {type(window).__name__}")
    _check(model, loader, 1, scores)
    index = model._recommend_index(loader)
    cand_ids, rows = candidate_rows(index, candidate_ids)
    win_all = None
    if window is not None:  # the candidates by publish time from here on: a target's position is its position after the sort
        cand_ids, rows, win_all = _by_publish_time(window, loader, cand_ids, rows)
    imp, target_ids = _target_pairs(loader, targets)
    first_pos = {}
    for j, a in enumerate(cand_ids.tolist()):
        first_pos.setdefault(a, j)
    pos_all = np.fromiter((first_pos.get(a, -1) for a in target_ids.tolist()), dtype=np.int32, count=len(target_ids))
    cache, news_all = model._recommend_cache(loader)
    news_all = news_all.contiguous()
    device = news_all.device
    cand_d = torch.from_numpy(rows).to(device)
    flags = torch.zeros(2, dtype=torch.int32, device=device)
    sigmoid = scores == "sigmoid"
    starts = np.searchsorted(imp, np.arange(len(loader.X) + 1))  # the pairs of impression r: starts[r] .. starts[r + 1]
    target_of_launch = []

    def repeat(first, n):
        lo, hi = starts[first], starts[first + n]
        target_of_launch.append(torch.from_numpy(pos_all[lo:hi]).to(device))
        return torch.from_numpy(imp[lo:hi] - first).to(device)

    def run(u, hh, wd, first, perm):
        tp = target_of_launch.pop()
        tp = (tp if perm is None else tp[perm]).contiguous()
        ex = hh if exclude_history else None
        if model_launch is not None:
            return model_launch(cache, u, cand_d, tp, wd, ex, sigmoid, flags)
        return target_rank(u, news_all, cand_d, tp, wd, ex, sigmoid, flags)

    outs = _launch_batches(model, cache, loader, device, exclude_history, exclude_history, win_all, users_per_call, run, repeat=repeat)
    cat = lambda k, dtype: (torch.cat([o[k] for o in outs]).cpu().numpy() if outs else np.zeros(0, dtype))
    rank, count, score = cat(0, np.int32), cat(1, np.int32), cat(2, np.float32)
    _raise_flags(flags)
    return TargetRanks(impression=imp, target_id=target_ids, rank=rank, count=count, score=score)
