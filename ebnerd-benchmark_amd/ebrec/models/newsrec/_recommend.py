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
launch is ``ebn_npa_topk_score_f32`` (``npa_topk`` below, ``NPAModel.recommend_pairwise``).

``rerank=MMR(lookup, key, lam, pool)`` (ebrec/evaluation/rerank.py) diversifies the lists: the same launch keeps each user's best
``pool``, their positions are mapped to rows of the lookup's unit table on the device, and ``ebn_mmr_rerank_f32`` picks ``top_n`` of
them greedily by lam * score + (1 - lam) * (distance to the nearest item already picked).
``rerank=Calibrated(lookup, key, lam, pool, alpha, target, history_weights)`` calibrates them instead: the pool is formed the same
way, ``ebn_label_target_f32`` turns the batch's history rows (mapped to the lookup's rows through one host-built int32 map) into
each user's target label distribution, and ``ebn_calibrated_rerank_f32`` picks ``top_n`` greedily by
lam * score - (1 - lam) * KL(target || the list's label distribution).

``window=Freshness(published, max_age, min_age)`` (ebrec/evaluation/freshness.py) restricts every impression to the candidates
published inside its own time window: the candidates are sorted by publish time, which makes an impression's admissible set one
range [lo, hi) of positions, the users of a launch are sorted by ``lo``, and ``ebn_topk_score_window_f32`` lets a 128-user
workgroup walk only the candidate tiles its users' ranges meet (``topk_window`` below).
"""
from __future__ import annotations

import numpy as np
import torch

from ebrec import _hip
from ebrec.evaluation.freshness import Freshness
from ebrec.evaluation.rerank import (
    MAX_HISTORY, MAX_LABELS, MAX_POOL, MMR, Calibrated, calibrated_select, check_alpha, check_history_weights, check_lam,
    given_target, label_target, mmr_select,
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
    if not isinstance(rerank, (MMR, Calibrated)):
        raise ValueError(f"rerank must be None or an MMR(lookup, key, lam, pool) or a Calibrated(lookup, key, ...), got {type(rerank).__name__}")
    check_lam(rerank.lam)
    pool = int(rerank.pool)
    if not top_n <= pool <= MAX_POOL:
        raise ValueError(f"the {type(rerank).__name__} pool must lie in [top_n, {MAX_POOL}] = [{top_n}, {MAX_POOL}], got {pool}")
    lookup, key = rerank.lookup, rerank.key
    if isinstance(rerank, Calibrated):
        return min(pool, len(cand_ids)), _check_calibrated(rerank, cand_ids)
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
    own (NPA)."""
    if window is not None:
        if getattr(model, "_recommend_topk", None) is not None:
            raise NotImplementedError(f"window= is not supported for {type(model).__name__}: its scoring launch has no windowed form")
        if not isinstance(window, Freshness):
            raise ValueError(f"window must be None or a Freshness(published, max_age, min_age), got {type(window).__name__}")
    _check(model, loader, top_n, scores)
    top_n = int(top_n)
    index = model._recommend_index(loader)
    cand_ids, rows = candidate_rows(index, candidate_ids)
    if top_n > len(rows):
        raise ValueError(f"top_n = {top_n} is larger than the number of candidates ({len(rows)})")
    if window is not None:  # the candidates by publish time from here on: positions, lookup rows and the final id mapping alike
        order, win_lo, win_hi = window.windows(cand_ids, window.impression_times(loader))
        cand_ids, rows = cand_ids[order], rows[order]
        win_all = np.ascontiguousarray(np.stack([win_lo, win_hi], 1), dtype=np.int32)  # [n_impressions, 2], loader order
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
        unit = rerank.lookup.device_table(rerank.key).to(device)  # MMR: the unit rows; Calibrated: the label table
        row_of_pos = torch.from_numpy(lookup_rows).to(device)  # candidate position -> row of the lookup's table
    if from_history:
        lookup_row_of_news = torch.from_numpy(_history_row_map(index, rerank.lookup, news_all.shape[0])).to(device)
        slot_w = check_history_weights(rerank.history_weights)
    elif calibrated:
        shared = torch.from_numpy(given_target(rerank.target, rerank.lookup.label_vocabulary(rerank.key)).astype(np.float32)).to(device)
    need_his = exclude_history or from_history
    sigmoid = scores == "sigmoid"
    model_topk = getattr(model, "_recommend_topk", None)  # the scoring launch: the model's own, or act(user . news)
    if window is not None:
        launch = lambda u, ex, k, w: topk_window(u, news_all, cand_d, w, ex, k, sigmoid, flags)
    elif model_topk is None:
        launch = lambda u, ex, k, w: topk(u, news_all, cand_d, ex, k, sigmoid, flags)
    else:
        launch = lambda u, ex, k, w: model_topk(cache, u, cand_d, ex, k, sigmoid, flags)
    pos_out, score_out, users, his, wins, pending = [], [], [], [], [], 0

    def flush():
        nonlocal pending
        if not users:
            return
        u = torch.cat(users).contiguous()
        hh = torch.cat(his).contiguous() if need_his else None
        wd = perm = None
        if window is not None:  # users, histories and windows sorted by lo (stable): neighbours share their candidate tiles
            wd = torch.from_numpy(np.concatenate(wins)).to(device)
            perm = torch.argsort(wd[:, 0], stable=True)
            u, wd = u[perm].contiguous(), wd[perm].contiguous()
            hh = hh[perm].contiguous() if need_his else None
        ex = hh if exclude_history else None
        if rerank is None:
            p, s = launch(u, ex, top_n, wd)
        else:  # the pool, its rows in the lookup's table (-1 stays -1), the greedy picks, and the picks' positions and scores
            pp, ps = launch(u, ex, pool, wd)
            pool_rows = torch.where(pp >= 0, row_of_pos[pp.clamp(min=0).long()], pp).contiguous()
            if not calibrated:
                sel, _ = mmr_select(unit, pool_rows, ps, top_n, rerank.lam, flags)
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
        if perm is not None:  # back to loader order
            p, s = torch.empty_like(p).index_copy_(0, perm, p), torch.empty_like(s).index_copy_(0, perm, s)
        pos_out.append(p)
        score_out.append(s)
        users.clear()
        his.clear()
        wins.clear()
        pending = 0

    for i in range(len(loader)):
        user, his_rows = model._user_vectors_cached(cache, loader, i)
        if need_his:
            h = torch.as_tensor(np.ascontiguousarray(his_rows, dtype=np.int32)).to(device)
            if exclude_history and h.shape[1] > MAX_EXCLUDE:
                raise ValueError(f"exclude_history supports histories of at most {MAX_EXCLUDE} articles, got {h.shape[1]}")
            if from_history and not 1 <= h.shape[1] <= MAX_HISTORY:
                raise ValueError(f"a history target supports histories of 1 to {MAX_HISTORY} articles, got {h.shape[1]}")
            if from_history and slot_w is not None and len(slot_w) != h.shape[1]:
                raise ValueError(f"history_weights has {len(slot_w)} entries, the loader's histories {h.shape[1]} slots")
            if his and his[0].shape[1] != h.shape[1]:
                flush()
            his.append(h)
        if window is not None:
            w = win_all[i * loader.batch_size: i * loader.batch_size + user.shape[0]]
            if len(w) != user.shape[0]:
                raise ValueError(f"batch {i} has {user.shape[0]} impressions, the loader's frame holds {len(w)} rows for it")
            wins.append(w)
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
