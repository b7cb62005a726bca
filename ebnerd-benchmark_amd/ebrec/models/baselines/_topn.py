"""Top-N lists and clicked-article ranks over the WHOLE catalogue for the baselines: the second outlet beside ``predict``, and the
counterpart of the neural models' ``recommend`` / ``rank_targets`` (ebrec/models/newsrec/_recommend.py).

    ids = cv.recommend(df_validation, history=df_history_validation, top_n=10)           # [n_impressions, 10] article ids
    ranks = cv.rank_targets(df_validation, history=df_history_validation)                # the clicked article among ALL articles
    rank_metrics(ranks.rank, ks=(5, 10), counts=ranks.count)                             # hit-rate@k, MRR, nDCG@k

``TopN`` is the host scaffolding ``CoVisitation``, ``ImplicitALS``, ``ContentSimilarity``, ``EASE`` and ``HistoryKNN`` share: the three call forms, the
candidate list, history exclusion, freshness windows, batching, the id mapping and the flags.  A class takes part by offering

    _topn_ids()                    -> the sorted article ids that name the catalogue rows
    _topn_rows_of(ids)             -> int32 catalogue rows, -1 for an unknown id
    _topn_session(histories)       -> a session over these histories (a RaggedLists of article ids): ``on_device``, and
        session.candidates(cand_rows [M] int32)
        session.topk(hist_idx [b], window [b, 2] | None, exclude [b, X] | None, k, flags)          -> (pos [b, k], score [b, k])
        session.rank(hist_idx [b], target_pos [b], window, exclude, flags)                         -> (rank [b], count [b], score [b])

with numpy arguments; the results are numpy on the host path and device tensors on the device path, ``flags`` [2] likewise.  Row
b of a launch uses history ``hist_idx[b]`` (-1: none).  A factory that names a ``history_keys`` parameter --
``_topn_session(histories, history_keys=None)`` -- is also handed one key per history (``HistoryKNN``'s ``exclude_self`` matches
them): the ``user_id`` the frames were joined on, the frame's own ``user_id`` column with a history per row, the caller's
``history_keys=`` with the list form; the other classes are called as before and refuse ``history_keys=``.  Co-visitation's session launches ``ebn_cv_topk_f32`` /
``ebn_cv_target_rank_f32`` (covisit.py), EASE's ``ebn_ease_topk_f32`` / ``ebn_ease_target_rank_f32`` (ease.py), history-kNN's
``ebn_knn_topk_f32`` / ``ebn_knn_target_rank_f32`` (knn.py); ``DenseSession`` below serves the two classes whose users are dense vectors -- ALS fold-in
rows, content-centroid profiles -- with the EXISTING ``ebn_topk_score_f32`` / ``ebn_topk_score_window_f32`` / ``ebn_target_rank_f32``
(columns zero-padded to a multiple of 4), and with float64 numpy twins on the host.

Out of scope: nearest-history top-N, the popularity baselines, re-rankers on baseline lists (DESIGN.md sections 31, 35 and 36)."""
from __future__ import annotations

import inspect

import numpy as np

from ebrec.evaluation.device_metrics import RaggedLists
from ebrec.evaluation.freshness import Freshness
from ebrec.utils._constants import DEFAULT_CLICKED_ARTICLES_COL, DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_USER_COL

from .popularity import _explode, _frame, _ragged_ids

MAX_TOP_N, MAX_EXCLUDE = 64, 256  # limits of the top-k kernels (include/ebnerd_hip.h)


# ---- float64 twins of the dense launches -----------------------------------------------------------------------------------------
def _dense_admissible(users, catalogue, cand_rows, window, exclude, flags):
    """per user: (admissible positions, their float64 scores)"""
    users, catalogue = np.asarray(users, np.float64), np.asarray(catalogue, np.float64)
    cand_rows = np.asarray(cand_rows, np.int64).ravel()
    M, n_rows = cand_rows.size, catalogue.shape[0]
    inside = (cand_rows >= 0) & (cand_rows < n_rows)
    table = catalogue[np.where(inside, cand_rows, 0)]
    for u in range(users.shape[0]):
        lo, hi = 0, M
        if window is not None:
            lo, hi = max(int(window[u][0]), 0), min(int(window[u][1]), M)
            if lo >= hi:
                lo = hi = 0
        adm = np.zeros(M, bool)
        adm[lo:hi] = True
        if (adm & ~inside).any():
            flags[0] = 1
        adm &= inside
        if exclude is not None:
            adm &= ~np.isin(cand_rows, np.asarray(exclude[u], np.int64))
        with np.errstate(all="ignore"):
            s = table @ users[u]
        if (adm & np.isnan(s)).any():
            flags[1] = 1
        adm &= ~np.isnan(s)
        pos = np.flatnonzero(adm)
        yield u, pos, s[pos]


def dense_topk_host(users, catalogue, cand_rows, window, exclude, k, flags):
    """float64 twin of ebn_topk_score_f32 / ebn_topk_score_window_f32 (mode 0) -> (pos [U, k] int32, score [U, k] float32)"""
    U = np.asarray(users).shape[0]
    out_pos, out_score = np.full((U, k), -1, np.int32), np.full((U, k), -np.inf, np.float32)
    for u, pos, s in _dense_admissible(users, catalogue, cand_rows, window, exclude, flags):
        best = np.lexsort((pos, -s))[:k]
        out_pos[u, :best.size], out_score[u, :best.size] = pos[best], s[best]
    return out_pos, out_score


def dense_target_rank_host(users, catalogue, cand_rows, target_pos, window, exclude, flags):
    """float64 twin of ebn_target_rank_f32 (mode 0) -> (rank [U] int32, count [U] int32, score [U] float32)"""
    U, M = np.asarray(users).shape[0], np.asarray(cand_rows).size
    target_pos = np.asarray(target_pos, np.int64).ravel()
    rank, count, t_out = np.zeros(U, np.int32), np.zeros(U, np.int32), np.full(U, -np.inf, np.float32)
    if (target_pos[:U] >= M).any():
        flags[0] = 1
    for u, pos, s in _dense_admissible(users, catalogue, cand_rows, window, exclude, flags):
        count[u] = pos.size
        at = np.flatnonzero(pos == target_pos[u])
        if at.size:
            t = s[at[0]]
            rank[u] = 1 + int(((s > t) | ((s == t) & (pos < target_pos[u]))).sum())
            t_out[u] = t
    return rank, count, t_out


def pad_columns(x):
    """[n, F] float32 with the columns zero-padded to a multiple of 4, at least 4 (numpy or a device tensor, contiguous)"""
    F = x.shape[1]
    Fp = max(4, (F + 3) // 4 * 4)
    if isinstance(x, np.ndarray):
        out = np.zeros((x.shape[0], Fp), np.float32)
        out[:, :F] = x
        return out
    import torch

    out = torch.zeros((x.shape[0], Fp), dtype=torch.float32, device=x.device)
    out[:, :F] = x
    return out


class DenseSession:
    """users [n_hists, F] float32 against catalogue [n_rows, F] float32 by the dot product (numpy arrays: the float64 twins; device
    tensors: the existing top-k / target-rank launches).  A history whose user row is all zero cannot be scored: empty list, rank 0."""

    def __init__(self, users, catalogue):
        self.on_device = not isinstance(users, np.ndarray)
        self.device = users.device if self.on_device else None
        self.users, self.catalogue = pad_columns(users), pad_columns(catalogue)
        live = (self.users != 0).any(1)
        self.scorable = live if not self.on_device else live.cpu().numpy()
        self.cand = None

    def candidates(self, cand_rows):
        self.cand = np.ascontiguousarray(cand_rows, dtype=np.int32)
        if self.on_device:
            import torch

            self.cand = torch.from_numpy(self.cand).to(self.users.device)

    def _rows(self, hist_idx):
        """(user rows of the launch, which of them can be scored)"""
        h = np.asarray(hist_idx, np.int64)
        n = self.scorable.size
        ok = (h >= 0) & (h < n)
        ok[ok] = self.scorable[h[ok]]
        h = np.where(ok, h, 0)
        if not self.on_device:
            return (self.users[h] if n else np.zeros((h.size, self.users.shape[1]), np.float32)), ok
        import torch

        dev = self.users.device
        if n == 0:
            return torch.zeros((h.size, self.users.shape[1]), dtype=torch.float32, device=dev), torch.from_numpy(ok).to(dev)
        return self.users[torch.from_numpy(h).to(dev)].contiguous(), torch.from_numpy(ok).to(dev)

    def topk(self, hist_idx, window, exclude, k, flags):
        u, ok = self._rows(hist_idx)
        if not self.on_device:
            pos, score = dense_topk_host(u, self.catalogue, self.cand, window, exclude, k, flags)
            pos[~ok], score[~ok] = -1, -np.inf
            return pos, score
        import torch

        from ebrec.models.newsrec._recommend import topk, topk_window

        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(u.device)
        with torch.cuda.device(u.device):
            if window is None:
                pos, score = topk(u, self.catalogue, self.cand, up(exclude), k, False, flags)
            else:
                pos, score = topk_window(u, self.catalogue, self.cand, up(window), up(exclude), k, False, flags)
        return torch.where(ok[:, None], pos, torch.full_like(pos, -1)), torch.where(ok[:, None], score, torch.full_like(score, float("-inf")))

    def rank(self, hist_idx, target_pos, window, exclude, flags):
        u, ok = self._rows(hist_idx)
        if not self.on_device:
            rank, count, score = dense_target_rank_host(u, self.catalogue, self.cand, target_pos, window, exclude, flags)
            rank[~ok], count[~ok], score[~ok] = 0, 0, -np.inf
            return rank, count, score
        import torch

        from ebrec.models.newsrec._recommend import target_rank

        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(u.device)
        with torch.cuda.device(u.device):
            rank, count, score = target_rank(u, self.catalogue, self.cand, up(target_pos), up(window), up(exclude), False, flags)
        zero = torch.zeros_like(rank)
        return torch.where(ok, rank, zero), torch.where(ok, count, zero), torch.where(ok, score, torch.full_like(score, float("-inf")))


# ---- the scaffolding ---------------------------------------------------------------------------------------------------------------
def _users(behaviors, history):
    """the three call forms -> (histories RaggedLists of ids, user_hist [n] int32 | None, the behaviours frame | None, n users)"""
    df = behaviors if isinstance(behaviors, RaggedLists) else _frame(behaviors)
    if not hasattr(df, "columns"):
        if history is not None:
            raise ValueError("history= goes with a behaviours frame; recommend(histories) takes the histories themselves")
        flat, off = _ragged_ids(df)
        off = np.ascontiguousarray(off, dtype=np.int64)
        return RaggedLists(np.asarray(flat).ravel(), off), None, None, off.size - 1
    if history is None:
        if DEFAULT_HISTORY_ARTICLE_ID_COL not in df.columns:
            raise ValueError(f"the behaviours frame lacks the column '{DEFAULT_HISTORY_ARTICLE_ID_COL}': pass history=")
        flat, off = _explode(df[DEFAULT_HISTORY_ARTICLE_ID_COL])
        return RaggedLists(flat, off), None, df, len(df)
    hf = _frame(history)
    for frame, col in ((df, DEFAULT_USER_COL), (hf, DEFAULT_USER_COL), (hf, DEFAULT_HISTORY_ARTICLE_ID_COL)):
        if col not in frame.columns:
            raise ValueError(f"a frame lacks the column '{col}'")
    users, first = np.unique(hf[DEFAULT_USER_COL].to_numpy(), return_index=True)  # one history per distinct user
    flat, off = _explode(hf[DEFAULT_HISTORY_ARTICLE_ID_COL].iloc[first])
    asked = df[DEFAULT_USER_COL].to_numpy()
    if users.size == 0:
        return RaggedLists(flat, off), np.full(asked.size, -1, np.int32), df, len(df)
    at = np.minimum(np.searchsorted(users, asked), users.size - 1)
    return RaggedLists(flat, off), np.where(users[at] == asked, at, -1).astype(np.int32), df, len(df)


def _history_keys(model, history, frame, history_keys):
    """(whether the model's session factory takes keys, one key per history of ``_users`` | None)"""
    wants = "history_keys" in inspect.signature(model._topn_session).parameters
    if history_keys is not None:
        if not wants:
            raise ValueError(f"{type(model).__name__} has no use for history_keys=")
        if frame is not None:
            raise ValueError("history_keys= belongs to the list form; the frames are joined on user_id")
        return wants, history_keys
    if not wants or frame is None:
        return wants, None
    if history is not None:
        return wants, np.unique(_frame(history)[DEFAULT_USER_COL].to_numpy())  # the order of _users' histories
    return wants, (frame[DEFAULT_USER_COL].to_numpy() if DEFAULT_USER_COL in frame.columns else None)


def _candidates(model, candidate_ids):
    """(ids [M], rows [M] int32): ``None`` is every fitted article in row order; an unknown or a repeated id raises"""
    if candidate_ids is None:
        ids = np.asarray(model._topn_ids())
        return ids, np.arange(ids.size, dtype=np.int32)
    ids = np.asarray(candidate_ids).reshape(-1)
    rows = model._topn_rows_of(ids)
    if (rows < 0).any():
        missing = list(dict.fromkeys(ids[rows < 0].tolist()))
        more = f" and {len(missing) - 5} more" if len(missing) > 5 else ""
        raise ValueError(f"candidate ids not among the fitted articles: {missing[:5]}{more}")
    if np.unique(rows).size != rows.size:
        raise ValueError("candidate_ids holds an article twice")
    return ids, rows.astype(np.int32)


def _exclusion(rows, offsets):
    """[n_hists, X] int32: each history's last (most recent) 256 distinct known rows, padded with -1"""
    lists = []
    for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
        r = rows[a:b][::-1]
        r = r[r >= 0]
        _, first = np.unique(r, return_index=True)
        lists.append(r[np.sort(first)[:MAX_EXCLUDE]])
    X = max((len(l) for l in lists), default=0)
    out = np.full((len(lists), X), -1, np.int32)
    for i, l in enumerate(lists):
        out[i, :len(l)] = l
    return out


def _raise_flags(flags):
    row_bad, nan_seen = (int(v) for v in (flags if isinstance(flags, np.ndarray) else flags.cpu().numpy()).tolist())
    if row_bad:
        raise IndexError("candidate row out of range for the fitted catalogue")
    if nan_seen:
        raise FloatingPointError("NaN scores: the fitted values or the history weights are not finite")


class _Plan:
    """what ``recommend`` and ``rank_targets`` share: users, candidates (by publish time under a window), windows, exclusion, session"""

    def __init__(self, model, behaviors, history, candidate_ids, exclude_history, window, impression_times, batch_users, history_keys=None):
        if window is not None and not isinstance(window, Freshness):
            raise ValueError(f"window must be None or a Freshness(published, max_age, min_age), got {type(window).__name__}")
        if isinstance(batch_users, (bool, np.bool_)) or int(batch_users) != batch_users or int(batch_users) < 1:
            raise ValueError(f"batch_users must be a positive integer, got {batch_users!r}")
        self.batch = int(batch_users)
        self.histories, self.user_hist, self.frame, self.n = _users(behaviors, history)
        wants_keys, keys = _history_keys(model, history, self.frame, history_keys)
        self.cand_ids, rows = _candidates(model, candidate_ids)
        self.win = None
        if window is not None:
            times = impression_times
            if times is None:
                if self.frame is None or window.time_col not in self.frame.columns:
                    raise ValueError(f"window= needs the impression times: a frame with the column '{window.time_col}' or impression_times=")
                times = self.frame[window.time_col]
            if len(times) != self.n:
                raise ValueError(f"{self.n} impressions but {len(times)} impression times")
            order, lo, hi = window.windows(self.cand_ids, times)  # the candidates by publish time from here on
            self.cand_ids, rows = self.cand_ids[order], rows[order]
            self.win = np.ascontiguousarray(np.stack([lo, hi], 1), dtype=np.int32)
        elif impression_times is not None:
            raise ValueError("impression_times= goes with window=")
        self.rows = np.ascontiguousarray(rows, dtype=np.int32)
        self.ex = None
        if exclude_history:
            flat, off = _ragged_ids(self.histories)
            self.ex = _exclusion(model._topn_rows_of(flat), np.asarray(off, np.int64))
        self.session = model._topn_session(self.histories, history_keys=keys) if wants_keys else model._topn_session(self.histories)
        self.session.candidates(self.rows)
        if self.session.on_device:
            import torch

            self.flags = torch.zeros(2, dtype=torch.int32, device=self.session.device)
        else:
            self.flags = np.zeros(2, np.int32)

    def hist_of(self, imp):
        """history index per impression index (-1: none)"""
        return imp.astype(np.int32) if self.user_hist is None else self.user_hist[imp]

    def launch_args(self, imp):
        h = self.hist_of(imp)
        win = None if self.win is None else np.ascontiguousarray(self.win[imp])
        ex = None
        if self.ex is not None and self.ex.size:
            ex = np.where((h >= 0)[:, None], self.ex[np.maximum(h, 0)], -1).astype(np.int32)
        return h, win, ex


def _cat(parts, on_device, empty):
    if not parts:
        return empty
    if on_device:
        import torch

        return torch.cat(parts)
    return np.concatenate(parts)


class TopN:
    """``recommend`` and ``rank_targets`` for a baseline (see the module docstring for what the class offers)."""

    def recommend(self, behaviors, candidate_ids=None, top_n=10, exclude_history=True, window=None, return_scores=False, fill_id=-1,
                  batch_users=65536, *, history=None, impression_times=None, history_keys=None):
        """ids [n, top_n]: each impression's ``top_n`` best of ``candidate_ids`` (``None``: every fitted article) by the model's score,
        best first, ties by position in ``candidate_ids``.  Call forms: ``recommend(behaviors, history=history_frame)`` joined on
        ``user_id``; ``recommend(behaviors)`` with ``article_id_fixed`` per row; ``recommend(histories)`` over a RaggedLists or lists
        of lists of article ids.  ``exclude_history`` drops the history's own articles (its last 256 distinct known ones);
        ``window=Freshness(...)`` offers an impression only the candidates published inside its window (impression times from the
        frame's column or ``impression_times=``; equal scores then go to the older article).  A list left shorter than ``top_n`` --
        a user that cannot be scored gets an empty one -- is padded with ``fill_id`` (score -inf).  ``return_scores``: also the
        float32 scores [n, top_n], numpy on the host path, a device tensor on the device path.  ``batch_users``: users per launch.
        ``history_keys``: one key per history of the list form, for a class that matches them (``HistoryKNN``'s ``exclude_self``)."""
        if isinstance(top_n, (bool, np.bool_)) or int(top_n) != top_n or not 1 <= int(top_n) <= MAX_TOP_N:
            raise ValueError(f"top_n must be an integer in [1, {MAX_TOP_N}], got {top_n!r}")
        k = int(top_n)
        plan = _Plan(self, behaviors, history, candidate_ids, exclude_history, window, impression_times, batch_users, history_keys)
        pos_parts, score_parts = [], []
        for a in range(0, plan.n, plan.batch):
            imp = np.arange(a, min(a + plan.batch, plan.n), dtype=np.int64)
            h, win, ex = plan.launch_args(imp)
            pos, score = plan.session.topk(h, win, ex, k, plan.flags)
            pos_parts.append(pos)
            score_parts.append(score)
        dev = plan.session.on_device
        pos = _cat(pos_parts, dev, np.zeros((0, k), np.int32))
        pos = (pos.cpu().numpy() if dev and pos_parts else pos).astype(np.int64)
        _raise_flags(plan.flags)
        cand = plan.cand_ids
        fill = np.asarray(fill_id, dtype=cand.dtype) if cand.size else np.asarray(fill_id)
        ids = np.where(pos >= 0, cand[np.maximum(pos, 0)], fill) if cand.size else np.full(pos.shape, fill)
        if not return_scores:
            return ids
        return ids, _cat(score_parts, dev, np.zeros((0, k), np.float32))

    def rank_targets(self, behaviors, targets=None, candidate_ids=None, exclude_history=True, window=None, batch_users=65536, *,
                     history=None, impression_times=None, history_keys=None):
        """Where each impression's target article stands among ALL of ``candidate_ids`` by the model's score, under ``recommend``'s
        rules: a ``TargetRanks`` (impression, target_id, rank, count, score) with one entry per (impression, target) pair, as the
        neural ``rank_targets`` returns it; ``rank`` r <= k holds exactly when ``recommend(..., top_n=k)`` has the target at index
        r - 1.  ``targets=None``: the clicked articles of the behaviours frame; else one id or a list of ids per impression.  A
        target that is no candidate, is excluded, lies outside the window or has no score comes back with rank 0."""
        from ebrec.models.newsrec._recommend import TargetRanks

        plan = _Plan(self, behaviors, history, candidate_ids, exclude_history, window, impression_times, batch_users, history_keys)
        if targets is None:
            if plan.frame is None or DEFAULT_CLICKED_ARTICLES_COL not in plan.frame.columns:
                raise ValueError(f"targets=None needs a behaviours frame with the column '{DEFAULT_CLICKED_ARTICLES_COL}'")
            per_row = [np.asarray([] if t is None else t).reshape(-1).tolist() for t in plan.frame[DEFAULT_CLICKED_ARTICLES_COL]]
        else:
            per_row = [np.asarray(t).reshape(-1).tolist() for t in targets]
            if len(per_row) != plan.n:
                raise ValueError(f"targets must hold one id or one list of ids per impression: {plan.n} impressions, got {len(per_row)}")
        imp_all = np.repeat(np.arange(plan.n, dtype=np.int64), [len(t) for t in per_row])
        flat = [a for t in per_row for a in t]
        target_ids = np.asarray(flat) if flat else np.zeros(0, np.int64)
        first_pos = {a: j for j, a in enumerate(plan.cand_ids.tolist())}
        tp_all = np.fromiter((first_pos.get(a, -1) for a in target_ids.tolist()), dtype=np.int32, count=len(target_ids))
        parts = []
        for a in range(0, imp_all.size, plan.batch):
            imp = imp_all[a:a + plan.batch]
            h, win, ex = plan.launch_args(imp)
            parts.append(plan.session.rank(h, np.ascontiguousarray(tp_all[a:a + plan.batch]), win, ex, plan.flags))
        dev = plan.session.on_device
        host = lambda t: t.cpu().numpy() if dev and parts else t
        rank, count, score = (host(_cat([p[i] for p in parts], dev, np.zeros(0, d))) for i, d in enumerate((np.int32, np.int32, np.float32)))
        _raise_flags(plan.flags)
        return TargetRanks(impression=imp_all, target_id=target_ids, rank=rank, count=count, score=score)
