"""Score blending: a weighted sum of several score columns over the same in-view lists, with the weights fitted by the listwise
softmax cross-entropy the neural models train with.

    blend = ScoreBlend(transforms=["zscore", "rank", "rrf"], l2=1e-3)
    blend.fit(labels, [scores_nrms, scores_pop, scores_cv])              # RaggedLists, lists of lists, or DataFrame columns
    blend.weights, blend.names, blend.losses, blend.converged, blend.n_lists_used, blend.n_one_class, blend.n_nonfinite
    scores = blend.predict([scores_nrms, scores_pop, scores_cv])         # RaggedLists of float64, the sources' offsets
    ScoreBlend.from_weights(["rrf"] * 3, [1.0, 1.0, 1.0])                # a fitted blend from given weights
    RankFusion(k=60.0).predict([...])                                    # unweighted reciprocal-rank fusion
    oof, fold_weights = blend.cross_fit_predict(labels, sources, folds=5, groups=user_ids)

The columns live on different scales (counts, cosines, dot products, sigmoids), so every source is first transformed PER LIST:
``raw`` s_i, ``zscore`` (s_i - mean) / sd (population sd, 0 for a constant list), ``minmax`` (s_i - min) / (max - min) (0 for a
constant list), ``rank`` (n - r_i) / (n - 1) with the mid-rank r_i = 1 + #{s_j > s_i} + #{j != i: s_j == s_i} / 2 (0 for n == 1) and
``rrf`` 1 / (rrf_k + r_i).  A feature is computed in float64 and rounded once to float32; the blend is
``out_i = sum_m w_m f_mi`` in float64.  A list in which some source holds a non-finite score is flagged: ``predict`` gives NaN for
its items and the fit skips it (``n_nonfinite``), as it skips the lists without a positive or without a negative (``n_one_class``).

The fit minimises ``J(w) = (1 / n_used) sum_l loss_l + (l2 / 2) |w|^2`` with ``loss_l = -sum_i t_i log softmax(w . f)_i`` and the
list's positives sharing the target mass, ``t_i = y_i / n_pos``.  J is convex: a damped Newton iteration from w = 0 on the host,
in float64, with the M x M system ``(H / n + l2 I) d = grad J`` and Armijo backtracking by halving (c = 1e-4); the Hessian is summed
in its centred form ``sum_i p_i (f_i - u)(f_i - u)^T``, which stays positive semi-definite for raw features of any size.  Every
evaluation of (sum loss, sum gradient, sum Hessian) is one pass over all lists.

``cross_fit_predict`` is what a results table must use for its blend row: every list is scored with weights fitted on the OTHER
folds (list l is in fold ``l % folds``; with ``groups`` -- user ids, say -- a group's fold is its index in order of first
appearance, modulo ``folds``, so a user never sits on both sides).

Two paths, as in the baselines.  With a visible GPU the transforms, the blend and the sums are the kernels of csrc/ebn_blend.hip
(``ebn_blend_features_f32``, ``ebn_blend_combine_f64``, ``ebn_blend_sums_f64``): the sources are stacked once into one device
tensor (float32 when every source is float32, else float64; a device tensor is used in place) and stay there.  ``device=None`` or
no GPU runs the numpy twins ``blend_features_host``, ``blend_combine_host`` and ``blend_sums_host``.  numpy on the host; torch is
imported only on the device path."""
from __future__ import annotations

import numpy as np

from ebrec.evaluation.device_metrics import RaggedLists, _is_tensor, device_available

# EBN_BL_* of include/ebnerd_hip.h
MAX_SOURCES = 16
RAW, ZSCORE, MINMAX, RANK, RRF = range(5)
KINDS = {"raw": RAW, "zscore": ZSCORE, "minmax": MINMAX, "rank": RANK, "rrf": RRF}
FLAG_NONFINITE = 2


def n_entries(M: int) -> int:
    """length of the sums vector: loss, gradient [M], upper triangle of the Hessian row-major"""
    return 1 + M + M * (M + 1) // 2


def unpack_sums(sums, M: int):
    """sums [1 + M + M (M + 1) / 2] -> (loss, g [M], H [M, M] symmetric)"""
    sums = np.asarray(sums, np.float64)
    H = np.zeros((M, M))
    iu = np.triu_indices(M)
    H[iu] = sums[1 + M:]
    H = H + np.triu(H, 1).T
    return float(sums[0]), sums[1:1 + M].copy(), H


# ---- the numpy twins -----------------------------------------------------------------------------------------------------------
def _segments(offsets, n_items):
    """(numbers of the well-formed lists, their begins, their lengths, list of every covered item, position of every covered item);
    a list whose offsets leave [0, n_items] or run backwards is empty"""
    off = np.asarray(offsets, np.int64)
    o0, o1 = off[:-1], off[1:]
    ok = (o0 >= 0) & (o1 >= o0) & (o1 <= n_items)
    beg, length = np.where(ok, o0, 0), np.where(ok, o1 - o0, 0)
    lid = np.repeat(np.arange(len(o0), dtype=np.int64), length)
    start = np.cumsum(length) - length
    pos = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(start, length) + np.repeat(beg, length)
    return beg, length, lid, pos


def _seg_reduce(ufunc, values, length, empty):
    """ufunc.reduceat over the consecutive segments of ``values`` with the given lengths (an empty segment gives ``empty``)"""
    out = np.full(len(length), empty, np.float64)
    full = length > 0
    if values.size:
        start = (np.cumsum(length) - length)[full]
        out[full] = ufunc.reduceat(values, start)
    return out


def _midranks(s, lid, length):
    """mid-ranks r_i = 1 + #{s_j > s_i} + #{j != i: s_j == s_i} / 2 inside each list (items gathered list by list)"""
    n = s.size
    if n == 0:
        return np.zeros(0)
    order = np.lexsort((-s, lid))  # by list, then descending score
    ls, ll = s[order], lid[order]
    new = np.ones(n, bool)
    new[1:] = (ls[1:] != ls[:-1]) | (ll[1:] != ll[:-1])  # first of a tie group
    first = np.flatnonzero(new)
    count = np.diff(np.append(first, n))
    start_of_list = (np.cumsum(length) - length)[ll[first]]
    r_group = 1.0 + (first - start_of_list) + 0.5 * (count - 1)
    r = np.empty(n)
    r[order] = np.repeat(r_group, count)
    return r


def blend_features_host(scores, offsets, kinds, params):
    """numpy twin of ebn_blend_features_f32 (same contract, include/ebnerd_hip.h): scores [M, n_items] float32 or float64 ->
    (features [M, n_items] float32, flags [n_lists] uint8).  Items outside every well-formed list keep 0."""
    scores = np.asarray(scores)
    if scores.ndim != 2 or not 1 <= scores.shape[0] <= MAX_SOURCES:
        raise ValueError(f"scores must be [M, n_items] with 1 <= M <= {MAX_SOURCES}")
    M, n_items = scores.shape
    beg, length, lid, pos = _segments(offsets, n_items)
    n_lists = len(length)
    features, flags = np.zeros((M, n_items), np.float32), np.zeros(n_lists, np.uint8)
    dn = length.astype(np.float64)
    with np.errstate(all="ignore"):
        for m in range(M):
            kind, param = int(kinds[m]), float(params[m])
            raw = scores[m][pos]
            s = raw.astype(np.float64)  # exact for float32: the same comparisons, the same sums
            nonf = np.bincount(lid, ~np.isfinite(s), minlength=n_lists) > 0
            flags[nonf] |= FLAG_NONFINITE
            if kind == RAW:
                features[m][pos] = raw.astype(np.float32)
                continue
            if kind in (ZSCORE, MINMAX):
                mn, mx = _seg_reduce(np.minimum, s, length, np.inf), _seg_reduce(np.maximum, s, length, -np.inf)
                const = (mx == mn)[lid]
                if kind == MINMAX:
                    f = (s - mn[lid]) / (mx[lid] - mn[lid])
                else:
                    mean = np.bincount(lid, s, minlength=n_lists) / dn
                    sd = np.sqrt(np.bincount(lid, (s - mean[lid]) ** 2, minlength=n_lists) / dn)
                    f = (s - mean[lid]) / sd[lid]
                    const = const | (sd == 0.0)[lid]
                f = np.where(const, 0.0, f)
            elif kind in (RANK, RRF):
                r = _midranks(s, lid, length)
                f = np.where(dn[lid] == 1, 0.0, (dn[lid] - r) / (dn[lid] - 1.0)) if kind == RANK else 1.0 / (param + r)
            else:
                f = np.full(s.size, np.nan)
            features[m][pos] = np.where(nonf[lid], np.nan, f).astype(np.float32)
    return features, flags


def blend_combine_host(scores, offsets, kinds, params, weights):
    """numpy twin of ebn_blend_combine_f64 -> (out [n_items] float64, flags [n_lists] uint8): the weighted sum, m ascending, of the
    float32-rounded features; NaN for every item of a flagged list"""
    features, flags = blend_features_host(scores, offsets, kinds, params)
    w = np.asarray(weights, np.float64)
    _, length, lid, pos = _segments(offsets, features.shape[1])
    out = np.zeros(features.shape[1])
    with np.errstate(all="ignore"):
        for m in range(features.shape[0]):
            out += w[m] * features[m].astype(np.float64)
    out[pos[(flags != 0)[lid]]] = np.nan
    return out, flags


def blend_sums_host(features, labels, offsets, weights, return_abs: bool = False):
    """numpy twin of ebn_blend_sums_f64 -> (sums [1 + M + M (M + 1) / 2] float64, counters [3] int64: lists used, one-class, with a
    feature that is not finite).  ``return_abs``: also the sums of the ABSOLUTE terms of every entry over the used lists,
    ``|loss_l|``, ``sum_i |p_i - t_i| |f_ia|`` and ``sum_i p_i |(f_ia - u_a)(f_ib - u_b)|`` -- the scale of each entry's rounding
    error."""
    f = np.asarray(features)
    if f.ndim != 2 or not 1 <= f.shape[0] <= MAX_SOURCES:
        raise ValueError(f"features must be [M, n_items] with 1 <= M <= {MAX_SOURCES}")
    M, n_items = f.shape
    w = np.asarray(weights, np.float64)
    beg, length, lid, pos = _segments(offsets, n_items)
    n_lists = len(length)
    F = f[:, pos].astype(np.float64)
    y = (np.asarray(labels)[pos] != 0).astype(np.float64)
    n_pos = np.bincount(lid, y, minlength=n_lists)
    one = ~((n_pos > 0) & (n_pos < length))
    bad = ~one & (np.bincount(lid, ~np.isfinite(F).all(axis=0), minlength=n_lists) > 0)
    used = ~one & ~bad
    counters = np.array([used.sum(), one.sum(), bad.sum()], np.int64)
    keep = used[lid]
    F, y, lid_k = F[:, keep], y[keep], lid[keep]
    len_k = np.where(used, length, 0)
    seg = lambda v: np.bincount(lid_k, v, minlength=n_lists)
    z = np.zeros(F.shape[1])
    for m in range(M):
        z += w[m] * F[m]
    zmax = _seg_reduce(np.maximum, z, len_k, 0.0)
    zc = z - zmax[lid_k]
    e = np.exp(zc)
    S = seg(e)
    with np.errstate(all="ignore"):
        p = e / S[lid_k]
        t = y / n_pos[lid_k]
        logp = zc - np.log(S)[lid_k]
        loss_l = -seg(y * logp) / n_pos
    d = p - t
    u = np.stack([seg(p * F[m]) for m in range(M)]) if F.shape[1] else np.zeros((M, n_lists))
    C = F - u[:, lid_k]
    sums, absum = np.zeros(n_entries(M)), np.zeros(n_entries(M))
    sums[0], absum[0] = loss_l[used].sum(), np.abs(loss_l[used]).sum()
    k = 1 + M
    for a in range(M):
        sums[1 + a], absum[1 + a] = (d * F[a]).sum(), (np.abs(d) * np.abs(F[a])).sum()
        for b in range(a, M):
            term = p * (C[a] * C[b])
            sums[k], absum[k] = term.sum(), np.abs(term).sum()
            k += 1
    return (sums, counters, absum) if return_abs else (sums, counters)


# ---- one launch each over device tensors ---------------------------------------------------------------------------------------
def _score_kind(scores):
    import torch

    return 0 if scores.dtype == torch.float32 else 1


def blend_features_call(scores, offsets, kinds, params, form: int = 0):
    """One ebn_blend_features_f32 launch: scores [M, n_items] float32 / float64 and offsets [n_lists + 1] int64 on the device ->
    (features [M, n_items] float32, flags [n_lists] uint8) on the device."""
    import torch

    from ebrec import _hip

    dev, (M, n), n_lists = scores.device, scores.shape, offsets.numel() - 1
    k = torch.tensor([int(v) for v in kinds], dtype=torch.int32, device=dev)
    p = torch.tensor([float(v) for v in params], dtype=torch.float64, device=dev)
    features = torch.zeros((M, n), dtype=torch.float32, device=dev)
    flags = torch.zeros(max(n_lists, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("ebn_blend_features_f32", _hip.ptr(scores), _score_kind(scores), M, n, _hip.ptr(offsets), n_lists, _hip.ptr(k), _hip.ptr(p),
                  form, _hip.ptr(features), _hip.ptr(flags), _hip.stream_handle())
    return features, flags[:n_lists]


def blend_combine_call(scores, offsets, kinds, params, weights, form: int = 0):
    """One ebn_blend_combine_f64 launch -> (out [n_items] float64, flags [n_lists] uint8) on the device."""
    import torch

    from ebrec import _hip

    dev, (M, n), n_lists = scores.device, scores.shape, offsets.numel() - 1
    k = torch.tensor([int(v) for v in kinds], dtype=torch.int32, device=dev)
    p = torch.tensor([float(v) for v in params], dtype=torch.float64, device=dev)
    w = torch.tensor([float(v) for v in weights], dtype=torch.float64, device=dev)
    out = torch.zeros(n, dtype=torch.float64, device=dev)
    flags = torch.zeros(max(n_lists, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("ebn_blend_combine_f64", _hip.ptr(scores), _score_kind(scores), M, n, _hip.ptr(offsets), n_lists, _hip.ptr(k), _hip.ptr(p),
                  _hip.ptr(w), form, _hip.ptr(out), _hip.ptr(flags), _hip.stream_handle())
    return out, flags[:n_lists]


class BlendSums:
    """The buffers of repeated ebn_blend_sums_f64 launches over one set of features: ``BlendSums(features, labels, offsets)(w)`` ->
    (sums, counters) as numpy arrays.  features [M, n_items] float32, labels [n_items] uint8, offsets int64, all on the device."""

    def __init__(self, features, labels, offsets, form: int = 0):
        import torch

        from ebrec import _hip

        self.features, self.labels, self.offsets, self.form = features, labels, offsets, form
        self.M, self.n = features.shape
        self.n_lists, dev = offsets.numel() - 1, features.device
        with torch.cuda.device(dev):
            self.ws_bytes = int(_hip.lib().ebn_blend_sums_workspace_bytes(self.n_lists, self.M))
        self.ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device=dev)
        self.w = torch.zeros(self.M, dtype=torch.float64, device=dev)
        self.sums = torch.zeros(n_entries(self.M), dtype=torch.float64, device=dev)
        self.counters = torch.zeros(3, dtype=torch.int64, device=dev)

    def launch(self, weights):
        import torch

        from ebrec import _hip

        self.w.copy_(torch.as_tensor(np.asarray(weights, np.float64)))
        with torch.cuda.device(self.features.device):
            _hip.call("ebn_blend_sums_f64", _hip.ptr(self.features), _hip.ptr(self.labels), self.M, self.n, _hip.ptr(self.offsets), self.n_lists,
                      _hip.ptr(self.w), self.form, _hip.ptr(self.sums), _hip.ptr(self.counters), _hip.ptr(self.ws), self.ws.numel(),
                      _hip.stream_handle())

    def __call__(self, weights):
        self.launch(weights)
        return self.sums.cpu().numpy(), self.counters.cpu().numpy()


# ---- the host layer ----------------------------------------------------------------------------------------------------------
def _as_ragged(x) -> RaggedLists:
    if isinstance(x, RaggedLists):
        return x
    if hasattr(x, "to_numpy") and not isinstance(x, np.ndarray):  # a DataFrame column
        x = x.to_list() if hasattr(x, "to_list") else list(x)
    return RaggedLists.from_lists([np.asarray(v) for v in x])


def _is_f32(flat) -> bool:
    return str(flat.dtype).endswith("float32")


def _kinds_of(transforms, M=None):
    names = [transforms] * (1 if M is None else M) if isinstance(transforms, str) else list(transforms)
    for t in names:
        if t not in KINDS:
            raise ValueError(f"unknown transform {t!r}: one of {sorted(KINDS)}")
    if M is not None and len(names) != M:
        raise ValueError(f"{len(names)} transforms for {M} sources")
    return names


class ScoreBlend:
    """A per-list-normalised weighted sum of score columns; see the module docstring.  ``transforms``: one name for every source or
    one name per source; ``l2``: the ridge on the weights; ``rrf_k``: the k of the ``rrf`` transform."""

    def __init__(self, transforms="zscore", l2: float = 1e-3, rrf_k: float = 60.0, max_iter: int = 50, tol: float = 1e-9, device="cuda"):
        _kinds_of(transforms)
        if not (np.isfinite(l2) and l2 >= 0 and np.isfinite(rrf_k) and tol > 0 and max_iter >= 1):
            raise ValueError("l2 >= 0, a finite rrf_k, tol > 0 and max_iter >= 1")
        self.transforms, self.l2, self.rrf_k, self.max_iter, self.tol, self.device = transforms, float(l2), float(rrf_k), int(max_iter), float(tol), device
        self.weights = self.names = None
        self.losses, self.converged, self.n_lists_used, self.n_one_class, self.n_nonfinite = [], False, 0, 0, 0

    @classmethod
    def from_weights(cls, transforms, weights, rrf_k: float = 60.0, names=None, device="cuda") -> "ScoreBlend":
        w = np.asarray(weights, np.float64).ravel()
        if not 1 <= w.size <= MAX_SOURCES:
            raise ValueError(f"1 to {MAX_SOURCES} sources, got {w.size}")
        out = cls(transforms=_kinds_of(transforms, w.size), rrf_k=rrf_k, device=device)
        out.weights, out.names, out.converged = w.copy(), list(names) if names is not None else [f"source_{m}" for m in range(w.size)], True
        return out

    # -- operands
    def _on_device(self) -> bool:
        return device_available(self.device)

    def _stack(self, sources):
        """-> (scores [M, n_items] float32 / float64: a device tensor or a numpy array, offsets [n_lists + 1] int64 numpy)"""
        if isinstance(sources, RaggedLists) or not hasattr(sources, "__len__"):
            raise ValueError("sources must be a list of score columns")
        cols = [_as_ragged(s) for s in sources]
        if not 1 <= len(cols) <= MAX_SOURCES:
            raise ValueError(f"1 to {MAX_SOURCES} sources, got {len(cols)}")
        offsets = cols[0].offsets
        for m, c in enumerate(cols[1:], 1):
            if not np.array_equal(c.offsets, offsets):
                raise ValueError(f"source {m} has other offsets than source 0: the columns must cover the same lists")
        f32 = all(_is_f32(c.flat) for c in cols)
        if not self._on_device():
            return np.stack([np.asarray(c.host_flat(), np.float32 if f32 else np.float64) for c in cols]), offsets
        import torch

        dtype, dev = (torch.float32 if f32 else torch.float64), torch.device(self.device)
        rows = [c.flat if _is_tensor(c.flat) else torch.from_numpy(np.array(c.flat)) for c in cols]  # a copy: read-only arrays are welcome
        rows = [r.to(device=dev, dtype=dtype) for r in rows]  # a device tensor of that type is used as it is
        if len(rows) == 1:
            return rows[0].contiguous().view(1, -1), offsets
        return torch.stack(rows), offsets

    def _labels(self, labels, offsets):
        lab = _as_ragged(labels)
        if not np.array_equal(lab.offsets, offsets):
            raise ValueError("the labels have other offsets than the sources")
        y = np.asarray(lab.host_flat())
        if y.size and not np.all((y == 0) | (y == 1)):
            raise ValueError("labels must be 0 or 1")
        return y.astype(np.uint8)

    def _kinds(self, M):
        names = _kinds_of(self.transforms, M)
        return [KINDS[t] for t in names], [self.rrf_k if t == "rrf" else 0.0 for t in names]

    def _sums_fn(self, stack, offsets, y):
        """the features of the stack (one launch) -> a function w -> (sums, counters)"""
        kinds, params = self._kinds(stack.shape[0])
        if _is_tensor(stack):
            import torch

            off = torch.tensor(offsets, device=stack.device)
            features, _ = blend_features_call(stack, off, kinds, params)
            return BlendSums(features, torch.from_numpy(y).to(stack.device), off)
        features, _ = blend_features_host(stack, offsets, kinds, params)
        return lambda w: blend_sums_host(features, y, offsets, w)

    def _objective(self, sums_fn, w):
        sums, counters = sums_fn(w)
        M, n = len(w), int(counters[0])
        if n == 0:
            raise ValueError("no usable list: every list is one-class or holds a non-finite score")
        loss, g, H = unpack_sums(sums, M)
        return loss / n + 0.5 * self.l2 * float(w @ w), g / n + self.l2 * w, H / n + self.l2 * np.eye(M), counters

    def _newton(self, sums_fn, M):
        """damped Newton from w = 0 -> (w, losses, converged, counters)"""
        w = np.zeros(M)
        J, grad, H, counters = self._objective(sums_fn, w)
        losses, converged = [J], False
        for _ in range(self.max_iter):
            if np.max(np.abs(grad)) <= self.tol:
                converged = True
                break
            try:
                d = np.linalg.solve(H, grad)
            except np.linalg.LinAlgError:
                d = np.linalg.lstsq(H, grad, rcond=None)[0]
            slope, step, accepted = float(grad @ d), 1.0, False
            while step >= 2.0 ** -40:
                w_new = w - step * d
                J_new, grad_new, H_new, _ = self._objective(sums_fn, w_new)
                # Armijo, c = 1e-4; the last term is the rounding of J itself, which near the optimum exceeds the decrease asked for
                if np.isfinite(J_new) and J_new <= J - 1e-4 * step * slope + 4 * np.finfo(np.float64).eps * abs(J):
                    w, J, grad, H, accepted = w_new, J_new, grad_new, H_new, True
                    break
                step *= 0.5
            if not accepted:
                break
            losses.append(J)
        else:
            converged = bool(np.max(np.abs(grad)) <= self.tol)
        return w, losses, converged, counters

    # -- the public calls
    def fit(self, labels, sources, names=None) -> "ScoreBlend":
        stack, offsets = self._stack(sources)
        M = stack.shape[0]
        if names is None:
            names = [getattr(s, "name", None) if isinstance(getattr(s, "name", None), str) else f"source_{m}" for m, s in enumerate(sources)]
        if len(names) != M:
            raise ValueError(f"{len(names)} names for {M} sources")
        sums_fn = self._sums_fn(stack, offsets, self._labels(labels, offsets))
        self.weights, self.losses, self.converged, counters = self._newton(sums_fn, M)
        self.names = list(names)
        self.n_lists_used, self.n_one_class, self.n_nonfinite = (int(c) for c in counters)
        return self

    def _combine(self, stack, offsets, weights):
        kinds, params = self._kinds(stack.shape[0])
        if _is_tensor(stack):
            import torch

            return blend_combine_call(stack, torch.tensor(offsets, device=stack.device), kinds, params, weights)[0]
        return blend_combine_host(stack, offsets, kinds, params, weights)[0]

    def predict(self, sources) -> RaggedLists:
        """float64 scores with the sources' offsets (a device tensor on the device path); NaN for the items of a flagged list"""
        if self.weights is None:
            raise ValueError("fit the blend (or build it with from_weights) before predict")
        stack, offsets = self._stack(sources)
        if stack.shape[0] != len(self.weights):
            raise ValueError(f"{stack.shape[0]} sources for {len(self.weights)} weights")
        return RaggedLists(self._combine(stack, offsets, self.weights), offsets)

    def cross_fit_predict(self, labels, sources, folds: int = 5, groups=None):
        """-> (out-of-fold scores as RaggedLists, fold_weights [folds, M]): fold f's lists are scored with weights fitted on the
        lists of every other fold.  The blend itself is left as it is."""
        stack, offsets = self._stack(sources)
        M, n_lists = stack.shape[0], len(offsets) - 1
        if not (isinstance(folds, (int, np.integer)) and 2 <= folds):
            raise ValueError("folds must be an integer >= 2")
        fold = fold_of_lists(n_lists, int(folds), groups)
        y = self._labels(labels, offsets)
        fold_item = np.repeat(fold, np.diff(offsets))
        fold_weights = np.zeros((int(folds), M))
        out = None
        for f in range(int(folds)):
            sums_fn = self._sums_fn(stack, offsets, np.where(fold_item == f, 0, y).astype(np.uint8))  # fold f's lists: no positive, skipped
            fold_weights[f], _, _, _ = self._newton(sums_fn, M)
            scores = self._combine(stack, offsets, fold_weights[f])
            if _is_tensor(scores):
                import torch

                pick = torch.from_numpy(fold_item == f).to(scores.device)
                out = torch.where(pick, scores, scores.new_zeros(()) if out is None else out)
            else:
                out = np.where(fold_item == f, scores, 0.0 if out is None else out)
        return RaggedLists(out, offsets), fold_weights


def fold_of_lists(n_lists: int, folds: int, groups=None) -> np.ndarray:
    """the fold of every list: ``l % folds``, or with ``groups`` the group's index in order of first appearance, modulo ``folds``"""
    if groups is None:
        return np.arange(n_lists, dtype=np.int64) % folds
    g = np.asarray(groups.to_numpy() if hasattr(groups, "to_numpy") else groups).ravel()
    if g.size != n_lists:
        raise ValueError(f"{n_lists} lists but {g.size} groups")
    _, first, inverse = np.unique(g, return_index=True, return_inverse=True)
    order = np.empty(len(first), np.int64)
    order[np.argsort(first, kind="stable")] = np.arange(len(first))
    return order[inverse.ravel()] % folds


class RankFusion:
    """Unweighted reciprocal-rank fusion (Cormack, Clarke, Buettcher 2009): ``sum_m 1 / (k + r_mi)`` with mid-ranks inside each list;
    ``ScoreBlend.from_weights(["rrf"] * M, ones)``."""

    def __init__(self, k: float = 60.0, device="cuda"):
        self.k, self.device = float(k), device

    def predict(self, sources) -> RaggedLists:
        M = len(sources) if hasattr(sources, "__len__") and not isinstance(sources, RaggedLists) else 0
        if not 1 <= M <= MAX_SOURCES:
            raise ValueError(f"1 to {MAX_SOURCES} sources, got {M}")
        return ScoreBlend.from_weights(["rrf"] * M, np.ones(M), rrf_k=self.k, device=self.device).predict(sources)
