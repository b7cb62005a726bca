"""``recommend`` / ``rank_targets`` of the baselines on the device (ebrec/models/baselines/_topn.py).

DENSE ROUTE, helper level: ``DenseSession`` over device tensors -- the EXISTING ebn_topk_score_f32 / ebn_topk_score_window_f32 /
ebn_target_rank_f32 behind zero-padded columns -- against its float64 twin.  Operands are small integers in [-2, 2], F in
{1, 3, 4, 33, 128}: every dot product is exact in fp32 in any order, so lists, scores, ranks and counts are equal EXACTLY, ties
included.
DENSE ROUTE, class level (fitted ImplicitALS and ContentSimilarity on the device): with the user rows x and catalogue rows y the
device path used, downloaded, every returned score lies within gamma_F sum_i |x_i y_i| of the float64 dot product
(gamma_F = F u / (1 - F u), u = 2^-24, F the padded width: the standard bound of a dot product, fused or not), and every listed
item's float64 score is at least every omitted admissible item's float64 score minus the two items' bounds (what the first bound
implies for a list that is sorted on the fp32 scores).
DENSE CLASSES AGAINST THE HOST PATH (``test_dense_classes_on_the_device_against_the_host_path``): each class built on the device AND
with ``device=None`` from the same fitted state (``ImplicitALS.from_factors`` with one factor matrix, ``ContentSimilarity`` over one
lookup dict), ``recommend`` / ``rank_targets`` called on both in the ``history=`` form, plain, with ``candidate_ids`` and under a
``Freshness`` window.  Counts and the not-ranked pattern are equal exactly.  A score may differ between the paths by B(u, c) =
gamma_F sum |x_i y_i| + the tolerance between the two paths' user rows carried through the dot product -- for ALS
``||y_c||_2 (residual bound / reg)`` of tests/test_als_gpu.py, for the centroid ``2 (n + D + 8) u (a . |T_c| / ||p|| + |s|) + (D + 8) u``
of tests/test_content_gpu.py -- + u |s| for the host score's one rounding to float32.  With B_u = max_c B(u, c): the j-th best score
of the two paths differs by at most B_u (order statistics of two score vectors that differ by at most B_u); the two lists hold the
same article at slot j wherever the host's neighbours at j - 1, j, j + 1 are more than 2 B_u apart; the host's score of every article
the device lists is within B(u, c) of the device's; and the device's rank of a target lies between 1 + #{host scores > s + 2 B_u} and
#{host scores >= s - 2 B_u}.
CO-VISITATION, class level: device against ``device=None`` on the golden frames, bit for bit -- with "count" values the two fitted
matrices are equal exactly; with "cosine" the host model is given the device's matrix."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from ebrec.models.baselines._topn import DenseSession
from ebrec.models.baselines.covisit import CoVisitation, CoVisitMatrix
from tests.test_baseline_topn_cpu import _histories, build

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "ebnerd"
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def frames():
    return pd.read_parquet(GOLDEN / "behaviors.parquet").iloc[:200].reset_index(drop=True), pd.read_parquet(GOLDEN / "history.parquet")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("F", [1, 3, 4, 33, 128])
def test_dense_sessions_equal_the_float64_twin_exactly(hip, F):
    rng = np.random.default_rng(F)
    n_hists, n_rows, M = 150, 300, 211  # more than one 128-user tile, more than one 128-candidate tile, no multiple of either
    users = rng.integers(-2, 3, (n_hists, F)).astype(np.float32)
    users[::9] = 0  # users that cannot be scored
    cat = rng.integers(-2, 3, (n_rows, F)).astype(np.float32)
    cand = rng.permutation(n_rows)[:M].astype(np.int32)
    hist_idx = np.concatenate([np.arange(n_hists), [-1, n_hists, 3, 3]]).astype(np.int32)
    b = hist_idx.size
    window = np.stack([rng.integers(-5, M // 2, b), rng.integers(M // 3, M + 9, b)], 1).astype(np.int32)
    window[::11] = (7, 7)
    exclude = rng.integers(-1, n_rows, (b, 17)).astype(np.int32)
    window[-1], exclude[-1] = window[3], exclude[3]  # the last row of a launch is user 3 again
    dev = DenseSession(torch.from_numpy(users).cuda(), torch.from_numpy(cat).cuda())
    host = DenseSession(users, cat)
    assert dev.on_device and not host.on_device and dev.users.shape[1] == max(4, (F + 3) // 4 * 4) and dev.users.is_contiguous()
    dev.candidates(cand)
    host.candidates(cand)
    ties = 0
    for win, ex, k in ((None, None, 64), (window, exclude, 10), (window, None, 1), (None, exclude, 5)):
        f_dev, f_host = torch.zeros(2, dtype=torch.int32, device="cuda"), np.zeros(2, np.int32)
        pos, score = dev.topk(hist_idx, win, ex, k, f_dev)
        w_pos, w_score = host.topk(hist_idx, win, ex, k, f_host)
        pos, score = pos.cpu().numpy(), score.cpu().numpy()
        assert np.array_equal(pos, w_pos) and np.array_equal(score, w_score) and f_dev.cpu().tolist() == f_host.tolist() == [0, 0]
        ties += int(((score[:, 1:] == score[:, :-1]) & (pos[:, 1:] >= 0)).sum())
        assert (pos[0::9][:16] == -1).all() and (pos[-4:-2] == -1).all() and np.array_equal(pos[-1], pos[3])
        for target in (w_pos[:, 0], w_pos[:, k - 1], np.full(b, -1), rng.integers(0, M, b)):
            target = np.ascontiguousarray(target, dtype=np.int32)
            got = dev.rank(hist_idx, target, win, ex, f_dev)
            want = host.rank(hist_idx, target, win, ex, f_host)
            for g, w, what in zip(got, want, ("rank", "count", "score")):
                assert np.array_equal(g.cpu().numpy(), w), what
    assert ties > 100


def _dense_operands(model, kind, lists):
    """what the device path used: (user rows float64 [n, Fp], catalogue float64 [n_rows, Fp], scorable [n]) downloaded"""
    session = model._topn_session(lists)
    assert session.on_device
    return session.users.cpu().numpy().astype(np.float64), session.catalogue.cpu().numpy().astype(np.float64), session.scorable


@pytest.mark.parametrize("kind", ["als", "content"])
@pytest.mark.parametrize("weights", [None, "exponential"])
def test_dense_classes_within_the_dot_product_bound(hip, frames, kind, weights):
    from ebrec.evaluation import RaggedLists

    behaviors, history = frames
    model = build(kind, history, device="cuda", weights=weights, factors=64 if kind == "als" else 30)
    lists = _histories(behaviors, history) + [[], [-5]]
    ragged = RaggedLists.from_lists([np.asarray(l, np.int64) for l in lists])
    X, Y, scorable = _dense_operands(model, kind, ragged)
    Fp = X.shape[1]
    gamma = Fp * U32 / (1 - Fp * U32)
    S, bound = X @ Y.T, gamma * (np.abs(X) @ np.abs(Y).T)
    ids_all = np.asarray(model._topn_ids())
    rows_of = {int(a): r for r, a in enumerate(ids_all)}
    for exclude_history in (True, False):
        ids, scores = model.recommend(ragged, top_n=10, return_scores=True, exclude_history=exclude_history)
        assert isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float32 and isinstance(ids, np.ndarray)
        scores = scores.cpu().numpy()
        ranks = model.rank_targets(ragged, targets=[[a for a in row[:3] if a >= 0] for row in ids], exclude_history=exclude_history)
        worst, checked = 0.0, 0
        for i, l in enumerate(lists):
            if not scorable[i]:
                assert (ids[i] == -1).all() and np.isneginf(scores[i]).all()
                continue
            listed = [rows_of[int(a)] for a in ids[i]]
            assert len(set(listed)) == 10
            err = np.abs(scores[i].astype(np.float64) - S[i, listed])
            assert np.all(err <= bound[i, listed]), (i, err, bound[i, listed])
            worst = max(worst, float((err / np.maximum(bound[i, listed], 1e-300)).max()))
            out = np.ones(len(ids_all), bool)
            out[listed] = False
            if exclude_history:
                out[[rows_of[int(a)] for a in list(dict.fromkeys(reversed(l)))[:256] if int(a) in rows_of]] = False
            omitted = np.flatnonzero(out)
            for r in listed:
                assert np.all(S[i, r] >= S[i, omitted] - (bound[i, r] + bound[i, omitted])), (i, r)
            assert np.all(np.diff(scores[i]) <= 0)
            for j in np.flatnonzero(ranks.impression == i):  # the rank is the slot, the score that slot's bits
                slot = ids[i].tolist().index(ranks.target_id[j])
                assert ranks.rank[j] == slot + 1 and _bits(ranks.score[j]) == _bits(scores[i, slot])
            checked += 1
        print(f"{kind} weights={weights} exclude_history={exclude_history}: {checked} users, largest error / bound = {worst:.3f}")
        assert checked > 100


@pytest.mark.parametrize("similarity,weights", [("count", None), ("cosine", "exponential"), ("conditional", "linear")])
def test_covisitation_on_the_device_equals_the_host_path(hip, frames, similarity, weights):
    from ebrec.evaluation.freshness import Freshness

    behaviors, history = frames
    kw = dict(max_gap=3, similarity=similarity, history_weights=weights, history_size=40, mode="sum" if similarity != "conditional" else "max")
    dev = CoVisitation(**kw).fit(history)
    host = CoVisitation(device=None, **kw).fit(history)
    assert dev.matrix.on_device and not host.matrix.on_device
    if similarity != "count":  # the values agree within 2 u: give the host path the device's own
        host.matrix = CoVisitMatrix(host.matrix.article_ids, *dev.matrix.host())
    t_dev, t_host = dev.matrix.transpose(), host.matrix.transpose()
    assert all(t.is_cuda for t in t_dev) and dev.matrix.transpose() is t_dev  # built once
    for a, b in zip(t_dev, t_host):
        assert np.array_equal(a.cpu().numpy(), b) and a.cpu().numpy().dtype == b.dtype
    ids_all = dev.matrix.article_ids
    rng = np.random.default_rng(0)
    published = {int(a): float(t) for a, t in zip(ids_all, rng.integers(0, 50, ids_all.size))}
    times = rng.integers(10, 60, len(behaviors)).astype(np.float64)
    for kwargs in (dict(), dict(exclude_history=False, top_n=64), dict(candidate_ids=ids_all[::-2], top_n=5, batch_users=37),
                   dict(window=Freshness(published, max_age=25.0), impression_times=times)):
        d_ids, d_scores = dev.recommend(behaviors, history=history, return_scores=True, **kwargs)
        h_ids, h_scores = host.recommend(behaviors, history=history, return_scores=True, **kwargs)
        assert isinstance(d_scores, torch.Tensor) and d_scores.is_cuda and isinstance(h_scores, np.ndarray)
        assert np.array_equal(d_ids, h_ids) and np.array_equal(_bits(d_scores.cpu().numpy()), _bits(h_scores)), kwargs
        assert (d_ids >= 0).sum() > 200
        kwargs.pop("top_n", None)
        d, h = dev.rank_targets(behaviors, history=history, **kwargs), host.rank_targets(behaviors, history=history, **kwargs)
        for f in ("impression", "target_id", "rank", "count"):
            assert np.array_equal(getattr(d, f), getattr(h, f)), (f, kwargs)
        assert np.array_equal(_bits(d.score), _bits(h.score))
        # targets the lists hold: slot s ranks s + 1 on both paths, with the slot's score bits
        targets = [[a for a in row[:2] if a >= 0] for row in d_ids]
        d, h = dev.rank_targets(behaviors, history=history, targets=targets, **kwargs), host.rank_targets(behaviors, history=history, targets=targets, **kwargs)
        assert np.array_equal(d.rank, h.rank) and np.array_equal(d.count, h.count) and np.array_equal(_bits(d.score), _bits(h.score))
        first = np.r_[True, d.impression[1:] != d.impression[:-1]]
        assert len(d) > 150 and np.array_equal(d.rank, np.where(first, 1, 2))
        assert np.array_equal(_bits(d.score), _bits(d_scores.cpu().numpy()[d.impression, d.rank - 1]))


def _als_pair(behaviors, history):
    """(device model, host model, bound [n_histories of the frame, n_items]) from one factor matrix; tests/test_als_gpu.py's bound"""
    from ebrec.models import ImplicitALS
    from ebrec.models.baselines.popularity import _explode
    from tests import als_cases as ac

    ids = np.unique(np.concatenate(list(history["article_id_fixed"])))
    F = 24
    Y = (np.random.default_rng(5).standard_normal((ids.size, F)) * 0.3).astype(np.float32)
    kw = dict(regularization=1.0, alpha=8.0, history_weights="exponential", lambda_factor=0.9, history_size=40)
    dev_m, host_m = ImplicitALS.from_factors(ids, Y, **kw), ImplicitALS.from_factors(ids, Y, device=None, **kw)
    flat, off, w = host_m._weighted(*_explode(history["article_id_fixed"]))
    indptr, cols, conf = host_m._csr(host_m.rows_of(flat), off, w, None)
    rows = host_m.fold_in(list(history["article_id_fixed"])).astype(np.float64)
    gram = (Y.astype(np.float64).T @ Y.astype(np.float64)).astype(np.float32)
    forward = np.zeros(len(history))
    for r, ref in ac.half_sweep_rows(Y, indptr, cols, conf, 1.0, gram=gram):
        forward[r] = ac.residual_bound(ref, rows[r]) / 1.0  # lambda_min(A) >= reg = 1
    Y64 = Y.astype(np.float64)
    S = rows @ Y64.T
    bound = forward[:, None] * np.linalg.norm(Y64, axis=1)[None, :] + ac.gamma(F) * (np.abs(rows) @ np.abs(Y64).T) + U32 * np.abs(S)
    return dev_m, host_m, bound, ids


def _content_pair(behaviors, history):
    """(device model, host model, bound [n_histories of the frame, n_items]) over one lookup dict; tests/test_content_gpu.py's bound"""
    from ebrec.evaluation.beyond_accuracy import DeviceLookup
    from ebrec.models import ContentSimilarity
    from ebrec.utils._decay import exponential_decay_weights
    from tests import content_cases as cc

    D = 30
    table = cc.synthetic_lookup(behaviors, history, D=D, key="v")
    kw = dict(mode="centroid", history_weights="exponential", lambda_factor=0.9, history_size=40)
    dev_m = ContentSimilarity(DeviceLookup(table, vector_keys=("v",)), "v", **kw)
    host_m = ContentSimilarity(table, "v", device=None, **kw)
    c = cc.frames_case(host_m, behaviors, history, lambda n: exponential_decay_weights(n, 0.9, ascending=True))
    T = c["table"].astype(np.float64)
    Dp = (D + 3) // 4 * 4
    bound = np.zeros((len(history), T.shape[0]))
    for h in range(len(history)):
        a0, a1 = int(c["hist_offsets"][h]), int(c["hist_offsets"][h + 1])
        rows, w = c["hist_rows"][a0:a1].astype(np.int64), c["hist_weights"][a0:a1].astype(np.float64)
        rows, w = rows[rows >= 0], w[rows >= 0]
        p, a = (w[:, None] * T[rows]).sum(0), np.abs(w[:, None] * T[rows]).sum(0)
        norm = float(np.sqrt((p * p).sum()))
        if norm > 0:
            s = (p / norm) @ T.T
            bound[h] = (2 * (rows.size + D + 8) * U32 * ((a / norm) @ np.abs(T).T + np.abs(s)) + (D + 8) * U32
                        + Dp * U32 / (1 - Dp * U32) * ((np.abs(p) / norm) @ np.abs(T).T) + U32 * np.abs(s))
    return dev_m, host_m, bound, np.asarray(host_m.lookup.ids)


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _against_the_host_path(dev_m, host_m, bound, ids_all, behaviors, history, need_device=True):
    from ebrec.evaluation.freshness import Freshness

    hist_of = {u: k for k, u in enumerate(history["user_id"].tolist())}
    h_idx = np.array([hist_of.get(u, -1) for u in behaviors["user_id"]])
    row_of = {int(a): r for r, a in enumerate(ids_all.tolist())}
    B_u = np.where(h_idx >= 0, bound.max(1)[np.maximum(h_idx, 0)], 0.0)
    rng = np.random.default_rng(2)
    published = {int(a): float(t) for a, t in zip(ids_all, rng.integers(0, 50, ids_all.size))}
    times = rng.integers(10, 60, len(behaviors)).astype(np.float64)
    equal = total = 0
    for kwargs in (dict(), dict(exclude_history=False, candidate_ids=ids_all[::-2]),
                   dict(window=Freshness(published, max_age=25.0), impression_times=times)):
        d_ids, d_s = dev_m.recommend(behaviors, history=history, top_n=10, return_scores=True, **kwargs)
        h_ids, h_s = host_m.recommend(behaviors, history=history, top_n=64, return_scores=True, **kwargs)
        assert isinstance(h_s, np.ndarray) and (not need_device or d_s.is_cuda)
        d_s = _host(d_s)
        assert np.array_equal(d_ids >= 0, h_ids[:, :10] >= 0), kwargs  # the same number of admissible articles, up to ten
        live = d_ids >= 0
        assert live.sum() > 1000
        # the j-th best scores
        err = np.abs(np.where(live, d_s.astype(np.float64) - h_s[:, :10], 0.0))
        assert np.all(err <= B_u[:, None]), (kwargs, float((err - B_u[:, None]).max()))
        # the same article wherever the host's neighbours are well apart
        H = np.where(h_ids >= 0, h_s.astype(np.float64), -np.inf)
        for j in range(10):
            up = np.full(len(H), np.inf) if j == 0 else H[:, j - 1] - H[:, j]
            apart = live[:, j] & (up > 2 * B_u) & (H[:, j] - H[:, j + 1] > 2 * B_u)
            assert np.array_equal(d_ids[apart, j], h_ids[apart, j]), (kwargs, j)
            equal += int((d_ids[live[:, j], j] == h_ids[live[:, j], j]).sum())
            total += int(live[:, j].sum())
        # the host's own score and rank of every article the device lists
        targets = [[a for a in row if a >= 0] for row in d_ids]
        rk = {k: v for k, v in kwargs.items()}
        d_r, h_r = dev_m.rank_targets(behaviors, history=history, targets=targets, **rk), host_m.rank_targets(behaviors, history=history, targets=targets, **rk)
        assert np.array_equal(d_r.impression, h_r.impression) and np.array_equal(d_r.target_id, h_r.target_id) and len(d_r) == int(live.sum())
        assert np.array_equal(d_r.count, h_r.count) and (h_r.rank > 0).all() and (d_r.count > 0).all()
        slot = np.concatenate([np.arange(n) for n in live.sum(1)])
        assert np.array_equal(d_r.rank, slot + 1)  # the device's rank is its own list's slot, with the slot's score bits
        assert np.array_equal(_bits(d_r.score), _bits(d_s[d_r.impression, slot]))
        b_pair = bound[h_idx[d_r.impression], [row_of[int(a)] for a in d_r.target_id]]
        e_pair = np.abs(d_r.score.astype(np.float64) - h_r.score)
        assert np.all(e_pair <= b_pair), (kwargs, float((e_pair / np.maximum(b_pair, 1e-300)).max()))
        Bp, Hp, sp = B_u[d_r.impression], H[d_r.impression], h_r.score.astype(np.float64)
        lo, hi = 1 + (Hp > (sp + 2 * Bp)[:, None]).sum(1), (Hp >= (sp - 2 * Bp)[:, None]).sum(1)
        assert np.all(hi < 64) and np.all((lo <= d_r.rank) & (d_r.rank <= hi)), kwargs
        print(f"{type(dev_m).__name__} {sorted(kwargs)}: largest score error / bound {float((e_pair / np.maximum(b_pair, 1e-300)).max()):.3f}, "
              f"ranks that differ between the paths {int((d_r.rank != h_r.rank).sum())} of {len(d_r)}")
        # the clicked articles: who is ranked, among how many, and the scores
        d_c, h_c = dev_m.rank_targets(behaviors, history=history, **rk), host_m.rank_targets(behaviors, history=history, **rk)
        assert np.array_equal(d_c.target_id, h_c.target_id) and np.array_equal(d_c.count, h_c.count)
        assert np.array_equal(d_c.rank > 0, h_c.rank > 0) and np.array_equal(np.isneginf(d_c.score), np.isneginf(h_c.score))
        on = d_c.rank > 0
        b_c = bound[h_idx[d_c.impression[on]], [row_of[int(a)] for a in d_c.target_id[on]]]
        assert np.all(np.abs(d_c.score[on].astype(np.float64) - h_c.score[on]) <= b_c), kwargs
    print(f"{type(dev_m).__name__}: {equal} of {total} list slots hold the same article on both paths")
    assert equal > 0.9 * total


@pytest.mark.parametrize("kind", ["als", "content"])
def test_dense_classes_on_the_device_against_the_host_path(hip, kind):
    behaviors, history = pd.read_parquet(GOLDEN / "behaviors.parquet").iloc[:300].reset_index(drop=True), pd.read_parquet(GOLDEN / "history.parquet")
    dev_m, host_m, bound, ids_all = (_als_pair if kind == "als" else _content_pair)(behaviors, history)
    assert dev_m._topn_session(list(history["article_id_fixed"])[:2]).on_device and not host_m._topn_session([[]]).on_device
    _against_the_host_path(dev_m, host_m, bound, ids_all, behaviors, history)
