"""Cases of ebn_npa_target_rank_f32 / NPAModel.rank_targets_pairwise shared by tests/test_npa_target_rank_cpu.py and
tests/test_npa_target_rank_gpu.py.  Nothing new is restated here: the float64 rule is target_rank_cases.rank_reference applied to
npa_recommend_cases.pair_scores64, the targets are target_rank_cases.targets (its eight kinds), the windows
recommend_window_cases.windows."""
import numpy as np

from tests.npa_recommend_cases import SHAPES as _TOPK_SHAPES
from tests.npa_recommend_cases import case as _topk_case
from tests.npa_recommend_cases import pair_scores64, tolerance  # noqa: F401
from tests.recommend_window_cases import PATTERNS, clamp, windows  # noqa: F401
from tests.target_rank_cases import KINDS, rank_reference, row_flag_is_open, targets, with_bad_rows  # noqa: F401

# (U, M, L, F, A): the seven of npa_recommend_cases.SHAPES without k
SHAPES = [s[:5] for s in _TOPK_SHAPES]
SPLIT_SHAPES = [SHAPES[2], SHAPES[-1]]
WINDOW_SHAPE = SHAPES[2]
BAND_SEED = {s[:5]: sum(s) for s in _TOPK_SHAPES}  # the seed of the float64 band cases: the sum of the shape WITH its k
assert SHAPES == [(1, 1, 1, 4, 4), (3, 7, 9, 32, 24), (65, 130, 30, 36, 24), (40, 50, 32, 32, 24), (40, 50, 33, 32, 24), (33, 40, 64, 8, 4),
                  (130, 300, 30, 400, 200)]


def shape_id(s):
    return "x".join(map(str, s))


def case(shape, seed, cand="null", exclude=None):
    """npa_recommend_cases.case for a shape without k -> dict(users, Q, Ua, Vd, cand_rows, exclude, n_rows)"""
    c = _topk_case(tuple(shape) + (1,), seed, cand=cand, exclude=exclude)
    del c["k"]
    return c


def scores64(c, cand_rows="case"):
    cand_rows = c["cand_rows"] if isinstance(cand_rows, str) else cand_rows
    return pair_scores64(c["users"], c["Q"], c["Ua"], c["Vd"], cand_rows)


def admissible(c, window=None, cand_rows="case", exclude="case"):
    """[U, M] bool: position in the clamped window, row inside the table, row not excluded (no NaN in these cases)"""
    cand_rows = c["cand_rows"] if isinstance(cand_rows, str) else cand_rows
    exclude = c["exclude"] if isinstance(exclude, str) else exclude
    U, n_rows = c["users"].shape[0], c["n_rows"]
    M = n_rows if cand_rows is None else len(cand_rows)
    rows = np.arange(M) if cand_rows is None else np.asarray(cand_rows, dtype=np.int64)
    w = clamp(window, M) if window is not None else np.tile([[0, M]], (U, 1))
    position = np.arange(M)
    ok = (position[None, :] >= w[:, :1]) & (position[None, :] < w[:, 1:]) & ((rows >= 0) & (rows < n_rows))[None, :]
    if exclude is not None:
        ok &= ~np.stack([np.isin(rows, exclude[u]) for u in range(U)])
    return ok


def band(s64, adm, target, tol):
    """per user (lo, hi) of the rank the float64 scores allow when every fp32 score is within tol of its float64 value:
    lo = 1 + #{admissible c: s64 > t64 + 2 tol}, hi = 1 + #{admissible c != target: s64 >= t64 - 2 tol}; (0, 0) where the target is
    absent or inadmissible"""
    U, M = s64.shape
    out = np.zeros((U, 2), np.int64)
    for u in range(U):
        tp = int(target[u])
        if 0 <= tp < M and adm[u, tp]:
            t = s64[u, tp]
            others = adm[u].copy()
            others[tp] = False
            out[u] = 1 + int((s64[u, adm[u]] > t + 2 * tol).sum()), 1 + int((s64[u, others] >= t - 2 * tol).sum())
    return out
