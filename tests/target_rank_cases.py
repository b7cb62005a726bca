"""Float64 restatement of ebn_target_rank_f32 / rank_targets(), and the case and target generators shared by
tests/test_target_rank_cpu.py and tests/test_target_rank_gpu.py.

The rule, per user u: position c is admissible when it lies in u's clamped window (every position without windows), its row
lies in [0, n_rows) and not in the user's exclusion list, and the score is not NaN.  count = the number of admissible
positions; rank = 0 without a target (target_pos < 0 or >= M) or with an inadmissible one, else 1 + the number of admissible
positions ahead of the target in recommend's order -- score descending, then position ascending.  Flags as in
recommend_window_cases.window_reference, plus: a target position >= M sets flags[0]."""
import numpy as np

from tests.recommend_cases import ROUNDED_SHAPES, integer_case, scores64, summation_bound  # noqa: F401
from tests.recommend_window_cases import PATTERNS, clamp, windows  # noqa: F401

# (U, M, F): 1x1, M below a tile, on the tile, off the tile in every dimension, the real width over two user tiles
EXACT_SHAPES = [(1, 1, 4), (3, 7, 4), (64, 128, 32), (65, 257, 36), (130, 1000, 400)]
SPLIT_SHAPES = [(65, 257, 36), (130, 1000, 400)]
KINDS = ["random", "random", "none", "past-the-end", "excluded", "outside-window", "bad-row", "duplicate"]


def rank_reference(scores, target_pos, window=None, cand_rows=None, n_rows=None, exclude=None):
    """scores [U, M] float64 by candidate POSITION (NaN / inf allowed), target_pos [U], window [U, 2] or None, cand_rows [M]
    (None: position == row), exclude [U, X] rows (None: nothing).  -> rank [U] int32, count [U] int32, flags (row out of range
    inside somebody's window or a target position >= M, NaN seen inside the user's window)."""
    scores = np.asarray(scores, dtype=np.float64)
    U, M = scores.shape
    w = clamp(window, M) if window is not None else np.tile([[0, M]], (U, 1))
    rows = np.arange(M) if cand_rows is None else np.asarray(cand_rows, dtype=np.int64)
    n_rows = M if n_rows is None else n_rows
    in_range = (rows >= 0) & (rows < n_rows)
    position = np.arange(M)
    rank, count = np.zeros(U, np.int32), np.zeros(U, np.int32)
    nan_seen = row_bad = False
    for u in range(U):
        inside = (position >= w[u, 0]) & (position < w[u, 1])
        row_bad |= bool((inside & ~in_range).any())
        ok = inside & in_range
        nan_seen |= bool((np.isnan(scores[u]) & ok).any())
        ok &= ~np.isnan(scores[u])
        if exclude is not None:
            ok &= ~np.isin(rows, np.asarray(exclude[u]))
        count[u] = ok.sum()
        tp = int(target_pos[u])
        row_bad |= tp >= M
        if 0 <= tp < M and ok[tp]:
            t = scores[u, tp]
            ahead = ok & ((scores[u] > t) | ((scores[u] == t) & (position < tp)))
            rank[u] = 1 + ahead.sum()
    return rank, count, (int(row_bad), int(nan_seen))


def row_flag_is_open(window, cand_rows, n_rows, M):
    """the header's either-value clause: a row outside the table inside [min lo, max hi) of the non-empty windows -- whether it is
    seen depends on the 128-user workgroups.  True when flags[0] may come back set although no window holds such a row."""
    if window is None or cand_rows is None:
        return False
    w = clamp(window, M)
    w = w[w[:, 0] < w[:, 1]]
    if not len(w):
        return False
    bad = np.flatnonzero((np.asarray(cand_rows) < 0) | (np.asarray(cand_rows) >= n_rows))
    return bool(((bad >= w[:, 0].min()) & (bad < w[:, 1].max())).any())


def with_bad_rows(cand_rows, n_rows):
    """a copy with two entries outside the table (n_rows and -1) where the list is long enough"""
    out = np.array(cand_rows, dtype=np.int32)
    if len(out) >= 7:
        out[len(out) // 2], out[1] = n_rows, -1
    return out


def targets(U, M, seed, window=None, cand_rows=None, n_rows=None, exclude=None):
    """[U] int32 target positions, user u of kind KINDS[(u + seed) % 8]: a random position; none (-1 and below); past the end
    (>= M: sets flags[0]); a position whose row the user excludes; a position outside the user's window; a position of a row
    outside the table; one of two positions of the same row.  A kind the case cannot serve falls back to a random position."""
    rng = np.random.default_rng(seed)
    rows = np.arange(M) if cand_rows is None else np.asarray(cand_rows, dtype=np.int64)
    n_rows = M if n_rows is None else n_rows
    w = clamp(window, M) if window is not None else np.tile([[0, M]], (U, 1))
    position = np.arange(M)
    _vals, first, counts = np.unique(rows, return_index=True, return_counts=True)
    twice = np.flatnonzero(np.isin(rows, rows[first[counts > 1]]) & (rows >= 0) & (rows < n_rows))
    bad = np.flatnonzero((rows < 0) | (rows >= n_rows))
    out = rng.integers(0, max(M, 1), U)
    for u in range(U):
        kind = KINDS[(u + seed) % len(KINDS)]
        pick = None
        if kind == "none":
            out[u] = -1 - (u % 3)
        elif kind == "past-the-end":
            out[u] = M + (u % 3)
        elif kind == "excluded" and exclude is not None:
            pick = np.flatnonzero(np.isin(rows, np.asarray(exclude[u])))
        elif kind == "outside-window":
            pick = np.flatnonzero((position < w[u, 0]) | (position >= w[u, 1]))
        elif kind == "bad-row":
            pick = bad
        elif kind == "duplicate":
            pick = twice
        if pick is not None and len(pick):
            out[u] = rng.choice(pick)
    return out.astype(np.int32)
