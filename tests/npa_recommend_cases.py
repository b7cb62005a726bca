"""Float64 restatement of the pair score of ebn_npa_topk_score_f32 / NPAModel.recommend_pairwise, and the case generators shared
by tests/test_npa_recommend_cpu.py and tests/test_npa_recommend_gpu.py.  The selection is recommend_cases.topk_reference.

    s_l = Q[u] . Ua[row, l];  w = softmax_l(s) (max-subtracted);  score[u, c] = sum_l w_l (users[u] . Vd[row, l])
"""
import numpy as np

from tests.recommend_cases import topk_reference  # noqa: F401  (the selection rule is the same)

# (U, M, L, F, A, k): smallest possible; M < k (short lists); off the tile in every dimension; L on the tile; L spilling into the
# second tile; largest L with the smallest A; the real widths with the largest k
SHAPES = [(1, 1, 1, 4, 4, 1), (3, 7, 9, 32, 24, 10), (65, 130, 30, 36, 24, 10), (40, 50, 32, 32, 24, 5), (40, 50, 33, 32, 24, 5),
          (33, 40, 64, 8, 4, 5), (130, 300, 30, 400, 200, 64)]
SPLIT_SHAPES = [SHAPES[2], SHAPES[-1]]


def pair_scores64(users, Q, Ua, Vd, cand_rows=None):
    """float64 scores [U, M] by candidate position: users [U, F], Q [U, A], Ua [n_rows, L, A], Vd [n_rows, L, F]; a cand_rows entry
    outside the catalogue scores 0 (the selection skips it anyway)"""
    users, Q = np.asarray(users, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    Ua, Vd = np.asarray(Ua, dtype=np.float64), np.asarray(Vd, dtype=np.float64)
    n_rows = Ua.shape[0]
    rows = np.arange(n_rows) if cand_rows is None else np.asarray(cand_rows, dtype=np.int64)
    ok = (rows >= 0) & (rows < n_rows)
    safe = np.where(ok, rows, 0)
    s = np.einsum("ua,mla->uml", Q, Ua[safe])
    w = np.exp(s - s.max(2, keepdims=True))
    w /= w.sum(2, keepdims=True)
    d = np.einsum("uf,mlf->uml", users, Vd[safe])
    return np.where(ok[None, :], (w * d).sum(2), 0.0)


def pooled_then_dot64(users, Q, Ua, Vd, cand_rows=None):
    """the same score in the order of ebn_pap_indexed_f32 (and _ref64 of tests/test_npa_cached_scoring_gpu.py): pool the news vector,
    then dot it with the user"""
    users, Q = np.asarray(users, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    Ua, Vd = np.asarray(Ua, dtype=np.float64), np.asarray(Vd, dtype=np.float64)
    rows = np.arange(Ua.shape[0]) if cand_rows is None else np.asarray(cand_rows, dtype=np.int64)
    s = np.einsum("ua,mla->uml", Q, Ua[rows])
    w = np.exp(s - s.max(2, keepdims=True))
    w /= w.sum(2, keepdims=True)
    pooled = np.einsum("uml,mlf->umf", w, Vd[rows])
    return np.einsum("umf,uf->um", pooled, users)


def catalogue(rng, n_rows, L, F, A):
    """(Ua, Vd) float32 in the distribution of _catalogue of tests/test_npa_cached_scoring_gpu.py: pre-activations of O(1) and a small
    bias through tanh, conv outputs in [0, 1)"""
    U = rng.uniform(-2, 2, (n_rows, L, A)).astype(np.float32)
    ba = rng.uniform(-0.1, 0.1, A).astype(np.float32)
    Ua = np.tanh(U.astype(np.float64) + ba).astype(np.float32)
    Vd = rng.uniform(0, 1, (n_rows, L, F)).astype(np.float32)
    return Ua, Vd


def user_side(rng, U, F, A):
    """(users [U, F] uniform / sqrt(F): scores of both signs, Q [U, A] in [-1, 1])"""
    users = (rng.uniform(-1, 1, (U, F)) / np.sqrt(F)).astype(np.float32)
    Q = rng.uniform(-1, 1, (U, A)).astype(np.float32)
    return users, Q


def case(shape, seed, cand="null", exclude=None):
    """-> dict(users, Q, Ua, Vd, cand_rows, exclude, n_rows, k).  cand "null": the M candidates are the catalogue's rows; "subset":
    the catalogue has M + 5 rows and cand_rows draws M of them with replacement (duplicates are distinct candidates).  exclude
    None | "x3" as recommend_cases.integer_case: X = 3, rows of the case, -1 padding and rows past the table, which match nothing."""
    U, M, L, F, A, k = shape
    rng = np.random.default_rng(seed)
    n_rows = M if cand == "null" else M + 5
    Ua, Vd = catalogue(rng, n_rows, L, F, A)
    users, Q = user_side(rng, U, F, A)
    cand_rows = None if cand == "null" else rng.integers(0, n_rows, M).astype(np.int32)
    rows = np.arange(M, dtype=np.int32) if cand_rows is None else cand_rows
    ex = None
    if exclude == "x3":
        ex = rng.choice(rows, (U, 3)).astype(np.int32)
        ex[rng.random((U, 3)) < 0.3] = -1
        ex[rng.random((U, 3)) < 0.1] = n_rows + 3
    return dict(users=users, Q=Q, Ua=Ua, Vd=Vd, cand_rows=cand_rows, exclude=ex, n_rows=n_rows, k=k)


def tolerance(score64):
    """The project's tolerance for this score against float64 (test_indexed_pooling_and_scores_vs_float64: rtol 1e-4, atol 1e-6),
    at the largest score of the case"""
    return 1e-4 * float(np.abs(score64).max()) + 1e-6
