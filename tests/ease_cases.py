"""The yardstick of the EASE tests (plain helpers: nothing collected from here): a plain-Python / float64 brute force -- a
dict-of-sets Gram matrix, ``numpy.linalg.inv`` in float64, the scores as nested loops -- and the small cases both test files share.

CONDITIONING.  Every system the tests invert comes from at most 400 users of at most 20 clicks and reg >= 1, so that
lambda_max(G) <= trace(G) <= 8000, lambda_min(G + reg I) >= reg >= 1 and kappa(A) <= 8001; ``system`` ASSERTS kappa <= 1e4 from the
float64 eigenvalues, on the CPU, when it builds a case.

BOUNDS.  ``invert_bound``: a backward-stable Cholesky inverse in fp32 has |P_dev - P| <= c(n) kappa eps32 |P| in norm; the bound
has that FORM, C * kappa * eps32 * max |P_ref|, and the same form (against 1) holds for the residual max |A P_dev - I|.  C is
measured, not derived: see INVERT_C.  ``score_bound``: (m + 7) eps32 sum_j |w_j B[h_j, c]| for a history of m entries: m products and
m + 6 adds (the lane's own partial sums and the six butterfly levels), each rounding once."""
from functools import lru_cache

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
MAX_USERS, MAX_CLICKS, KAPPA_MAX = 400, 20, 1e4

# C = 8 x the worst measured ratio (the factor 8 covers other summation orders of the GEMM planner across shapes).  Measured on
# an MI355X over n in {1, 2, NB - 1, NB, NB + 1, 2 NB + 3, 300} at lda = n and n + 5 (at NB = 128, the library's block, and at
# NB = 64), and over n = NB + 1 and 300 at the block sizes 32 / 64 / 128:
#   max |P_dev - P_ref| / (kappa eps32 max |P_ref|)   worst 0.2031 (n = 1, kappa = 1; 0.0534 at n = 2, at most 0.026 from n = 33 on)
#   max |A P_dev - I| / (kappa eps32)                 worst 0.2873 (n = 2, kappa = 30; 0.128 at n = 33, at most 0.106 from n = 63 on)
INVERT_C_MEASURED = (0.2031, 0.2873)  # (worst error ratio, worst residual ratio)
INVERT_C = 2.3  # 8 x 0.2873


# ---- the brute force -------------------------------------------------------------------------------------------------------------
def brute_gram(sequences, n_items) -> np.ndarray:
    """G [n, n] int64, full and symmetric: G[i][j] = the users whose sequence holds both i and j (sets: duplicates count once;
    entries outside [0, n_items) are dropped)"""
    G = [[0] * n_items for _ in range(n_items)]
    for seq in sequences:
        held = {int(i) for i in seq if 0 <= int(i) < n_items}
        for i in held:
            for j in held:
                G[i][j] += 1
    return np.array(G, np.int64).reshape(n_items, n_items)


def kappa(A) -> float:
    ev = np.linalg.eigvalsh(np.asarray(A, np.float64))
    return float(ev[-1] / ev[0])


def system(G, reg, small=True) -> np.ndarray:
    """A = G + reg I in float64, with the conditioning of every case asserted here (``small=False``: a system of the fixture
    frames, more users than MAX_USERS; kappa is asserted all the same)"""
    A = np.asarray(G, np.float64) + float(reg) * np.eye(len(G))
    assert reg >= 1 and (not small or np.trace(np.asarray(G, np.float64)) <= MAX_USERS * MAX_CLICKS)
    assert kappa(A) <= KAPPA_MAX, kappa(A)
    return A


def weights_of(P) -> np.ndarray:
    B = -P / np.diag(P)[None, :]
    B[np.diag_indices_from(B)] = 0.0
    return B


def brute_weights(G, reg) -> np.ndarray:
    """B [n, n] float64 from the full Gram matrix"""
    return weights_of(np.linalg.inv(system(G, reg)))


def brute_scores(B, hist_rows, hist_weights, hist_offsets, list_hist, cand_rows, cand_offsets):
    """(scores, sums of |w_j B[h_j, c]|, history lengths) float64 per item, as nested loops"""
    n = len(B)
    n_hists = len(hist_offsets) - 1
    out, absum, length = np.zeros(len(cand_rows)), np.zeros(len(cand_rows)), np.zeros(len(cand_rows), np.int64)
    for l in range(len(cand_offsets) - 1):
        u = l if list_hist is None else int(list_hist[l])
        for i in range(int(cand_offsets[l]), int(cand_offsets[l + 1])):
            c = int(cand_rows[i])
            if not (0 <= u < n_hists and 0 <= c < n):
                continue
            for j in range(int(hist_offsets[u]), int(hist_offsets[u + 1])):
                h = int(hist_rows[j])
                if 0 <= h < n:
                    term = (1.0 if hist_weights is None else float(hist_weights[j])) * float(B[h][c])
                    out[i] += term
                    absum[i] += abs(term)
                    length[i] += 1
    return out, absum, length


def score_bound(absum, length) -> np.ndarray:
    return (length + 7) * EPS32 * absum


def invert_bound(A64, P_ref) -> float:
    return INVERT_C * kappa(A64) * EPS32 * float(np.abs(P_ref).max())


def residual_bound(A64) -> float:
    return INVERT_C * kappa(A64) * EPS32


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def click_sequences(n_items, n_users, seed, max_clicks=MAX_CLICKS, zipf=1.1):
    """``n_users`` (<= 400) sequences of 1 to ``max_clicks`` (<= 20) Zipf-distributed rows of [0, n_items), repeats included"""
    assert n_users <= MAX_USERS and max_clicks <= MAX_CLICKS
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_items + 1) ** zipf
    p /= p.sum()
    return [rng.choice(n_items, size=int(rng.integers(1, max_clicks + 1)), p=p).tolist() for _ in range(n_users)]


@lru_cache(maxsize=None)
def spd_case(n, reg=2.0, seed=0):
    """(A float32 [n, n], A float64, P_ref float64): the system of 400 users over n items; counts + reg are exact in float32"""
    G = brute_gram(click_sequences(n, min(MAX_USERS, 40 + 3 * n), seed + n), n)
    A64 = system(G, reg)
    A32 = A64.astype(np.float32)
    assert np.array_equal(A32.astype(np.float64), A64)
    for a in (A32, A64):
        a.setflags(write=False)
    P = np.linalg.inv(A64)
    P.setflags(write=False)
    return A32, A64, P


def invert_sizes(nb):
    return [1, 2, nb - 1, nb, nb + 1, 2 * nb + 3, 300]


def gram_case(n_items, seed=0):
    """CSR rows as the kernel takes them (int64 indptr, int32 cols): users with 0, 1 and 60 entries, entries of -1 and >= n_items,
    repeats where 60 entries do not fit n_items; the other rows ascending and distinct"""
    rng = np.random.default_rng(seed + n_items)
    rows = [[], [0], np.sort(rng.integers(0, n_items, 60)).tolist(), [-1, 0, n_items, n_items + 7], []]
    for _ in range(40):
        rows.append(np.unique(rng.integers(0, n_items, int(rng.integers(1, 21)))).tolist())
    rows.append([-1] + np.unique(rng.integers(0, n_items, 12)).tolist() + [n_items])
    indptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    return indptr, np.array([c for r in rows for c in r], np.int32), rows


SCORE_CASES = ("weighted", "unweighted_no_list_hist")


@lru_cache(maxsize=None)
def score_case(name):
    """(operands dict, want, bound): histories of length 0, 1, 64, 65 and 200, repeated entries, unknown (-1, >= n) history entries
    and candidates, a history of unknown entries only, list_hist given (with -1 and an index past the histories) or NULL"""
    rng = np.random.default_rng(5)
    n = 50
    B = rng.standard_normal((n, n)).astype(np.float32)
    B[np.diag_indices(n)] = 0.0
    lengths = [0, 1, 64, 65, 200, 3, 2]
    hists = [rng.integers(0, n, m).tolist() for m in lengths]
    hists[2][5] = hists[2][6]  # a repeat
    hists[3][10], hists[3][64] = -1, n  # unknown entries
    hists[5] = [-1, n, n + 3]  # nothing present
    hist_offsets = np.zeros(len(hists) + 1, np.int64)
    np.cumsum([len(h) for h in hists], out=hist_offsets[1:])
    hist_rows = np.array([h for hs in hists for h in hs], np.int32)
    weighted = name == "weighted"
    hist_weights = rng.uniform(0.1, 1.0, hist_rows.size).astype(np.float32) if weighted else None
    if weighted:
        list_hist = np.array([4, 0, 2, -1, 3, 1, 7, 5, 2], np.int32)
        cands = [rng.integers(0, n, 7).tolist() for _ in list_hist]
    else:
        list_hist = None
        cands = [rng.integers(0, n, 5).tolist() for _ in hists]
    cands[2][1], cands[2][3] = -1, n  # unknown candidates
    cands[1 if weighted else 6] = []  # an empty list
    cand_offsets = np.zeros(len(cands) + 1, np.int64)
    np.cumsum([len(c) for c in cands], out=cand_offsets[1:])
    cand_rows = np.array([c for cs in cands for c in cs], np.int32)
    c = dict(B=B, hist_rows=hist_rows, hist_weights=hist_weights, hist_offsets=hist_offsets, list_hist=list_hist, cand_rows=cand_rows,
             cand_offsets=cand_offsets)
    want, absum, length = brute_scores(B.astype(np.float64), hist_rows, hist_weights, hist_offsets, list_hist, cand_rows, cand_offsets)
    for a in (B, want):
        a.setflags(write=False)
    return c, want, score_bound(absum, length), length
