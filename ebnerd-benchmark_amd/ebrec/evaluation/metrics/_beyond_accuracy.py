"""Beyond-accuracy metric functions (reference: evaluation/metrics/_beyond_accuracy.py), float64 numpy.  The reference
takes sklearn's cosine_distances as its default pairwise distance; the package does not import sklearn (precedent:
_sklearn.py), so cosine_distances is restated here with sklearn's semantics and pinned against the reference through
tests/golden/beyond_accuracy_golden.npz."""
from __future__ import annotations

from collections import Counter
from typing import Callable

import numpy as np


def _unit_rows(X: np.ndarray) -> np.ndarray:
    """sklearn.preprocessing.normalize(X): rows divided by their L2 norm; a zero row is divided by 1 and stays zero."""
    norms = np.sqrt(np.einsum("ij,ij->i", X, X))
    norms[norms == 0.0] = 1.0
    return X / norms[:, None]


def cosine_distances(X, Y=None) -> np.ndarray:
    """1 - cosine similarity of the rows of X and Y (sklearn.metrics.pairwise.cosine_distances): rows are L2-normalised
    (a zero row stays zero, so its distance to everything is 1), D = 1 - Xn @ Yn.T is clipped to [0, 2], and the diagonal
    is set to exactly 0 only when Y is X (the same object) or None."""
    same = Y is None or Y is X
    Xa = np.asarray(X, dtype=np.float64)
    if Xa.ndim != 2:
        raise ValueError(f"Expected 2D array, got {Xa.ndim}D array instead")
    Xn = _unit_rows(Xa)
    if same:
        Yn = Xn
    else:
        Ya = np.asarray(Y, dtype=np.float64)
        if Ya.ndim != 2:
            raise ValueError(f"Expected 2D array, got {Ya.ndim}D array instead")
        if Ya.shape[1] != Xa.shape[1]:
            raise ValueError(f"Incompatible dimension for X and Y matrices: X.shape[1] == {Xa.shape[1]} while "
                             f"Y.shape[1] == {Ya.shape[1]}")
        Yn = _unit_rows(Ya)
    D = 1.0 - Xn @ Yn.T
    np.clip(D, 0.0, 2.0, out=D)
    if same:
        np.fill_diagonal(D, 0.0)
    return D


def intralist_diversity(R: np.ndarray, pairwise_distance_function: Callable = cosine_distances) -> float:
    """Diversity(R) = sum_{i != j} dist(i, j) / (|R| (|R| - 1)) (Smyth and McClave, 2001); NaN for fewer than two rows.
    The distance function is called as f(R, R): with cosine_distances that zeroes the diagonal.

    >>> intralist_diversity(np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]]))
    0.022588438516842262
    """
    R_n = R.shape[0]
    if R_n <= 1:
        return np.nan
    return np.sum(pairwise_distance_function(R, R)) / (R_n * (R_n - 1))


def serendipity(R: np.ndarray, H: np.ndarray, pairwise_distance_function: Callable = cosine_distances) -> float:
    """Mean distance between every recommendation and every history item (Lu, Dumitrache and Graus, 2020).

    >>> serendipity(np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]]), np.array([[0.7, 0.8, 0.9], [0.1, 0.2, 0.3]]))
    0.016941328887631724
    """
    return np.mean(pairwise_distance_function(R, H))


def coverage_count(R: np.ndarray) -> int:
    """Number of distinct items in R."""
    return np.unique(R).size


def coverage_fraction(R: np.ndarray, C: np.ndarray) -> float:
    """Distinct items of R over distinct items of the candidate set C."""
    return np.unique(R).size / np.unique(C).size


def novelty(R) -> float:
    """Mean self-information -log2(p_i) of the popularity scores in R (Zhou et al., 2010; Vargas and Castells, 2011).

    >>> novelty([0.1, 0.2, 0.3, 0.4, 0.5])
    1.9405499757656586
    """
    return np.mean(-np.log2(R))


def index_of_dispersion(x) -> float:
    """D = k (N^2 - sum f^2) / (N^2 (k - 1)) over the category frequencies f of x (k categories, N items); NaN for a
    single item, 0 for a single category."""
    N = len(x)
    count = Counter(x)
    k = len(count)
    if k == 1:
        return np.nan if N == 1 else 0
    f_squared = [f**2 for f in count.values()]
    return k * (N**2 - sum(f_squared)) / (N**2 * (k - 1))
