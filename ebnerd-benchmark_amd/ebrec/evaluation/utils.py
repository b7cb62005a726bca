"""Helpers of the evaluator that the metric wrappers use (reference: evaluation/utils.py:6-10,13-32)."""
from __future__ import annotations

from typing import Iterable

import numpy as np


def convert_to_binary(y_pred: np.ndarray, threshold: float):
    """1 where y_pred >= threshold else 0.  Like the reference (utils.py:6-10) this works IN PLACE on
    an ndarray argument (np.asarray does not copy), so a later metric sees the binarised scores."""
    y_pred = np.asarray(y_pred)
    hit = y_pred >= threshold
    y_pred[hit] = 1
    y_pred[~hit] = 0
    return y_pred


def is_iterable_nested_dtype(iterable: Iterable, dtypes) -> bool:
    return isinstance(iterable[0], dtypes)


# ---- helpers of the beyond-accuracy metrics (reference: evaluation/utils.py:36-198) ----
def compute_combinations(n: int, r: int) -> int:
    """nCr, exact.  (The reference divides float factorials taken from np.math, which numpy 2 removed.)"""
    import math

    return math.comb(n, r)


def scale_range(m: np.ndarray, r_min: float = None, r_max: float = None, t_min: float = 0, t_max: float = 1.0):
    """m in [r_min, r_max] -> [t_min, t_max]; a bound that is None (or, as in the reference, 0) is taken from m."""
    if not r_min:
        r_min = np.min(m)
    if not r_max:
        r_max = np.max(m)
    return ((m - r_min) / (r_max - r_min)) * (t_max - t_min) + t_min


def compute_item_popularity_scores(R: Iterable[np.ndarray]) -> dict:
    """p_i = (number of users' lists that hold item i) / (number of lists); every list holds an item at most once."""
    from collections import Counter

    U = len(R)
    return {item: n / U for item, n in Counter(np.concatenate(R)).items()}


def compute_normalized_distribution(R, weights=None, distribution: dict = None) -> dict:
    """{representation: summed weight}; the default weight of every element is 1 / len(R).  `distribution`, when given,
    is added to in place."""
    n_elements = len(R)
    distr = distribution if distribution is not None else {}
    weights = weights if weights is not None else np.ones(n_elements) / n_elements
    for item, weight in zip(R, weights):
        distr[item] = weight + distr.get(item, 0.0)
    return distr


def get_keys_in_dict(id_list, dictionary) -> list:
    """The ids of id_list that are keys of dictionary, in order, repeats kept."""
    return [id_ for id_ in id_list if id_ in dictionary]


def check_key_in_all_nested_dicts(dictionary, key: str) -> None:
    """ValueError unless every value of dictionary is a dict that holds `key`."""
    for dict_key, sub_dict in dictionary.items():
        if not isinstance(sub_dict, dict) or key not in sub_dict:
            raise ValueError(f"'{key}' is not present in '{dict_key}' nested dictionary.")
