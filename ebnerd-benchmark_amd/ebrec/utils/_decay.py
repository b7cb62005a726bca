"""Decay weights over the slots of a click history (reference: utils/_decay.py:7-51): the oldest slot first when
``ascending``, so the most recent click weighs 1.  They are the natural ``history_weights`` of
ebrec.evaluation.rerank.Calibrated / calibrated_rerank / history_distribution."""
from __future__ import annotations


def linear_decay_weights(n: int, ascending: bool = True, **kwargs) -> list:
    """n weights 1/n, 2/n, ..., 1 (``ascending``) or 1, ..., 1/n.

    >>> linear_decay_weights(5, True)
    [0.2, 0.4, 0.6, 0.8, 1.0]
    >>> linear_decay_weights(10, False)
    [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1]
    """
    falling = [(n - i) / n for i in range(n)]
    return falling[::-1] if ascending else falling


def exponential_decay_weights(n: int, lambda_factor: float, ascending: bool = True, **kwargs) -> list:
    """n weights lambda_factor^(n-1), ..., lambda_factor, 1 (``ascending``) or 1, lambda_factor, ..., lambda_factor^(n-1).

    >>> exponential_decay_weights(5, 0.5, True)
    [0.0625, 0.125, 0.25, 0.5, 1.0]
    >>> exponential_decay_weights(10, 0.5, False)
    [1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125, 0.00390625, 0.001953125]
    """
    rising = [lambda_factor ** (n - 1 - i) for i in range(n)]
    return rising if ascending else rising[::-1]
