"""Shared by tests/golden/make_beyond_accuracy_golden.py (which writes the fixtures from the reference's outputs) and the
beyond-accuracy tests (which read them): how a fixture file turns back into a lookup dict and ragged id lists.

A fixture holds, per case: `ids` [n_items] strings, `vec` [n_items, D] float32, `popularity`, `sentiment` [n_items] float32,
`category` [n_items] strings, `sub_flat` / `sub_off` (list-valued sub-category), `universe` (ids + ids absent from the lookup),
and ragged lists as int16 indices into `universe` with int64 CSR offsets (`R_flat` / `R_off`, `H_flat` / `H_off`, ...)."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = {"d96": "beyond_accuracy_golden.npz", "d768": "beyond_accuracy_golden_d768.npz"}
VEC, POP, SENT, CAT, SUB = "vec", "popularity", "sentiment", "category", "subcategory"


def load(case: str):
    return np.load(GOLDEN / CASES[case], allow_pickle=False)


def build_lookup(g) -> dict:
    """id -> attributes; vectors and scalars are float64 copies of the stored float32 values (exactly representable, so a
    float32 device table sees the same inputs)."""
    sub_off = g["sub_off"]
    return {str(i): {VEC: g["vec"][r].astype(np.float64), POP: float(g["popularity"][r]), SENT: float(g["sentiment"][r]),
                     CAT: str(g["category"][r]), SUB: [str(s) for s in g["sub_flat"][sub_off[r]:sub_off[r + 1]]]}
            for r, i in enumerate(g["ids"])}


def ragged(g, name: str) -> list:
    """The ragged id lists stored as `<name>_flat` / `<name>_off`: a list of 1-D string arrays."""
    flat, off, universe = g[name + "_flat"], g[name + "_off"], g["universe"]
    return [universe[flat[off[i]:off[i + 1]]] for i in range(len(off) - 1)]
