"""Beyond-accuracy evaluation (reference: evaluation/beyond_accuracy.py): IntralistDiversity, Distribution, Coverage,
Sentiment, Serendipity, Novelty -- same names, call signatures and return types -- and Calibration, the KL divergence between a
user's click history and a list over a label attribute (what ebrec.evaluation.rerank.Calibrated optimises).

Two paths.  With a plain dict as `lookup_dict` everything runs on the host in float64 numpy, list by list, as the reference
does.  With a `DeviceLookup` (a read-only Mapping over the same dict that also keeps its vector / scalar columns on the GPU),
a key it holds and the default distance function, diversity, serendipity, sentiment and novelty run through the HIP kernels
of csrc/ebn_beyond.hip: ids are mapped to table rows in bulk (one np.searchsorted per call), a missing id becomes row -1,
which the kernels skip.  Coverage, Distribution and the candidate sorts are counting over ids and stay on the host.
torch is imported only on the device path."""
from __future__ import annotations

from collections.abc import Mapping
from itertools import chain, combinations
from typing import Callable, Iterable

import numpy as np

from ebrec.evaluation.metrics._beyond_accuracy import (
    cosine_distances, coverage_count, coverage_fraction, intralist_diversity, novelty, serendipity,
)
from ebrec.evaluation.utils import (
    check_key_in_all_nested_dicts, compute_combinations, compute_normalized_distribution, get_keys_in_dict,
    is_iterable_nested_dtype,
)

# candidates whose m x m distance matrix _candidate_diversity keeps on the device (256 MiB of fp32 at the limit)
_MAX_DEVICE_CANDIDATES = 8192


class DeviceLookup(Mapping):
    """A `lookup_dict` that also lives on the GPU.

    As a Mapping it has exactly the items of `lookup_dict` (which it references, not copies, and treats as read-only), so
    every class below accepts it on the host path too.  In addition it holds the ids sorted (`ids`, row r of every table
    belongs to `ids[r]`), per key of `vector_keys` an [n_items, D] float32 table and per key of `scalar_keys` an [n_items]
    float32 array.  The tables are uploaded at the first device call; vector tables are normalised to unit rows there
    (ebn_ba_unit_rows_f32).  `device=None` keeps everything on the host: the classes then take their host path.

    Per key of `label_keys` -- a categorical attribute such as `category` (one label) or `topics` (a list of labels) -- it holds
    the sorted distinct labels (`label_vocabulary`) and the label table W [n_items, C] float32: a one-hot row for a single label,
    1 / n on each of the n distinct labels of a list, a zero row for `None` or an empty list.  It is uploaded as it is.

    The ids must be sortable against each other (all strings or all integers)."""

    def __init__(self, lookup_dict: dict, vector_keys: Iterable[str] = (), scalar_keys: Iterable[str] = (), device="cuda", *,
                 label_keys: Iterable[str] = ()):
        self._dict = lookup_dict
        self.vector_keys, self.scalar_keys, self.label_keys = tuple(vector_keys), tuple(scalar_keys), tuple(label_keys)
        self.device = device
        for key in self.vector_keys + self.scalar_keys + self.label_keys:
            check_key_in_all_nested_dicts(lookup_dict, key)
        keys = np.asarray(list(lookup_dict))
        if keys.dtype.kind not in "iuUS" and len(keys):
            raise TypeError(f"DeviceLookup needs ids that are all strings or all integers, got dtype {keys.dtype}")
        order = np.argsort(keys, kind="stable")
        self.ids = keys[order]
        self._key_list = [k for k in lookup_dict]
        self._order = order
        self._host, self._dev, self._labels = {}, {}, {}

    # ---- Mapping ----
    def __getitem__(self, key):
        return self._dict[key]

    def __iter__(self):
        return iter(self._dict)

    def __len__(self):
        return len(self._dict)

    def __contains__(self, key):
        return key in self._dict

    # ---- host side of the device path ----
    def holds(self, key: str) -> bool:
        return self.device is not None and (key in self.vector_keys or key in self.scalar_keys or key in self.label_keys)

    def _label_table(self, key: str):
        """(vocabulary, W [n_items, C] float64) of a label key, built once"""
        if key not in self._labels:
            if key not in self.label_keys:
                raise KeyError(key)
            per_item = [distinct_labels(self._dict[self._key_list[i]][key]) for i in self._order]
            vocab = sorted(set(chain.from_iterable(per_item)))
            column = {label: c for c, label in enumerate(vocab)}
            W = np.zeros((len(per_item), len(vocab)))
            for r, labels in enumerate(per_item):
                for label in labels:
                    W[r, column[label]] = 1.0 / len(labels)
            self._labels[key] = (vocab, W)
        return self._labels[key]

    def label_vocabulary(self, key: str) -> list:
        """The sorted distinct labels of a label key: column c of its table belongs to label_vocabulary(key)[c]."""
        return list(self._label_table(key)[0])

    def host_table(self, key: str) -> np.ndarray:
        """float32 column `key` in row order: [n_items, D] for a vector key (as stored, NOT normalised), [n_items] for a scalar
        key, the label table [n_items, C] for a label key."""
        if key not in self._host and key in self.label_keys:
            self._host[key] = self._label_table(key)[1].astype(np.float32)
        if key not in self._host:
            if key not in self.vector_keys and key not in self.scalar_keys:
                raise KeyError(key)
            col = [self._dict[self._key_list[i]][key] for i in self._order]
            arr = np.asarray(col, dtype=np.float32)
            want = 2 if key in self.vector_keys else 1
            if len(col) and arr.ndim != want:
                raise ValueError(f"'{key}' is not a {'vector' if want == 2 else 'scalar'} of one size in every item")
            self._host[key] = arr.reshape((0, 0) if want == 2 and not len(col) else arr.shape)
        return self._host[key]

    def rows_of(self, ids) -> np.ndarray:
        """int32 table rows of a flat array of ids, -1 where the id is not a key: one searchsorted, no per-id dict lookup."""
        flat = np.asarray(ids).ravel()
        n = len(self.ids)
        if flat.size == 0 or n == 0:
            return np.full(flat.size, -1, np.int32)
        a, b = self.ids.dtype.kind, flat.dtype.kind
        if not ((a in "iu" and b in "iu") or (a == b and a in "US")):
            # ids of another type (objects, floats, strings against integer keys): the dict decides, id by id
            row = {k: r for r, k in enumerate(self.ids.tolist())}
            return np.fromiter((row.get(i, -1) if i in self._dict else -1 for i in flat.tolist()), np.int32, flat.size)
        pos = np.minimum(np.searchsorted(self.ids, flat), n - 1)
        return np.where(self.ids[pos] == flat, pos, -1).astype(np.int32)

    def map_lists(self, lists):
        """(rows int32 [n_ids], offsets int64 [n_lists + 1]) of a 2-D id array or of ragged lists (one concatenate)."""
        if isinstance(lists, np.ndarray) and lists.ndim == 2 and lists.dtype != object:
            offsets = np.arange(lists.shape[0] + 1, dtype=np.int64) * lists.shape[1]
            return self.rows_of(lists), offsets
        arrs = [np.asarray(x).ravel() for x in lists]
        offsets = np.zeros(len(arrs) + 1, np.int64)
        np.cumsum([a.size for a in arrs], out=offsets[1:])
        filled = [a for a in arrs if a.size]
        flat = np.concatenate(filled) if filled else np.empty(0, self.ids.dtype)
        return self.rows_of(flat), offsets

    # ---- device side ----
    def device_table(self, key: str):
        """The uploaded column: unit rows [n_items, D] for a vector key, values [n_items] for a scalar key, the label table
        [n_items, C] as it is for a label key (torch tensors)."""
        if key not in self._dev:
            import torch

            from ebrec import _hip

            host = self.host_table(key)
            t = torch.from_numpy(np.ascontiguousarray(host)).to(self.device)
            if key in self.vector_keys and t.numel():
                with torch.cuda.device(t.device):
                    _hip.call("ebn_ba_unit_rows_f32", _hip.ptr(t), _hip.ptr(t), t.shape[0], t.shape[1], _hip.stream_handle())
            self._dev[key] = t
        return self._dev[key]


def distinct_labels(value) -> list:
    """The distinct labels of one item's attribute, in order of first appearance: [] for None, the elements of a list / tuple /
    set / array (None among them dropped), otherwise the value itself as the only label."""
    if value is None:
        return []
    if isinstance(value, (list, tuple, set, frozenset, np.ndarray)):
        return list(dict.fromkeys(v.item() if isinstance(v, np.generic) else v for v in value if v is not None))
    return [value.item() if isinstance(value, np.generic) else value]


def label_lookup(lookup_dict, lookup_key: str) -> DeviceLookup:
    """`lookup_dict` itself when it is a DeviceLookup with `lookup_key` among its label keys, else a host-only one over the same
    items: ONE rule for the vocabulary and the label table, whichever path uses them."""
    if isinstance(lookup_dict, DeviceLookup):
        if lookup_key in lookup_dict.label_keys:
            return lookup_dict
        lookup_dict = lookup_dict._dict
    return DeviceLookup(lookup_dict, label_keys=(lookup_key,), device=None)


def _on_device(lookup_dict, lookup_key, pairwise_distance_function=cosine_distances) -> bool:
    return (isinstance(lookup_dict, DeviceLookup) and lookup_dict.holds(lookup_key)
            and pairwise_distance_function is cosine_distances)


def _dev_lists(lookup: DeviceLookup, lists, device):
    import torch

    rows, offsets = lookup.map_lists(lists)
    return torch.from_numpy(rows).to(device), torch.from_numpy(offsets).to(device), len(offsets) - 1


def _device_call(name: str, table, n_lists: int, make_args):
    """Run an ebn_ba_* entry point that writes one fp32 per list; float64 numpy out, like the host path."""
    import torch

    from ebrec import _hip

    out = torch.empty(n_lists, dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        _hip.call(name, *make_args(out), _hip.stream_handle())
    return out.cpu().numpy().astype(np.float64)


def _device_intralist(lookup: DeviceLookup, key: str, R, form: int = 0) -> np.ndarray:
    from ebrec import _hip

    unit = lookup.device_table(key)
    ids, off, n = _dev_lists(lookup, R if hasattr(R, "__len__") else list(R), unit.device)
    if n == 0:
        return np.empty(0, np.float64)
    return _device_call("ebn_ba_intralist_f32", unit, n, lambda out: (
        _hip.ptr(unit), unit.shape[0], unit.shape[1], _hip.ptr(ids), ids.numel(), _hip.ptr(off), n, form, _hip.ptr(out)))


def _device_cross(lookup: DeviceLookup, key: str, R, H, form: int = 0) -> np.ndarray:
    from ebrec import _hip

    unit = lookup.device_table(key)
    ids_r, off_r, n = _dev_lists(lookup, R, unit.device)
    ids_h, off_h, _ = _dev_lists(lookup, H, unit.device)
    if n == 0:
        return np.empty(0, np.float64)
    return _device_call("ebn_ba_cross_f32", unit, n, lambda out: (
        _hip.ptr(unit), unit.shape[0], unit.shape[1], _hip.ptr(ids_r), ids_r.numel(), _hip.ptr(off_r), _hip.ptr(ids_h),
        ids_h.numel(), _hip.ptr(off_h), n, form, _hip.ptr(out)))


def _device_list_mean(lookup: DeviceLookup, key: str, R, transform: int) -> np.ndarray:
    from ebrec import _hip

    values = lookup.device_table(key)
    ids, off, n = _dev_lists(lookup, R if hasattr(R, "__len__") else list(R), values.device)
    if n == 0:
        return np.empty(0, np.float64)
    return _device_call("ebn_ba_list_mean_f32", values, n, lambda out: (
        _hip.ptr(values), values.shape[0], _hip.ptr(ids), ids.numel(), _hip.ptr(off), n, transform, _hip.ptr(out)))


def _device_subset_diversity(lookup: DeviceLookup, key: str, cand_rows: np.ndarray, subsets: np.ndarray) -> np.ndarray:
    """Diversity of every index tuple of `subsets` [n_subsets, k] over the candidates `cand_rows` (table rows)."""
    import torch

    from ebrec import _hip

    unit = lookup.device_table(key)
    m, (n_sub, k) = len(cand_rows), subsets.shape
    ids = torch.from_numpy(np.ascontiguousarray(cand_rows, dtype=np.int32)).to(unit.device)
    sub = torch.from_numpy(np.ascontiguousarray(subsets, dtype=np.int32)).to(unit.device)
    dist = torch.empty(m * m, dtype=torch.float32, device=unit.device)
    with torch.cuda.device(unit.device):
        _hip.call("ebn_ba_pairdist_f32", _hip.ptr(unit), unit.shape[0], unit.shape[1], _hip.ptr(ids), m, _hip.ptr(dist),
                  _hip.stream_handle())
    return _device_call("ebn_ba_subset_sums_f32", unit, n_sub, lambda out: (_hip.ptr(dist), m, _hip.ptr(sub), k, n_sub, _hip.ptr(out)))


### IntralistDiversity
class IntralistDiversity:
    """Intralist diversity (Smyth and McClave, 2001): the average pairwise distance between the items of each
    recommendation list.

    >>> div = IntralistDiversity()
    >>> R = np.array([['item1', 'item2'], ['item2', 'item3'], ['item3', 'item4']])
    >>> lookup_dict = {'item1': {'vector': [0.1, 0.2]}, 'item2': {'vector': [0.2, 0.3]},
    ...                'item3': {'vector': [0.3, 0.4]}, 'item4': {'vector': [0.4, 0.5]}}
    >>> div(R, lookup_dict, 'vector')
    array([0.00772212, 0.00153965, 0.00048792])
    >>> div._candidate_diversity(list(lookup_dict), 2, lookup_dict, 'vector')
    (0.0004879239129211843, 0.02219758592259058)
    """

    def __init__(self) -> None:
        self.name = "intralist_diversity"

    def __call__(self, R, lookup_dict, lookup_key: str, pairwise_distance_function: Callable = cosine_distances) -> np.ndarray:
        """One diversity per list of R.  Ids that are not keys of `lookup_dict` are dropped; a list left with no id, or
        with one, gives NaN."""
        if _on_device(lookup_dict, lookup_key, pairwise_distance_function):
            return _device_intralist(lookup_dict, lookup_key, R)
        check_key_in_all_nested_dicts(lookup_dict, lookup_key)
        diversity_scores = []
        for sample in R:
            ids = get_keys_in_dict(sample, lookup_dict)
            if len(ids) == 0:
                score = np.nan
            else:
                vectors = np.array([lookup_dict[id_].get(lookup_key) for id_ in ids])
                score = intralist_diversity(vectors, pairwise_distance_function=pairwise_distance_function)
            diversity_scores.append(score)
        return np.asarray(diversity_scores)

    def _candidate_diversity(self, R, n_recommendations: int, lookup_dict, lookup_key: str,
                             pairwise_distance_function: Callable = cosine_distances, max_number_combinations: int = 20000,
                             seed: int = None):
        """(min, max) diversity over the `n_recommendations`-subsets of the candidates R: every combination when there
        are at most `max_number_combinations`, otherwise that many random subsets drawn from numpy's legacy global
        generator after np.random.seed(seed)."""
        check_key_in_all_nested_dicts(lookup_dict, lookup_key)
        R = get_keys_in_dict(R, lookup_dict)
        n_items = len(R)
        if n_recommendations > n_items:
            raise ValueError("'n_recommendations' cannot exceed the number of items in R (items in candidate list). "
                             f"{n_recommendations} > {n_items}")
        sample = compute_combinations(n_items, n_recommendations) > max_number_combinations
        if (_on_device(lookup_dict, lookup_key, pairwise_distance_function) and n_items <= _MAX_DEVICE_CANDIDATES
                and n_recommendations >= 1):
            # the same subsets as index tuples: np.random.choice(R, n, replace=False) is R[permutation(len(R))[:n]], so drawing
            # from range(len(R)) consumes the generator identically
            if sample:
                np.random.seed(seed)
                subsets = np.stack([np.random.choice(n_items, n_recommendations, replace=False)
                                    for _ in range(max_number_combinations)])
            else:
                subsets = np.array(list(combinations(range(n_items), n_recommendations)), dtype=np.int32)
            scores = _device_subset_diversity(lookup_dict, lookup_key, lookup_dict.rows_of(np.asarray(R)), subsets)
            return scores.min(), scores.max()
        if sample:
            np.random.seed(seed)
            aids_iterable = chain(np.random.choice(R, n_recommendations, replace=False) for _ in range(max_number_combinations))
        else:
            aids_iterable = combinations(R, n_recommendations)
        diversity_scores = self.__call__(aids_iterable, lookup_dict=lookup_dict, lookup_key=lookup_key,
                                         pairwise_distance_function=pairwise_distance_function)
        return diversity_scores.min(), diversity_scores.max()


### Distribution
class Distribution:
    """Normalised distribution of an attribute over all items of R; list-valued attributes are concatenated.

    >>> lookup_dict = {"item1": {"g": "Action", "sg": ["Action", "Thriller"]}, "item2": {"g": "Action", "sg": ["Action", "Comedy"]},
    ...                "item3": {"g": "Comedy", "sg": ["Comedy"]}}
    >>> Distribution()(np.array([['item1', 'item2'], ['item2', 'item3']]), lookup_dict, 'g')
    {'Action': 0.75, 'Comedy': 0.25}
    """

    def __init__(self) -> None:
        self.name = "distribution"

    def __call__(self, R, lookup_dict, lookup_key: str) -> dict:
        check_key_in_all_nested_dicts(lookup_dict, lookup_key)
        R_flat = get_keys_in_dict(np.asarray(R).ravel(), lookup_dict)
        item_representations = [lookup_dict[id_].get(lookup_key) for id_ in R_flat]
        if is_iterable_nested_dtype(item_representations, (list, np.ndarray)):
            item_representations = np.concatenate(item_representations)
        return compute_normalized_distribution(item_representations)


### Coverage
class Coverage:
    """(number of distinct recommended items, that number over the distinct items of the candidate set C); the
    fraction is -inf when C is empty.

    >>> Coverage()(np.array([['item1', 'item2'], ['item2', 'item3'], ['item4', 'item3']]),
    ...            np.array(['item1', 'item2', 'item3', 'item4', 'item5', 'item6']))
    (4, 0.6666666666666666)
    """

    def __init__(self) -> None:
        self.name = "coverage"

    def __call__(self, R, C=[]):
        coverage_c = coverage_count(R)
        coverage_f = coverage_fraction(R, C) if len(C) > 0 else -np.inf
        return coverage_c, coverage_f


### Sentiment
class Sentiment:
    """Mean sentiment score of each list of R.

    >>> lookup_dict = {"item1": {"s": 1.00}, "item2": {"s": 0.50}, "item3": {"s": 0.25}, "item4": {"s": 0.00}}
    >>> Sentiment()(np.array([['item1', 'item2'], ['item2', 'item3'], ['item2', 'item5']]), lookup_dict, 's')
    array([0.75 , 0.375, 0.5  ])
    """

    def __init__(self) -> None:
        self.name = "sentiment"

    def __call__(self, R, lookup_dict, lookup_key: str) -> np.ndarray:
        if _on_device(lookup_dict, lookup_key):
            return _device_list_mean(lookup_dict, lookup_key, R, 0)
        check_key_in_all_nested_dicts(lookup_dict, lookup_key)
        sentiment_scores = []
        for sample in R:
            ids = get_keys_in_dict(sample, lookup_dict)
            sentiment_scores.append(np.mean([lookup_dict[id_].get(lookup_key) for id_ in ids]))  # no valid id: np.mean([]) = NaN
        return np.asarray(sentiment_scores)

    def _candidate_sentiment(self, R, n_recommendations: int, lookup_dict, lookup_key: str):
        """(mean of the n highest scores, mean of the n lowest) among the candidates R -- in that order."""
        check_key_in_all_nested_dicts(lookup_dict, lookup_key)
        R = get_keys_in_dict(R, lookup_dict)
        sentiment_scores = sorted([lookup_dict[id_].get(lookup_key) for id_ in R])
        return np.mean(sentiment_scores[-n_recommendations:]), np.mean(sentiment_scores[:n_recommendations])


### Serendipity
class Serendipity:
    """Mean distance between each recommendation list and the same user's click history.

    >>> R = [np.array(['item1', 'item2']), np.array(['item3', 'item4'])]
    >>> H = [np.array(['itemA', 'itemB']), np.array(['itemC', 'itemD'])]
    >>> lookup_dict = {'item1': {'vector': [0.1, 0.2]}, 'item2': {'vector': [0.2, 0.3]}, 'item3': {'vector': [0.3, 0.4]},
    ...                'item4': {'vector': [0.4, 0.5]}, 'itemA': {'vector': [0.5, 0.6]}, 'itemB': {'vector': [0.6, 0.7]},
    ...                'itemC': {'vector': [0.7, 0.8]}, 'itemD': {'vector': [0.8, 0.9]}}
    >>> Serendipity()(R, H, lookup_dict, 'vector')
    array([0.01734935, 0.00215212])
    """

    def __init__(self) -> None:
        self.name = "serendipity"

    def __call__(self, R, H, lookup_dict, lookup_key: str, pairwise_distance_function: Callable = cosine_distances) -> np.ndarray:
        """One score per (R[u], H[u]); NaN when either side has no id that is a key of `lookup_dict`."""
        if len(R) != len(H):
            raise ValueError(f"The lengths of 'R' and 'H' do not match ({len(R)} != {len(H)}).")
        if _on_device(lookup_dict, lookup_key, pairwise_distance_function):
            return _device_cross(lookup_dict, lookup_key, R, H)
        check_key_in_all_nested_dicts(lookup_dict, lookup_key)
        serendipity_scores = []
        for r_u, ch_u in zip(R, H):
            r_u = get_keys_in_dict(np.asarray(r_u).ravel(), lookup_dict)
            ch_u = get_keys_in_dict(np.asarray(ch_u).ravel(), lookup_dict)
            r_vectors = [lookup_dict[id_].get(lookup_key) for id_ in r_u]
            ch_vectors = [lookup_dict[id_].get(lookup_key) for id_ in ch_u]
            if len(r_vectors) == 0 or len(ch_vectors) == 0:
                score = np.nan
            else:
                score = serendipity(r_vectors, ch_vectors, pairwise_distance_function)
            serendipity_scores.append(score)
        return np.asarray(serendipity_scores)


### Novelty
class Novelty:
    """Mean -log2(popularity) of each list of R.

    >>> R = [np.array(['item1', 'item2']), np.array(['item3', 'item4'])]
    >>> lookup_dict = {'item1': {'popularity': 0.05}, 'item2': {'popularity': 0.1}, 'item3': {'popularity': 0.2},
    ...                'item4': {'popularity': 0.3}, 'item5': {'popularity': 0.4}}
    >>> Novelty()(R, lookup_dict, 'popularity')
    array([3.82192809, 2.02944684])
    >>> Novelty()._candidate_novelty(list(lookup_dict), 2, lookup_dict, 'popularity')
    (1.5294468445267841, 3.8219280948873626)
    """

    def __init__(self) -> None:
        self.name = "novelty"

    def __call__(self, R, lookup_dict, lookup_key: str) -> np.ndarray:
        if _on_device(lookup_dict, lookup_key):
            return _device_list_mean(lookup_dict, lookup_key, R, 1)
        check_key_in_all_nested_dicts(lookup_dict, lookup_key)
        novelty_scores = []
        for r_u in R:
            r_u = get_keys_in_dict(r_u, lookup_dict)
            novelty_scores.append(novelty([lookup_dict[id_].get(lookup_key) for id_ in r_u]))
        return np.asarray(novelty_scores)

    def _candidate_novelty(self, R, n_recommendations: int, lookup_dict, lookup_key: str):
        """(novelty of the n most popular candidates, novelty of the n least popular) = (min, max)."""
        check_key_in_all_nested_dicts(lookup_dict, lookup_key)
        R = get_keys_in_dict(R, lookup_dict)
        popularity_scores = sorted([lookup_dict[id_].get(lookup_key) for id_ in R])
        return novelty(popularity_scores[-n_recommendations:]), novelty(popularity_scores[:n_recommendations])


### Calibration
class Calibration:
    """KL(p || q~) between each user's click history and recommendation list over a label attribute (Steck, RecSys 2018): p is
    the mean label row of the history, q the mean label row of the list, q~ = (1 - alpha) q + alpha p.  An item's label row is
    one-hot for a single label, 1 / n on each of the n distinct labels of a list, zeros for None.  Ids that are not keys of
    `lookup_dict` are dropped; a history left empty gives 0 (nothing to be calibrated to), a list left empty NaN.

    >>> lookup_dict = {"item1": {"g": "Action"}, "item2": {"g": "Action"}, "item3": {"g": "Comedy"}, "item4": {"g": None}}
    >>> R = [np.array(["item1", "item3"]), np.array(["item1", "item2"]), np.array(["item3", "item4"])]
    >>> H = [np.array(["item1", "item3"]), np.array(["item1", "item3"]), np.array(["itemX"])]
    >>> Calibration()(R, H, lookup_dict, "g")
    array([0.        , 1.95851777, 0.        ])
    """

    def __init__(self) -> None:
        self.name = "calibration"

    def __call__(self, R, H, lookup_dict, lookup_key: str, alpha: float = 0.01) -> np.ndarray:
        if len(R) != len(H):
            raise ValueError(f"The lengths of 'R' and 'H' do not match ({len(R)} != {len(H)}).")
        if not 0.0 < float(alpha) < 1.0:
            raise ValueError(f"alpha must lie in (0, 1), got {alpha}")
        lookup = label_lookup(lookup_dict, lookup_key)
        W = lookup._label_table(lookup_key)[1]

        def mean_rows(lists):  # [n, C] mean label row of the valid ids of each list, and their number [n]
            rows, off = lookup.map_lists(lists if isinstance(lists, np.ndarray) else [np.asarray(x) for x in lists])
            owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
            ok = rows >= 0
            total = np.zeros((len(off) - 1, W.shape[1]))
            np.add.at(total, owner[ok], W[rows[ok]])
            count = np.bincount(owner[ok], minlength=len(off) - 1)
            return total / np.maximum(count, 1)[:, None], count

        p, _ = mean_rows(H)
        q, n_r = mean_rows(R)
        q = (1.0 - alpha) * q + alpha * p
        with np.errstate(divide="ignore", invalid="ignore"):
            kl = np.where(p > 0, p * np.log(p / q), 0.0).sum(1)
        return np.where(n_r > 0, kl, np.nan)
