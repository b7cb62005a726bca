"""Generates tests/golden/beyond_accuracy_golden.npz (300 ids x 96 dims) and beyond_accuracy_golden_d768.npz (48 ids x 768
dims) by running the REFERENCE's own beyond-accuracy evaluator (/root/reference/src/ebrec/evaluation, numpy + sklearn) on
seeded ragged lists.  Run in the build container only; the reference never travels, the fixtures (inputs + expected outputs,
data only) do.  The layout of a fixture and how it turns back into a lookup dict: tests/beyond_accuracy_cases.py."""
import json
import math
import sys
import warnings
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import beyond_accuracy_cases as bc  # noqa: E402
import sklearn  # noqa: E402
from ebrec.evaluation.beyond_accuracy import (Coverage, Distribution, IntralistDiversity, Novelty, Sentiment,  # noqa: E402
                                              Serendipity)
from ebrec.evaluation.metrics._beyond_accuracy import (coverage_count, coverage_fraction, index_of_dispersion,  # noqa: E402
                                                       intralist_diversity, novelty, serendipity)
from sklearn.metrics.pairwise import cosine_distances  # noqa: E402

warnings.filterwarnings("ignore")  # np.mean([]) of a list without a valid id
# compute_combinations (reference utils.py:53-55) calls np.math.factorial, which numpy 2 removed: give the reference's own
# code the module it expects, in this process only, so that _candidate_diversity's expectation is still the reference's
np.math = math

LENGTHS = [0, 1, 2, 5, 10, 33, 64, 65, 250]
CATEGORIES = ["nyheder", "sport", "krimi", "underholdning", "forbrug"]
SUBCATS = ["a", "b", "c", "d", "e", "f", "g"]


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, np.int16) for x in lists] + [np.empty(0, np.int16)])
    return flat.astype(np.int16), off


def make_case(seed, n_items, D, n_lists, n_absent=24):
    rng = np.random.default_rng(seed)
    g = {}
    numbers = rng.choice(np.arange(9_000_000, 9_900_000), size=n_items + n_absent, replace=False)
    g["ids"] = np.array([f"n{v}" for v in numbers[:n_items]])
    g["universe"] = np.array([f"n{v}" for v in numbers])  # the last n_absent are not in the lookup
    vec = (rng.standard_normal((n_items, D)) + rng.standard_normal(D) * 0.7).astype(np.float32)
    vec[7] = 0.0  # an all-zero row: distance exactly 1 to everything
    vec[11] = vec[10]  # two identical rows
    g["vec"] = vec
    g["popularity"] = rng.uniform(1e-4, 1.0, n_items).astype(np.float32)
    g["popularity"][3] = 1.0
    g["sentiment"] = rng.uniform(0.0, 1.0, n_items).astype(np.float32)
    g["category"] = np.array([CATEGORIES[i] for i in rng.integers(0, len(CATEGORIES), n_items)])
    subs = [list(rng.choice(SUBCATS, size=int(rng.integers(1, 4)), replace=False)) for _ in range(n_items)]
    g["sub_off"] = np.concatenate([[0], np.cumsum([len(s) for s in subs])]).astype(np.int64)
    g["sub_flat"] = np.array([s for ss in subs for s in ss])
    R, H = [], []
    for i in range(n_lists):
        n = LENGTHS[i % len(LENGTHS)]
        r = rng.integers(0, n_items, n)
        if n and i % 10 < 3:
            r = rng.choice(n_items, size=min(n, n_items), replace=False)  # distinct ids
            r = np.concatenate([r, rng.integers(0, n_items, n - len(r))])
        if i % 7 == 3:  # some ids absent from the lookup
            r = np.where(rng.random(n) < 0.3, rng.integers(n_items, n_items + n_absent, n), r)
        if i % 29 == 5:  # every id absent
            r = rng.integers(n_items, n_items + n_absent, n)
        if i % 11 == 4 and n >= 2:  # a repeated id
            r[-1] = r[0]
        if i % 23 == 6 and n >= 2:  # the zero row and the identical pair in one list
            r[:3] = [7, 10, 11][:len(r[:3])]
        h_len = 700 if i % 40 == 0 else (0 if i % 13 == 0 else int(rng.integers(1, 60)))
        h = rng.integers(0, n_items, h_len)
        if i % 5 == 2:
            h = np.where(rng.random(h_len) < 0.2, rng.integers(n_items, n_items + n_absent, h_len), h)
        if i % 31 == 7:
            h = rng.integers(n_items, n_items + n_absent, h_len)
        R.append(r)
        H.append(h)
    g["R_flat"], g["R_off"] = csr(R)
    g["H_flat"], g["H_off"] = csr(H)
    R2 = rng.integers(0, n_items, (40, 10))
    R2[3, 2], R2[9, :] = n_items + 1, n_items + 2  # one absent id; a row of absent ids
    g["R2"] = R2.astype(np.int16)
    g["cand_small"] = np.concatenate([rng.choice(n_items, 11, replace=False), [n_items + 3], [7, 10, 11]]).astype(np.int16)
    g["cand_large"] = rng.choice(n_items + n_absent, 40, replace=False).astype(np.int16)
    return g


def expected(g, with_functions):
    lookup = bc.build_lookup(g)
    R, H, U = bc.ragged(g, "R"), bc.ragged(g, "H"), g["universe"]
    div, ser, nov, sent, dist, cov = IntralistDiversity(), Serendipity(), Novelty(), Sentiment(), Distribution(), Coverage()
    e = {"names": [div.name, dist.name, cov.name, sent.name, ser.name, nov.name]}
    g["exp_diversity"] = div(R, lookup, bc.VEC)
    g["exp_serendipity"] = ser(R, H, lookup, bc.VEC)
    g["exp_novelty"] = nov(R, lookup, bc.POP)
    g["exp_sentiment"] = sent(R, lookup, bc.SENT)
    R2 = U[g["R2"]]
    g["exp_diversity_R2"] = div(R2, lookup, bc.VEC)
    g["exp_novelty_R2"] = nov(R2, lookup, bc.POP)
    g["exp_sentiment_R2"] = sent(R2, lookup, bc.SENT)
    for key, tag in ((bc.CAT, "cat"), (bc.SUB, "sub")):
        d = dist(R2, lookup, key)
        g[f"exp_dist_{tag}_keys"], g[f"exp_dist_{tag}_vals"] = np.array(list(d)), np.array(list(d.values()), np.float64)
    e["coverage"] = list(map(float, cov(R2, U)))
    e["coverage_empty_C"] = list(map(float, cov(R2)))
    small, large = U[g["cand_small"]], U[g["cand_large"]]
    e["cand_div_exhaustive"] = {"n": 3, "max": 1000, "out": list(map(float, div._candidate_diversity(small, 3, lookup, bc.VEC, max_number_combinations=1000)))}
    e["cand_div_sampled"] = {"n": 5, "max": 60, "seed": 123,
                             "out": list(map(float, div._candidate_diversity(large, 5, lookup, bc.VEC, max_number_combinations=60, seed=123)))}
    e["cand_sentiment"] = {"n": 5, "out": list(map(float, sent._candidate_sentiment(large, 5, lookup, bc.SENT)))}
    e["cand_novelty"] = {"n": 5, "out": list(map(float, nov._candidate_novelty(large, 5, lookup, bc.POP)))}
    if with_functions:
        X = g["vec"][[0, 7, 10, 11, 1, 2, 3, 4]].astype(np.float64)
        Y = g["vec"][[5, 7, 10, 6, 8]].astype(np.float64)
        g["fn_X"], g["fn_Y"] = X, Y
        g["exp_cos_XX"], g["exp_cos_X"], g["exp_cos_XY"] = cosine_distances(X, X), cosine_distances(X), cosine_distances(X, Y)
        g["exp_cos_Xcopy"] = cosine_distances(X, X.copy())  # a different object: the diagonal is NOT zeroed
        e["fn_intralist"], e["fn_intralist_one_row"] = float(intralist_diversity(X)), float(intralist_diversity(X[:1]))
        e["fn_serendipity"] = float(serendipity(X, Y))
        e["fn_novelty"] = float(novelty(g["popularity"][:20].astype(np.float64)))
        ints = [1, 2, 3, 4, 5, 5, 6]
        e["fn_coverage"] = [int(coverage_count(np.array(ints))), float(coverage_fraction(np.array(ints), np.arange(1, 11)))]
        iod = [[1] * 25 + [2] * 42 + [3] * 13 + [4] * 8 + [5] * 13, [3], [3, 3, 3], [1, 2], list(g["category"][:50])]
        e["iod_inputs"], e["iod"] = [[str(v) for v in x] for x in iod], [float(index_of_dispersion([str(v) for v in x])) for x in iod]
        # the reference's docstring examples, run here
        ld = {f"item{i}": {"vector": [0.1 * i, 0.1 * i + 0.1]} for i in range(1, 5)}
        Rd = np.array([["item1", "item2"], ["item2", "item3"], ["item3", "item4"]])
        e["doc_diversity"] = list(map(float, div(Rd, ld, "vector")))
        e["doc_cand_diversity"] = list(map(float, div._candidate_diversity(list(ld), 2, ld, "vector")))
        ls = {"item1": {"vector": [0.1, 0.2]}, "item2": {"vector": [0.2, 0.3]}, "item3": {"vector": [0.3, 0.4]}, "item4": {"vector": [0.4, 0.5]},
              "itemA": {"vector": [0.5, 0.6]}, "itemB": {"vector": [0.6, 0.7]}, "itemC": {"vector": [0.7, 0.8]}, "itemD": {"vector": [0.8, 0.9]}}
        e["doc_serendipity"] = list(map(float, ser([np.array(["item1", "item2"]), np.array(["item3", "item4"])],
                                                   [np.array(["itemA", "itemB"]), np.array(["itemC", "itemD"])], ls, "vector")))
        lp = {"item1": {"popularity": 0.05}, "item2": {"popularity": 0.1}, "item3": {"popularity": 0.2}, "item4": {"popularity": 0.3},
              "item5": {"popularity": 0.4}}
        e["doc_novelty"] = list(map(float, nov([np.array(["item1", "item2"]), np.array(["item3", "item4"])], lp, "popularity")))
        e["doc_cand_novelty"] = list(map(float, nov._candidate_novelty(list(lp), 2, lp, "popularity")))
        lsent = {"item1": {"s": 1.00, "na": []}, "item2": {"s": 0.50, "na": []}, "item3": {"s": 0.25, "na": []}, "item4": {"s": 0.00, "na": []}}
        e["doc_sentiment"] = list(map(float, sent(np.array([["item1", "item2"], ["item2", "item3"], ["item2", "item5"]]), lsent, "s")))
        e["doc_cand_sentiment"] = list(map(float, sent._candidate_sentiment(list(lsent), 1, lsent, "s")))
        lg = {"item1": {"g": "Action", "sg": ["Action", "Thriller"]}, "item2": {"g": "Action", "sg": ["Action", "Comedy"]},
              "item3": {"g": "Comedy", "sg": ["Comedy"]}}
        Rg = np.array([["item1", "item2"], ["item2", "item3"]])
        e["doc_distribution_g"], e["doc_distribution_sg"] = dist(Rg, lg, "g"), dist(Rg, lg, "sg")
        e["doc_coverage"] = list(map(float, cov(np.array([["item1", "item2"], ["item2", "item3"], ["item4", "item3"]]),
                                                np.array(["item1", "item2", "item3", "item4", "item5", "item6"]))))
        e["doc_fn_intralist"] = float(intralist_diversity(np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]])))
        e["doc_fn_intralist_same"] = float(intralist_diversity(np.array([[0.1, 0.2], [0.1, 0.2]])))
        e["doc_fn_serendipity"] = float(serendipity(np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]]), np.array([[0.7, 0.8, 0.9], [0.1, 0.2, 0.3]])))
        e["doc_fn_novelty"] = [float(novelty([0.1, 0.2, 0.3, 0.4, 0.5])), float(novelty([0.9, 0.9, 0.9, 1.0, 0.5]))]
        # what the reference raises
        raised = {}
        for tag, call in (("serendipity_length_mismatch", lambda: ser(R[:3], H[:2], lookup, bc.VEC)),
                          ("candidate_n_exceeds_items", lambda: div._candidate_diversity(small[:4], 5, lookup, bc.VEC)),
                          ("lookup_key_missing_somewhere", lambda: div(R[:3], {**lookup, "x": {"other": 1}}, bc.VEC)),
                          ("novelty_key_missing", lambda: nov(R[:3], lookup, "no_such_key"))):
            try:
                call()
                raised[tag] = None
            except Exception as ex:  # noqa: BLE001
                raised[tag] = type(ex).__name__
        e["raises"] = raised
    e["source"] = ("ebanalyse/ebnerd-benchmark src/ebrec/evaluation/beyond_accuracy.py run in the build container (numpy %s, sklearn %s); "
                   "for _candidate_diversity alone numpy.math was set to the math module in the generating process, because the "
                   "reference's compute_combinations calls np.math.factorial, which numpy 2 removed" % (np.__version__, sklearn.__version__))
    g["meta"] = np.array(json.dumps(e))


if __name__ == "__main__":
    for case, (seed, n_items, D, n_lists) in {"d96": (20241016, 300, 96, 306), "d768": (20241017, 48, 768, 99)}.items():
        g = make_case(seed, n_items, D, n_lists)
        expected(g, with_functions=(case == "d96"))
        path = bc.GOLDEN / bc.CASES[case]
        np.savez_compressed(path, **g)
        print(case, path.name, path.stat().st_size, "bytes;", int(np.isnan(g["exp_diversity"]).sum()), "NaN diversities,",
              int(np.isnan(g["exp_serendipity"]).sum()), "NaN serendipities")
