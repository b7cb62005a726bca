"""Host side of the device metric evaluator (no GPU): flattening, dispatch by exact metric type, the host route, the numpy
restatement of the kernel's two flags, and the reference-generated fixture against the repository's host functions."""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import ranking_cases as rc

G = json.loads((Path(__file__).parent / "golden" / "metrics_golden.json").read_text())


def test_ragged_lists_flatten_in_one_pass_and_round_trip():
    from ebrec.evaluation import RaggedLists

    lists = [[0.5, 0.25], [], [1.0], [0.1, 0.2, 0.3]]
    R = RaggedLists.from_lists(lists)
    assert R.flat.dtype == np.float64 and R.flat.tolist() == [0.5, 0.25, 1.0, 0.1, 0.2, 0.3]
    assert R.offsets.dtype == np.int64 and R.offsets.tolist() == [0, 2, 2, 3, 6] and len(R) == 4 and R.lengths.tolist() == [2, 0, 1, 3]
    assert R.to_lists() == lists and R.row(3) == [0.1, 0.2, 0.3] and RaggedLists.from_lists(R) is R
    assert RaggedLists.from_lists([[0, 1], [1]]).flat.dtype == np.int64  # labels stay integers
    assert RaggedLists.from_lists([[0, 0.5], [1]]).flat.tolist() == [0.0, 0.5, 1.0]  # an integer first score does not truncate the rest
    arrays = [np.array([0.5, 0.25], np.float32), np.array([1.0], np.float32)]
    A = RaggedLists.from_lists(arrays)
    assert A.flat.dtype == np.float32 and A.offsets.tolist() == [0, 2, 3]
    assert len(RaggedLists.from_lists([])) == 0 and RaggedLists.from_lists([]).to_lists() == []
    flat = np.arange(5, dtype=np.float32)
    D = RaggedLists(flat, [0, 2, 5])
    assert D.flat is flat and D.to_lists() == [[0.0, 1.0], [2.0, 3.0, 4.0]]  # flat arrays are used as they are
    for bad in ([1, 2, 5], [0, 3, 2, 5], [0, 2, 4]):
        with pytest.raises(ValueError):
            RaggedLists(flat, bad)


def test_dispatch_is_by_exact_metric_type():
    from ebrec.evaluation import AucScore, F1Score, NdcgScore
    from ebrec.evaluation.device_metrics import _slot_of

    assert [_slot_of(m) for m in rc.metrics()] == rc.SLOTS

    class MyAuc(AucScore):
        pass

    class Custom:
        name = "custom"

        def __call__(self, y_true, y_pred):
            return 1.0

    assert _slot_of(MyAuc()) is None and _slot_of(Custom()) is None and _slot_of(len) is None
    assert _slot_of(NdcgScore(k=0)) is None and _slot_of(NdcgScore(k=2.5)) is None and _slot_of(F1Score(threshold="x")) is None
    assert _slot_of(NdcgScore(k=np.int64(7))) == (2, 7.0) and _slot_of(F1Score(threshold=1)) == (6, 1.0)


def test_device_none_equals_the_host_evaluator_and_keeps_its_surface():
    from ebrec.evaluation import DeviceMetricEvaluator, MetricEvaluator, RaggedLists

    host = MetricEvaluator(G["labels"], G["predictions"], rc.metrics()).evaluate()
    ev = DeviceMetricEvaluator(G["labels"], G["predictions"], rc.metrics(), device=None)
    assert str(ev) == "<MetricEvaluator class>: {}"
    assert ev.evaluate() is ev and not ev.on_device
    assert list(ev.evaluations) == rc.NAMES and ev.evaluations == host.evaluations and str(ev) == str(host)
    assert ev.n_impressions == 300
    # RaggedLists in, arrays untouched: the host's in-place binarisation of ndarray inputs is not reproduced
    P = RaggedLists.from_lists([np.array(p) for p in G["predictions"]])
    before = P.flat.copy()
    ev2 = DeviceMetricEvaluator(RaggedLists.from_lists(G["labels"]), P, rc.metrics(), device=None).evaluate()
    assert ev2.evaluations == host.evaluations and np.array_equal(P.flat, before)
    with pytest.raises(TypeError, match="not callable"):
        DeviceMetricEvaluator(G["labels"], G["predictions"], [rc.metrics()[0], 3], device=None)
    with pytest.raises(TypeError, match="not callable"):
        DeviceMetricEvaluator(G["labels"], G["predictions"], [], device=None)
    with pytest.raises(ValueError):
        DeviceMetricEvaluator([[0, 1]], [[0.5, 0.2, 0.1]], rc.metrics(), device=None).evaluate()


def test_ragged_ranks_on_the_host_route_equal_the_list_function():
    from ebrec.utils._python import rank_predictions_by_score, rank_predictions_by_score_ragged

    lists = [[0.2, 0.9, 0.5], [0.1], [], [0.3, 0.3, 0.7]]
    want = [rank_predictions_by_score(x) for x in lists]
    flat, off = np.array([v for x in lists for v in x]), [0, 3, 4, 4, 7]
    for got in (rank_predictions_by_score_ragged(lists, device=None), rank_predictions_by_score_ragged(flat, off, device=None),
                rank_predictions_by_score_ragged(None, lists, device=None)):
        assert len(got) == 4 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert want[0].tolist() == [3, 1, 2]


def test_flag_definitions_in_numpy():
    from ebrec.evaluation.device_metrics import tie_ambiguous_and_nonfinite as f

    assert f([1, 0, 0], [0.5, 0.4, 0.3]) == (False, False)
    assert f([1, 0, 0], [0.5, 0.4, 0.4]) == (False, False)  # a tie among negatives: any order gives the same mrr / ndcg
    assert f([1, 1, 0], [0.5, 0.5, 0.4]) == (False, False)  # a tie among positives
    assert f([1, 0, 0], [0.4, 0.4, 0.3]) == (True, False)  # a positive and a negative share a score
    assert f([1, 0], [0.0, -0.0]) == (True, False)  # -0.0 == 0.0
    assert f([1, 0], [float("nan"), float("nan")]) == (False, True)  # NaN equals nothing
    assert f([1, 0], [float("inf"), float("inf")]) == (True, True)
    assert f([], []) == (False, False) and f([1], [0.3]) == (False, False)
    # float32 scores are compared as float32: two values that differ only past its precision tie
    a = np.array([0.1, 0.1 + 1e-10])
    assert f([1, 0], a) == (False, False) and f([1, 0], a.astype(np.float32)) == (True, False)
    flagged = [f(y, p)[0] for y, p in zip(G["labels"], G["predictions"])]
    assert sum(flagged) == 79  # of the 300 lists of tests/golden/metrics_golden.json


def test_fixture_rows_equal_the_host_functions_and_the_counting_formulas():
    """The reference's per-row values of tests/golden/ranking_golden.npz against (a) the repository's host wrappers, every row,
    and (b) the counting formulas the kernel uses, on every list that is not tie-ambiguous (there the order inside a tie group
    does not matter)."""
    for group in ("main", "one"):
        g = rc.load(group)
        got = rc.host_values(g["labels"], g["scores"], g["offsets"])
        assert np.array_equal(np.isnan(got), np.isnan(g["ref"])), group
        ok = ~np.isnan(got)
        assert np.all(np.abs(got[ok] - g["ref"][ok]) <= 1e-12 * np.abs(g["ref"][ok])), group
        flags = rc.flags_numpy(g["labels"], g["scores"], g["offsets"])
        ys, ss = rc.split(g["labels"], g["offsets"]), rc.split(g["scores"], g["offsets"])
        for l in np.flatnonzero(flags == 0):
            mine = np.array(rc.counting_values(ys[l], ss[l]))
            want = g["ref"][:, l]
            assert np.array_equal(np.isnan(mine), np.isnan(want)), (group, l)
            fin = ~np.isnan(want)
            assert np.all(np.abs(mine[fin] - want[fin]) <= 1e-12 * np.abs(want[fin])), (group, l, mine, want)
    g = rc.load("main")
    lens = np.diff(g["offsets"])
    assert set([2, 15, 16, 17, 63, 64, 65, 250, 255, 256, 257, 1023, 1024, 1025, 5000]) <= set(lens.tolist()) and len(lens) > 3000
    flags = rc.flags_numpy(g["labels"], g["scores"], g["offsets"])
    assert 0 < flags.mean() <= 0.10 and np.all(g["scores"].astype(np.float32) == g["scores"])
    assert 1 in np.diff(rc.load("one")["offsets"]).tolist()
