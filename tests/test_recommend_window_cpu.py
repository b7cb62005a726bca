"""Host side of recommend(window=Freshness(...)): Freshness.windows against a brute-force loop, its errors, the float64
restatement of the windowed selection, and what recommend() and the entry point refuse before the device works.  No GPU."""
import datetime
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from ebrec.evaluation.freshness import Freshness
from ebrec.utils._constants import (
    DEFAULT_ARTICLE_ID_COL, DEFAULT_ARTICLE_PUBLISHED_TIMESTAMP_COL, DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_IMPRESSION_TIMESTAMP_COL,
)
from tests import recommend_window_cases as wc
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)


# ------------------------------------------------------------------------------------------------ Freshness.windows
def brute_force(pub, cand, times, max_age, min_age):
    """(order, lo, hi) from the definitions: a stable sort written as a key with the position, the ends by counting"""
    order = sorted(range(len(cand)), key=lambda j: (pub[cand[j]], j))
    sorted_pub = [pub[cand[j]] for j in order]
    lo = [0 if max_age is None else sum(p < t - max_age for p in sorted_pub) for t in times]
    hi = [sum(p <= t - min_age for p in sorted_pub) for t in times]
    return order, lo, hi


def check_against_brute_force(pub, cand, times, max_age, min_age, zero):
    order, lo, hi = Freshness(pub, max_age=max_age, **({} if min_age is None else {"min_age": min_age})).windows(cand, times)
    min_age = zero if min_age is None else min_age
    want_order, want_lo, want_hi = brute_force(pub, cand, times, max_age, min_age)
    assert order.dtype == np.int64 and lo.dtype == hi.dtype == np.int32
    assert order.tolist() == want_order and lo.tolist() == want_lo and hi.tolist() == want_hi
    for i, t in enumerate(times):  # the range IS the admissible set
        inside = {int(j) for j in order[lo[i]:hi[i]]}
        want = {j for j, a in enumerate(cand) if (max_age is None or t - max_age <= pub[a]) and pub[a] <= t - min_age}
        assert inside == want, i
    return lo, hi


def test_windows_equal_a_brute_force_loop_on_datetimes():
    day, hour = datetime.timedelta(days=1), datetime.timedelta(hours=1)
    t0 = datetime.datetime(2023, 2, 23)
    rng = np.random.default_rng(0)
    pub = {100 + a: t0 + int(h) * hour for a, h in enumerate(rng.integers(0, 8 * 24 // 6, 40) * 6)}  # six-hour steps: many ties
    assert len(set(pub.values())) < len(pub)
    cand = rng.permutation(np.array(list(pub) + [100, 101, 100]))  # duplicates are distinct candidates
    times = [t0 + int(h) * hour for h in rng.integers(0, 8 * 24, 25)]
    times += [t0 - 3 * day, t0 + 30 * day, pub[105], pub[105] + 2 * day]  # before and after every article, and on the ends
    for max_age, min_age in ((2 * day, None), (None, None), (2 * day, 6 * hour), (None, day), (day, day), (0 * day, None)):
        lo, hi = check_against_brute_force(pub, cand.tolist(), times, max_age, min_age, 0 * day)
        assert lo[25] == hi[25] == 0  # earlier than every article: nothing, whatever the ages
        if max_age is None:
            assert lo[26] == 0 and hi[26] == len(cand)  # later than every article and no oldest age: everything
        else:
            assert lo[26] == hi[26] == len(cand)
    # the same through the other spellings: np.datetime64 / pd.Timestamp times, np.timedelta64 / pd.Timedelta ages, a frame
    want = Freshness(pub, max_age=2 * day).windows(cand, times)
    frame = pd.DataFrame({DEFAULT_ARTICLE_ID_COL: list(pub), DEFAULT_ARTICLE_PUBLISHED_TIMESTAMP_COL: pd.to_datetime(list(pub.values())), "x": 0})
    for fresh, tt in ((Freshness(frame, max_age=np.timedelta64(2, "D")), pd.Series(pd.to_datetime(times))),
                      (Freshness({a: np.datetime64(p) for a, p in pub.items()}, max_age=pd.Timedelta(days=2)), np.array(times, dtype="datetime64[ms]"))):
        got = fresh.windows(cand, tt)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_windows_equal_a_brute_force_loop_on_plain_numbers():
    rng = np.random.default_rng(1)
    pub = {a: float(rng.integers(0, 30)) / 2 for a in range(50)}
    cand = rng.permutation(50)[:35].tolist()
    times = rng.uniform(-2, 18, 30).tolist() + [-5.0, 99.0, 7.5]
    for max_age, min_age in ((3, None), (None, None), (3.5, 1), (None, 2), (0, None)):
        lo, hi = check_against_brute_force(pub, cand, times, max_age, min_age, 0)
        assert lo[30] == hi[30] == 0 and hi[31] == len(cand)
    order, lo, hi = Freshness({7: 1, 8: 2}).windows([], [1.5])  # no candidates: empty ranges
    assert len(order) == 0 and lo.tolist() == hi.tolist() == [0]
    order, lo, hi = Freshness({7: 1, 8: 2}).windows([8, 7], [])  # no impressions
    assert order.tolist() == [1, 0] and len(lo) == len(hi) == 0


# ------------------------------------------------------------------------------------------------ its errors
def test_freshness_errors():
    day = datetime.timedelta(days=1)
    t0 = datetime.datetime(2023, 2, 23)
    pub = {a: t0 + a * day for a in range(8)}
    pub[8], pub[9] = pd.NaT, None
    with pytest.raises(ValueError, match=r"without a publish time: \[8, 20, 21, 22, 23\] and 2 more"):
        Freshness(pub).windows([1, 8, 20, 21, 22, 8, 23, 24, 9], [t0])
    with pytest.raises(ValueError, match=r"without a publish time: \[3\]"):
        Freshness({1: 1.0, 3: float("nan")}).windows([1, 3], [2.0])
    for bad in (dict(max_age=-day), dict(min_age=-day), dict(max_age=day, min_age=2 * day)):
        with pytest.raises(ValueError, match="negative|larger than max_age"):
            Freshness(pub, **bad)
    for bad in (dict(max_age=-1), dict(min_age=-0.5), dict(max_age=1, min_age=2)):
        with pytest.raises(ValueError, match="negative|larger than max_age"):
            Freshness({1: 1.0}, **bad)
    # the two kinds of time do not mix: ages against publish times, impression times against publish times
    with pytest.raises(TypeError, match="plain number but the times are datetimes"):
        Freshness(pub, max_age=2)
    with pytest.raises(TypeError, match="timedelta but the times are plain numbers"):
        Freshness({1: 1.0}, max_age=day)
    with pytest.raises(TypeError, match="do not mix"):
        Freshness(pub).windows([1], [3.0])
    with pytest.raises(TypeError, match="do not mix"):
        Freshness({1: 1.0}).windows([1], [t0])
    with pytest.raises(ValueError, match="impressions have no time"):
        Freshness(pub).windows([1], [t0, pd.NaT])
    with pytest.raises(ValueError, match="lacks the column 'published_time'"):
        Freshness(pd.DataFrame({DEFAULT_ARTICLE_ID_COL: [1]}))
    # 2^31 candidates (a zero-stride view: nothing that large is allocated) are refused before anything is looked up
    with pytest.raises(ValueError, match="at most 2147483647 candidates"):
        Freshness(pub).windows(np.broadcast_to(np.int64(1), (2 ** 31,)), [t0])


def test_importing_freshness_needs_no_torch():
    code = ("import sys; import ebrec.evaluation.freshness as f; assert 'torch' not in sys.modules, 'torch was imported'; "
            "print(f.Freshness({1: 1.0}, max_age=1).windows([1], [1.5])[2].tolist())")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                         env={"PYTHONPATH": ":".join(p for p in sys.path if p), "PATH": ""})
    assert out.returncode == 0 and out.stdout.strip() == "[1]", out.stderr


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("cand,exclude", [("null", None), ("subset", "x3")])
def test_the_restatement_with_every_window_open_is_the_unwindowed_restatement(cand, exclude):
    U, M, F, k = 37, 300, 8, 10
    users, news, cand_rows, ex = wc.integer_case(U, M, F, seed=3, cand=cand, exclude=exclude)
    s64 = wc.scores64(users, news, cand_rows)
    s64[3, 17] = np.nan
    if cand_rows is not None:
        cand_rows[40] = news.shape[0]  # a row outside the table
    want = wc.topk_reference(s64, k, cand_rows, news.shape[0], ex)
    for pattern in ("all", "outside"):
        got = wc.window_reference(s64, k, wc.windows(pattern, U, M), cand_rows, news.shape[0], ex)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_the_restatement_on_hand_written_windows():
    scores = np.array([[1.0, 3.0, 3.0, 2.0, 3.0, np.nan]] * 5)
    window = [[0, 6], [2, 5], [3, 3], [4, 2], [-7, 2]]
    pos, out, flags = wc.window_reference(scores, 3, window)
    assert pos.tolist() == [[1, 2, 4], [2, 4, 3], [-1, -1, -1], [-1, -1, -1], [1, 0, -1]] and flags == (0, 1)
    assert out[1].tolist() == [3.0, 3.0, 2.0] and np.isneginf(out[2]).all() and out[4, :2].tolist() == [3.0, 1.0]
    assert wc.window_reference(scores, 3, [[0, 5]] * 5)[2] == (0, 0)  # the NaN is in nobody's window
    # a row outside the table counts only inside somebody's window
    assert wc.window_reference(scores, 2, [[0, 3]] * 5, cand_rows=[0, 1, 2, 3, 9, 4], n_rows=6)[2] == (0, 0)
    assert wc.window_reference(scores[:2], 2, [[0, 3], [4, 5]], cand_rows=[0, 1, 2, 3, 9, 4], n_rows=6)[2] == (1, 0)


def test_window_patterns_are_what_they_say():
    for U, M in ((1, 1), (3, 7), (65, 257), (130, 1000)):
        for pattern in wc.PATTERNS:
            w = wc.windows(pattern, U, M)
            assert w.shape == (U, 2) and w.dtype == np.int32
            c = wc.clamp(w, M)
            width = c[:, 1] - c[:, 0]
            if pattern in ("all", "outside"):
                assert (width == M).all() and ((w[:, 0] < 0).all() and (w[:, 1] > M).all() if pattern == "outside" else True)
            elif pattern == "empty":
                assert (width == 0).all() and (U < 2 or ((w[::2, 0] == w[::2, 1]).all() and (w[1::2, 0] > w[1::2, 1]).all()))
            elif pattern == "one":
                assert (width == 1).all()
            elif pattern == "sliding":
                assert (width == max(1, M // 4)).all() and (np.diff(w[:, 0]) >= 0).all() and c[-1, 1] == M
    edges = wc.windows("edges", 130, 1000)
    assert set(np.unique(edges)) <= {0, 127, 128, 129, 999, 1000} and len(np.unique(edges)) == 6


# ------------------------------------------------------------------------------------------------ recommend(): validation
class _HostOnlyModel:
    """the hooks of a model, without a device: reaching the cache means the arguments passed validation"""
    _recommend_loader_method = "index_eval_batch"

    def _recommend_index(self, loader):
        return loader.lookup_article_index

    def _recommend_cache(self, loader):
        raise RuntimeError("validation passed")

    def _user_vectors_cached(self, cache, loader, i):
        raise AssertionError


def test_recommend_checks_the_window_before_the_device_works(frames):  # noqa: F811
    from ebrec.models.newsrec import NPAModel
    from ebrec.models.newsrec._recommend import recommend
    from ebrec.models.newsrec.dataloader import NRMSDataLoader

    beh, _train, mapping = frames
    beh = beh.iloc[:8].reset_index(drop=True)
    t0 = pd.Timestamp("2023-02-24")
    mk = lambda b: NRMSDataLoader(behaviors=b, article_dict=mapping, unknown_representation="zeros",
                                  history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=4, eval_mode=True)
    timed = beh.assign(**{DEFAULT_IMPRESSION_TIMESTAMP_COL: [t0 + pd.Timedelta(hours=h) for h in range(8)]})
    model, ids = _HostOnlyModel(), sorted(mapping)[:12]
    pub = {a: t0 - pd.Timedelta(days=30) for a in ids}  # far older than max_age: every window is empty, which is no error
    fresh = Freshness(pub, max_age=pd.Timedelta(days=2))
    with pytest.raises(RuntimeError, match="validation passed"):
        recommend(model, mk(timed), ids, top_n=12, window=fresh)
    with pytest.raises(ValueError, match="larger than the number of candidates"):
        recommend(model, mk(timed), ids, top_n=13, window=fresh)
    with pytest.raises(ValueError, match="lacks the column 'impression_time'"):
        recommend(model, mk(beh), ids, top_n=5, window=fresh)
    with pytest.raises(RuntimeError, match="validation passed"):
        recommend(model, mk(timed.rename(columns={DEFAULT_IMPRESSION_TIMESTAMP_COL: "when"})), ids, top_n=5,
                  window=Freshness(pub, max_age=pd.Timedelta(days=2), time_col="when"))
    with pytest.raises(ValueError, match=rf"without a publish time: \[{ids[3]}\]"):
        recommend(model, mk(timed), ids, top_n=5, window=Freshness({a: p for a, p in pub.items() if a != ids[3]}))
    with pytest.raises(ValueError, match="window must be None or a Freshness"):
        recommend(model, mk(timed), ids, top_n=5, window=(0, 5))
    # a model with a scoring launch of its own has no windowed form: refused before anything else is looked at
    with pytest.raises(NotImplementedError, match="window= is not supported for NPAModel"):
        NPAModel.recommend_pairwise(object.__new__(NPAModel), mk(timed), ids, window=fresh)


def test_window_entry_point_argument_checks_need_no_device():
    import ctypes

    from ebrec import _hip

    lib = _hip.lib()
    dev = ctypes.c_void_p(0x7E0000000000)
    call = lambda **kw: lib.ebn_topk_score_window_f32(*{**dict(users=dev, news=dev, n_rows=500, cand=None, M=500, window=dev, ex=None, X=0,
                                                               k=10, mode=1, n_splits=1, pos=dev, score=dev, flags=dev, ws=None,
                                                               ws_bytes=0, U=64, F=400, stream=None), **kw}.values())
    assert call(window=None) == -1 and call(window=None, M=0, n_rows=0) == -1
    assert call(k=65) == -2 and call(k=0) == -2 and call(ex=dev, X=257) == -2 and call(F=6) == -2 and call(F=8196) == -2
    assert call(users=ctypes.c_void_p(0x7E0000000004)) == -3 and call(news=ctypes.c_void_p(0x7E0000000008)) == -3
    assert call(users=None) == -1 and call(pos=None) == -1 and call(flags=None) == -1 and call(M=499) == -1 and call(mode=2) == -1
    assert call(U=-1) == -1 and call(U=1 << 31) == -1 and call(n_splits=-1) == -1
    assert call(n_splits=2, ws=dev, ws_bytes=lib.ebn_topk_workspace_bytes(64, 10, 2) - 1) == -1
    assert call(U=0, users=None, pos=None, window=None) == 0  # nothing to do
