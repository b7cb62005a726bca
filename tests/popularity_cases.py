"""Cases and the brute-force reference of the trailing-window counts (plain helpers: nothing is collected from here).

A case holds the operands of ebn_window_counts_i32 as numpy arrays: ``event_times`` / ``row_offsets`` (per-row ascending int64
times), ``item_rows`` int32, ``list_offsets`` / ``list_times`` int64, ``max_ages`` (Python ints, UNBOUNDED for no lower end) and
``min_age``.  The reference is ``brute_force``: #{ e : the event's row matches, lo <= e < hi } by numpy broadcasting over
(items x events), with lo = t - max_age and hi = t - min_age computed in Python ints and clipped at INT64_MIN -- neither the
kernel's nested searches nor the twin's composite-key searchsorted."""
import functools

import numpy as np

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
UNBOUNDED = I64_MAX

# events per row of the shared table: the ends of the binary search, an empty row, one row whose events are all equal (row 13)
ROW_EVENTS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 40, 50, 0, 200]
EQUAL_ROW = 13
SPAN = 120  # distinct time values of the shared table: rows of 1000 events are runs of equal times, 8 or 9 long
N_ITEMS = [0, 1, 63, 64, 65, 255, 256, 257, 515]


def brute_force(case) -> np.ndarray:
    ev = np.asarray(case["event_times"], np.int64)
    off = np.asarray(case["row_offsets"], np.int64)
    rows = np.asarray(case["item_rows"], np.int64)
    loff = [int(v) for v in case["list_offsets"]]
    lt = [int(v) for v in case["list_times"]]
    ages, min_age = [int(a) for a in case["max_ages"]], int(case["min_age"])
    n = rows.size
    t = [0] * n
    for l in range(len(lt)):
        for i in range(loff[l], min(loff[l + 1], n)):
            t[i] = lt[l]
    hi = np.array([max(v - min_age, I64_MIN) for v in t], dtype=np.int64).reshape(n)
    ev_row = np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off))
    out = np.zeros((len(ages), n), np.int32)
    for w, age in enumerate(ages):
        lo = np.array([I64_MIN if age == UNBOUNDED else max(v - age, I64_MIN) for v in t], dtype=np.int64).reshape(n)
        for a in range(0, n, 256):  # (items x events) one block of items at a time
            b = min(a + 256, n)
            hit = (ev_row[None, :] == rows[a:b, None]) & (ev[None, :] >= lo[a:b, None]) & (ev[None, :] < hi[a:b, None])
            out[w, a:b] = hit.sum(1)
    return out


def _table(rng, t0, events=ROW_EVENTS, span=SPAN, scale=1):
    """(event_times, row_offsets): row r has events[r] times t0 + v * scale, v drawn from ``span`` values (Python-int exact), sorted"""
    off = np.zeros(len(events) + 1, np.int64)
    np.cumsum(events, out=off[1:])
    ev = np.zeros(off[-1], np.int64)
    for r, m in enumerate(events):
        d = np.sort(rng.integers(0, span, m)) if r != EQUAL_ROW else np.full(m, span // 2)
        ev[off[r]:off[r + 1]] = np.array([t0 + int(v) * scale for v in d], dtype=np.int64)
    return ev, off


def _case(rng, lengths, max_ages, min_age, t0=1000, events=ROW_EVENTS, span=SPAN, t_pad=20, scale=1, times=None):
    """items with random rows from [-1, n_rows] (both ends unknown), every row of the table asked for when there is room; list times
    drawn from [t0 - t_pad, t0 + span + t_pad]: with ages below the span most window ends fall ON event times, inside runs of equal
    times"""
    ev, off = _table(rng, t0, events, span, scale)
    n_rows = len(events)
    loff = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=loff[1:])
    n = int(loff[-1])
    rows = rng.integers(-1, n_rows + 1, n).astype(np.int32)
    if n >= n_rows + 2:
        rows[rng.permutation(n)[:n_rows + 2]] = np.arange(-1, n_rows + 1)
    lt = np.array(times, dtype=np.int64) if times is not None else np.array([min(max(t0 + int(v) * scale, I64_MIN), I64_MAX) for v in rng.integers(-t_pad, span + t_pad + 1, len(lengths))], dtype=np.int64)
    assert len(lt) == len(lengths)
    case = dict(event_times=ev, row_offsets=off, item_rows=rows, list_offsets=loff, list_times=lt,
                max_ages=[int(a) for a in max_ages], min_age=int(min_age))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _lengths(rng, n_items):
    """random list lengths that add up to n_items, some of them empty"""
    out = []
    while sum(out) < n_items:
        out.append(int(min(rng.choice([0, 1, 2, 5, 12, 40]), n_items - sum(out))))
    return out or [0]


def _builders():
    b = {}
    for n in N_ITEMS:
        b[f"items_{n}"] = lambda rng, n=n: _case(rng, _lengths(rng, n), [30, 7, 60], 0, **({"times": [1080], "events": [600]} if n == 1 else {}))
        b[f"items_{n}_min_age"] = lambda rng, n=n: _case(rng, _lengths(rng, n), [25], 3, **({"times": [1080], "events": [600]} if n == 1 else {}))
    # list shapes
    b["empty_lists_first_last_mid"] = lambda rng: _case(rng, [0, 0, 5, 7, 0, 0, 0, 9, 1, 0, 30, 0], [30, 7], 0)
    b["one_list_of_600"] = lambda rng: _case(rng, [600], [30, 7, 60], 1, times=[1075])
    b["lists_3_600_2"] = lambda rng: _case(rng, [3, 600, 2], [30, 7, 60], 0)
    b["300_one_item_lists"] = lambda rng: _case(rng, [1] * 300, [30, 7, 60], 0)
    b["300_empty_lists_in_a_row"] = lambda rng: _case(rng, [4] + [0] * 300 + [5, 0, 270, 3], [30, 7], 0)  # > 256 boundaries in one tile
    b["700_empty_lists_then_items"] = lambda rng: _case(rng, [0] * 700 + [2, 300] + [0] * 300, [30], 0)
    # windows and ages
    b["zero_ages"] = lambda rng: _case(rng, _lengths(rng, 257), [0], 0)
    b["unbounded"] = lambda rng: _case(rng, _lengths(rng, 257), [UNBOUNDED], 0)
    b["unbounded_among_others"] = lambda rng: _case(rng, _lengths(rng, 257), [10, UNBOUNDED, 50, UNBOUNDED], 5)
    b["min_age_above_a_max_age"] = lambda rng: _case(rng, _lengths(rng, 257), [5, 40, 10, 11], 10)
    b["windows_ascending"] = lambda rng: _case(rng, _lengths(rng, 257), [1, 6, 24, 100], 0)
    b["windows_descending"] = lambda rng: _case(rng, _lengths(rng, 257), [100, 24, 6, 1], 0)
    b["windows_mixed_with_duplicate"] = lambda rng: _case(rng, _lengths(rng, 257), [24, 1, 100, 24, 6], 2)
    b["one_window"] = lambda rng: _case(rng, _lengths(rng, 300), [17], 0)
    b["eight_windows"] = lambda rng: _case(rng, _lengths(rng, 300), [3, 90, 1, 45, UNBOUNDED, 0, 45, 12], 1)
    # extreme times
    b["times_above_2_32"] = lambda rng: _case(rng, _lengths(rng, 257), [30, 7, 2 ** 33], 0, t0=2 ** 40 + 12345)
    b["times_differ_above_bit_32_only"] = lambda rng: _case(rng, _lengths(rng, 257), [30 * 2 ** 32, 7 * 2 ** 32], 2 ** 32, t0=5,
                                                            scale=2 ** 32)  # a compare of the low words alone sees all times equal
    b["negative_times"] = lambda rng: _case(rng, _lengths(rng, 257), [30, 7, 60], 0, t0=-2 ** 40)
    b["times_across_zero"] = lambda rng: _case(rng, _lengths(rng, 257), [30, 7, 60], 1, t0=-SPAN // 2)
    b["near_int64_min"] = lambda rng: _case(rng, _lengths(rng, 257), [30, 2 ** 62, I64_MAX - 1, UNBOUNDED], 0, t0=I64_MIN, t_pad=0)
    b["near_int64_min_min_age_saturates"] = lambda rng: _case(rng, _lengths(rng, 257), [2 ** 62, UNBOUNDED], 2 ** 61, t0=I64_MIN + 7, t_pad=0)
    b["near_int64_max"] = lambda rng: _case(rng, _lengths(rng, 257), [30, 2 ** 62, I64_MAX - 1, UNBOUNDED], 0, t0=I64_MAX - SPAN, t_pad=0)
    b["hand_written_window_ends"] = _hand
    return b


def _hand(rng=None):
    """one row, events 10 10 20 20 20 30: an event AT t - max_age is counted, an event AT t - min_age is not (HAND_WANT)"""
    ev = np.array([10, 10, 20, 20, 20, 30], np.int64)
    # lists at t = 30 and t = 31; windows 20, 10, 0 and unbounded; min_age 10: [10, 20) [20, 20) [30, 20) (-inf, 20) | [11, 21) [21, 21) ...
    return dict(event_times=ev, row_offsets=np.array([0, 6], np.int64), item_rows=np.array([0, 0], np.int32),
                list_offsets=np.array([0, 1, 2], np.int64), list_times=np.array([30, 31], np.int64), max_ages=[20, 10, 0, UNBOUNDED], min_age=10)


HAND_WANT = np.array([[2, 3], [0, 0], [0, 0], [2, 5]], np.int32)


BUILDERS = _builders()
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(case, brute-force counts): built once, shared, read-only"""
    c = BUILDERS[name](np.random.default_rng(NAMES.index(name) + 1))
    want = brute_force(c)
    want.setflags(write=False)
    return c, want
