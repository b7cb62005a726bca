"""Guard-banded operands, assertion helpers and numpy stand-ins for the evaluation and re-ranking kernels (plain helpers: no
fixtures, nothing collected from here).  Shared by tests/test_guarded_rerank_gpu.py, tests/test_guarded_beyond_gpu.py and
tests/test_guarded_rank_metrics_gpu.py, which hand the operands to the HIP entry points, and by tests/test_guarded_eval_cpu.py,
which hands the SAME operands (device="cpu") to the stand-ins below, plants one defect and pushes the result through the SAME
check_* helpers: a reviewer without a GPU can tell there that the guards bite.

Guard values, chosen so that a read of one SHOWS (tests/guarded.py: a read whose value is discarded cannot be seen):
  float tables, targets, scalar columns, distance matrices   NaN        raises flags[1] / gives a NaN value / changes a pick
  row numbers, ids, subset indices                           a VALID one the entry is used: one more term in a mean, one more candidate
  relevances, history weights                                3e18       a present entry that wins round 0 (a pick >= P, a wrong first pick)
  int64 offsets (as int32 word pairs)                        0          the list runs backwards: empty, its value NaN
  float64 scores / parameters (as int32 word pairs)          0x7FF00000 two such words are a NaN: flag bit 1
  uint8 labels (four to an int32 word)                       0x01010101 an over-read label is a positive
Outputs sit in canaries with a pre-filled payload (guarded.guard_out); flags[2] of the re-rankers is a zeroed in/out payload in
canaries; byte / int64 / float64 outputs are int32 words, a byte array's last word keeps the pre-fill in its unused bytes."""
import numpy as np
import torch

from tests import guarded
from tests.guarded import PREFILL_I32, guard_in, guard_out

GUARD = 4096          # elements per side of the flat operands (nothing here strides by a leading dimension)
BIG = 3e18            # guard of relevances and weights
F64_NAN_WORD = 0x7FF00000
LABEL_WORD = 0x01010101
NAN = float("nan")


def _np(t):
    return t.detach().cpu().numpy()


def table_guard(ld):
    """two rows of guard on each side of a table (a multiple of four elements, at least GUARD)"""
    return max(GUARD, (2 * int(ld) + 3) // 4 * 4)


# ------------------------------------------------------------------------------------------------ operands seen as int32 words
def words_in(x, fill_word, device="cuda"):
    """a uint8 / int64 / float64 array as int32 words inside guards of `fill_word` -> (view, handle); a byte array that ends
    inside a word is padded with that word's bytes"""
    b = np.ascontiguousarray(x).view(np.uint8).ravel()
    tail = np.array([fill_word], np.uint32).view(np.uint8)[len(b) % 4:] if len(b) % 4 else np.empty(0, np.uint8)
    words = np.concatenate([b, tail]).view(np.int32)
    return guard_in(words, fill=int(np.array([fill_word], np.uint32).view(np.int32)[0]), device=device, guard=GUARD)


def words_out(n_bytes, device="cuda"):
    """an output of n_bytes bytes as int32 words in canaries, every word pre-filled -> (view, handle)"""
    return guard_out(((int(n_bytes) + 3) // 4,), dtype=torch.int32, device=device, guard=GUARD)


def read_words(handle, dtype, n):
    """the first n elements of `dtype` of a word operand's payload, as numpy"""
    return _np(handle.payload()).view(dtype)[:n].copy()


def raw_as(handle, dtype):
    """CPU only: the operand as C sees it from its first payload element on, as `dtype` -- index 0 is element 0, an index past
    the payload lands in the guard behind it"""
    flat, start = handle.raw()
    tail, size = flat[start:].view(np.uint8), np.dtype(dtype).itemsize
    return tail[:len(tail) // size * size].view(dtype)


def check_byte_tail(handle, n_bytes, what):
    """the bytes of a byte output's last word behind its n_bytes elements still hold the pre-fill"""
    got = _np(handle.payload()).view(np.uint8)[n_bytes:]
    want = np.array([PREFILL_I32], np.int32).view(np.uint8)[n_bytes % 4:] if n_bytes % 4 else np.empty(0, np.uint8)
    assert np.array_equal(got, want), f"{what}: bytes behind element {n_bytes - 1} of the last word were written: {got.tolist()}"


def zeroed_flags(n, device):
    """an in/out flag array the kernels only ever set: a zero payload inside canaries"""
    view, h = guard_out((n,), dtype=torch.int32, device=device, guard=GUARD)
    h.fill_payload(np.zeros(n, np.int32))
    return view, h


def csr(lists):
    """-> (flat int32 ids, int64 offsets) of ragged id lists"""
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.empty(0, np.int64)]).astype(np.int32)
    return flat, off


# ------------------------------------------------------------------------------------------------ the re-ranking pools
def name_both_ends(table, rows, rel):
    """The case with the first entry of user 0 on table row 0 and the last entry of the last user on the last row, both present (a
    one-entry case: a one-row table): row 0's first float4 and the last row's last one are then read."""
    table, rows, rel = np.array(table), np.array(rows), np.array(rel)
    if rows.size == 1:
        table = table[:1]
    rows[0, 0], rows[-1, -1] = 0, len(table) - 1
    for u, i in ((0, 0), (-1, -1)):
        if not np.isfinite(rel[u, i]):
            rel[u, i] = 0.5
    assert_names_both_ends(table, rows, rel)
    return table, rows, rel


def assert_names_both_ends(table, rows, rel):
    named = np.asarray(rows)[np.isfinite(np.asarray(rel, np.float64))]
    assert (named == 0).any() and (named == len(table) - 1).any(), "the pool must name row 0 and the last row of the table"


class PoolOps:
    """The operands of one ebn_mmr_rerank_f32 / ebn_dpp_rerank_f32 / ebn_calibrated_rerank_f32 call.  `off`: pointer offset (in
    elements) of pool_rows, pool_rel, out_sel, out_obj and target; `table_off`: that of the table (the calibrated W only)."""

    def __init__(self, table, rows, rel, k, device="cuda", off=0, table_off=0, target=None):
        assert_names_both_ends(table, rows, rel)
        self.U, self.P = rows.shape
        self.n_rows, self.D = table.shape
        self.k = int(k)
        n = self.U * self.k
        self.h = {}
        self.table, self.h["table"] = guard_in(table, fill=NAN, device=device, offset=table_off, guard=table_guard(self.D))
        self.rows, self.h["pool_rows"] = guard_in(np.asarray(rows, np.int32).reshape(-1), fill=0, device=device, offset=off, guard=GUARD)
        self.rel, self.h["pool_rel"] = guard_in(np.asarray(rel, np.float32).reshape(-1), fill=BIG, device=device, offset=off, guard=GUARD)
        self.sel, self.h["out_sel"] = guard_out((n,), dtype=torch.int32, device=device, offset=off, guard=GUARD)
        self.obj, self.h["out_obj"] = guard_out((n,), device=device, offset=off, guard=GUARD)
        self.flags, self.h["flags"] = zeroed_flags(2, device)
        self.target = None
        if target is not None:
            self.target, self.h["target"] = guard_in(np.asarray(target, np.float32).reshape(-1), fill=NAN, device=device, offset=off, guard=GUARD)

    def check(self):
        for name, h in self.h.items():
            h.check(name)

    def results(self):
        """-> (sel [U, k] int32, obj [U, k] float32, flags (2,))"""
        shape = (self.U, self.k)
        return (_np(self.h["out_sel"].payload()).reshape(shape), _np(self.h["out_obj"].payload()).reshape(shape),
                tuple(int(f) for f in _np(self.h["flags"].payload())))


def check_pool_result(ops, want_flags, want=None, greedy=None):
    """What every guarded re-ranking test asserts after the call: no operand written, every canary intact, every output written;
    the flags; every pick inside [-1, P); then the picks and objectives EQUAL to `want` = (sel, obj float64) where the case is
    exact, or the greedy property `greedy(sel, obj)` (the existing checkers, which assert with the existing tolerances)."""
    ops.check()
    sel, obj, flags = ops.results()
    assert flags == tuple(want_flags), f"flags {flags}, want {tuple(want_flags)}"
    assert ((sel >= -1) & (sel < ops.P)).all(), f"a pick outside the pool: {sel[(sel < -1) | (sel >= ops.P)][:4]}"
    if want is not None:
        assert np.array_equal(sel, want[0]), "picks differ from the restatement"
        assert np.array_equal(obj.astype(np.float64), want[1]), "objectives differ from the restatement"
    if greedy is not None:
        greedy(sel, obj)
    return sel, obj


def standin_mmr(ops, lam, defect=None):
    """The index walk of ebn_mmr_rerank_f32 over the operands as C sees them, in float32 numpy: workgroups of one user (P > 32) or
    two (P <= 32, one `u < U` guard for a user's loads and stores), the pool, the gather of D floats per present entry, the
    distances, the greedy rounds (tests/rerank_cases.py), k stores per user.  Planted defects:
      pool_entry_P     a user's pool is read one entry too far
      phantom_user     the `u < U` guard of a half-empty workgroup is missing
      table_round32    the gather takes D rounded up to the 32-deep slab on the last table row
      store_k_plus_1   k + 1 picks are stored
      flags2           flags[2] is written"""
    (t, t0), (r, r0), (x, x0) = ops.h["table"].raw(), ops.h["pool_rows"].raw(), ops.h["pool_rel"].raw()
    (s, s0), (o, o0), (f, f0) = ops.h["out_sel"].raw(), ops.h["out_obj"].raw(), ops.h["flags"].raw()
    U, P, D, k, n_rows = ops.U, ops.P, ops.D, ops.k, ops.n_rows
    upw = 2 if P <= 32 else 1
    lam32 = np.float32(lam)
    oml = np.float32(1) - lam32
    d_pad = -(-D // 32) * 32
    for wg in range(-(-U // upw)):
        for g in range(upw):
            u = wg * upw + g
            if u >= U and defect != "phantom_user":
                continue
            n = P + 1 if defect == "pool_entry_P" else P
            rows_u, rel_u = r[r0 + u * P:r0 + u * P + n].astype(np.int64), x[x0 + u * P:x0 + u * P + n]
            row_ok, rel_ok = (rows_u >= 0) & (rows_u < n_rows), np.isfinite(rel_u)
            if (~row_ok & (rows_u != -1)).any():
                f[f0] = 1
            if (~rel_ok & ~np.isneginf(rel_u)).any():
                f[f0 + 1] = 1
            present = row_ok & rel_ok
            vec = np.zeros((n, d_pad), np.float32)
            for i in np.flatnonzero(present):
                width = d_pad if defect == "table_round32" and rows_u[i] == n_rows - 1 else D
                vec[i, :width] = t[t0 + rows_u[i] * D:t0 + rows_u[i] * D + width]
            with np.errstate(invalid="ignore", over="ignore"):
                dots = vec @ vec.T
            nan = np.isnan(dots)
            if (nan & present[:, None] & present[None, :] & ~np.eye(n, dtype=bool)).any():
                f[f0 + 1] = 1
            dist = np.where(nan, np.float32(0), np.minimum(np.maximum(np.float32(1) - np.where(nan, np.float32(0), dots), np.float32(0)), np.float32(2)))
            n_store = k + 1 if defect == "store_k_plus_1" else k
            sel, obj = np.full(n_store, -1, np.int32), np.full(n_store, -np.inf, np.float32)
            left, mind, rel0 = present.copy(), np.full(n, np.inf, np.float32), np.where(present, rel_u, np.float32(0))
            for round_ in range(k):
                if not left.any():
                    break
                cur = np.where(left, rel0 if round_ == 0 else lam32 * rel0 + oml * np.where(left, mind, np.float32(0)), -np.inf).astype(np.float32)
                best = int(np.argmax(cur))
                sel[round_], obj[round_] = best, cur[best]
                left[best] = False
                mind = np.minimum(mind, dist[best])
            s[s0 + u * k:s0 + u * k + n_store] = sel
            o[o0 + u * k:o0 + u * k + n_store] = obj
    if defect == "flags2":
        f[f0 + 2] = 1


def mmr_float32_equals(table, rows, rel, k, lam, want):
    """whether the float32 restatement of the walk (standin_mmr on host operands) gives the float64 restatement's picks and
    objectives bit for bit: the case is then exact, and the kernel is held to equality"""
    ops = PoolOps(table, rows, rel, k, device="cpu")
    standin_mmr(ops, lam)
    sel, obj, flags = ops.results()
    return np.array_equal(sel, want[0]) and np.array_equal(obj.astype(np.float64), want[1]) and flags == tuple(want[2])


# ------------------------------------------------------------------------------------------------ id lists over a table
class ListOps:
    """The operands of one ebn_ba_list_mean_f32 / ebn_ba_intralist_f32 call: a table (`values` [n_rows] or [n_rows, D]) in NaN,
    the ids inside a VALID row number, the int64 offsets as word pairs inside zero words, the output in canaries."""

    def __init__(self, table, lists, device="cuda", table_off=0, guard_id=1):
        table = np.asarray(table, np.float32)
        self.n_rows = len(table)
        self.D = table.shape[1] if table.ndim == 2 else 1
        ids, off = csr(lists)
        assert len(ids) > 0 and 0 <= guard_id < self.n_rows
        self.n_ids, self.n_lists = len(ids), len(lists)
        self.h = {}
        self.table, self.h["table"] = guard_in(table, fill=NAN, device=device, offset=table_off, guard=table_guard(self.D))
        self.ids, self.h["ids"] = guard_in(ids, fill=guard_id, device=device, guard=GUARD)
        self.off, self.h["offsets"] = words_in(off, 0, device)
        self.out, self.h["out"] = guard_out((self.n_lists,), device=device, guard=GUARD)

    def check(self):
        for name, h in self.h.items():
            h.check(name)

    def result(self):
        return _np(self.h["out"].payload()).astype(np.float64)


def check_list_values(ops, want, check):
    """after an id-list call: no operand written, every canary intact, every output written; then `check(got float64, want)`,
    one of the existing comparisons (check_dist / check_mean of tests/test_beyond_accuracy_gpu.py)"""
    ops.check()
    check(ops.result(), want)


def list_mean_reference(values, lists, transform):
    """-> (float64 means, the largest |term| of each list), NaN for a list without a valid id"""
    fn = (lambda v: v) if transform == 0 else (lambda v: -np.log2(v))
    terms = [fn(np.asarray(values, np.float64)[[i for i in x if 0 <= i < len(values)]]) for x in lists]
    return (np.array([t.mean() if len(t) else np.nan for t in terms]), np.array([np.abs(t).max() if len(t) else np.nan for t in terms]))


def standin_list_mean(ops, transform, defect=None):
    """The index walk of ebn_ba_list_mean_f32: list l spans ids[off[l] : off[l + 1]] (a span that runs backwards or leaves
    [0, n_ids] is empty), an id outside the table is skipped.  Planted defect  id_past_end: every list is read one id too far."""
    (v, v0), ids, off, out = ops.h["table"].raw(), raw_as(ops.h["ids"], np.int32), raw_as(ops.h["offsets"], np.int64), raw_as(ops.h["out"], np.float32)
    for l in range(ops.n_lists):
        o0, o1 = int(off[l]), int(off[l + 1])
        if not (0 <= o0 <= o1 <= ops.n_ids):
            o0 = o1 = 0
        span = ids[o0:o1 + 1] if defect == "id_past_end" else ids[o0:o1]
        terms = np.array([v[v0 + i] for i in span if 0 <= i < ops.n_rows], np.float64)
        if transform == 1:
            terms = -np.log2(terms)
        out[l] = np.float32(terms.mean()) if len(terms) else np.float32(np.nan)


# ------------------------------------------------------------------------------------------------ ranking metrics
RM_LPB = 256      # lists per workgroup of csrc/ebn_rankmetrics.hip
RM_SLOTS_MAX = 16


def rank_case(lens, seed, ties=(3, 5)):
    """Ragged lists of the given lengths: distinct float32 scores in (0, 1), labels positive with probability 0.3; the lists
    numbered in `ties` (where they hold two candidates or more) get two equal scores with different labels.
    -> (labels uint8, scores float32, offsets int64)"""
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    n = int(off[-1])
    scores = (rng.permutation(n).astype(np.float32) + np.float32(0.5)) / np.float32(max(n, 1))  # distinct: n < 2^23
    labels = (rng.random(n) < 0.3).astype(np.uint8)
    for l in ties:
        if l < len(lens) and lens[l] >= 2:
            a = int(off[l])
            scores[a + 1], labels[a], labels[a + 1] = scores[a], 0, 1
    return labels, scores, off


def rank_reference(labels, scores, off):
    """-> (values float64 [8, n_lists] by ranking_cases.counting_values, flags uint8 by ranking_cases.flags_numpy, counters [3])"""
    from tests import ranking_cases as rc

    n_lists = len(off) - 1
    values = np.array([rc.counting_values(y, s) for y, s in zip(rc.split(labels, off), rc.split(scores, off))]).T.reshape(8, n_lists)
    flags = rc.flags_numpy(labels, scores, off)
    one_class = sum(int(y.sum()) in (0, len(y)) for y in rc.split(labels, off))
    return values, flags, np.array([one_class, int((flags & 1).sum()), int(((flags & 2) != 0).sum())], np.int64)


class RankOps:
    """The operands of one ebn_rank_metrics call (f32 or f64 scores, the eight slots of ranking_cases.SLOTS) with the workspace
    at exactly `ws_bytes`, poisoned; `ranks` and `rank_flags` are the outputs of ebn_list_ranks over the same lists."""

    def __init__(self, labels, scores, off, ws_bytes, f64=False, per_list=True, device="cuda"):
        from tests import ranking_cases as rc

        self.n_items, self.n_lists, self.n_slots, self.f64, self.ws_bytes = len(scores), len(off) - 1, len(rc.SLOTS), f64, int(ws_bytes)
        self.h = {}
        if f64:
            self.scores, self.h["scores"] = words_in(np.asarray(scores, np.float64), F64_NAN_WORD, device)
        else:
            self.scores, self.h["scores"] = guard_in(np.asarray(scores, np.float32), fill=NAN, device=device, guard=GUARD)
        self.labels, self.h["labels"] = words_in(np.asarray(labels, np.uint8), LABEL_WORD, device)
        self.off, self.h["offsets"] = words_in(np.asarray(off, np.int64), 0, device)
        self.kinds, self.h["slot_kind"] = guard_in(np.array([k for k, _ in rc.SLOTS], np.int32), fill=6, device=device, guard=GUARD)
        self.params, self.h["slot_param"] = words_in(np.array([p for _, p in rc.SLOTS], np.float64), F64_NAN_WORD, device)
        self.sums, self.h["sums"] = words_out(8 * self.n_slots, device)
        self.flags, self.h["flags"] = words_out(self.n_lists, device)
        self.counters, self.h["counters"] = words_out(24, device)
        self.per_list = None
        if per_list:
            self.per_list, self.h["per_list"] = words_out(8 * self.n_slots * self.n_lists, device)
        self.ws, self.h["workspace"] = words_out(self.ws_bytes, device)
        self.h["workspace"].fill_payload(np.full(self.ws_bytes // 4, -1, np.int32))  # poison: every byte 0xFF
        self.ranks, self.h["ranks"] = guard_out((self.n_items,), dtype=torch.int32, device=device, guard=GUARD)
        self.rank_flags, self.h["rank_flags"] = words_out(self.n_lists, device)

    def check(self, names):
        for name in names:
            self.h[name].check(name)

    def metric_results(self):
        """-> (sums [8], flags uint8 [n_lists], counters int64 [3], per-list values [8, n_lists] or None)"""
        values = read_words(self.h["per_list"], np.float64, self.n_slots * self.n_lists).reshape(self.n_slots, self.n_lists) if self.per_list is not None else None
        return (read_words(self.h["sums"], np.float64, self.n_slots), read_words(self.h["flags"], np.uint8, self.n_lists),
                read_words(self.h["counters"], np.int64, 3), values)

    def rank_results(self):
        return _np(self.h["ranks"].payload()), read_words(self.h["rank_flags"], np.uint8, self.n_lists)


METRIC_OPERANDS = ("scores", "labels", "offsets", "slot_kind", "slot_param", "sums", "flags", "counters", "workspace")
RANK_OPERANDS = ("scores", "offsets", "ranks", "rank_flags")


def check_metric_result(ops, ref, what):
    """after ebn_rank_metrics: inputs untouched, canaries intact (the workspace's too), every output written, the unused bytes of
    the flags' last word untouched; flags and counters exact, per-list values and sums within the existing bounds (`close` and
    `check_sums` of tests/test_device_metrics_gpu.py).  -> the sums, for the bit comparisons between runs"""
    from tests.test_device_metrics_gpu import check_sums, close

    values_ref, flags_ref, counters_ref = ref
    ops.check(METRIC_OPERANDS + (("per_list",) if ops.per_list is not None else ()))
    check_byte_tail(ops.h["flags"], ops.n_lists, f"{what}: flags")
    sums, flags, counters, values = ops.metric_results()
    assert np.array_equal(flags, flags_ref), f"{what}: flags differ at lists {np.flatnonzero(flags != flags_ref)[:8]}"
    assert counters.tolist() == counters_ref.tolist(), (what, counters.tolist(), counters_ref.tolist())
    if values is not None:  # as tests/test_device_metrics_gpu.py: a tie-ambiguous list's mrr / ndcg are the host's to decide
        from tests.ranking_cases import RANKED_ROWS

        plain, rest = flags_ref == 0, [m for m in range(ops.n_slots) if m not in RANKED_ROWS]
        close(values[:, plain], values_ref[:, plain], f"{what}: per-list values of the unflagged lists")
        close(values[rest], values_ref[rest], f"{what}: per-list auc / logloss / rmse / accuracy / f1 of every list")
    check_sums(sums, values_ref, flags_ref, what)
    return sums


def check_rank_result(ops, labels, scores, off, what):
    """after ebn_list_ranks: ranks equal to rank_predictions_by_score list by list, zeros and flag bit 0 for a list with two equal
    scores (there the host decides)"""
    from ebrec.utils._python import rank_predictions_by_score
    from tests import ranking_cases as rc

    ops.check(RANK_OPERANDS)
    check_byte_tail(ops.h["rank_flags"], ops.n_lists, f"{what}: flags")
    ranks, flags = ops.rank_results()
    for l, (r, s) in enumerate(zip(rc.split(ranks, off), rc.split(scores, off))):
        tied = len(np.unique(s)) < len(s)
        assert flags[l] == (1 if tied else 0), (what, l, int(flags[l]))
        assert (not r.any()) if tied else np.array_equal(r, rank_predictions_by_score(s)), (what, l)


def standin_rank_metrics(ops, defect=None):
    """The index walk of ebn_rank_metrics (form 0, f32 scores) over the operands as C sees them: workgroup b owns lists
    [256 b, 256 b + 256), a list of at most 16 candidates runs in a 16-lane group whose lanes `gl < len` load, every list stores a
    flag byte and its eight values, every workgroup one partial per slot and three counts into the workspace, a closing pass
    adds them in workgroup order.  Values by ranking_cases.counting_values.  Planted defects:
      short_reads_16        the 16-lane form loads 16 candidates whatever len is
      workspace_one_more    partials are stored for one workgroup more than there are"""
    from ebrec.evaluation.device_metrics import tie_ambiguous_and_nonfinite
    from tests import ranking_cases as rc

    (s, s0), lab, off = ops.h["scores"].raw(), raw_as(ops.h["labels"], np.uint8), raw_as(ops.h["offsets"], np.int64)
    flags, per_list = raw_as(ops.h["flags"], np.uint8), raw_as(ops.h["per_list"], np.float64)
    sums, counters, ws = raw_as(ops.h["sums"], np.float64), raw_as(ops.h["counters"], np.int64), raw_as(ops.h["workspace"], np.float64)
    n_lists, n_slots = ops.n_lists, ops.n_slots
    blocks = -(-n_lists // RM_LPB)
    part_cnt = ws[RM_SLOTS_MAX * blocks:].view(np.int64)
    for b in range(blocks + (1 if defect == "workspace_one_more" else 0)):
        acc, cnt = np.zeros(RM_SLOTS_MAX), np.zeros(3, np.int64)
        for l in range(b * RM_LPB, min(b * RM_LPB + RM_LPB, n_lists)):
            o0, o1 = int(off[l]), int(off[l + 1])
            beg, n = (o0, o1 - o0) if 0 <= o0 <= o1 <= ops.n_items else (0, 0)
            if n <= 16 and defect == "short_reads_16":
                n = 16
            y, sc = lab[beg:beg + n].copy(), s[s0 + beg:s0 + beg + n].copy()
            tie, bad = tie_ambiguous_and_nonfinite(y, sc)
            with np.errstate(all="ignore"):
                vals = rc.counting_values(y != 0, sc)
            flags[l] = (1 if tie else 0) | (2 if bad else 0)
            one_class = int((y != 0).sum()) in (0, n)
            cnt += (int(one_class), int(tie), int(bad))
            for m in range(n_slots):
                per_list[m * n_lists + l] = vals[m]
                if not (bad or (tie and m in rc.RANKED_ROWS) or (one_class and m in rc.TWO_CLASS_ROWS)):
                    acc[m] += vals[m]
        ws[b * RM_SLOTS_MAX:(b + 1) * RM_SLOTS_MAX] = acc
        part_cnt[3 * b:3 * b + 3] = cnt
    for m in range(n_slots):
        sums[m] = sum(float(ws[b * RM_SLOTS_MAX + m]) for b in range(blocks))
    for c in range(3):
        counters[c] = sum(int(part_cnt[3 * b + c]) for b in range(blocks))
