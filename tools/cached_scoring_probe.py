"""Times scorer.predict over a synthetic eval-mode loader with the article catalogue encoded once against the per-batch path, for
LSTUR (lstur-c1), NAML (naml-c1) or NPA (npa-c1), in ONE run on one GPU: the per-batch figure is the baseline of the cached figure beside it.

Loader (flags for its size): 20 000 articles, 100 000 impressions, in-view lengths 4 + geometric with mean about 11.6 and 0.2 % of
the lists 250 long (the me-c1 distribution), H = 20 (left-padded histories of different lengths), batch 1024; 32000 x 300 word table.
Model shapes: lstur-c1 (T 30, filter_num = gru_unit 400, window 3, attention_hidden_dim 200, n_users 50000, --type ini|con) and
naml-c1 (T 30, body 40, 100 x 10 vert / subvert tables, filter_num 400, attention_hidden_dim 200); npa-c1 (T 30, filter_num 400,
window 3, attention_hidden_dim 200, user_emb_dim 400, n_users 50000) over the LSTUR leg's loader.  Reported per run:
  * impressions/s of scorer.predict with the cache and without it (wall clock around the call: loader slicing, uploads, launches,
    the download of every batch's scores), `--reps` rounds each, interleaved, after a warm-up of both paths on the first batches;
  * the catalogue build on its own (encode_catalogue, synchronised);
  * NAML: the indexed pooling-and-scoring kernel over the WHOLE loader in one launch (HIP events), as row-read bandwidth
    (history + candidate rows x F x 4 bytes / time) beside this box's float4-copy calibration measured in the same run (the
    library's gather kernel over the identity permutation of 4 KB rows, 1 GiB, (read + write bytes) / time);
    LSTUR: the indexed GRU (H launches) of one full batch;
    NPA: the indexed personalised pooling fused with the score over EVERY candidate of the loader in one launch, as catalogue-read
    bandwidth (candidates x T x (F + A) x 4 bytes / time: the bytes it must read) beside the same float4-copy calibration, and the
    catalogue's bytes.  The NPA result line is also appended to profiles/cached_scoring_npa_c1.jsonl (--out).
Prints ONE JSON line; asserts that the two paths agree to 2e-6 and (LSTUR, NAML) that the cached path is the faster one by more
than 4 %; for NPA the line carries "cached_is_faster" instead (the default of the cached path follows it).
One model per process.  Run the two models as two steps, each under its own time limit, chained with && :
    timeout -k 10 900 python tools/cached_scoring_probe.py --model lstur && timeout -k 10 900 python tools/cached_scoring_probe.py --model naml
Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/cached_scoring_probe.py ...`.
usage: cached_scoring_probe.py --model lstur|naml|npa [--out FILE] [--type ini|con] [--articles N] [--impressions N] [--history H] [--batch B] [--reps K]"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np
import pandas as pd
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec import _hip  # noqa: E402

V, E = 32000, 300


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def float4_copy_gbs(reps):
    n = (1 << 30) // 4
    src, dst = torch.empty(n, device="cuda").normal_(), torch.empty(n, device="cuda")
    rows = n // 1024
    ids = torch.arange(rows, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    fn = lambda: _hip.call("ebn_gather_rows_f32", _hip.ptr(ids), _hip.ptr(src), _hip.ptr(dst), rows, 1024, rows, None, -1,
                           ctypes.c_float(0.0), _hip.ptr(flag), _hip.stream_handle())
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return (2.0 * n * 4 + rows * 4) / events_ms(fn, reps) / 1e6


def make_frame(n_articles, n_impressions, H, seed=0, long_share=0.002):
    """behaviors with the me-c1 in-view lengths; article ids 1000.., 2 % of the in-view ids unknown, histories left-padded with 0"""
    rng = np.random.default_rng(seed)
    ids = np.arange(1000, 1000 + n_articles)
    lens = np.minimum(4 + rng.geometric(1 / 7.6, n_impressions), 100)
    lens[rng.random(n_impressions) < long_share] = 250
    flat = rng.choice(ids, int(lens.sum()))
    flat[rng.random(flat.size) < 0.02] = 7
    inview = np.split(flat, np.cumsum(lens)[:-1])
    his = rng.choice(ids, (n_impressions, H))
    his[np.arange(H)[None, :] < rng.integers(0, H // 2 + 1, n_impressions)[:, None]] = 0
    df = pd.DataFrame({"user_id": rng.integers(0, 60000, n_impressions), "article_id_fixed": list(his), "article_ids_inview": inview,
                       "labels": [np.zeros(n, np.int8) for n in lens]})
    return df, ids, lens


def build(a):
    from ebrec.models.newsrec import LSTURModel, NAMLModel, NPAModel
    from ebrec.models.newsrec.dataloader import LSTURDataLoader, NAMLDataLoader

    rng = np.random.default_rng(1)
    df, ids, lens = make_frame(a.articles, a.impressions, a.history)
    T, Tb = 30, 40
    titles = rng.integers(1, V, (len(ids), T))
    titles[:, 20:] = 0  # title padding
    title_map = dict(zip(ids.tolist(), titles.tolist()))
    common = dict(behaviors=df, article_dict=title_map, history_column="article_id_fixed", unknown_representation="zeros", eval_mode=True,
                  batch_size=a.batch)
    if a.model == "lstur":
        class hp:
            title_size, history_size, n_users, cnn_activation, type = T, a.history, 50000, "relu", a.type
            attention_hidden_dim, gru_unit, filter_num, window_size = 200, 400, 400, 3
            optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-4

        loader = LSTURDataLoader(user_id_mapping={u: u + 1 for u in range(50000)}, **common)
        model = LSTURModel(hp, vocab_size=V, word_emb_dim=E, seed=1)
        with torch.no_grad():  # the user table is zeros at initialisation: give the "ini" GRU something to start from
            model._engine.user_table.uniform_(-0.1, 0.1)
    elif a.model == "npa":
        class hp:
            title_size, history_size, n_users, cnn_activation = T, a.history, 50000, "relu"
            attention_hidden_dim, user_emb_dim, filter_num, window_size = 200, 400, 400, 3
            optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-4

        loader = LSTURDataLoader(user_id_mapping={u: u + 1 for u in range(50000)}, **common)
        model = NPAModel(hp, vocab_size=V, word_emb_dim=E, seed=1)
        with torch.no_grad():  # zeros at initialisation: every user would carry the same two queries
            model._engine.user_table.uniform_(-0.5, 0.5)
    else:
        class hp:
            title_size, body_size, history_size = T, Tb, a.history
            vert_num, vert_emb_dim, subvert_num, subvert_emb_dim = 100, 10, 100, 10
            dense_activation, cnn_activation = "relu", "relu"
            attention_hidden_dim, filter_num, window_size = 200, 400, 3
            optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-4

        bodies = rng.integers(1, V, (len(ids), Tb))
        loader = NAMLDataLoader(body_mapping=dict(zip(ids.tolist(), bodies.tolist())),
                                category_mapping=dict(zip(ids.tolist(), rng.integers(0, 100, len(ids)).tolist())),
                                subcategory_mapping=dict(zip(ids.tolist(), rng.integers(0, 100, len(ids)).tolist())), **common)
        model = NAMLModel(hp, vocab_size=V, word_emb_dim=E, seed=1)
    return model, loader, hp, lens


class _Head:
    """the first `n` batches of a loader (warm-up)"""

    def __init__(self, loader, n):
        self._l, self._n = loader, min(n, len(loader))

    def __len__(self):
        return self._n

    def __getattr__(self, name):
        return getattr(self._l, name)

    def __getitem__(self, i):
        return self._l[i]


def timed_predict(model, loader, cache):
    model.scorer.cache_articles = cache
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.scorer.predict(loader)  # ends in the download of the last batch's scores: synchronised
    dt = time.perf_counter() - t0
    model.scorer.cache_articles = True
    return out, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, choices=["lstur", "naml", "npa"])
    ap.add_argument("--out", default=None, help="file the result line is appended to (npa: profiles/cached_scoring_npa_c1.jsonl)")
    ap.add_argument("--type", default="ini", choices=["ini", "con"])
    ap.add_argument("--articles", type=int, default=20_000)
    ap.add_argument("--impressions", type=int, default=100_000)
    ap.add_argument("--history", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    model, loader, hp, lens = build(a)
    if a.model == "naml":
        loader.article_catalogue()  # the loader's one-off host work: not part of a predict
    t_loader = time.perf_counter() - t0
    eng = model._engine
    n_imp, n_cand = len(lens), int(lens.sum())

    head = _Head(loader, 2)
    for cache in (True, False):  # warm-up: allocator, kernel loading
        timed_predict(model, head, cache)
    rounds = {"cached": [], "per_batch": []}
    scores = {}
    for _ in range(a.reps):  # interleaved rounds in one process
        for name, cache in (("cached", True), ("per_batch", False)):
            scores[name], dt = timed_predict(model, loader, cache)
            rounds[name].append(dt)
    diff = float(np.abs(scores["cached"] - scores["per_batch"]).max())
    best = {k: min(v) for k, v in rounds.items()}

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache = model._build_article_cache(loader)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0

    S, P = _hip.stream_handle, _hip.ptr
    copy_gbs = float4_copy_gbs(10)
    F = hp.filter_num
    if a.model == "naml":  # kernel (b) over the whole loader in one launch
        his = torch.from_numpy(np.ascontiguousarray(loader._his_cidx)).cuda()
        cand = torch.from_numpy(np.ascontiguousarray(loader._inv_cidx)).cuda()
        off = torch.from_numpy(np.ascontiguousarray(loader._inv_off, dtype=np.int64)).cuda()
        out = torch.empty(n_cand, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        fn = lambda: _hip.call("ebn_indexed_attpool_score_f32", P(cache.news_all), P(cache.a_all), cache.n_rows, P(his), P(cand), P(off),
                               n_cand, P(out), None, P(flag), n_imp, a.history, F, 1, S())
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = sorted(events_ms(fn, 10) for _ in range(3))[1]
        row_bytes = (n_imp * a.history + n_cand) * F * 4
        kernel = {"kernel": "ebn_indexed_attpool_score_f32", "impressions": n_imp, "rows_read": n_imp * a.history + n_cand,
                  "ms": round(ms, 4), "row_read_gbs": round(row_bytes / ms / 1e6, 1),
                  "row_read_of_float4_copy": round(row_bytes / ms / 1e6 / copy_gbs, 4),
                  "catalogue_mb": round(cache.n_rows * F * 4 / 1e6, 1)}
    elif a.model == "npa":  # the candidate leg (pooling + score, nothing written but the scores) over the whole loader in one launch
        T, A = hp.title_size, hp.attention_hidden_dim
        parts, base = [], 0
        for i in range(len(loader)):
            user, _h, cand_idx, rows, _y = loader.user_index_eval_batch(i)
            parts.append((np.asarray(cand_idx).reshape(-1), np.asarray(rows).reshape(-1) + base))
            base += len(user)
        cand = torch.from_numpy(np.concatenate([c for c, _ in parts]).astype(np.int32)).cuda()
        imp = torch.from_numpy(np.concatenate([r for _, r in parts]).astype(np.int32)).cuda()
        assert base == n_imp and cand.numel() == n_cand
        Q = torch.empty(n_imp, A, device="cuda").uniform_(-1, 1)
        users = torch.empty(n_imp, F, device="cuda").uniform_(-0.05, 0.05)
        out = torch.empty(n_cand, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        fn = lambda: _hip.call("ebn_pap_indexed_f32", P(cache.Ua_all), P(cache.Vd_all), cache.n_rows, P(cand), P(Q), P(imp), n_imp, None,
                               P(users), P(out), 1, P(flag), n_cand, T, F, A, S())
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        ms = sorted(events_ms(fn, 5) for _ in range(3))[1]
        must_read = n_cand * T * (F + A) * 4
        kernel = {"kernel": "ebn_pap_indexed_f32", "sequences": n_cand, "bytes_per_pair": T * (F + A) * 4, "ms": round(ms, 4),
                  "catalogue_read_gbs": round(must_read / ms / 1e6, 1),
                  "catalogue_read_of_float4_copy": round(must_read / ms / 1e6 / copy_gbs, 4),
                  "catalogue_bytes": eng.catalogue_bytes(cache.n_rows), "catalogue_mb": round(eng.catalogue_bytes(cache.n_rows) / 1e6, 1)}
    else:  # the indexed GRU of one full batch
        user, his_idx, _c, _r, _y = loader.user_index_eval_batch(0)
        B, U = len(user), hp.gru_unit
        hi = torch.from_numpy(np.ascontiguousarray(his_idx, dtype=np.int32).reshape(-1)).cuda()
        hw, ho = torch.empty(B, U, device="cuda"), torch.empty(B, U, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        fn = lambda: _hip.call("ebn_gru_infer_indexed_f32", P(cache.gx_all), P(cache.live), cache.n_rows, P(hi), P(eng.params.view("gru_r")),
                               P(eng.params.view("gru_b")), None, P(hw), P(ho), B, a.history, U, P(flag), S())
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = sorted(events_ms(fn, 10) for _ in range(3))[1]
        kernel = {"kernel": "ebn_gru_infer_indexed_f32", "B": B, "launches": a.history, "ms_per_batch": round(ms, 4),
                  "us_per_launch": round(ms * 1e3 / a.history, 2), "row_read_gbs": "not applicable"}

    res = {"what": "cached_scoring_probe", "model": a.model, "config": f"{a.model}-c1" + (f"-{a.type}" if a.model == "lstur" else ""),
           "device": torch.cuda.get_device_name(0), "articles": a.articles, "catalogue_rows": int(cache.n_rows), "impressions": n_imp,
           "candidates": n_cand, "mean_inview": round(n_cand / n_imp, 2), "share_250_long": 0.002, "H": a.history, "batch": a.batch,
           "batches": len(loader), "reps": a.reps, "loader_build_s": round(t_loader, 2),
           "cached_s": [round(v, 3) for v in rounds["cached"]], "per_batch_s": [round(v, 3) for v in rounds["per_batch"]],
           "cached_impressions_per_s": round(n_imp / best["cached"], 1), "per_batch_impressions_per_s": round(n_imp / best["per_batch"], 1),
           "speedup": round(best["per_batch"] / best["cached"], 2), "catalogue_build_s": round(t_build, 4),
           "max_abs_diff_cached_vs_per_batch": diff, "float4_copy_gbs": round(copy_gbs, 1), "hot_kernel": kernel}
    if a.model == "npa":
        res["cached_is_faster"] = bool(best["cached"] < best["per_batch"])
    print(json.dumps(res))
    out_path = a.out or (str(ROOT / "profiles" / "cached_scoring_npa_c1.jsonl") if a.model == "npa" else None)
    if out_path:
        with open(out_path, "a") as fh:
            fh.write(json.dumps(res) + "\n")
    assert diff <= 2e-6, f"cached and per-batch scores differ by {diff:.3e}"
    if a.model != "npa":
        assert best["per_batch"] / best["cached"] > 1.04, "the cached path is not faster than the per-batch path beyond the 4 % spread"


if __name__ == "__main__":
    main()
