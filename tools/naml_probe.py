"""Times one NAML training step at the naml-c1 shape on one GPU.

naml-c1: 32000 x 300 trainable word table, B = 32, H = 20, C = 5, title 30, body 40, filter_num 400, window 3,
attention_hidden_dim 200, vert / subvert tables 100 x 10.  The step is NAMLModel's captured hipGraph (warm-up replays first, then
back-to-back timed steps between two HIP events).  Static FLOP count of a step (N = B (H + C) articles, R = N (T + Tb) tokens):
  3 . 2 R (window E) F   (both Conv1D forwards, backward-data, backward-weight)
+ 3 . 2 R F A            (both AttLayer2's Vd.Wa and their two gradient products)
+ 3 . 2 (4 N) F A        (the view attention's x.W and its two gradient products)
+ 3 . 2 B H F A          (the user AttLayer2's x.W and its two gradient products)
+ 3 . 2 N (Kv + Ks) F    (the two categorical Dense layers, forward and two gradient products)
Prints ONE JSON line.  Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python
tools/naml_probe.py --steps 20`.
usage: naml_probe.py [--steps K] [--warmup W]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec import _hip  # noqa: E402

PEAK_TFLOPS = 157.3  # exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) peak of the MI355X


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from ebrec.models.newsrec import NAMLModel, hparams_naml

    hp = hparams_naml
    V, E, B, H, C, T, Tb = 32000, 300, 32, hp.history_size, 5, hp.title_size, hp.body_size
    F, A, W, Kv, Ks = hp.filter_num, hp.attention_hidden_dim, hp.window_size, hp.vert_emb_dim, hp.subvert_emb_dim
    rng = np.random.default_rng(0)
    model = NAMLModel(hp, vocab_size=V, word_emb_dim=E, seed=1)
    batches = []
    for _ in range(4):
        ht, hb = rng.integers(1, V, (B, H, T)), rng.integers(1, V, (B, H, Tb))
        ht[:, :, 20:] = 0  # title and body padding
        hb[:, :, 30:] = 0
        for b in range(B):  # histories of different lengths: left-padded, as the loader writes them
            n_pad = rng.integers(0, H // 2)
            ht[b, :n_pad], hb[b, :n_pad] = 0, 0
        cats = lambda n, s: rng.integers(0, n, s + (1,))
        y = np.zeros((B, C), np.int8)
        y[np.arange(B), rng.integers(0, C, B)] = 1
        batches.append((ht, hb, cats(hp.vert_num, (B, H)), cats(hp.subvert_num, (B, H)), rng.integers(1, V, (B, C, T)),
                        rng.integers(1, V, (B, C, Tb)), cats(hp.vert_num, (B, C)), cats(hp.subvert_num, (B, C)), y))
    eng = model._engine
    for i in range(a.warmup):
        eng.train_step(*batches[i % 4])
    torch.cuda.synchronize()
    n0 = int(_hip.lib().ebn_launch_count())
    eng.use_graph = False
    eng.train_step(*batches[0])  # one eager step: the library's launches per step
    eng.use_graph = True
    launches = int(_hip.lib().ebn_launch_count()) - n0
    torch.cuda.synchronize()
    # the timed loop replays the captured step on staged batches (host staging of fresh arrays is not part of the GPU time)
    g = eng._graphs[(B, C, eng.loss_kind, eng.train_embedding, eng.fuse_user_head)]
    t0 = time.perf_counter()
    ms = events_ms(g.replay, a.steps)
    wall = (time.perf_counter() - t0) / a.steps * 1e3
    loss = float(eng.loss_dev.item())
    eng.check_oob()

    N = B * (H + C)
    R = N * (T + Tb)
    flop = (3 * 2 * R * (W * E) * F + 3 * 2 * R * F * A + 3 * 2 * 4 * N * F * A + 3 * 2 * B * H * F * A
            + 3 * 2 * N * (Kv + Ks) * F)
    out = {"what": "naml_probe", "config": "naml-c1", "device": torch.cuda.get_device_name(0), "B": B, "H": H, "C": C, "T": T,
           "body": Tb, "V": V, "E": E, "F": F, "A": A, "window": W, "vert": [hp.vert_num, Kv], "subvert": [hp.subvert_num, Ks],
           "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 4), "host_wall_ms_per_step": round(wall, 4),
           "impressions_per_s": round(B / ms * 1e3, 1), "step_gflop": round(flop / 1e9, 3),
           "step_tflops": round(flop / ms / 1e9, 2), "fraction_of_fp32_peak": round(flop / ms / 1e9 / PEAK_TFLOPS, 4),
           "launches_per_step": launches, "loss": loss}
    line = json.dumps(out)
    assert len(line) <= 4096
    print(line)


if __name__ == "__main__":
    main()
