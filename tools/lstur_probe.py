"""Times one LSTUR training step at the lstur-c1 shape on one GPU, and the GRU recurrence launches inside it.

lstur-c1: 32000 x 300 trainable word table, n_users = 50000, B = 32, H = 20 (--history 50 for the long-history variant), C = 5,
T = 30, filter_num = gru_unit = 400, window 3, attention_hidden_dim 200, type "ini".  The step is LSTURModel's captured hipGraph
(warm-up replays first, then back-to-back timed steps between two HIP events).  The GRU forward (H launches) and backward
(H + 1 launches) are then timed on their own, replayed on the step's buffers.  Static FLOP count of a step (R = B (H + C) T):
  3 . 2 R (window E) F   (Conv1D forward, backward-data, backward-weight)
+ 3 . 2 R F A            (AttLayer2's Vd.Wa and its two gradient products)
+ 3 . 2 B H F 3U + 3 . 2 B H U 3U   (the GRU's input and recurrent products, forward and two gradient products each)
Prints ONE JSON line.  Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python
tools/lstur_probe.py --steps 20`.
usage: lstur_probe.py [--steps K] [--warmup W] [--reps N] [--history H] [--type ini|con]"""
import argparse
import ctypes
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--history", type=int, default=20)
    ap.add_argument("--type", default="ini", choices=["ini", "con"])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from ebrec.models.newsrec import LSTURModel

    class hp:
        title_size, history_size, n_users, cnn_activation, type = 30, a.history, 50000, "relu", a.type
        attention_hidden_dim, gru_unit, filter_num, window_size = 200, 400, 400, 3
        optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-4

    V, E, B, H, C, T = 32000, 300, 32, hp.history_size, 5, hp.title_size
    F, A, W, U = hp.filter_num, hp.attention_hidden_dim, hp.window_size, hp.gru_unit
    rng = np.random.default_rng(0)
    model = LSTURModel(hp, vocab_size=V, word_emb_dim=E, seed=1)
    batches = []
    for _ in range(4):
        his = rng.integers(1, V, (B, H, T))
        his[:, :, 20:] = 0  # title padding
        for b in range(B):  # histories of different lengths: left-padded, as the loader writes them
            his[b, : rng.integers(0, H // 2)] = 0
        y = np.zeros((B, C), np.int8)
        y[np.arange(B), rng.integers(0, C, B)] = 1
        batches.append((rng.integers(0, hp.n_users + 1, (B, 1)), his, rng.integers(1, V, (B, C, T)), y))
    eng = model._engine
    for i in range(a.warmup):
        eng.train_step(*batches[i % 4])
    torch.cuda.synchronize()
    # the timed loop replays the captured step on staged batches (host staging of fresh arrays is not part of the GPU time)
    g = eng._graphs[(B, C, False, eng.type, eng.loss_kind, eng.train_embedding)]
    t0 = time.perf_counter()
    ms = events_ms(g.replay, a.steps)
    wall = (time.perf_counter() - t0) / a.steps * 1e3
    loss = float(eng.loss_dev.item())
    eng.check_oob()

    # the recurrence on its own, on the step's buffers (its inputs are what the last replay left there)
    b = eng._bufs[(B, C)]
    Pv, S, P = eng.params.view, _hip.stream_handle, _hip.ptr
    his_nv = b.NV[: B * H]
    h0 = P(b.Eu) if eng.type == "ini" else None
    dhH = b.duser if eng.type == "ini" else b.dhH
    dh0 = torch.empty(B, U, device="cuda")
    fwd = lambda: _hip.call("ebn_gru_fwd_f32", P(b.gx), P(his_nv), P(Pv("gru_r")), P(Pv("gru_b")), h0, P(b.Hs), P(b.act), B, H, F,
                            U, S())
    bwd = lambda: _hip.call("ebn_gru_bwd_f32", P(dhH), P(his_nv), P(Pv("gru_r")), P(b.Hs), P(b.act), P(b.dgx), P(b.dgh), P(dh0), B,
                            H, F, U, S())
    for fn in (fwd, bwd):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t_fwd, t_bwd = [], []
    for _ in range(3):  # interleaved rounds in one process
        t_fwd.append(events_ms(fwd, a.reps))
        t_bwd.append(events_ms(bwd, a.reps))
    med = lambda v: sorted(v)[len(v) // 2]
    masked = float((~(his_nv.view(B, H, F) != 0).any(-1)).float().mean())

    R = B * (H + C) * T
    flop = 3 * 2 * R * (W * E) * F + 3 * 2 * R * F * A + 3 * 2 * B * H * F * 3 * U + 3 * 2 * B * H * U * 3 * U
    gru_ms = med(t_fwd) + med(t_bwd)
    out = {"what": "lstur_probe", "config": "lstur-c1" if H == 20 else f"lstur-c1-h{H}", "type": eng.type,
           "device": torch.cuda.get_device_name(0), "B": B, "H": H, "C": C, "T": T, "V": V, "E": E, "F": F, "U": U, "A": A,
           "window": W, "n_users": hp.n_users, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": round(ms, 4), "host_wall_ms_per_step": round(wall, 4), "impressions_per_s": round(B / ms * 1e3, 1),
           "step_gflop": round(flop / 1e9, 3), "step_tflops": round(flop / ms / 1e9, 2),
           "fraction_of_fp32_peak": round(flop / ms / 1e9 / PEAK_TFLOPS, 4), "loss": loss,
           "masked_history_steps": round(masked, 4),
           "gru": {"fwd_launches": H, "bwd_launches": H + 1, "fwd_ms": round(med(t_fwd), 4), "bwd_ms": round(med(t_bwd), 4),
                   "us_per_fwd_launch": round(med(t_fwd) * 1e3 / H, 2), "us_per_bwd_launch": round(med(t_bwd) * 1e3 / (H + 1), 2),
                   "share_of_step": round(gru_ms / ms, 4),
                   "rounds_ms": {"fwd": [round(v, 4) for v in t_fwd], "bwd": [round(v, 4) for v in t_bwd]}}}
    line = json.dumps(out)
    assert len(line) <= 4096
    print(line)


if __name__ == "__main__":
    main()
