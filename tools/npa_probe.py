"""Times one NPA training step at the npa-c1 shape on one GPU and A/Bs the forward Conv1D kernel against im2col + ebn_gemm_f32.

npa-c1: 32000 x 300 trainable word table, n_users = 50000, B = 32, H = 20, C = 5, T = 30, filter_num 400, window 3,
attention_hidden_dim 200, user_emb_dim 400.  The step is NPAModel's captured hipGraph (warm-up replays first, then
back-to-back timed steps between two HIP events).  Static FLOP count of a step (R = B (H + C) T token rows):
  3 . 2 R (window E) F   (Conv1D forward, backward-data, backward-weight)
+ 3 . 2 R F A            (the news pooling's Vd.Wa and its two gradient products)
+ 3 . 2 B H F A          (the same for the user pooling)
Prints ONE JSON line.  Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python
tools/npa_probe.py --steps 20`.
usage: npa_probe.py [--steps K] [--warmup W] [--reps N]"""
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


class hp:
    title_size, history_size, n_users, cnn_activation = 30, 20, 50000, "relu"
    attention_hidden_dim, user_emb_dim, filter_num, window_size = 200, 400, 400, 3
    optimizer, loss, dropout, learning_rate = "adam", "cross_entropy_loss", 0.2, 1e-4


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
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from ebrec.models.newsrec import NPAModel

    V, E, B, H, C, T = 32000, 300, 32, hp.history_size, 5, hp.title_size
    F, A, W = hp.filter_num, hp.attention_hidden_dim, hp.window_size
    rng = np.random.default_rng(0)
    model = NPAModel(hp, vocab_size=V, word_emb_dim=E, seed=1)
    batches = []
    for _ in range(4):
        y = np.zeros((B, C), np.int8)
        y[np.arange(B), rng.integers(0, C, B)] = 1
        batches.append((rng.integers(0, hp.n_users + 1, (B, 1)), rng.integers(0, V, (B, H, T)), rng.integers(0, V, (B, C, T)), y))
    eng = model._engine
    for i in range(a.warmup):
        eng.train_step(*batches[i % 4])
    torch.cuda.synchronize()
    # the timed loop replays the captured step on staged batches (host staging of fresh arrays is not part of the GPU time)
    g = eng._graphs[(B, C, False, eng.loss_kind, eng.train_embedding)]
    t0 = time.perf_counter()
    ms = events_ms(g.replay, a.steps)
    wall = (time.perf_counter() - t0) / a.steps * 1e3
    loss = float(eng.loss_dev.item())
    eng.check_oob()

    R = B * (H + C) * T
    flop = 3 * 2 * R * (W * E) * F + 3 * 2 * R * F * A + 3 * 2 * B * H * F * A
    # A/B: the forward Conv1D kernel vs im2col (a test-side gather into (R, window*E)) + ebn_gemm_f32 on the same data
    b = eng._bufs[(B, C)]
    X = torch.randn(R, E, device="cuda")
    Wb = eng.params.view("conv_Wb")
    Vd = torch.empty(R, F, device="cuda")
    N = B * (H + C)
    S, P = _hip.stream_handle, _hip.ptr
    conv = lambda: _hip.call("ebn_conv1d_fwd_f32", P(X), P(Wb), P(Wb[W * E]), P(Vd), N, T, E, F, W, None, -1, ctypes.c_float(0.0), -1,
                             ctypes.c_float(0.0), S())
    Xp = torch.nn.functional.pad(X.view(N, T, E), (0, 0, (W - 1) // 2, W - 1 - (W - 1) // 2))
    cols = torch.empty(N, T, W * E, device="cuda")
    im2col = lambda: torch.cat([Xp[:, j:j + T] for j in range(W)], -1, out=cols)
    Y = torch.empty(R, F, device="cuda")
    gemm = lambda: _hip.call("ebn_gemm_f32", 0, 0, R, F, W * E, ctypes.c_float(1.0), P(cols), W * E, P(Wb), F, ctypes.c_float(0.0),
                             P(Y), F, S())
    for fn in (conv, im2col, gemm):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t_conv, t_gemm, t_both = [], [], []
    for _ in range(3):  # interleaved rounds in one process
        t_conv.append(events_ms(conv, a.reps))
        t_gemm.append(events_ms(gemm, a.reps))
        t_both.append(events_ms(lambda: (im2col(), gemm()), a.reps))
    im2col()
    gemm()
    conv()
    torch.cuda.synchronize()
    relu_y = torch.relu(Y + Wb[W * E])
    err = float((relu_y - Vd).abs().max())
    conv_flop = 2 * R * (W * E) * F
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"what": "npa_probe", "config": "npa-c1", "device": torch.cuda.get_device_name(0), "B": B, "H": H, "C": C, "T": T,
           "V": V, "E": E, "F": F, "A": A, "window": W, "n_users": hp.n_users, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": round(ms, 4), "host_wall_ms_per_step": round(wall, 4), "impressions_per_s": round(B / ms * 1e3, 1),
           "step_gflop": round(flop / 1e9, 3), "step_tflops": round(flop / ms / 1e9, 2),
           "fraction_of_fp32_peak": round(flop / ms / 1e9 / PEAK_TFLOPS, 4), "loss": loss,
           "conv_fwd_ab": {"gflop": round(conv_flop / 1e9, 3), "conv1d_kernel_ms": round(med(t_conv), 4),
                           "gemm_only_ms": round(med(t_gemm), 4), "im2col_plus_gemm_ms": round(med(t_both), 4),
                           "conv1d_kernel_tflops": round(conv_flop / med(t_conv) / 1e9, 2),
                           "gemm_only_tflops": round(conv_flop / med(t_gemm) / 1e9, 2),
                           "rounds_ms": {"conv": [round(v, 4) for v in t_conv], "gemm": [round(v, 4) for v in t_gemm],
                                         "im2col_gemm": [round(v, 4) for v in t_both]},
                           "max_abs_diff_vs_im2col_gemm": err}}
    line = json.dumps(out)
    assert len(line) <= 4096
    print(line)


if __name__ == "__main__":
    main()
