"""Times one Fastformer training step at the ff-c1 or the ff-bert shape on one GPU, and the same step of the float32 torch oracle.

ff-c1: 32000 x 300 trainable word table, hidden 256, 16 heads, 2 layers, intermediate 256, dropout 0.2, T = 30 tokens, H = 20
history slots, 32 impressions x 5 candidates = 160 (history, candidate) pairs per step, torch.optim.Adam.  The history is repeated
per candidate, as the reference's dataset does.  ff-bert: hidden 768, 12 heads, everything else as ff-c1 (a shape only the
streamed attention pair takes: --attention streamed or auto).  A step is forward + BCELoss + backward + optimizer step, eager (no graph), timed
between two HIP events after warm-up.  Static FLOP count of the GEMMs of a step (R = 160 * 21 * 30 token rows; forward, data and
weight gradient each 2 R K N): 3 * 2 R (E D + layers (5 D D + 2 D I) + D D) with the pooler's att_fc1 as the last term.
The oracle (tests/fastformer_oracle.py, float32, autograd, torch's own dropout-free arithmetic with the same masks multiplied in)
runs eagerly on the same GPU with the same optimizer.  Prints ONE JSON line.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/fastformer_probe.py --steps 10 --no-oracle`.
usage: fastformer_probe.py [--config ff-c1|ff-bert] [--attention resident|streamed|auto] [--steps K] [--warmup W] [--no-oracle]"""
import argparse
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "ebnerd-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from ebrec import _hip  # noqa: E402

PEAK_TFLOPS = 157.3  # exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) peak of the MI355X
CONFIGS = {"ff-c1": (256, 16), "ff-bert": (768, 12)}  # hidden size, heads


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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="ff-c1")
    ap.add_argument("--attention", choices=("resident", "streamed", "auto"), default="resident")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from ebrec.models.fastformer import Fastformer
    from tests import fastformer_oracle as fo

    V, E, layers, I, T, H, B, C, p = 32000, 300, 2, 256, 30, 20, 32, 5, 0.2
    D, heads = CONFIGS[a.config]
    cfg = SimpleNamespace(hidden_size=D, num_attention_heads=heads, num_hidden_layers=layers, intermediate_size=I, max_position_embeddings=512,
                          hidden_dropout_prob=p, layer_norm_eps=1e-12, initializer_range=0.02, hidden_act="gelu", pooler_type="weightpooler",
                          vocab_size=V)
    torch.manual_seed(0)
    model = Fastformer(cfg, word_embedding=torch.nn.Embedding(V, E), seed=1, attention=a.attention).cuda().train()
    rng = np.random.default_rng(0)
    N = B * C
    batches = []
    for _ in range(4):
        hist = rng.integers(1, V, (B, H, T))
        hist[:, :, 20:] = 0  # title padding
        for b in range(B):  # histories of different lengths, left-padded; slot 0 stays real so that first_slot keeps the user
            hist[b, 1:1 + rng.integers(0, H // 2)] = 0
        hist = np.repeat(hist, C, axis=0)
        cand = rng.integers(1, V, (N, 1, T))
        cand[:, :, 22:] = 0
        y = np.zeros((B, C), np.float32)
        y[np.arange(B), rng.integers(0, C, B)] = 1
        batches.append(tuple(torch.as_tensor(x).cuda() for x in (hist.astype(np.int32), cand.astype(np.int32), y.reshape(N, 1))))
    crit = torch.nn.BCELoss()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    state = {"i": 0, "loss": None}

    def step():
        hist, cand, y = batches[state["i"] % 4]
        state["i"] += 1
        opt.zero_grad()
        loss = crit(model(hist, cand), y)
        loss.backward()
        opt.step()
        state["loss"] = loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    n0 = int(_hip.lib().ebn_launch_count())
    step()
    launches = int(_hip.lib().ebn_launch_count()) - n0
    ms = events_ms(step, a.steps)
    loss = float(state["loss"].item())

    oracle_ms = None
    if not a.no_oracle:
        Pt = {n: t.detach().clone().requires_grad_(True) for n, t in model.state_dict().items()}
        oopt = torch.optim.Adam(list(Pt.values()), lr=1e-4)
        keep = 1.0 - p
        masks = [torch.bernoulli(torch.full((N * (H + 1), T, D), keep, device="cuda")) / keep for _ in range(1 + 2 * layers)]
        drop_mult, fo.drop_mult = fo.drop_mult, (lambda shape, seed, step_, site, p_, dt, dev: masks[site])  # masks as given tensors
        ostate = {"i": 0}

        def ostep():
            hist, cand, y = batches[ostate["i"] % 4]
            ostate["i"] += 1
            oopt.zero_grad()
            crit(fo.forward(Pt, hist, cand, heads, 1e-12, "first_slot", drop=(p, 0, 0)), y).backward()
            oopt.step()

        try:
            for _ in range(max(2, a.warmup // 2)):
                ostep()
            oracle_ms = events_ms(ostep, max(3, a.steps // 2))
        finally:
            fo.drop_mult = drop_mult

    R = N * (H + 1) * T
    flop = 3 * 2 * R * (E * D + layers * (5 * D * D + 2 * D * I) + D * D)
    out = {"what": "fastformer_probe", "config": a.config, "attention": model._engine.attention_kind(T, True), "device": torch.cuda.get_device_name(0), "pairs": N, "H": H, "T": T, "V": V, "E": E,
           "hidden": D, "heads": heads, "layers": layers, "intermediate": I, "dropout": p, "optimizer": "torch.optim.Adam", "steps": a.steps,
           "warmup": a.warmup, "ms_per_step": round(ms, 4), "pairs_per_s": round(N / ms * 1e3, 1), "gemm_gflop_per_step": round(flop / 1e9, 2),
           "gemm_tflops_over_step": round(flop / ms / 1e9, 2), "fraction_of_fp32_peak": round(flop / ms / 1e9 / PEAK_TFLOPS, 4),
           "launches_per_step": launches, "loss": loss,
           "torch_oracle_eager_ms_per_step": None if oracle_ms is None else round(oracle_ms, 4)}
    line = json.dumps(out)
    assert len(line) <= 4096
    print(line)


if __name__ == "__main__":
    main()
