"""Times one Fastformer_wu training step at the wu-c1 or the wu-bert shape on one GPU, and the same step of the float32 torch oracle.

wu-c1: 32000 x 300 trainable word table, hidden 256, 16 heads, 2 layers, intermediate 256, dropout 0.2, N = 64 texts of T = 256
tokens (tail-padded to different lengths), torch.optim.Adam.  wu-bert: hidden 768, 12 heads, intermediate 768, N = 16, T = 512,
everything else as wu-c1.  Both are past the resident attention pair: attention="auto" (the default) runs the streamed one.  A step
is forward (loss and logits) + backward + optimizer step, eager (no graph), timed between two HIP events after warm-up.  Static FLOP
count of the GEMMs of a step (R = N * T token rows; forward, data and weight gradient each 2 R K N):
3 * 2 R (E D + layers (5 D D + 2 D I) + D D) with the pooler's att_fc1 as the last term.  The oracle (tests/fastformer_wu_oracle.py,
float32, autograd, the same number of dropout masks multiplied in) runs eagerly on the same GPU with the same optimizer.  Prints ONE
JSON line and appends it to --out (default profiles/fastformer_wu_probe.jsonl).  There is no pass / fail threshold on a time.
usage: fastformer_wu_probe.py [--config wu-c1|wu-bert] [--attention resident|streamed|auto] [--steps K] [--warmup W] [--no-oracle] [--out FILE]"""
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
CONFIGS = {"wu-c1": (256, 16, 64, 256), "wu-bert": (768, 12, 16, 512)}  # hidden size (= intermediate), heads, N, T


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
    ap.add_argument("--config", choices=sorted(CONFIGS), default="wu-c1")
    ap.add_argument("--attention", choices=("resident", "streamed", "auto"), default="auto")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fastformer_wu_probe.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from ebrec.models.fastformer import Fastformer_wu
    from tests import fastformer_wu_oracle as fw

    V, E, layers, p = 32000, 300, 2, 0.2
    D, heads, N, T = CONFIGS[a.config]
    I = D
    cfg = SimpleNamespace(hidden_size=D, num_attention_heads=heads, num_hidden_layers=layers, intermediate_size=I, max_position_embeddings=512,
                          hidden_dropout_prob=p, layer_norm_eps=1e-12, initializer_range=0.02, hidden_act="gelu", pooler_type="weightpooler",
                          vocab_size=V)
    torch.manual_seed(0)
    model = Fastformer_wu(cfg, torch.nn.Embedding(V, E), seed=1, attention=a.attention).cuda().train()
    rng = np.random.default_rng(0)
    batches = []
    for _ in range(4):
        ids = rng.integers(1, V, (N, T))
        for n in range(N):
            ids[n, rng.integers(T // 2, T + 1):] = 0  # texts of different lengths, padded at the tail
        batches.append((torch.as_tensor(ids.astype(np.int32)).cuda(), torch.as_tensor(rng.integers(0, 4, N)).cuda()))
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    state = {"i": 0, "loss": None}

    def step():
        ids, y = batches[state["i"] % 4]
        state["i"] += 1
        opt.zero_grad()
        loss, _ = model(ids, y)
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
        masks = [torch.bernoulli(torch.full((N, T, D), keep, device="cuda")) / keep for _ in range(1 + 2 * layers)]
        drop_mult, fw.drop_mult = fw.drop_mult, (lambda shape, seed, step_, site, p_, dt, dev: masks[site])  # masks as given tensors
        ostate = {"i": 0}

        def ostep():
            ids, y = batches[ostate["i"] % 4]
            ostate["i"] += 1
            oopt.zero_grad()
            fw.forward(Pt, ids, y, heads, 1e-12, drop=(p, 0, 0))[0].backward()
            oopt.step()

        try:
            for _ in range(max(2, a.warmup // 2)):
                ostep()
            oracle_ms = events_ms(ostep, max(3, a.steps // 2))
        finally:
            fw.drop_mult = drop_mult

    R = N * T
    flop = 3 * 2 * R * (E * D + layers * (5 * D * D + 2 * D * I) + D * D)
    out = {"what": "fastformer_wu_probe", "config": a.config, "attention": model.fastformer_model._engine.attention_kind(T, True),
           "device": torch.cuda.get_device_name(0), "N": N, "T": T, "V": V, "E": E, "hidden": D, "heads": heads, "layers": layers, "intermediate": I,
           "dropout": p, "optimizer": "torch.optim.Adam", "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 4),
           "texts_per_s": round(N / ms * 1e3, 1), "tokens_per_s": round(R / ms * 1e3, 1), "gemm_gflop_per_step": round(flop / 1e9, 2),
           "gemm_tflops_over_step": round(flop / ms / 1e9, 2), "fraction_of_fp32_peak": round(flop / ms / 1e9 / PEAK_TFLOPS, 4),
           "launches_per_step": launches, "loss": loss,
           "torch_oracle_eager_ms_per_step": None if oracle_ms is None else round(oracle_ms, 4)}
    line = json.dumps(out)
    assert len(line) <= 4096
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
