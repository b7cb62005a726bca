"""Writes tests/golden/fastformer_wu_ref_small.npz and fastformer_wu_ref_traj.npz (the float64 weights after 3 SGD steps) from the
REFERENCE's own Fastformer_wu class (data only; run on a machine that has the reference checkout and `transformers`):
    python tests/golden/make_fastformer_wu_golden.py <reference checkout>

The small model of make_fastformer_golden.py (word dim != hidden size, 2 layers, 4 heads, initializer_range 0.3, dropout 0) with a
position table of 16 rows and sequences of 13 tokens, so that rows 13..15 of the table must get zero gradient: the float32
state_dict (biases and LayerNorm weights nudged off their trivial initial values), input ids and targets, and from the reference
run in float64: score (the [N, 4] logits), the CrossEntropyLoss, every parameter gradient; score and loss of the same run in
float32; the weights after 3 steps of SGD(lr = 0.1) in float64 (the _traj file); and the reference-float32 error measures E_fwd
(logits, relative to max|logit64|), E_ref (gradients) and E_traj (weights after 3 steps), measured as
tests/fastformer_oracle.measure does."""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
CFG = dict(hidden_size=24, num_attention_heads=4, num_hidden_layers=2, intermediate_size=40, max_position_embeddings=16,
           hidden_dropout_prob=0.0, layer_norm_eps=1e-12, initializer_range=0.3, hidden_act="gelu", pooler_type="weightpooler",
           vocab_size=40)
WORD_DIM, N, T = 20, 7, 13


def inputs():
    rng = np.random.default_rng(17)
    ids = rng.integers(1, CFG["vocab_size"], (N, T))
    for n, length in enumerate((13, 9, 4, 11, 0, 1, 7)):  # tail-padded sequences of different lengths; sample 4 is all padding
        ids[n, length:] = 0
    targets = np.array([0, 1, 2, 3, 1, 3, 0], np.int64)  # all four classes
    return ids, targets


def main(ref_root):
    sys.path[:0] = [str(Path(ref_root) / "src" / "ebrec"), str(Path(ref_root) / "src")]
    from transformers import BertConfig
    from models.fastformer.fastformer_wu import Fastformer_wu

    torch.manual_seed(23)
    cfg = BertConfig(**CFG)
    model = Fastformer_wu(cfg, word_embedding=torch.nn.Embedding(CFG["vocab_size"], WORD_DIM))
    with torch.no_grad():  # off their trivial initial values, so that every gradient path carries signal
        for name, p in model.named_parameters():
            if name.endswith("bias") or "LayerNorm.weight" in name:
                p.add_(torch.randn_like(p) * 0.2)
    model = model.float()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ids, targets = inputs()
    ti, tt = torch.as_tensor(ids), torch.as_tensor(targets)
    out = {"ids": ids.astype(np.int32), "targets": targets, "names": np.array(list(state))}
    out.update({"cfg_" + k: np.array(v) for k, v in CFG.items()})
    out["word_dim"] = np.array(WORD_DIM)
    runs = {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        model.load_state_dict(state)
        model = model.to(dt)
        model.train()
        model.zero_grad()
        loss, score = model(ti, tt)
        loss.backward()
        r = {"score": score.detach().numpy(), "loss": np.array(loss.item())}
        r.update({"grad." + k: p.grad.numpy().copy() for k, p in model.named_parameters()})
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        for _ in range(3):
            opt.zero_grad()
            model(ti, tt)[0].backward()
            opt.step()
        r.update({"traj." + k: v.detach().numpy().copy() for k, v in model.state_dict().items()})
        runs[tag] = r
        model = model.float()
    names = list(state)
    G = max(np.abs(runs["f64"]["grad." + k]).max() for k in names)
    meas = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-4 * G))
    out["G"] = np.array(G)
    s64 = runs["f64"]["score"]
    out["E_fwd"] = np.array(np.abs(runs["f32"]["score"].astype(np.float64) - s64).max() / np.abs(s64).max())
    per = {k: meas(runs["f32"]["grad." + k], runs["f64"]["grad." + k]) for k in names}
    out["E_ref"] = np.array(max(per.values()))
    out["E_traj"] = np.array(max(meas(runs["f32"]["traj." + k], runs["f64"]["traj." + k]) for k in names))
    for k in names:
        out["param." + k] = state[k].numpy()
    traj = {}
    for k, v in runs["f64"].items():
        (traj if k.startswith("traj.") else out)["f64." + k] = v
    for k in ("score", "loss"):  # the float32 run's gradients and trajectory are kept only as E_ref / E_traj (file size)
        out["f32." + k] = runs["f32"][k]
    path = HERE / "fastformer_wu_ref_small.npz"
    np.savez_compressed(path, **out)
    np.savez_compressed(HERE / "fastformer_wu_ref_traj.npz", **traj)
    print("fastformer_wu_ref_traj.npz:", (HERE / "fastformer_wu_ref_traj.npz").stat().st_size, "bytes")
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:4]
    print(f"{path.name}: {path.stat().st_size} bytes, {len(names)} entries, {sum(v.numel() for v in state.values())} parameters, G = {G:.4g}, "
          f"E_fwd = {float(out['E_fwd']):.3g}, E_ref = {float(out['E_ref']):.3g}, E_traj = {float(out['E_traj']):.3g}")
    print("largest reference-float32 gradient measures:", worst)


if __name__ == "__main__":
    main(sys.argv[1])
