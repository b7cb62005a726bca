"""Writes tests/golden/fastformer_ref_long.npz from the REFERENCE's own Fastformer class (data only; run on a machine that has the
reference checkout and `transformers`):  python tests/golden/make_fastformer_long_golden.py <reference checkout>

Titles of T = 500 tokens at hidden 24 / 4 heads / 2 layers, N = 3 samples of H = 2 history slots: beyond what the resident
attention pair takes (its forward stops at T = 492 there), so this pins the streamed pair to the reference where nothing else does.
As make_fastformer_golden.py: the float32 state_dict, inputs, labels; from the reference run in float64 the scores, BCELoss and
every parameter gradient; the float32 run's scores and loss; and the reference-float32 error measures E_fwd (scores, absolute) and
E_ref (gradients, as tests/fastformer_oracle.measure).  No trajectory; the file stays under 300 kB."""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
CFG = dict(hidden_size=24, num_attention_heads=4, num_hidden_layers=2, intermediate_size=40, max_position_embeddings=8,
           hidden_dropout_prob=0.0, layer_norm_eps=1e-12, initializer_range=0.3, hidden_act="gelu", pooler_type="weightpooler",
           vocab_size=40)
WORD_DIM, N, H, T = 20, 3, 2, 500


def inputs():
    rng = np.random.default_rng(17)
    hist = rng.integers(1, CFG["vocab_size"], (N, H, T))
    cand = rng.integers(1, CFG["vocab_size"], (N, 1, T))
    for n in range(N):
        for h in range(H):
            hist[n, h, rng.integers(300, T + 1):] = 0  # titles padded at the tail
        cand[n, 0, rng.integers(300, T + 1):] = 0
    hist[0, 0, 70:] = 0     # a slot-0 title shorter than the others: first_slot masks the tail of every slot of sample 0
    hist[2, 1] = 0          # a later all-padding slot
    cand[1, 0, 499] = 7     # a live last token
    y = np.array([[1.0], [0.0], [1.0]], np.float32)
    return hist, cand, y


def main(ref_root):
    sys.path[:0] = [str(Path(ref_root) / "src" / "ebrec"), str(Path(ref_root) / "src")]
    from transformers import BertConfig
    from models.fastformer.fastformer import Fastformer

    torch.manual_seed(23)
    cfg = BertConfig(**CFG)
    model = Fastformer(cfg, word_embedding=torch.nn.Embedding(CFG["vocab_size"], WORD_DIM))
    with torch.no_grad():  # off their trivial initial values, so that every gradient path carries signal
        for name, p in model.named_parameters():
            if name.endswith("bias") or "LayerNorm.weight" in name:
                p.add_(torch.randn_like(p) * 0.2)
    model = model.float()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    hist, cand, y = inputs()
    th, tc, ty = torch.as_tensor(hist), torch.as_tensor(cand), torch.as_tensor(y)
    out = {"hist": hist.astype(np.int32), "cand": cand.astype(np.int32), "labels": y, "names": np.array(list(state))}
    out.update({"cfg_" + k: np.array(v) for k, v in CFG.items()})
    out["word_dim"] = np.array(WORD_DIM)
    runs = {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        model.load_state_dict(state)
        model = model.to(dt)
        model.train()
        model.zero_grad()
        score = model(th, tc)
        loss = torch.nn.BCELoss()(score, ty.to(dt))
        loss.backward()
        r = {"score": score.detach().numpy(), "loss": np.array(loss.item())}
        r.update({"grad." + k: p.grad.numpy().copy() for k, p in model.named_parameters()})
        runs[tag] = r
        model = model.float()
    names = list(state)
    G = max(np.abs(runs["f64"]["grad." + k]).max() for k in names)
    meas = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-4 * G))
    out["G"] = np.array(G)
    out["E_fwd"] = np.array(np.abs(runs["f32"]["score"].astype(np.float64) - runs["f64"]["score"]).max())
    per = {k: meas(runs["f32"]["grad." + k], runs["f64"]["grad." + k]) for k in names}
    out["E_ref"] = np.array(max(per.values()))
    for k in names:
        out["param." + k] = state[k].numpy()
    for k, v in runs["f64"].items():
        out["f64." + k] = v
    for k in ("score", "loss"):
        out["f32." + k] = runs["f32"][k]
    path = HERE / "fastformer_ref_long.npz"
    np.savez_compressed(path, **out)
    worst = sorted(per.items(), key=lambda kv: -kv[1])[:4]
    print(f"{path.name}: {path.stat().st_size} bytes, {sum(v.numel() for v in state.values())} parameters, G = {G:.4g}, "
          f"E_fwd = {float(out['E_fwd']):.3g}, E_ref = {float(out['E_ref']):.3g}")
    print("largest reference-float32 gradient measures:", worst)


if __name__ == "__main__":
    main(sys.argv[1])
