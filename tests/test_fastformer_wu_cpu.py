"""Fastformer_wu without a GPU: the float64 oracle (tests/fastformer_wu_oracle.py) pinned to what the REFERENCE's own Fastformer_wu
computed (tests/golden/fastformer_wu_ref_small.npz, written by tests/golden/make_fastformer_wu_golden.py), the modules' state_dict
surface, their argument checks and the light import."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import fastformer_oracle as fo
from tests import fastformer_wu_oracle as fw

GOLDEN = Path(__file__).resolve().parent / "golden"


def load_golden():
    z = np.load(GOLDEN / "fastformer_wu_ref_small.npz")
    names = [str(n) for n in z["names"]]
    cfg = SimpleNamespace(**{k[4:]: z[k].item() for k in z.files if k.startswith("cfg_")})
    return z, names, cfg


def make_model(cfg, word_dim, **kw):
    from ebrec.models.fastformer import Fastformer_wu

    return Fastformer_wu(cfg, torch.nn.Embedding(cfg.vocab_size, word_dim), **kw)


def test_oracle_reproduces_the_reference_in_float64():
    z, names, cfg = load_golden()
    P = {n: torch.tensor(z["param." + n], dtype=torch.float64, requires_grad=True) for n in names}
    ids, targets = torch.as_tensor(z["ids"]), torch.as_tensor(z["targets"])
    loss, score = fw.forward(P, ids, targets, cfg.num_attention_heads, cfg.layer_norm_eps)
    loss.backward()
    assert np.abs(score.detach().numpy() - z["f64.score"]).max() < 1e-9
    assert abs(loss.item() - z["f64.loss"].item()) < 1e-9
    G = z["G"].item()
    for n in names:
        g = P[n].grad.numpy() if P[n].grad is not None else np.zeros(P[n].shape)
        assert fo.measure(g, z["f64.grad." + n], G) < 1e-9, n
    # what the fixture's inputs exercise: every token its own position row, rows >= T never read; an all-padding sequence whose logits
    # are the head's bias; tail padding of different lengths; all four classes
    T = z["ids"].shape[1]
    dpos = z["f64.grad.fastformer_model.position_embeddings.weight"]
    assert T < cfg.max_position_embeddings and (dpos[T:] == 0).all() and all(np.abs(dpos[t]).max() > 0 for t in range(T))
    assert (z["ids"][4] == 0).all() and np.abs(z["f64.score"][4] - z["param.output_layer.bias"]).max() < 1e-6
    assert len({int((row != 0).sum()) for row in z["ids"]}) == len(z["ids"])
    assert sorted(set(z["targets"].tolist())) == [0, 1, 2, 3]


def test_state_dict_has_the_reference_names_and_loads_strictly():
    z, names, cfg = load_golden()
    model = make_model(cfg, z["word_dim"].item())
    sd = model.state_dict()
    assert len(names) == 52 and list(sd) == names
    for n in names:
        assert tuple(sd[n].shape) == z["param." + n].shape, n
    model.load_state_dict({n: torch.as_tensor(z["param." + n]) for n in names}, strict=True)
    assert np.array_equal(model.state_dict()[names[7]].numpy(), z["param." + names[7]])
    fresh = make_model(cfg, z["word_dim"].item())
    enc = fresh.fastformer_model
    amax = lambda t: float(t.detach().abs().max())
    assert float(enc.LayerNorm.weight.detach().min()) == 1.0 and amax(enc.LayerNorm.weight) == 1.0 and amax(enc.LayerNorm.bias) == 0.0
    assert amax(fresh.embedding_transform.bias) == 0.0 and amax(fresh.output_layer.bias) == 0.0
    assert tuple(fresh.output_layer.weight.shape) == (4, cfg.hidden_size)
    for w in (enc.encoders[0].attention.self.query.weight, fresh.word_embedding.weight, enc.position_embeddings.weight):
        assert 0.8 * cfg.initializer_range < float(w.detach().std()) < 1.2 * cfg.initializer_range
    from ebrec.models.fastformer import Fastformer_wu

    table = torch.nn.Embedding(cfg.vocab_size, 20, padding_idx=0)  # a passed table is re-initialised, its declared padding row zeroed
    assert Fastformer_wu(cfg, table).word_embedding is table and amax(table.weight[0]) == 0.0 and amax(table.weight[1]) > 0


def test_stand_alone_encoder_names_and_poolers():
    from ebrec.models.fastformer import StandardFastformerEncoder

    z, names, cfg = load_golden()
    enc = StandardFastformerEncoder(cfg, pooler_count=2)
    pre = "fastformer_model."
    want = [n[len(pre):] for n in names if n.startswith(pre)]
    got = list(enc.state_dict())
    assert got[:len(want)] == want and got[len(want):] == [f"poolers.1.att_fc{i}.{k}" for i in (1, 2) for k in ("weight", "bias")]
    assert enc.attention == "auto" and make_model(cfg, 20).attention == "auto"


def test_import_is_light_and_transformers_free():
    import subprocess
    import sys

    code = ("import sys; import ebrec.models.fastformer as f; assert 'torch' not in sys.modules; "
            "from ebrec.models.fastformer import Fastformer_wu, StandardFastformerEncoder; "
            "from ebrec.models.fastformer.fastformer_wu import Fastformer_wu as W; assert W is Fastformer_wu; "
            "assert 'transformers' not in sys.modules")
    root = Path(__file__).resolve().parents[1]
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root / "ebnerd-benchmark_amd")


def test_argument_checks():
    from ebrec.models.fastformer import StandardFastformerEncoder

    _, _, cfg = load_golden()
    d = vars(cfg)
    for make in (lambda c, **kw: make_model(c, 20, **kw), StandardFastformerEncoder):
        with pytest.raises(ValueError, match="gelu"):
            make(SimpleNamespace(**{**d, "hidden_act": "relu"}))
        with pytest.raises(ValueError, match="pooler_type"):
            make(SimpleNamespace(**{**d, "pooler_type": "cls"}))
        with pytest.raises(ValueError, match="attention"):
            make(cfg, attention="flash")
        with pytest.raises(ValueError, match="multiple"):
            make(SimpleNamespace(**{**d, "num_attention_heads": 5}))
    with pytest.raises(TypeError):
        from ebrec.models.fastformer import Fastformer_wu

        Fastformer_wu(cfg)  # word_embedding is required, as in the reference
    model = make_model(cfg, 20)
    too_long = cfg.max_position_embeddings + 1
    with pytest.raises(IndexError, match="max_position_embeddings"):  # known on the host: raised before the device is looked at
        model(torch.ones(2, too_long, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))
    enc = StandardFastformerEncoder(cfg, pooler_count=2)
    x, mask = torch.zeros(2, 5, cfg.hidden_size), torch.ones(2, 5)
    with pytest.raises(IndexError, match="max_position_embeddings"):
        enc(torch.zeros(2, too_long, cfg.hidden_size), torch.ones(2, too_long))
    for bad in (2, -1):
        with pytest.raises(IndexError, match="pooler"):
            enc(x, mask, pooler_index=bad)
    assert "ignore_index" in type(model).__doc__ and "ignore_index" in __import__("ebrec.models.fastformer.fastformer_wu", fromlist=["x"]).__doc__


def test_forward_on_the_cpu_raises():  # CPU tensors: no GPU at all, or a model that was never moved to it
    from ebrec.models.fastformer import StandardFastformerEncoder

    z, _, cfg = load_golden()
    model = make_model(cfg, 20)
    with pytest.raises(RuntimeError):
        model(torch.as_tensor(z["ids"]), torch.as_tensor(z["targets"]))
    enc = StandardFastformerEncoder(cfg)
    with pytest.raises(RuntimeError):
        enc(torch.zeros(2, 5, cfg.hidden_size), torch.ones(2, 5))
