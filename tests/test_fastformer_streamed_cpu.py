"""Fastformer's `attention` option without a GPU: its argument check, the state_dict surface under every value, and the float64
oracle (tests/fastformer_oracle.py) pinned to what the REFERENCE's own Fastformer computed on titles of 500 tokens
(tests/golden/fastformer_ref_long.npz, written by tests/golden/make_fastformer_long_golden.py) -- a length only the streamed
attention pair takes; tests/test_fastformer_streamed_gpu.py holds the HIP path to the same file."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import fastformer_oracle as fo
from tests.test_fastformer_cpu import GOLDEN, load_golden, make_model


def load_long():
    z = np.load(GOLDEN / "fastformer_ref_long.npz")
    names = [str(n) for n in z["names"]]
    cfg = SimpleNamespace(**{k[4:]: z[k].item() for k in z.files if k.startswith("cfg_")})
    return z, names, cfg


def test_invalid_attention_value_raises():
    _, _, cfg = load_golden()
    with pytest.raises(ValueError, match="attention"):
        make_model(cfg, 20, attention="flash")
    with pytest.raises(ValueError, match="attention"):
        make_model(cfg, 20, attention=None)


def test_attention_option_changes_no_parameter():
    z, names, cfg = load_golden()
    sds = {}
    for kind in ("resident", "streamed", "auto"):
        model = make_model(cfg, z["word_dim"].item(), attention=kind)
        assert model.attention == kind
        model.load_state_dict({n: torch.as_tensor(z["param." + n]) for n in names}, strict=True)  # a reference checkpoint loads strictly
        sds[kind] = model.state_dict()
    assert make_model(cfg, z["word_dim"].item()).attention == "resident"
    for kind, sd in sds.items():
        assert list(sd) == names, kind
        assert [tuple(v.shape) for v in sd.values()] == [z["param." + n].shape for n in names], kind


def test_oracle_reproduces_the_long_title_reference_in_float64():
    z, names, cfg = load_long()
    assert z["hist"].shape == (3, 2, 500) and cfg.hidden_size == 24 and cfg.num_attention_heads == 4 and cfg.num_hidden_layers == 2
    P = {n: torch.tensor(z["param." + n], dtype=torch.float64, requires_grad=True) for n in names}
    hist, cand, y = torch.as_tensor(z["hist"]), torch.as_tensor(z["cand"]), torch.tensor(z["labels"], dtype=torch.float64)
    score = fo.forward(P, hist, cand, cfg.num_attention_heads, cfg.layer_norm_eps)
    loss = torch.nn.BCELoss()(score, y)
    loss.backward()
    assert np.abs(score.detach().numpy() - z["f64.score"]).max() < 1e-9
    assert abs(loss.item() - z["f64.loss"].item()) < 1e-9
    G = z["G"].item()
    for n in names:
        g = P[n].grad.numpy() if P[n].grad is not None else np.zeros(P[n].shape)
        assert fo.measure(g, z["f64.grad." + n], G) < 1e-9, n
    # what the fixture's inputs exercise: a short slot-0 title, an all-padding later slot, a live last token
    assert (z["hist"][0, 0, 70:] == 0).all() and (z["hist"][2, 1] == 0).all() and z["cand"][1, 0, 499] != 0
    assert 0 < z["E_fwd"].item() < 1e-5 and 0 < z["E_ref"].item() < 1e-3
