"""LSTUR without a GPU: the float64 oracle's GRU (tests/lstur_oracle.py) against torch.nn.GRU and an explicit masked loop, its
gradients, the masked AttLayer2, hparams_lstur, the argument checks of the new C entry points and the lazy export of
LSTURModel."""
import ctypes

import numpy as np
import pytest
import torch

from tests import lstur_oracle as lo


def _gru_inputs(B, H, F, U, seed):
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    g = lambda *s: rng.uniform(-1, 1, s) * np.sqrt(6.0 / (s[0] + s[-1]))
    return t(rng.normal(size=(B, H, F))), t(rng.normal(size=(B, U)) * 0.5), t(g(F, 3 * U)), t(g(U, 3 * U)), \
        t(rng.uniform(-0.3, 0.3, (2, 3 * U)))


def test_oracle_gru_equals_torch_gru_on_unmasked_sequences():
    """Independent check of the gate algebra: Keras [z, r, h] column blocks with reset_after=True are torch.nn.GRU with its
    [r, z, n] row blocks, the input bias row as b_ih and the recurrent bias row as b_hh."""
    B, H, F, U = 4, 6, 5, 3
    X, h0, Wk, Wr, bias = _gru_inputs(B, H, F, U, 0)
    perm = lambda W: torch.cat([W[..., U:2 * U], W[..., :U], W[..., 2 * U:]], -1)
    gru = torch.nn.GRU(F, U, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(perm(Wk).T)
        gru.weight_hh_l0.copy_(perm(Wr).T)
        gru.bias_ih_l0.copy_(perm(bias[0]))
        gru.bias_hh_l0.copy_(perm(bias[1]))
        _, hn = gru(X, h0[None])
    got = lo.gru_keras(X, h0, Wk, Wr, bias)
    torch.testing.assert_close(got, hn[0], rtol=1e-12, atol=1e-12)


def _loop_gru(X, h0, Wk, Wr, bias, mask):
    """explicit per-sequence, per-step loop in numpy: a masked step carries h unchanged"""
    X, h0, Wk, Wr, bias = (a.numpy() for a in (X, h0, Wk, Wr, bias))
    U = h0.shape[1]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    out = np.zeros_like(h0)
    for b in range(X.shape[0]):
        h = h0[b].copy()
        for t in range(X.shape[1]):
            if not mask[b, t]:
                continue
            gx, gh = X[b, t] @ Wk + bias[0], h @ Wr + bias[1]
            z, r = sig(gx[:U] + gh[:U]), sig(gx[U:2 * U] + gh[U:2 * U])
            n = np.tanh(gx[2 * U:] + r * gh[2 * U:])
            h = z * h + (1 - z) * n
        out[b] = h
    return out


def test_oracle_masked_gru_equals_explicit_loop():
    B, H, F, U = 5, 7, 4, 3
    X, h0, Wk, Wr, bias = _gru_inputs(B, H, F, U, 1)
    mask = np.ones((B, H), bool)
    mask[0, :3] = False          # left padding
    mask[1, 5:] = False          # right padding
    mask[2, [1, 4]] = False      # holes
    mask[3, :] = False           # everything padded: the output is h0
    X = X * torch.from_numpy(mask[..., None].astype(np.float64))  # Masking(0.0) derives exactly this mask
    got = lo.gru_keras(X, h0, Wk, Wr, bias)
    np.testing.assert_allclose(got.numpy(), _loop_gru(X, h0, Wk, Wr, bias, mask), rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(got[3].numpy(), h0[3].numpy())
    assert not np.allclose(got[4].numpy(), h0[4].numpy())


def test_oracle_gru_gradcheck():
    B, H, F, U = 2, 3, 3, 2
    X, h0, Wk, Wr, bias = _gru_inputs(B, H, F, U, 2)
    X[0, 1] = 0.0  # one masked step
    args = [a.clone().requires_grad_(True) for a in (X, h0, Wk, Wr, bias)]
    mask = (X != 0).any(-1)
    assert torch.autograd.gradcheck(lambda *a: lo.gru_keras(*a, mask=mask), args, eps=1e-6, atol=1e-8)


def test_masked_attlayer2_padding_and_zero_rows():
    rng = np.random.default_rng(3)
    n, L, F, A = 3, 5, 4, 6
    Y = torch.from_numpy(rng.uniform(0.1, 1.0, (n, L, F)))
    ids = torch.from_numpy(rng.integers(1, 9, (n, L)))
    ids[0] = 0                     # a title of padding only
    ids[1, 3:] = 0                 # right padding: those rows take no part (unlike NRMS)
    Y[2, 1] = 0.0                  # a real token whose conv row was dropped / ReLU'd to zero is masked too
    W, b, q = (torch.from_numpy(rng.normal(size=s)) for s in ((F, A), (A,), (A, 1)))
    out, w = lo.masked_attlayer2(Y, ids, W, b, q)
    assert (out[0] == 0).all() and (w[0] == 0).all()
    assert (w[1, 3:] == 0).all() and w[2, 1] == 0
    for i, rows in ((1, [0, 1, 2]), (2, [0, 2, 3, 4])):  # equals plain AttLayer2 over the live rows
        a = torch.exp(torch.tanh(Y[i, rows] @ W + b) @ q).squeeze(-1)
        want = (a / (a.sum() + 1e-7)) @ Y[i, rows]
        torch.testing.assert_close(out[i], want, rtol=1e-12, atol=1e-12)


def test_hparams_lstur_defaults():
    from ebrec.models.newsrec import hparams_lstur, hparams_to_dict

    want = {"title_size": 30, "history_size": 20, "n_users": 50000, "cnn_activation": "relu", "type": "ini",
            "attention_hidden_dim": 200, "gru_unit": 400, "filter_num": 400, "window_size": 3, "optimizer": "adam",
            "loss": "cross_entropy_loss", "dropout": 0.2, "learning_rate": 1e-4}
    assert hparams_to_dict(hparams_lstur) == want


def test_lstur_model_is_a_lazy_export():
    import ebrec.models.newsrec as nr

    from ebrec.models.newsrec import LSTURModel

    assert LSTURModel.__name__ == "LSTURModel" and nr.LSTURModel is LSTURModel
    assert "LSTUR" in nr.__doc__ and "NPA, LSTUR" not in nr.__doc__


@pytest.mark.parametrize("bad", [{"type": "sum"}, {"filter_num": 64}])
def test_lstur_model_rejects_bad_hparams_before_touching_a_device(bad):
    from ebrec.models.newsrec import LSTURModel, hparams_lstur

    hp = type("hp", (hparams_lstur,), dict(bad))
    with pytest.raises(ValueError):
        LSTURModel(hp, vocab_size=10, word_emb_dim=8, seed=1)


def test_gru_and_masked_pool_entry_points_check_their_arguments():
    """Rejected before any launch, so no device is needed: shapes the kernels do not support, sizes up to 2^62, and the
    empty batch (nothing to enqueue)."""
    from ebrec import _hip

    lib = _hip.lib()
    p = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below returns before a launch
    fwd = lambda B, H, F, U, h0=p: lib.ebn_gru_fwd_f32(p, p, p, p, h0, p, p, B, H, F, U, None)
    bwd = lambda B, H, F, U: lib.ebn_gru_bwd_f32(p, p, p, p, p, p, p, ctypes.c_void_p(1 << 21), B, H, F, U, None)
    for call in (fwd, bwd):
        assert call(0, 20, 400, 400) == 0              # empty batch
        assert call(4, 0, 400, 400) == -1              # no steps
        assert call(4, 20, 400, 402) == -2             # U % 4 != 0
        assert call(4, 20, 398, 400) == -2             # F % 4 != 0
        assert call(1 << 62, 20, 400, 400) == -2
        assert call((1 << 31) - 1, 20, 400, 400) == -2  # B (H + 1) U elements past the index budget
        assert call(4, 1 << 30, 400, 400) == -2
    assert fwd(0, 20, 400, 400, h0=None) == 0          # NULL h0 is allowed (type "con" starts from zeros)
    assert lib.ebn_gru_fwd_f32(None, p, p, p, p, p, p, 4, 20, 400, 400, None) == -1
    assert lib.ebn_gru_bwd_f32(p, p, p, p, p, p, p, p, 4, 20, 400, 400, None) == -1  # dh0 aliases dhH
    pool = lambda n, L, E, A, ids=p: lib.ebn_attpool_masked_fwd_f32(p, p, p, p, ids, p, p, n, L, E, A, None)
    assert pool(0, 30, 400, 200) == 0
    assert pool(4, 30, 400, 200, ids=None) == -1
    assert pool(4, 0, 400, 200) == -1
    assert pool(1 << 62, 30, 400, 200) == -2
    assert pool(4, 1 << 20, 400, 200) == -2


def test_lstur_model_refuses_more_than_one_rank(monkeypatch):
    from ebrec.models.newsrec import LSTURModel, hparams_lstur

    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="one rank"):
        LSTURModel(hparams_lstur, vocab_size=10, word_emb_dim=8, seed=1, process_group=object())
