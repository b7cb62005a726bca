"""NAML without a GPU: the float64 oracle (tests/naml_oracle.py) against finite differences, hparams_naml, NAMLDataLoader on
the reference's parquet fixtures, the lazy export of NAMLModel and its Keras parameter count."""
import math

import numpy as np
import pytest
import torch

from oracle import nrms_numpy as on
from tests import naml_oracle as nao
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture of the reference loader test)

from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_INVIEW_ARTICLES_COL


def test_hparams_naml_defaults():
    from ebrec.models.newsrec import hparams_naml, hparams_to_dict

    want = {"title_size": 30, "history_size": 20, "body_size": 40, "vert_num": 100, "vert_emb_dim": 10, "subvert_num": 100,
            "subvert_emb_dim": 10, "dense_activation": "relu", "cnn_activation": "relu", "attention_hidden_dim": 200,
            "filter_num": 400, "window_size": 3, "optimizer": "adam", "loss": "cross_entropy_loss", "dropout": 0.2,
            "learning_rate": 1e-4}
    assert hparams_to_dict(hparams_naml) == want


def test_naml_model_is_a_lazy_export():
    import ebrec.models.newsrec as nr

    from ebrec.models.newsrec import NAMLModel

    assert NAMLModel.__name__ == "NAMLModel" and nr.NAMLModel is NAMLModel
    assert "NAML" in nr.__doc__ and "out of scope" not in nr.__doc__


def test_count_params_is_the_keras_formula_without_a_gpu():
    """NAMLEngine.count_params() is pure arithmetic: evaluate it on a stand-in with the engine's attributes."""
    from ebrec.models.newsrec._engine_naml import NAMLEngine
    from ebrec.models.newsrec import hparams_naml as hp

    class Stub:
        table = torch.empty(0)
        window, E, F, A = hp.window_size, 300, hp.filter_num, hp.attention_hidden_dim
        n_vert, Kv, n_sub, Ks = hp.vert_num, hp.vert_emb_dim, hp.subvert_num, hp.subvert_emb_dim

    assert NAMLEngine.count_params(Stub()) == 1_053_200
    Stub.table = torch.empty(32000, 300)
    assert NAMLEngine.count_params(Stub()) == 1_053_200 + 32000 * 300
    Stub.window, Stub.E, Stub.F, Stub.A, Stub.n_vert, Stub.Kv, Stub.n_sub, Stub.Ks = 5, 16, 24, 8, 7, 3, 11, 6
    Stub.table = torch.empty(50, 16)
    V, E, F, A, W, nv, Kv, ns, Ks = 50, 16, 24, 8, 5, 7, 3, 11, 6
    want = V * E + 2 * (W * E * F + F) + 4 * (F * A + 2 * A) + nv * Kv + ns * Ks + (Kv + Ks) * F + 2 * F
    assert NAMLEngine.count_params(Stub()) == want
    # and it is the number of elements of the oracle's parameter set (the engine's get_weights() order)
    P = nao.random_params(V, E, F, A, W, nv, Kv, ns, Ks)
    assert sum(v.size for v in P.values()) == want and list(P) == nao.WEIGHT_ORDER


def _tiny(seed=4):
    V, E, F, A, window, nv, Kv, ns, Ks = 13, 8, 8, 4, 3, 5, 3, 4, 2
    P = nao.random_params(V, E, F, A, window, nv, Kv, ns, Ks, seed=3)
    rng = np.random.default_rng(seed)
    B, H, C, T, Tb = 2, 3, 2, 4, 5
    xs = (rng.integers(0, V, (B, H, T)), rng.integers(0, V, (B, H, Tb)), rng.integers(0, nv, (B, H, 1)),
          rng.integers(0, ns, (B, H, 1)), rng.integers(0, V, (B, C, T)), rng.integers(0, V, (B, C, Tb)),
          rng.integers(0, nv, (B, C, 1)), rng.integers(0, ns, (B, C, 1)))
    xs[2][0, :, 0] = 1  # a duplicated category: its table row's gradient sums over the articles
    y = np.zeros((B, C))
    y[:, 0] = 1
    return P, xs, y


@pytest.mark.parametrize("loss", ["cross_entropy_loss", "log_loss"])
def test_oracle_gradients_match_finite_differences(loss):
    P, xs, y = _tiny()
    drop = on.Drop(0.2, 11, 1)
    L, _, _, g = nao.naml_loss_and_grads(xs, y, P, 0.2, drop, loss)
    rng = np.random.default_rng(5)
    h = 1e-6
    for name, w in P.items():
        flat = w.reshape(-1)
        for i in rng.choice(flat.size, size=min(6, flat.size), replace=False):
            old = flat[i]
            flat[i] = old + h
            lp = nao.naml_loss_and_grads(xs, y, P, 0.2, drop, loss)[0]
            flat[i] = old - h
            lm = nao.naml_loss_and_grads(xs, y, P, 0.2, drop, loss)[0]
            flat[i] = old
            fd = (lp - lm) / (2 * h)
            assert abs(fd - g[name].reshape(-1)[i]) <= 1e-6 + 1e-5 * abs(fd), (name, i, fd, g[name].reshape(-1)[i])
    assert np.isfinite(L)
    assert np.abs(g["v_emb"][1]).max() > 0 and np.abs(g["s_emb"]).max() > 0


def test_oracle_news_encoder_is_attention_over_four_views():
    """With identical views the view attention's weights are 1/4 each (up to the 1e-7 of the denominator)."""
    P, xs, _ = _tiny()
    T = {k: torch.tensor(v) for k, v in P.items()}
    x = torch.ones(3, 4, P["va_W"].shape[0], dtype=torch.float64)
    out, w = nao.att_layer2(x, T["va_W"], T["va_b"], T["va_q"])
    np.testing.assert_allclose(w.numpy(), 0.25, rtol=1e-6)
    np.testing.assert_allclose(out.numpy(), 1.0, rtol=1e-6)


def _naml_mappings(mapping, beh):
    """body_mapping = the article mapping; a category mapping keyed by article id as the reference test builds it (one row
    number per distinct category); a third of the articles carry no category (-> the unknown value)."""
    ids = sorted(mapping)
    cats = {a: int(a) % 7 for a in ids}
    distinct = {c: i for i, c in enumerate(sorted(set(cats.values())))}
    category_mapping = {a: distinct[c] + 1 for j, (a, c) in enumerate(cats.items()) if j % 3}
    return mapping, category_mapping


def test_naml_loader_train_mode_like_reference_test(frames):  # noqa: F811
    """test_newsrec.py:152-190: len, 8 inputs, integer dtypes, integer labels, and the reference's shapes."""
    from ebrec.models.newsrec.dataloader import NAMLDataLoader

    beh, train, mapping = frames
    body_mapping, category_mapping = _naml_mappings(mapping, beh)
    body_mapping = {k: list(v) + [int(k) % 5 + 1] * 2 for k, v in body_mapping.items()}  # bodies 12 tokens long, own matrix
    loader = NAMLDataLoader(behaviors=train, article_dict=mapping, body_mapping=body_mapping, category_mapping=category_mapping,
                            unknown_representation="zeros", subcategory_mapping=category_mapping,
                            history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=100)
    assert len(loader) == int(np.ceil(len(train) / 100))
    batch = loader[0]
    assert len(batch) == 2 and len(batch[0]) == 8
    for a in batch[0]:
        assert isinstance(a.ravel()[0], np.integer)
    assert isinstance(batch[1].ravel()[0], np.integer)
    (ht, hb, hv, hs, pt, pb, pv, ps), y = batch
    n, C = min(100, len(train)), int(train["n"].min())
    assert ht.shape == (n, 3, 10) and hb.shape == (n, 3, 12) and hv.shape == (n, 3, 1) and hs.shape == (n, 3, 1)
    assert pt.shape == (n, C, 10) and pb.shape == (n, C, 12) and pv.shape == (n, C, 1) and ps.shape == (n, C, 1)
    assert y.shape == (n, C)
    # every article's values, one by one against the mappings
    his_ids = train[DEFAULT_HISTORY_ARTICLE_ID_COL].iloc[:n].tolist()
    inv_ids = train[DEFAULT_INVIEW_ARTICLES_COL].iloc[:n].tolist()
    for i in range(n):
        for arts, t, bo, v, s in ((his_ids[i], ht, hb, hv, hs), (inv_ids[i], pt, pb, pv, ps)):
            for j, a in enumerate(arts):
                np.testing.assert_array_equal(t[i, j], mapping.get(a, [0] * 10))
                np.testing.assert_array_equal(bo[i, j], body_mapping.get(a, [0] * 12))
                assert v[i, j, 0] == category_mapping.get(a, 0) and s[i, j, 0] == category_mapping.get(a, 0)
    assert sum(len(loader[i][1]) for i in range(len(loader))) == len(train)


def test_naml_loader_unknown_articles_take_category_0_and_body_row_0(frames):  # noqa: F811
    from ebrec.models.newsrec.dataloader import NAMLDataLoader

    beh, train, mapping = frames
    body_mapping, category_mapping = _naml_mappings(mapping, beh)
    loader = NAMLDataLoader(behaviors=train, article_dict=mapping, body_mapping=body_mapping, category_mapping=category_mapping,
                            subcategory_mapping={}, unknown_subcategory_value=3, unknown_representation="zeros",
                            history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=64)
    seen_unknown = False
    for i in range(len(loader)):
        (ht, hb, hv, hs, pt, pb, pv, ps), _y = loader[i]
        lo = i * 64
        arts = train[DEFAULT_INVIEW_ARTICLES_COL].iloc[lo: lo + len(pt)].tolist()
        for r, row in enumerate(arts):
            for j, a in enumerate(row):
                if a not in mapping:
                    seen_unknown = True
                    assert pv[r, j, 0] == 0 and (pb[r, j] == 0).all() and (pt[r, j] == 0).all()
        assert (hs == 3).all() and (ps == 3).all()  # an empty subcategory mapping: every article is unknown
    assert seen_unknown


def test_naml_loader_eval_mode_layout(frames):  # noqa: F811
    """Eval mode (the reference raises here): histories repeated once per candidate, pred_* of shape (sum C_i, 1, .);
    compact_eval_batch holds the same values without the repetition."""
    from ebrec.models.newsrec.dataloader import NAMLDataLoader

    beh, _train, mapping = frames
    body_mapping, category_mapping = _naml_mappings(mapping, beh)
    loader = NAMLDataLoader(behaviors=beh, article_dict=mapping, body_mapping=body_mapping, category_mapping=category_mapping,
                            subcategory_mapping=category_mapping, unknown_representation="zeros",
                            history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=100, eval_mode=True)
    (ht, hb, hv, hs, pt, pb, pv, ps), y = loader[0]
    want = int(beh["n"].iloc[:100].sum())
    assert len(y) == want and y.shape == (want, 1)
    assert ht.shape == (want, 3, 10) and hb.shape == (want, 3, 10) and hv.shape == (want, 3, 1) and hs.shape == (want, 3, 1)
    assert pt.shape == (want, 1, 10) and pb.shape == (want, 1, 10) and pv.shape == (want, 1, 1) and ps.shape == (want, 1, 1)
    c = loader.compact_eval_batch(0)
    rows = c[8]
    for full, comp in zip((ht, hb, hv, hs), c[:4]):
        np.testing.assert_array_equal(comp[rows], full)
    for full, comp in zip((pt, pb, pv, ps), c[4:8]):
        np.testing.assert_array_equal(comp.reshape(full.shape), full)
    np.testing.assert_array_equal(c[9], y)
    assert sum(len(loader[i][1]) for i in range(len(loader))) == int(beh["n"].sum())
    assert len(loader) == math.ceil(len(beh) / 100)


def test_two_rank_process_group_and_non_relu_activations_raise(monkeypatch):
    from ebrec.models.newsrec import NAMLModel, hparams_naml

    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="one rank"):
        NAMLModel(hparams_naml, vocab_size=10, word_emb_dim=8, seed=1, process_group=object())
    for attr in ("cnn_activation", "dense_activation"):
        hp = type("hp", (hparams_naml,), {attr: "tanh"})
        with pytest.raises(ValueError, match=attr):
            NAMLModel(hp, vocab_size=10, word_emb_dim=8, seed=1)
