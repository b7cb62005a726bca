"""NPA without a GPU: the float64 oracle (tests/npa_oracle.py) against first principles, hparams_npa, LSTURDataLoader on the
reference's parquet fixtures, and the lazy export of NPAModel."""
import numpy as np
import pandas as pd
import pytest
import torch

from oracle import nrms_numpy as on
from tests import npa_oracle as npo
from tests.test_data_pipeline import DATA, frames  # noqa: F401  (the fixture of the reference loader test)

from ebrec.utils._constants import DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_USER_COL


@pytest.mark.parametrize("window", [1, 3, 5])
@pytest.mark.parametrize("T", [1, 2, 7])
def test_oracle_conv_matches_explicit_loop(window, T):
    rng = np.random.default_rng(window * 10 + T)
    X, W, b = rng.normal(size=(3, T, 8)), rng.normal(size=(window, 8, 6)), rng.normal(size=6)
    got = npo.conv1d_same(torch.from_numpy(X), torch.from_numpy(W), torch.from_numpy(b)).numpy()
    np.testing.assert_allclose(got, npo.conv1d_loop(X, W, b), rtol=1e-12, atol=1e-12)


def test_oracle_conv_same_padding_split():
    """Keras "same" with an even window pads (window-1)//2 rows on the left and the rest on the right."""
    X = np.zeros((1, 4, 1))
    X[0, 0, 0] = 1.0
    W = np.arange(1, 5, dtype=np.float64).reshape(4, 1, 1)  # taps j = 0..3, left pad 1
    out = npo.conv1d_same(torch.from_numpy(X), torch.from_numpy(W), torch.zeros(1, dtype=torch.float64)).numpy()[0, :, 0]
    # out[t] = sum_j X[t + j - 1] W[j]: X[0] reaches t = 1 through j = 0 and t = 0 through j = 1
    np.testing.assert_array_equal(out, [2.0, 1.0, 0.0, 0.0])
    np.testing.assert_array_equal(npo.conv1d_loop(X, W, np.zeros(1))[0, :, 0], out)


def _tiny():
    V, E, n_users, Du, F, A, window = 13, 8, 5, 6, 8, 4, 3
    P = npo.random_params(V, E, n_users, Du, F, A, window, seed=3)
    rng = np.random.default_rng(4)
    B, H, C, T = 2, 3, 2, 4
    user = np.array([1, 1])  # a duplicate user: its embedding gradient sums over both impressions
    his, pred = rng.integers(0, V, (B, H, T)), rng.integers(0, V, (B, C, T))
    y = np.zeros((B, C))
    y[:, 0] = 1
    return P, user, his, pred, y


@pytest.mark.parametrize("loss", ["cross_entropy_loss", "log_loss"])
def test_oracle_gradients_match_finite_differences(loss):
    P, user, his, pred, y = _tiny()
    drop = on.Drop(0.2, 11, 1)
    L, _, g = npo.npa_loss_and_grads(user, his, pred, y, P, 0.2, drop, loss)
    rng = np.random.default_rng(5)
    h = 1e-6
    for name, w in P.items():
        flat = w.reshape(-1)
        for i in rng.choice(flat.size, size=min(6, flat.size), replace=False):
            old = flat[i]
            flat[i] = old + h
            lp = npo.npa_loss_and_grads(user, his, pred, y, P, 0.2, drop, loss)[0]
            flat[i] = old - h
            lm = npo.npa_loss_and_grads(user, his, pred, y, P, 0.2, drop, loss)[0]
            flat[i] = old
            fd = (lp - lm) / (2 * h)
            assert abs(fd - g[name].reshape(-1)[i]) <= 1e-6 + 1e-5 * abs(fd), (name, i, fd, g[name].reshape(-1)[i])
    assert np.isfinite(L)


def test_oracle_user_embedding_gradient_lands_on_used_rows_only():
    P, user, his, pred, y = _tiny()
    _, _, g = npo.npa_loss_and_grads(user, his, pred, y, P, 0.0, None)
    used = np.zeros(P["user_emb"].shape[0], bool)
    used[user] = True
    assert np.abs(g["user_emb"][~used]).max() == 0 and np.abs(g["user_emb"][used]).max() > 0


def test_hparams_npa_defaults():
    from ebrec.models.newsrec import hparams_npa, hparams_to_dict

    want = {"title_size": 30, "history_size": 20, "n_users": 50000, "cnn_activation": "relu", "attention_hidden_dim": 200,
            "user_emb_dim": 400, "filter_num": 400, "window_size": 3, "optimizer": "adam", "loss": "cross_entropy_loss",
            "dropout": 0.2, "learning_rate": 1e-4}
    assert hparams_to_dict(hparams_npa) == want


def test_npa_model_is_a_lazy_export():
    import ebrec.models.newsrec as nr

    from ebrec.models.newsrec import NPAModel

    assert NPAModel.__name__ == "NPAModel" and nr.NPAModel is NPAModel
    assert "NPA" in nr.__doc__ and "NPA, LSTUR" not in nr.__doc__


def _user_mapping(beh):
    users = sorted(pd.unique(beh[DEFAULT_USER_COL]))
    known = users[: len(users) * 3 // 4]  # the rest stay unknown -> unknown_user_value
    return {u: i + 1 for i, u in enumerate(known)}, set(users) - set(known)


def test_lstur_loader_train_mode_like_reference_test(frames):  # noqa: F811
    """test_newsrec.py:109-131: len, (user_indexes, his, pred) structure, integer dtypes, integer labels."""
    from ebrec.models.newsrec.dataloader import LSTURDataLoader

    beh, train, mapping = frames
    umap, unknown = _user_mapping(beh)
    loader = LSTURDataLoader(behaviors=train, article_dict=mapping, user_id_mapping=umap,
                             history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, unknown_representation="zeros", batch_size=100)
    assert len(loader) == int(np.ceil(len(train) / 100))
    batch = loader[0]
    assert len(batch) == 2 and len(batch[0]) == 3
    (user, his, pred), y = batch
    n, C = min(100, len(train)), int(train["n"].min())
    assert user.shape == (n, 1) and his.shape == (n, 3, 10) and pred.shape == (n, C, 10) and y.shape == (n, C)
    for a in (user, his, pred, y):
        assert np.issubdtype(a.dtype, np.integer)
    want = [umap.get(u, 0) for u in train[DEFAULT_USER_COL].iloc[:n]]
    assert user[:, 0].tolist() == want
    assert any(u in unknown for u in train[DEFAULT_USER_COL]) and 0 in user  # unknown users map to 0
    (his2, pred2), y2 = super(LSTURDataLoader, loader).__getitem__(0)  # the NRMS batch is unchanged
    np.testing.assert_array_equal(his2, his)
    np.testing.assert_array_equal(pred2, pred)
    (ui, hi, pi), yi = loader.index_batch(0)
    np.testing.assert_array_equal(ui, user[:, 0])
    np.testing.assert_array_equal(loader.lookup_article_matrix[hi], his)
    np.testing.assert_array_equal(loader.lookup_article_matrix[pi], pred)
    np.testing.assert_array_equal(yi, y)


def test_lstur_loader_eval_mode_like_reference_test(frames):  # noqa: F811
    """test_newsrec.py:133-149: every candidate is unfolded; user and history repeat once per candidate."""
    from ebrec.models.newsrec.dataloader import LSTURDataLoader

    beh, _train, mapping = frames
    umap, _ = _user_mapping(beh)
    loader = LSTURDataLoader(behaviors=beh, article_dict=mapping, user_id_mapping=umap,
                             history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, unknown_representation="zeros", batch_size=100,
                             eval_mode=True, unknown_user_value=0)
    (user, his, pred), y = loader[0]
    want = int(beh["n"].iloc[:100].sum())
    assert len(y) == want and user.shape == (want, 1) and his.shape == (want, 3, 10) and pred.shape == (want, 1, 10)
    reps = beh["n"].iloc[:100].to_numpy()
    np.testing.assert_array_equal(user[:, 0], np.repeat([umap.get(u, 0) for u in beh[DEFAULT_USER_COL].iloc[:100]], reps))
    uc, hc, pc, rows, yc = loader.compact_eval_batch(0)
    np.testing.assert_array_equal(uc[rows], user[:, 0])
    np.testing.assert_array_equal(hc[rows], his)
    np.testing.assert_array_equal(pc, pred[:, 0])
    np.testing.assert_array_equal(yc, y)
    assert sum(len(loader[i][1]) for i in range(len(loader))) == int(beh["n"].sum())
