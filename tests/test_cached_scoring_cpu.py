"""Loader side of scoring from a once-encoded article catalogue (no GPU): NAMLDataLoader's lazily built catalogue and indexed
eval batch, and LSTURDataLoader's indexed eval batch with user indexes, reproduce ``compact_eval_batch`` exactly; the existing
loader methods are unchanged by them."""
import numpy as np
import pandas as pd
import pytest

from ebrec.models.newsrec.dataloader import LSTURDataLoader, NAMLDataLoader
from ebrec.utils._constants import (DEFAULT_HISTORY_ARTICLE_ID_COL, DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_LABELS_COL,
                                    DEFAULT_USER_COL)
from tests.test_data_pipeline import frames  # noqa: F401  (the fixture parquets under tests/golden/ebnerd)


def _fixture_naml(frames, **kw):  # noqa: F811
    beh, _train, mapping = frames
    rng = np.random.default_rng(5)
    # bodies: their own dictionary that names other articles than the title dictionary does (title row 0 with a body, and back)
    body = {a: rng.integers(1, 20, 12).tolist() for j, a in enumerate(sorted(mapping)) if j % 5}
    extra = sorted({a for l in beh[DEFAULT_INVIEW_ARTICLES_COL] for a in l} - set(mapping))[:7]
    body.update({a: rng.integers(1, 20, 12).tolist() for a in extra})
    cats = {a: int(a) % 6 + 1 for j, a in enumerate(sorted(mapping)) if j % 4}
    subcats = {a: int(a) % 9 for a in sorted(mapping)}
    return NAMLDataLoader(behaviors=beh.iloc[:120].reset_index(drop=True), article_dict=mapping, body_mapping=body, category_mapping=cats,
                          subcategory_mapping=subcats, unknown_representation="zeros", unknown_category_value=0,
                          unknown_subcategory_value=11, history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=16, eval_mode=True, **kw)


def _synthetic_frame():
    """unknown ids (7, 9999), a null id inside a list, a null in-view cell, an empty in-view list, repeated ids"""
    return pd.DataFrame({
        DEFAULT_USER_COL: [3, 4, 3, 77, 5],
        DEFAULT_HISTORY_ARTICLE_ID_COL: [[501, 0, 502], [9999, 503, 503], [None, 501, 504], [0, 0, 0], [504, 505, 7]],
        DEFAULT_INVIEW_ARTICLES_COL: [[501, 7, 505, 505], [502], None, [], [9999, 503, 501]],
        DEFAULT_LABELS_COL: [[1, 0, 0, 0], [1], [0], [], [0, 1, 0]]})


def _synthetic_naml():
    rng = np.random.default_rng(2)
    titles = {a: rng.integers(1, 30, 6).tolist() for a in (501, 502, 503, 504)}  # 505 has no title
    bodies = {a: rng.integers(1, 30, 8).tolist() for a in (502, 503, 505, 7)}     # 7 and 505 have a body only
    return NAMLDataLoader(behaviors=_synthetic_frame(), article_dict=titles, body_mapping=bodies, category_mapping={501: 4, 502: 4, 505: 2},
                          subcategory_mapping={503: 1, 7: 6}, unknown_representation="zeros", unknown_category_value=9,
                          unknown_subcategory_value=0, history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, batch_size=2, eval_mode=True)


def _check_naml(loader):
    t_rows, b_rows, vert, subvert = loader.article_catalogue()
    assert len({len(t_rows), len(b_rows), len(vert), len(subvert)}) == 1
    rows = np.stack([np.asarray(a, dtype=np.int64) for a in (t_rows, b_rows, vert, subvert)], axis=1)
    assert len(np.unique(rows, axis=0)) == len(rows), "duplicate catalogue rows"
    known = set(loader.lookup_article_index) | set(loader.lookup_article_index_body) | set(loader.category_mapping or {}) | set(
        loader.subcategory_mapping or {})
    assert len(rows) <= len(known) + 1  # one row per known article at most, plus the unknown row
    tm, bm = loader.lookup_article_matrix[t_rows], loader.lookup_article_matrix_body[b_rows]
    for i in range(len(loader)):
        his, cand, imp, y = loader.index_eval_batch(i)
        assert his.dtype == np.int32 and cand.dtype == np.int32 and his.ndim == 2 and cand.ndim == 1
        ht, hb, hv, hs, ct, cb, cv, cs, rows_c, y_c = loader.compact_eval_batch(i)
        for got, want in ((tm[his], ht), (bm[his], hb), (vert[his][:, :, None], hv), (subvert[his][:, :, None], hs), (tm[cand], ct),
                          (bm[cand], cb), (vert[cand], cv), (subvert[cand], cs), (imp, rows_c), (y, y_c)):
            np.testing.assert_array_equal(got, want)


def test_naml_catalogue_and_indexed_batch_reproduce_the_compact_batch_on_the_fixtures(frames):  # noqa: F811
    _check_naml(_fixture_naml(frames))


def test_naml_catalogue_and_indexed_batch_on_unknown_ids_and_null_cells():
    loader = _synthetic_naml()
    _check_naml(loader)
    t_rows, b_rows, vert, subvert = loader.article_catalogue()
    # 505: no title (row 0) but a body and a category; an unknown id: the all-unknown row
    assert ((t_rows == 0) & (b_rows != 0)).any() and ((t_rows == 0) & (b_rows == 0) & (vert == 9) & (subvert == 0)).any()


def test_lstur_user_indexed_batch_reproduces_the_compact_batch(frames):  # noqa: F811
    beh, _train, mapping = frames
    users = sorted(pd.unique(beh[DEFAULT_USER_COL]))
    umap = {u: i + 1 for i, u in enumerate(users[:-3])}
    fixture = LSTURDataLoader(behaviors=beh.iloc[:120].reset_index(drop=True), article_dict=mapping, user_id_mapping=umap,
                              history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, unknown_representation="zeros", batch_size=16, eval_mode=True)
    synthetic = LSTURDataLoader(behaviors=_synthetic_frame(), article_dict={a: [a % 7 + 1, 2, 0] for a in (501, 502, 503, 504)},
                                user_id_mapping={3: 1, 4: 2, 5: 3}, unknown_user_value=0, history_column=DEFAULT_HISTORY_ARTICLE_ID_COL,
                                unknown_representation="zeros", batch_size=2, eval_mode=True)
    for loader in (fixture, synthetic):
        m = loader.lookup_article_matrix
        for i in range(len(loader)):
            user, his, cand, imp, y = loader.user_index_eval_batch(i)
            u_c, h_c, c_c, rows_c, y_c = loader.compact_eval_batch(i)
            for got, want in ((user, u_c), (m[his], h_c), (m[cand], c_c), (imp, rows_c), (y, y_c)):
                np.testing.assert_array_equal(got, want)
    assert synthetic.user_index_eval_batch(1)[0].tolist() == [1, 0]  # user 77 is not in the mapping


def _same(a, b):
    if isinstance(a, tuple):
        assert isinstance(b, tuple) and len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    else:
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("eval_mode", [True, False])
def test_existing_loader_methods_are_unchanged_by_the_catalogue(frames, eval_mode):  # noqa: F811
    """Return arity and values of the existing methods on a loader that has built its catalogue == on one that has not."""
    beh, train, mapping = frames
    df = (beh.iloc[:60] if eval_mode else train.iloc[:60]).reset_index(drop=True)
    mk = lambda: NAMLDataLoader(behaviors=df, article_dict=mapping, body_mapping=mapping, category_mapping={a: int(a) % 5 for a in mapping},
                                subcategory_mapping={}, unknown_representation="zeros", history_column=DEFAULT_HISTORY_ARTICLE_ID_COL,
                                batch_size=16, eval_mode=eval_mode)
    plain, built = mk(), mk()
    assert getattr(plain, "_catalogue", None) is None  # lazily built: constructing a loader costs nothing new
    built.article_catalogue()
    if eval_mode:
        built.index_eval_batch(0)
    assert len(plain) == len(built)
    for i in range(len(plain)):
        xs, y = built[i]
        assert len(xs) == 8
        _same(plain[i], built[i])
        if eval_mode:
            assert len(built.compact_eval_batch(i)) == 10
            _same(plain.compact_eval_batch(i), built.compact_eval_batch(i))
    assert getattr(plain, "_catalogue", None) is None
    # LSTUR: the 4-tuple of index_eval_batch and the 5-tuple of compact_eval_batch stay as they are
    ls = LSTURDataLoader(behaviors=beh.iloc[:40].reset_index(drop=True), article_dict=mapping, user_id_mapping={}, eval_mode=True,
                         history_column=DEFAULT_HISTORY_ARTICLE_ID_COL, unknown_representation="zeros", batch_size=16)
    before = ls.index_eval_batch(1)
    ls.user_index_eval_batch(1)
    assert len(before) == 4 and len(ls.compact_eval_batch(1)) == 5
    _same(before, ls.index_eval_batch(1))
