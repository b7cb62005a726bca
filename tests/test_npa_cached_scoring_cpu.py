"""Host side of NPA's cached scoring: the catalogue's size arithmetic, the hooks ScorerModel.predict looks for, and recommend()."""
import numpy as np
import pytest


def _engine(T, F, A):
    from ebrec.models.newsrec._engine_npa import NPAEngine

    eng = object.__new__(NPAEngine)  # no device: catalogue_bytes is host arithmetic over the shape
    eng.T, eng.F, eng.A = T, F, A
    return eng


def test_catalogue_bytes_is_rows_times_title_times_filters_plus_attention_dim():
    eng = _engine(30, 400, 200)
    assert eng.catalogue_bytes(0) == 0
    assert eng.catalogue_bytes(1) == 30 * 600 * 4 == 72000          # 72 KB per article at npa-c1
    assert eng.catalogue_bytes(20000) == 1_440_000_000
    assert eng.catalogue_bytes(np.int32(125_000)) == 9_000_000_000   # ebnerd_large: past 2^32, no int32 wrap
    assert isinstance(eng.catalogue_bytes(np.int64(7)), int)
    assert _engine(9, 32, 24).catalogue_bytes(41) == 41 * 9 * 56 * 4


def test_npa_model_exposes_the_cache_hooks_and_a_bounded_default_budget():
    from ebrec.models.newsrec import NPAModel
    from ebrec.models.newsrec._keras_like import ScorerModel
    from ebrec.models.newsrec.dataloader import LSTURDataLoader

    assert NPAModel._cache_loader_method == "user_index_eval_batch"
    assert hasattr(LSTURDataLoader, NPAModel._cache_loader_method)
    assert callable(NPAModel._build_article_cache) and callable(NPAModel._score_cached)
    assert ScorerModel.cache_articles is True
    assert NPAModel.catalogue_max_bytes == 16 * 2 ** 30
    assert _engine(30, 400, 200).catalogue_bytes(125_000) < NPAModel.catalogue_max_bytes  # ebnerd_large fits the default


def test_a_catalogue_over_the_budget_is_not_built():
    from ebrec.models.newsrec import NPAModel

    class Loader:
        lookup_article_matrix = np.zeros((5, 30), np.int32)

    class Engine:
        def catalogue_bytes(self, n):
            return _engine(30, 400, 200).catalogue_bytes(n)

        def encode_catalogue(self, tokens):
            return ("built", tokens.shape)

    m = object.__new__(NPAModel)
    m._engine = Engine()
    assert m._build_article_cache(Loader()) == ("built", (5, 30))
    m.catalogue_max_bytes = 5 * 72000 - 1
    assert m._build_article_cache(Loader()) is None
    m.catalogue_max_bytes = 5 * 72000
    assert m._build_article_cache(Loader()) is not None


def test_npa_recommend_still_raises():
    from ebrec.models.newsrec import NPAModel

    with pytest.raises(NotImplementedError, match="depends on the user"):
        NPAModel.recommend(object.__new__(NPAModel), None)
    assert "36 kFLOP" in NPAModel.recommend.__doc__


def test_the_header_declares_the_new_entry_points():
    from ebrec import _hip

    lib = _hip.lib()
    assert hasattr(lib, "ebn_pap_indexed_f32") and hasattr(lib, "ebn_bias_tanh_rows_f32")
