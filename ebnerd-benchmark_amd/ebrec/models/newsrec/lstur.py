"""LSTURModel on MI355X: the reference's constructor-and-attribute surface (lstur.py:12-201) over hand-written HIP kernels.

    model = LSTURModel(hparams=hparams_lstur, word2vec_embedding=emb, seed=42)
    model.model.fit(train_loader, validation_data=val_loader, epochs=5)      # LSTURDataLoader batches
    scores = model.scorer.predict(test_loader)

Inputs are ``(user_indexes (B,1), his_input_title (B,H,T), pred_input_title (B,C,T))`` as in the reference
(lstur.py:195 ``keras.Model([user_indexes, his_input_title, pred_input_title], preds)``).  Deliberate differences:
  * one GPU, through libebnerd_hip.so only (RuntimeError otherwise -- no CPU fallback, no multi-rank form);
  * dropout uses the build's counter-based stream, not TF's (statistical parity only);
  * weights are saved as a named torch file (``model.model.save_weights``); TF weight lists are not imported.
"""
from __future__ import annotations

import numpy as np
import torch

from ._engine_lstur import LSTUREngine
from ._keras_like import ModelBase


class LSTURModel(ModelBase):
    """LSTUR (An et al., ACL 2019): CNN title encoder with masked additive attention, and a GRU over the clicked titles
    combined with a trainable long-term user-id embedding -- as the GRU's initial state (type "ini") or concatenated with its
    output (type "con") (reference lstur.py)."""

    def __init__(self, hparams, word2vec_embedding: np.ndarray = None, word_emb_dim: int = 300, vocab_size: int = 32000,
                 seed: int = None, *, train_embedding: bool = True, device=None, process_group=None, bce_on: str = "logits"):
        self._preface(hparams, seed, word2vec_embedding, word_emb_dim, vocab_size)
        if getattr(hparams, "cnn_activation", "relu") != "relu":
            raise ValueError(f"cnn_activation {hparams.cnn_activation!r}: the HIP Conv1D implements relu")
        self._engine = LSTUREngine(
            np.asarray(self.word2vec_embedding), hparams.n_users, hparams.title_size, hparams.history_size, hparams.filter_num,
            hparams.window_size, hparams.attention_hidden_dim, hparams.gru_unit, getattr(hparams, "type", "ini"), hparams.dropout,
            hparams.learning_rate, hparams.loss, seed=seed, train_embedding=train_embedding, device=device,
            process_group=process_group, bce_on=bce_on)
        self.model, self.scorer = self._build_graph()

    # -- scorer bodies (lstur.py:191-200: sigmoid(news(pred_one) . user)) ------------------------------------------------------
    def _score_pairs(self, user, his, pred_one) -> torch.Tensor:
        """sigmoid(cand_i . user_i) for every row i of (user (N,1), his (N,H,T), pred_one (N,1,T))."""
        his = np.asarray(his)
        n = his.shape[0]
        cands = np.asarray(pred_one).reshape(-1, self._engine.T)
        if cands.shape[0] != n:
            raise ValueError(f"scorer expects one candidate per history row, got {his.shape} vs {np.shape(pred_one)}")
        return self._engine.pair_scores(np.asarray(user).reshape(-1), his, cands, np.arange(n), sigmoid=True)

    def _score_compact(self, user, his, cands, rows) -> torch.Tensor:
        """The same scores for the loader's compact eval layout: user (b,), his (b,H,T) once per impression, cands (n,T),
        rows[i] = impression of candidate i.  Every title is encoded per batch (``scorer.cache_articles = False``, or a loader
        without ``user_index_eval_batch``)."""
        return self._engine.pair_scores(np.asarray(user).reshape(-1), np.asarray(his), np.asarray(cands), np.asarray(rows),
                                        sigmoid=True)

    # -- scorer from a once-encoded catalogue: ScorerModel.predict builds the cache per call (it is valid for the current weights only)
    _cache_loader_method = "user_index_eval_batch"  # what an eval loader must offer for the cached path (otherwise: per-batch encoding)

    def _build_article_cache(self, loader):
        """news vectors, GRU input projections and step masks of every row of an eval loader's article matrix."""
        return self._engine.encode_catalogue(np.asarray(loader.lookup_article_matrix))

    def _score_cached(self, cache, loader, i) -> torch.Tensor:
        """Scores of eval batch i from the cache: user-table gather, indexed GRU, ragged pair dot."""
        user, his_idx, cand_idx, rows, _y = loader.user_index_eval_batch(i)
        return self._engine.score_cached(cache, user, his_idx, cand_idx, rows, sigmoid=True)

    # -- top-N lists from the once-encoded catalogue (_recommend.py) ------------------------------------------------------------
    _recommend_loader_method = "user_index_eval_batch"

    def _recommend_index(self, loader):
        return loader.lookup_article_index

    def _recommend_cache(self, loader):
        cache = self._build_article_cache(loader)
        return cache, cache.news_all

    def _user_vectors_cached(self, cache, loader, i):
        user, his_idx = loader.user_index_eval_batch(i)[:2]
        return self._engine.user_vectors_cached(cache, user, his_idx), his_idx

    def train_step(self, user, his, pred, y):
        """One optimizer step on raw arrays; returns the batch loss (device tensor)."""
        return self._engine.train_step(user, his, pred, y)
