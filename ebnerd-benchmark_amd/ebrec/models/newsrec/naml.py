"""NAMLModel on MI355X: the reference's constructor-and-attribute surface (naml.py:13-369) over hand-written HIP kernels.

    model = NAMLModel(hparams=hparams_naml, word2vec_embedding=emb, seed=42)
    model.model.fit(train_loader, validation_data=val_loader, epochs=5)      # NAMLDataLoader batches
    scores = model.scorer.predict(test_loader)                               # NAMLDataLoader(eval_mode=True)

Inputs are the reference's eight arrays ``(his_input_title (B,H,T), his_input_body (B,H,Tb), his_input_vert (B,H,1),
his_input_subvert (B,H,1), pred_input_title (B,C,T), pred_input_body (B,C,Tb), pred_input_vert (B,C,1),
pred_input_subvert (B,C,1))`` (naml.py ``keras.Model([...8 inputs...], preds)``); the scorer takes C = 1.  Deliberate
differences:
  * one GPU, through libebnerd_hip.so only (RuntimeError otherwise -- no CPU fallback, no multi-rank form);
  * dropout uses the build's counter-based stream, not TF's (statistical parity only);
  * weights are saved as a named torch file (``model.model.save_weights``); TF weight lists are not imported.
"""
from __future__ import annotations

import numpy as np
import torch

from ._engine_naml import NAMLEngine
from ._keras_like import ModelBase


class NAMLModel(ModelBase):
    """NAML (Wu et al., IJCAI 2019): attentive multi-view news encoder -- CNN + additive attention over the title and over the
    body, Dense views of the category and subcategory, additive attention over the four views -- and additive attention over
    the clicked news as the user encoder (reference naml.py)."""

    def __init__(self, hparams, word2vec_embedding: np.ndarray = None, word_emb_dim: int = 300, vocab_size: int = 32000,
                 seed: int = None, *, n_users: int = 50000, train_embedding: bool = True, device=None, process_group=None,
                 bce_on: str = "logits"):
        self._preface(hparams, seed, word2vec_embedding, word_emb_dim, vocab_size)
        self.n_users = n_users  # accepted and unused, as in the reference
        for attr in ("cnn_activation", "dense_activation"):
            if getattr(hparams, attr, "relu") != "relu":
                raise ValueError(f"{attr} {getattr(hparams, attr)!r}: the HIP Conv1D and categorical Dense implement relu")
        self._engine = NAMLEngine(
            np.asarray(self.word2vec_embedding), hparams.title_size, hparams.body_size, hparams.history_size, hparams.filter_num,
            hparams.window_size, hparams.attention_hidden_dim, hparams.vert_num, hparams.vert_emb_dim, hparams.subvert_num,
            hparams.subvert_emb_dim, hparams.dropout, hparams.learning_rate, hparams.loss, seed=seed,
            train_embedding=train_embedding, device=device, process_group=process_group, bce_on=bce_on)
        self.model, self.scorer = self._build_graph()

    # -- scorer bodies (naml.py: sigmoid(news(pred_one) . user)) -------------------------------------------------------------
    def _score_pairs(self, *xs) -> torch.Tensor:
        """sigmoid(cand_i . user_i) for every row i of the 8 scorer inputs (histories (N,H,.), candidates (N,1,.))."""
        n = np.shape(xs[0])[0]
        if np.shape(xs[4])[:2] != (n, 1):
            raise ValueError(f"scorer expects one candidate per history row, got {np.shape(xs[0])} vs {np.shape(xs[4])}")
        return self._engine.pair_scores(xs[:4], xs[4:8], np.arange(n), sigmoid=True)

    def _score_compact(self, *xs) -> torch.Tensor:
        """The same scores for the loader's compact eval layout: the 4 history arrays once per impression (b,H,.), the 4
        candidate arrays (n,.), rows[i] = impression of candidate i.  Every article is encoded per batch (``scorer.cache_articles =
        False``, or a loader without an article catalogue)."""
        return self._engine.pair_scores(xs[:4], xs[4:8], np.asarray(xs[8]), sigmoid=True)

    # -- scorer from a once-encoded catalogue: ScorerModel.predict builds the cache per call (it is valid for the current weights only)
    _cache_loader_method = "article_catalogue"  # what an eval loader must offer for the cached path (otherwise: per-batch encoding)

    def _build_article_cache(self, loader):
        """news vectors and user-attention logits of every distinct article of an eval loader (``article_catalogue()``)."""
        t_rows, b_rows, vert, subvert = loader.article_catalogue()
        return self._engine.encode_catalogue(np.asarray(loader.lookup_article_matrix)[t_rows],
                                             np.asarray(loader.lookup_article_matrix_body)[b_rows], vert, subvert)

    def _score_cached(self, cache, loader, i) -> torch.Tensor:
        """Scores of eval batch i from the cache: one indexed pooling-and-scoring launch."""
        his_idx, cand_idx, rows, _y = loader.index_eval_batch(i)
        return self._engine.score_cached(cache, his_idx, cand_idx, rows, sigmoid=True)

    # -- top-N lists from the once-encoded catalogue (_recommend.py) ------------------------------------------------------------
    _recommend_loader_method = "article_catalogue"

    def _recommend_index(self, loader):
        """The cache's rows are those of ``article_catalogue()``: an article id is a candidate when its title row is in it
        (the unknown title, row 0, may stand for several catalogue rows and belongs to no id)."""
        t_rows = np.asarray(loader.article_catalogue()[0])
        row_of_title = {int(t): r for r, t in enumerate(t_rows.tolist()) if t != 0}
        return {k: row_of_title[t] for k, t in loader.lookup_article_index.items() if t in row_of_title}

    def _recommend_cache(self, loader):
        cache = self._build_article_cache(loader)
        return cache, cache.news_all

    def _user_vectors_cached(self, cache, loader, i):
        his_idx = loader.index_eval_batch(i)[0]
        none = np.zeros(0, np.int32)
        _scores, user = self._engine.score_cached(cache, his_idx, none, none, sigmoid=True, return_user=True)
        return user, his_idx

    def train_step(self, *xs):
        """One optimizer step on raw arrays (the 8 inputs and y); returns the batch loss (device tensor)."""
        return self._engine.train_step(*xs)
