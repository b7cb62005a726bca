"""NPAModel on MI355X: the reference's constructor-and-attribute surface (npa.py:14-190) over hand-written HIP kernels.

    model = NPAModel(hparams=hparams_npa, word2vec_embedding=emb, seed=42)
    model.model.fit(train_loader, validation_data=val_loader, epochs=5)      # LSTURDataLoader batches
    scores = model.scorer.predict(test_loader)

Inputs are ``(user_indexes (B,1), his_input_title (B,H,T), pred_input_title (B,C,T))`` as in the reference
(npa.py:196 ``keras.Model([user_indexes, his_input_title, pred_input_title], preds)``).  Deliberate differences:
  * one GPU, through libebnerd_hip.so only (RuntimeError otherwise -- no CPU fallback, no multi-rank form);
  * dropout uses the build's counter-based stream, not TF's (statistical parity only);
  * weights are saved as a named torch file (``model.model.save_weights``); TF weight lists are not imported;
  * ``scorer.predict`` over an eval-mode loader encodes the loader's article matrix ONCE per call: the conv output ``Vd`` and the
    attention keys ``Ua = tanh(Vd.Wa + ba)`` of a title do not depend on the user (only the logits ``q(user) . Ua_l`` do), so a
    batch is scored from row numbers by an indexed pooling kernel.  ``scorer.cache_articles = False`` is the per-batch path, and a
    catalogue above ``NPAModel.catalogue_max_bytes`` takes it too;
  * ``recommend_pairwise(loader, candidate_ids, top_n=...)`` gives each impression's top-N of one shared candidate list from the
    same once-encoded catalogue: NPA has no per-article vector, so ``ebn_npa_topk_score_f32`` computes every (user, candidate)
    pair's logits and dots on the matrix cores, pools and selects in one launch (``_recommend.py``); ``recommend`` still raises;
  * ``recommend_pairwise_windowed(loader, candidate_ids, window=Freshness(...), top_n=...)`` gives the same lists inside each
    impression's freshness window (``ebn_npa_topk_score_window_f32``: a workgroup walks only the candidate steps its users'
    windows meet); ``recommend_pairwise(..., window=...)`` still raises;
  * ``rank_targets_pairwise(loader, targets, candidate_ids, ...)`` is the accuracy side of those lists: the place of each clicked
    article among all candidates, from ``ebn_npa_target_rank_f32`` -- the same step with a count in place of the selection, also
    inside ``window=Freshness(...)``, where the lists are ``recommend_pairwise_windowed``'s; ``rank_targets`` still raises.
"""
from __future__ import annotations

import numpy as np
import torch

from ._engine_npa import NPAEngine
from ._keras_like import ModelBase
from ._recommend import TargetRanks, _rank_targets, _recommend, npa_target_rank, npa_topk, npa_topk_window, recommend


class NPAModel(ModelBase):
    """NPA (Wu et al., KDD 2019): CNN title encoder and personalized attentive pooling at the word and news levels, both
    queried by a trainable user-id embedding (reference npa.py)."""

    def __init__(self, hparams, word2vec_embedding: np.ndarray = None, word_emb_dim: int = 300, vocab_size: int = 32000,
                 seed: int = None, *, train_embedding: bool = True, device=None, process_group=None, bce_on: str = "logits"):
        self._preface(hparams, seed, word2vec_embedding, word_emb_dim, vocab_size)
        if getattr(hparams, "cnn_activation", "relu") != "relu":
            raise ValueError(f"cnn_activation {hparams.cnn_activation!r}: the HIP Conv1D implements relu")
        self._engine = NPAEngine(
            np.asarray(self.word2vec_embedding), hparams.n_users, hparams.title_size, hparams.history_size, hparams.filter_num,
            hparams.window_size, hparams.attention_hidden_dim, hparams.user_emb_dim, hparams.dropout, hparams.learning_rate,
            hparams.loss, seed=seed, train_embedding=train_embedding, device=device, process_group=process_group, bce_on=bce_on)
        self.model, self.scorer = self._build_graph()

    # -- scorer bodies (npa.py:188-199: sigmoid(news(pred_one) . user)) ------------------------------------------------------
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
        rows[i] = impression of candidate i."""
        return self._engine.pair_scores(np.asarray(user).reshape(-1), np.asarray(his), np.asarray(cands), np.asarray(rows),
                                        sigmoid=True)

    # -- scorer from a once-encoded catalogue: ScorerModel.predict builds the cache per call (it is valid for the current weights only)
    _cache_loader_method = "user_index_eval_batch"  # what an eval loader must offer for the cached path (otherwise: per-batch encoding)
    # the catalogue is T * (F + A) floats per article (72 KB at npa-c1, against 1.6 KB for a news vector): the default holds
    # ebnerd_large (about 125 k articles, 9 GB) and nothing unbounded; above it predict() encodes per batch
    catalogue_max_bytes = 16 * 2 ** 30

    def _build_article_cache(self, loader):
        """Conv output and tanh'd attention keys of every row of an eval loader's article matrix; None when they would not fit
        ``catalogue_max_bytes`` (ScorerModel.predict then takes the per-batch path)."""
        tokens = np.asarray(loader.lookup_article_matrix)
        if self._engine.catalogue_bytes(tokens.shape[0]) > self.catalogue_max_bytes:
            return None
        return self._engine.encode_catalogue(tokens)

    def _score_cached(self, cache, loader, i) -> torch.Tensor:
        """Scores of eval batch i from the cache: user-table gather, query Dense, indexed pooling of the history, user stage,
        indexed pooling of the candidates fused with the score."""
        user, his_idx, cand_idx, rows, _y = loader.user_index_eval_batch(i)
        return self._engine.score_cached(cache, user, his_idx, cand_idx, rows, sigmoid=True)

    def recommend(self, loader, candidate_ids=None, **kwargs):
        """Not implemented.  The encoded catalogue of ``scorer.predict`` does not give a per-article vector to rank against: with a
        shared candidate list the score of a (user, candidate) pair is sum_l w_l (u . Vd_l) with user-dependent w, about
        T * (F + A) MACs (36 kFLOP at npa-c1) per pair -- a different kernel from the top-k over news vectors of ``_recommend.py``.
        ``recommend_pairwise`` is that kernel behind this method's signature."""
        raise NotImplementedError("NPAModel.recommend: NPA's news vector depends on the user (personalised attention, npa.py), so "
                                  "there is no per-article catalogue to rank against")

    # -- top-N lists from the once-encoded catalogue (_recommend.py): every (user, candidate) pair is pooled and scored ------------
    _recommend_loader_method = "user_index_eval_batch"

    def _recommend_index(self, loader):
        return loader.lookup_article_index

    def _recommend_cache(self, loader):
        """(cache, Vd_all): the catalogue of ``scorer.predict``.  Ranking has no per-batch fallback, so a catalogue that does not
        fit raises."""
        cache = self._build_article_cache(loader)
        if cache is None:
            need = self._engine.catalogue_bytes(np.asarray(loader.lookup_article_matrix).shape[0])
            raise ValueError(f"the encoded catalogue needs {need} bytes, above catalogue_max_bytes = {self.catalogue_max_bytes}: "
                             "recommend_pairwise ranks from the whole catalogue (raise catalogue_max_bytes)")
        return cache, cache.Vd_all

    def _user_vectors_cached(self, cache, loader, i):
        """(user_vec | Qn [b, F + A], his_idx): what a candidate is scored with, one row per impression of eval batch i"""
        user, his_idx = loader.user_index_eval_batch(i)[:2]
        user_vec, Qn = self._engine.user_state_cached(cache, user, his_idx)
        return torch.cat([user_vec, Qn], 1), his_idx

    def _recommend_topk(self, cache, users, cand_rows, exclude, k, sigmoid, flags):
        """The scoring launch of ``_recommend.recommend`` for rows ``user_vec | Qn``: ebn_npa_topk_score_f32."""
        F = self._engine.F
        return npa_topk(users[:, :F].contiguous(), users[:, F:].contiguous(), cache.Ua_all, cache.Vd_all, cand_rows, exclude, k, sigmoid,
                        flags)

    def recommend_pairwise(self, loader, candidate_ids=None, **kwargs):
        """Each impression's top_n of one shared candidate list (``_recommend.recommend``: the same arguments, defaults, results and
        errors as the other models' ``recommend``), every (user, candidate) pair scored by personalised pooling from the
        once-encoded catalogue.  ``window=`` raises here: the lists inside freshness windows are ``recommend_pairwise_windowed``'s."""
        return recommend(self, loader, candidate_ids, **kwargs)

    def _recommend_topk_window(self, cache, users, cand_rows, window, exclude, k, sigmoid, flags):
        """The windowed scoring launch of ``_recommend._recommend`` for rows ``user_vec | Qn``: ebn_npa_topk_score_window_f32."""
        F = self._engine.F
        return npa_topk_window(users[:, :F].contiguous(), users[:, F:].contiguous(), cache.Ua_all, cache.Vd_all, cand_rows, window, exclude,
                               k, sigmoid, flags)

    def recommend_pairwise_windowed(self, loader, candidate_ids=None, *, window, **kwargs):
        """``recommend_pairwise`` inside freshness windows: the arguments, defaults, results and errors of the other models'
        ``recommend(..., window=Freshness(...))``, ``rerank=`` included.  An impression at time t is only offered the candidates
        published in [t - max_age, t - min_age]: the candidates are sorted by publish time, the users of a launch by the start of
        their range, and ``ebn_npa_topk_score_window_f32`` lets a 128-user workgroup pool and score only the candidate steps its
        users' ranges meet.  A pair's score has the bits ``recommend_pairwise`` gives it.  ``window`` is required."""
        if window is None:
            raise ValueError("recommend_pairwise_windowed needs window=Freshness(...); the lists without windows are recommend_pairwise's")
        return _recommend(self, loader, candidate_ids, window=window, model_window_launch=self._recommend_topk_window, **kwargs)

    # -- the accuracy side of the same lists: ``rank_targets`` still raises, ``rank_targets_pairwise`` does the work ----------------
    def _rank_launch(self, cache, users, cand_rows, target_pos, window, exclude, sigmoid, flags):
        """The counting launch of ``_recommend._rank_targets`` for rows ``user_vec | Qn``: ebn_npa_target_rank_f32."""
        F = self._engine.F
        return npa_target_rank(users[:, :F].contiguous(), users[:, F:].contiguous(), cache.Ua_all, cache.Vd_all, cand_rows, target_pos,
                               window, exclude, sigmoid, flags)

    def rank_targets_pairwise(self, loader, targets=None, candidate_ids=None, **kwargs) -> TargetRanks:
        """Where each impression's clicked article stands among ALL of ``candidate_ids`` (``_recommend.rank_targets``: the same
        arguments, defaults, results and errors as the other models' ``rank_targets``, ``window=Freshness(...)`` included), every
        (user, candidate) pair scored by personalised pooling from the once-encoded catalogue and counted in the same launch
        (``ebn_npa_target_rank_f32``).  The rule: ``rank`` r <= k holds exactly when ``recommend_pairwise(loader, candidate_ids,
        top_n=k, exclude_history=...)`` has the target at index r - 1, and ``score`` is that slot's score, bit for bit.  Under
        ``window=`` the list is ``recommend_pairwise_windowed``'s with the same window and the rule holds inside each impression's
        window (windowed lists under the name ``recommend_pairwise`` do not exist yet: its ``window=`` raises).  A catalogue above
        ``catalogue_max_bytes`` raises, as it does for ``recommend_pairwise``."""
        return _rank_targets(self, loader, targets, candidate_ids, model_launch=self._rank_launch, **kwargs)

    def train_step(self, user, his, pred, y):
        """One optimizer step on raw arrays; returns the batch loss (device tensor)."""
        return self._engine.train_step(user, his, pred, y)
