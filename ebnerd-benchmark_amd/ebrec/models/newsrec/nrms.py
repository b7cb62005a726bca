"""NRMSModel on MI355X: the reference's constructor-and-attribute surface (nrms.py:23-54,
192-193, 207-208) over hand-written HIP kernels.

    model = NRMSModel(hparams=hparams_nrms, word2vec_embedding=emb, seed=42)
    model.model.fit(train_loader, validation_data=val_loader, epochs=5, callbacks=[...])
    scores = model.scorer.predict(test_loader)

Differences from the reference that are deliberate and visible:
  * runs on a GPU through libebnerd_hip.so only (RuntimeError otherwise -- no CPU fallback);
  * ``shard_table=True`` row-shards the word-embedding table over the ranks of the process group
    (BASELINE config 5) -- rows travel over RCCL, table gradients are never all-reduced;
  * ``train_embedding=False`` freezes the word-embedding table (BASELINE.json config 2,
    "frozen lookup"); the reference always trains it (nrms.py:129);
  * dropout uses the build's own counter-based stream, not TF's (statistical parity only);
  * weights are saved as a named torch file; ``from_keras_weight_list`` imports the 13 arrays of
    ``tf_model.model.get_weights()`` for a 1e-4 forward-parity experiment against TF.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ebrec import _hip

from ._engine import NRMSEngine
from ._keras_like import EncoderModel, ModelBase, dedup_rows

WEIGHT_NAMES = ["news.emb", "news.attn.WQ", "news.attn.WK", "news.attn.WV", "news.att.W", "news.att.b", "news.att.q",
                "user.attn.WQ", "user.attn.WK", "user.attn.WV", "user.att.W", "user.att.b", "user.att.q"]


class NRMSModel(ModelBase):
    """NRMS (Wu et al., EMNLP-IJCNLP 2019) with the reference's quirks kept: P^T.V attention
    (layers.py:249), no masks, un-stabilised +1e-7 additive attention (layers.py:71-77)."""

    def __init__(self, hparams, word2vec_embedding: np.ndarray = None, word_emb_dim: int = 300,
                 vocab_size: int = 32000, seed: int = None, *, train_embedding: bool = True, device=None,
                 process_group=None, shard_table: bool = False, shard_mode: str = "alltoall",
                 deterministic: bool = True, shard_partition: str | None = None, shard_capacity_factor: float = 1.25,
                 table_grad_exchange: str = "auto", bce_on: str = "logits", precision: str = "exact"):
        self._preface(hparams, seed, word2vec_embedding, word_emb_dim, vocab_size)
        self._engine = NRMSEngine(
            np.asarray(self.word2vec_embedding), hparams.title_size, hparams.history_size, hparams.head_num,
            hparams.head_dim, hparams.attention_hidden_dim, hparams.dropout, hparams.learning_rate, hparams.loss,
            seed=seed, train_embedding=train_embedding, device=device, process_group=process_group,
            shard_table=shard_table, shard_mode=shard_mode, deterministic=deterministic,
            shard_partition=shard_partition, shard_capacity_factor=shard_capacity_factor,
            table_grad_exchange=table_grad_exchange, bce_on=bce_on, precision=precision,
            units=getattr(hparams, "newsencoder_units_per_layer", None),
            l2=getattr(hparams, "newsencoder_l2_regularization", 0.0))
        self.model, self.scorer = self._build_graph()

    # -- same helper names as the reference ------------------------------------------
    def _build_graph(self):
        self.newsencoder = EncoderModel(self._encode_news, "news_encoder")
        self.userencoder = EncoderModel(self._encode_users, "user_encoder")
        return super()._build_graph()

    # -- sub-model bodies --------------------------------------------------------------
    def _encode_news(self, ids):
        ids = np.asarray(ids)
        return self._engine.encode_news(ids.reshape(-1, ids.shape[-1]))

    def _encode_users(self, his):
        return self._engine.encode_users(np.asarray(his))

    def _score_pairs(self, his: np.ndarray, pred_one: np.ndarray) -> torch.Tensor:
        """sigmoid(news(pred_one[i]) . user(his[i])) for every row i, encoding each distinct
        history and each distinct candidate title of the batch once."""
        eng = self._engine
        T = eng.T
        cands = pred_one.reshape(-1, T)
        if his.shape[0] != cands.shape[0]:
            raise ValueError(f"scorer expects one candidate per history row, got {his.shape} vs {pred_one.shape}")
        his_u, u_inv = dedup_rows(his)
        cand_u, c_inv = dedup_rows(cands)
        user = eng.encode_users(his_u)
        news = eng.encode_news(cand_u)
        ui = torch.from_numpy(u_inv).to(eng.device)
        ci = torch.from_numpy(c_inv).to(eng.device)
        return eng.pair_scores(user, news, ui, ci, sigmoid=True)

    def _score_compact(self, his: np.ndarray, cands: np.ndarray, rows: np.ndarray) -> torch.Tensor:
        """Same scores for the loader's compact eval layout: his (b,H,T) once per impression, cands (n,T),
        rows[i] = impression of candidate i."""
        eng = self._engine
        cand_u, c_inv = dedup_rows(cands)
        user = eng.encode_users(his)
        news = eng.encode_news(cand_u)
        ui = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(eng.device)
        ci = torch.from_numpy(c_inv).to(eng.device)
        return eng.pair_scores(user, news, ui, ci, sigmoid=True)

    def _encode_article_matrix(self, matrix) -> torch.Tensor:
        """news vectors (n_articles+1, E) of every row of a loader's token matrix, on the device."""
        return self._engine.encode_news(np.asarray(matrix))

    def _users_indexed(self, news_all: torch.Tensor, his_idx) -> torch.Tensor:
        """user vectors (b, E) of one eval batch from cached news vectors: his_idx (b,H) are rows of news_all."""
        eng = self._engine
        hi = torch.from_numpy(np.ascontiguousarray(np.asarray(his_idx).reshape(-1), dtype=np.int32)).to(eng.device)
        b, H = len(his_idx), np.asarray(his_idx).shape[1]  # H from the batch: the history-length sweep scores truncated histories
        NEh = torch.empty(b * H, eng.E, device=eng.device)
        _hip.call("ebn_gather_rows_f32", _hip.ptr(hi), _hip.ptr(news_all), _hip.ptr(NEh), b * H, eng.E, news_all.shape[0],
                  None, -1, ctypes.c_float(0.0), None, _hip.stream_handle())
        return eng.encode_users_from_news(NEh.view(b, H, eng.E))

    def _score_indexed(self, news_all: torch.Tensor, his_idx, cand_idx, rows) -> torch.Tensor:
        """Scores of one eval batch from cached news vectors: his_idx (b,H) / cand_idx (n,) are rows of news_all,
        rows[i] = impression of candidate i."""
        eng = self._engine
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(eng.device)
        user = self._users_indexed(news_all, his_idx)
        return eng.pair_scores(user, news_all, dev(rows), dev(cand_idx), sigmoid=True)

    # -- top-N lists from the once-encoded catalogue (_recommend.py) ------------------------------------------------------------
    _recommend_loader_method = "index_eval_batch"

    def _recommend_index(self, loader):
        return loader.lookup_article_index

    def _recommend_cache(self, loader):
        news_all = self._encode_article_matrix(loader.lookup_article_matrix)
        return news_all, news_all

    def _user_vectors_cached(self, cache, loader, i):
        his_idx = loader.index_eval_batch(i)[0]
        return self._users_indexed(cache, his_idx), his_idx

    # -- interchange ------------------------------------------------------------------
    def from_keras_weight_list(self, weights):
        """Load ``tf_model.model.get_weights()`` (13 arrays, SURVEY.md A.6 order)."""
        self._engine.set_weights(weights)
        return self

    def train_step(self, his, pred, y):
        """One optimizer step on raw arrays; returns the batch loss (device tensor)."""
        return self._engine.train_step(his, pred, y)
