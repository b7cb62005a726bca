"""NRMSDocVec on MI355X: the reference's surface (nrms_docvec.py:21-39, 182-188) over the HIP kernels.

    model = NRMSDocVec(hparams=hparams_nrms_docvec, seed=123)
    model.model.fit(train_loader, validation_data=val_loader, ...)     # loaders built from {article_id: doc vector}
    scores = model.scorer.predict(test_loader)

The news encoder consumes pre-computed document vectors of width ``hparams.title_size`` (768): per
article ``[Dense(u, relu, l2) -> BatchNormalization -> Dropout] x units -> Dense(head_num*head_dim, relu)``
(nrms_docvec.py:113-135); user encoder, scorer, loss and optimizer are those of NRMS.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ebrec import _hip

from ._engine_docvec import DocVecEngine
from ._keras_like import EncoderModel, ModelBase, dedup_rows


class NRMSDocVec(ModelBase):
    def __init__(self, hparams, seed: int = None, *, device=None, process_group=None, bce_on: str = "logits"):
        self._preface(hparams, seed)
        self._engine = DocVecEngine(
            hparams.title_size, hparams.newsencoder_units_per_layer, hparams.history_size, hparams.head_num,
            hparams.head_dim, hparams.attention_hidden_dim, hparams.dropout, hparams.learning_rate, hparams.loss,
            hparams.newsencoder_l2_regularization, seed=seed, device=device, process_group=process_group, bce_on=bce_on)
        self.model, self.scorer = self._build_graph()

    def _build_graph(self):
        self.newsencoder = EncoderModel(lambda x: self._engine.encode_news(np.asarray(x, dtype=np.float32).reshape(-1, self._engine.Din)),
                                        "news_encoder")
        self.userencoder = EncoderModel(lambda x: self._engine.encode_users(np.asarray(x, dtype=np.float32)), "user_encoder")
        return super()._build_graph()

    def _score_pairs(self, his: np.ndarray, pred_one: np.ndarray) -> torch.Tensor:
        eng = self._engine
        cands = np.asarray(pred_one, dtype=np.float32).reshape(-1, eng.Din)
        his = np.asarray(his, dtype=np.float32)
        if his.shape[0] != cands.shape[0]:
            raise ValueError(f"scorer expects one candidate per history row, got {his.shape} vs {pred_one.shape}")
        his_u, u_inv = dedup_rows(his)
        cand_u, c_inv = dedup_rows(cands)
        return eng.pair_scores(eng.encode_users(his_u), eng.encode_news(cand_u), torch.from_numpy(u_inv).to(eng.device),
                               torch.from_numpy(c_inv).to(eng.device), sigmoid=True)

    def _score_compact(self, his: np.ndarray, cands: np.ndarray, rows: np.ndarray) -> torch.Tensor:
        eng = self._engine
        cand_u, c_inv = dedup_rows(np.asarray(cands, dtype=np.float32))
        user = eng.encode_users(np.asarray(his, dtype=np.float32))
        news = eng.encode_news(cand_u)
        return eng.pair_scores(user, news, torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(eng.device),
                               torch.from_numpy(c_inv).to(eng.device), sigmoid=True)

    def _encode_article_matrix(self, matrix) -> torch.Tensor:
        """news vectors (n_articles+1, E) of every document vector of a loader's matrix, on the device."""
        return self._engine.encode_news(np.asarray(matrix, dtype=np.float32))

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

    def train_step(self, his, pred, y):
        return self._engine.train_step(his, pred, y)
