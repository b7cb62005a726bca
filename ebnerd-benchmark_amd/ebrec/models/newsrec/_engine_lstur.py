"""Device engine of the MI355X LSTUR path (reference lstur.py, layers.py:55-81, 273-309), one rank.

Per impression b with user index u_b (lstur.py:56-201):
  title:  X = Dropout(p)(emb[tokens]) -> Vd = Dropout(p)(relu(conv1d_same(X) + b_c))
          -> U = tanh(Vd.Wa + ba), m_l = (token_l != 0) && any(Vd_l != 0), w = AttLayer2 weights under m, news = sum_l w_l Vd_l
  user:   long_b = user_emb[u_b];  GRU over the H history news vectors (steps with an all-zero vector are skipped: Masking(0.0))
          type "ini": h0 = long_b, user = h_H;  type "con": h0 = 0, user = [h_H, long_b].Wd + bd
  scores = cand . user -> softmax + compiled loss (training), sigmoid (scorer)
The news encoder does not depend on the user: scorer.predict over an eval loader encodes the loader's article matrix once
(encode_catalogue) and runs each batch from the cached news vectors, GRU input projections and step masks (score_cached).

Data layout in HBM (fp32 row-major):
  table        (V, E)              word embeddings (trainable: fixed-point gradient accumulator + fused Adam sweep)
  user_table   (n_users + 1, U)    zeros-initialised long-term user embeddings (same gradient path, dropout-free)
  dense        flat buffer         conv_Wb (window*E + 1, F) = Conv1D kernel rows | bias row, att_W, att_b, att_q, gru_k (F, 3U),
                                   gru_r (U, 3U), gru_b (2, 3U) [, dense_W (2U, U), dense_b (U,) for "con"] -> one Adam launch
  titles       N = B*(H+C) per step, history titles first (b*H + h), then candidates (B*H + b*C + c)
  GRU          Hs (H+1, B, U) time-major states, act (H, B, 4U) gate activations, gx / dgx (B*H, 3U), dgh (H, B, 3U)

Shared with the other engines and defined in _engine_base.py: constructor scaffolding, step state, flags (_check_oob), staging and
train_step, forward / eval_loss / pair_scores, the Adam launches, the Conv1D backward block (UserTableEngine <- ConvEngineBase).  Here:
buffers, shapes, weight order, the encoders, the backward up to the Conv1D, and scoring from an encoded catalogue.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from ebrec import _hip

from ._engine_base import BETA1, BETA2, ConvView, UserTableEngine, glorot_uniform_np, pair_score_tail

SITE_NEWS_IN, SITE_CONV = 0, 2

WEIGHT_NAMES = ["news.emb", "user.emb", "news.conv.W", "news.conv.b", "news.att.W", "news.att.b", "news.att.q", "user.gru.kernel",
                "user.gru.recurrent_kernel", "user.gru.bias"]
CON_WEIGHT_NAMES = ["user.dense.W", "user.dense.b"]
TYPES = ("ini", "con")


class _Bufs:
    """Activations and backward scratch of one (B, n_cand) shape."""

    def __init__(self, eng, B, n_cand, train):
        dev, H, T, E, F, A, U = eng.device, eng.H, eng.T, eng.E, eng.F, eng.A, eng.U
        f = lambda *s: torch.empty(*s, device=dev)
        N = B * H + n_cand
        R = N * T
        BH = B * H
        self.B, self.n_cand, self.N, self.R = B, n_cand, N, R
        self.ids, self.uidx = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        self.X, self.Vd, self.Ua, self.w = f(R, E), f(R, F), f(R, A), f(R)
        self.NV, self.Eu, self.user = f(N, F), f(B, U), f(B, U)
        self.gx, self.Hs, self.act = f(BH, 3 * U), f(H + 1, B, U), f(H, B, 4 * U)
        self.ones = torch.ones(max(R, BH, B), device=dev)
        if train:
            self.labels, self.scores, self.probs = f(n_cand), f(n_cand), f(n_cand)
            self.loss_rows = f(B)
            self.dNV, self.duser, self.dEu = f(N, F), f(B, U), f(B, U)
            self.dgx, self.dgh = f(BH, 3 * U), f(H, B, 3 * U)
            self.dhH, self.dh0 = f(B, U), f(B, U)  # "con": the GRU's output gradient and its (unused) initial-state gradient
            self.de, self.dVd, self.dX = f(R), f(R, F), f(R, E)
            lib = _hip.lib()
            self.part = f(max(int(lib.ebn_attpool_partials_len(R, A)), 1))
            self.splits = int(lib.ebn_conv1d_wgrad_splits(N, T, E, F, eng.window))
            self.wpart = f(max(int(lib.ebn_conv1d_wgrad_workspace_floats(N, T, E, F, eng.window, self.splits)), 1))
            wsf = lib.ebn_gemm_workspace_floats
            self.ws = f(max(int(wsf(F, A, R)), int(wsf(U, 3 * U, BH)), int(wsf(F, 3 * U, BH)), int(wsf(1, 3 * U, BH)), 1))


class LSTUREngine(UserTableEngine):
    MODEL = "LSTUR"

    def __init__(self, table: np.ndarray, n_users: int, title_size: int, history_size: int, filter_num: int, window_size: int,
                 attention_hidden_dim: int, gru_unit: int, user_type: str, dropout: float, learning_rate: float, loss: str,
                 seed=None, train_embedding: bool = True, device=None, process_group=None, bce_on: str = "logits"):
        self._require_one_rank(process_group)
        if user_type not in TYPES:
            raise ValueError(f"LSTUR type must be 'ini' or 'con', got {user_type!r}")
        if int(filter_num) != int(gru_unit):
            raise ValueError(f"filter_num ({filter_num}) must equal gru_unit ({gru_unit}): the score is cand . user")
        self._init_table(table, device)
        self.n_users, self.type = int(n_users), user_type
        self.T, self.H, self.F, self.A, self.window = int(title_size), int(history_size), int(filter_num), int(attention_hidden_dim), int(window_size)
        self.U = int(gru_unit)
        if self.E % 4 or self.F % 4:
            raise ValueError(f"word_emb_dim ({self.E}) and filter_num ({self.F}) must be multiples of 4 for the HIP Conv1D and GRU")
        W, E, F, A, U = self.window, self.E, self.F, self.A, self.U
        shapes = {"conv_Wb": (W * E + 1, F), "att_W": (F, A), "att_b": (A,), "att_q": (A,), "gru_k": (F, 3 * U),
                  "gru_r": (U, 3 * U), "gru_b": (2, 3 * U)}
        if self.type == "con":
            shapes.update({"dense_W": (2 * U, U), "dense_b": (U,)})
        self._init_state(shapes, U, dropout, learning_rate, loss, seed, train_embedding, bce_on)  # user table: lstur.py:71-76
        self._init_weights(seed)

    # ------------------------------------------------------------------ parameters
    def _init_weights(self, seed):
        pv = self.params.view
        F, A, U = self.F, self.A, self.U
        self._conv_init("conv_Wb", seed)
        with torch.no_grad():
            pv("att_W").copy_(torch.from_numpy(glorot_uniform_np((F, A), seed)))
            pv("att_q").copy_(torch.from_numpy(glorot_uniform_np((A, 1), seed).reshape(A)))
            # kernel (F, 3U) and recurrent kernel (U, 3U) are glorot_uniform(seed) of one shape: identical at init (F == U)
            pv("gru_k").copy_(torch.from_numpy(glorot_uniform_np((F, 3 * U), seed)))
            pv("gru_r").copy_(torch.from_numpy(glorot_uniform_np((U, 3 * U), seed)))
            for name in ("att_b", "gru_b"):
                pv(name).zero_()
            if self.type == "con":
                pv("dense_W").copy_(torch.from_numpy(glorot_uniform_np((2 * U, U), seed)))
                pv("dense_b").zero_()

    def weight_names(self):
        return list(WEIGHT_NAMES) + (list(CON_WEIGHT_NAMES) if self.type == "con" else [])

    def _dense_names(self):
        return ["att_W", "att_b", "att_q", "gru_k", "gru_r", "gru_b"] + (["dense_W", "dense_b"] if self.type == "con" else [])

    def get_weights(self):
        pv = lambda n: self.params.view(n).cpu().numpy()
        A = self.A
        out = [self.table.cpu().numpy(), self.user_table.cpu().numpy()] + self._conv_get("conv_Wb")
        for name in self._dense_names():
            a = pv(name)
            out.append(a.reshape(A, 1) if name == "att_q" else a)
        return out

    def set_weights(self, weights):
        names = self.weight_names()
        if len(weights) != len(names):
            raise ValueError(f"expected {len(names)} weight arrays ({', '.join(names)}), got {len(weights)}")
        w = [np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in weights]
        W, E, F = self.window, self.E, self.F
        want = [tuple(self.table.shape), tuple(self.user_table.shape), (W, E, F), (F,)]
        want += [(self.A, 1) if n == "att_q" else tuple(self.params.shapes[n]) for n in self._dense_names()]
        for a, s, n in zip(w, want, names):
            if a.shape != s:
                raise ValueError(f"{n}: shape {a.shape} != {s}")
        t = lambda a: torch.from_numpy(a)
        with torch.no_grad():
            self.table.copy_(t(w[0]))
            self.user_table.copy_(t(w[1]))
            pv = self.params.view
            self._conv_set("conv_Wb", w[2], w[3])
            for name, a in zip(self._dense_names(), w[4:]):
                pv(name).copy_(t(a.reshape(pv(name).shape)))

    def count_params(self):
        W, E, F, A, U = self.window, self.E, self.F, self.A, self.U
        n = self.table.numel() + self.user_table.numel() + W * E * F + F + F * A + 2 * A + 3 * U * F + 3 * U * U + 6 * U
        return n + (2 * U * U + U if self.type == "con" else 0)

    # ------------------------------------------------------------------ kernels
    def _encode(self, b: _Bufs, train: bool, expand=None):
        """Forward of every title and user of the buffers' batch (ids / uidx already staged); training: dropout on."""
        self._encode_news(b, train, expand)
        self._encode_users(b)

    def _encode_news(self, b: _Bufs, train: bool, expand=None, users: bool = True):
        """The title encoder over the buffers' N titles -> b.NV; users: also the gather of the batch's user-table rows -> b.Eu."""
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        P = self.params
        st = pt(self.state) if train else None
        B, N, R, T, E, F, A, U = b.B, b.N, b.R, self.T, self.E, self.F, self.A, self.U
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        p_in = self.p if train else 0.0
        if expand is not None:  # article-row numbers -> token ids on the device (dataloader.py:169-179)
            call("ebn_expand_titles_i32", pt(expand), pt(self.article_matrix), pt(b.ids), N, T, self.article_matrix.shape[0],
                 pt(self.oob_flag), S())
        call("ebn_gather_rows_f32", pt(b.ids), pt(self.table), pt(b.X), R, E, self.V, st, SITE_NEWS_IN if p_in > 0 else -1,
             ctypes.c_float(p_in), pt(self.oob_flag), S())
        if users:
            call("ebn_gather_rows_f32", pt(b.uidx), pt(self.user_table), pt(b.Eu), B, U, self.n_users + 1, None, -1, f0,
                 pt(self.user_oob_flag), S())
        Wb = P.view("conv_Wb")
        call("ebn_conv1d_fwd_f32", pt(b.X), pt(Wb), pt(Wb[self.window * E]), pt(b.Vd), N, T, E, F, self.window, st,
             SITE_CONV if p_in > 0 else -1, ctypes.c_float(p_in), -1, f0, S())
        call("ebn_gemm_f32", 0, 0, R, A, F, f1, pt(b.Vd), F, pt(P.view("att_W")), A, f0, pt(b.Ua), A, S())
        call("ebn_attpool_masked_fwd_f32", pt(b.Ua), pt(P.view("att_b")), pt(P.view("att_q")), pt(b.Vd), pt(b.ids), pt(b.NV),
             pt(b.w), N, T, F, A, S())

    def _encode_users(self, b: _Bufs):
        """The user encoder over the first B*H news vectors of b.NV (b.Eu gathered): GRU, and for "con" the Dense."""
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        P = self.params
        B, F, U, H = b.B, self.F, self.U, self.H
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        his = b.NV[: B * H]
        call("ebn_gemm_f32", 0, 0, B * H, 3 * U, F, f1, pt(his), F, pt(P.view("gru_k")), 3 * U, f0, pt(b.gx), 3 * U, S())
        h0 = pt(b.Eu) if self.type == "ini" else None
        call("ebn_gru_fwd_f32", pt(b.gx), pt(his), pt(P.view("gru_r")), pt(P.view("gru_b")), h0, pt(b.Hs), pt(b.act), B, H, F, U,
             S())
        if self.type == "con":
            self._con_dense(b.Hs[H], b.Eu, b.user, b.ones, B)

    def _con_dense(self, hH, Eu, user, ones, B):
        """type "con": Dense(U)(concat[h_H, long_u]) = 1.bd + h_H.Wd[:U] + long_u.Wd[U:]"""
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        P, U = self.params, self.U
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        Wd = P.view("dense_W")
        call("ebn_gemm_f32", 0, 0, B, U, 1, f1, pt(ones), 1, pt(P.view("dense_b")), U, f0, pt(user), U, S())
        call("ebn_gemm_f32", 0, 0, B, U, U, f1, pt(hH), U, pt(Wd[:U]), U, f1, pt(user), U, S())
        call("ebn_gemm_f32", 0, 0, B, U, U, f1, pt(Eu), U, pt(Wd[U:]), U, f1, pt(user), U, S())

    def _user_vec(self, b: _Bufs):
        return b.Hs[self.H] if self.type == "ini" else b.user

    def _train_kernels(self, b: _Bufs, C: int, expand=None):
        """One optimizer step on the staged batch: step advance, forward, loss, backward, Adam (dense, word table, user table)."""
        self._grad_kernels(b, C, expand)
        self._optimizer_kernels()

    def _grad_kernels(self, b: _Bufs, C: int, expand=None):
        """Step advance, forward, loss and backward: the dense gradients land in params.grad, the table gradients in the
        fixed-point accumulators table_acc / user_acc."""
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        P = self.params
        st = pt(self.state)
        B, N, R, T, E, F, A, U, H = b.B, b.N, b.R, self.T, self.E, self.F, self.A, self.U, self.H
        BH = B * H
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        ws, wsn = pt(b.ws), b.ws.numel()
        call("ebn_step_advance", st, BETA1, BETA2, S())
        self._encode(b, True, expand)
        cand = b.NV[BH:]
        call("ebn_score_loss_train_f32", pt(cand), pt(self._user_vec(b)), pt(b.labels), pt(b.scores), pt(b.probs),
             pt(b.loss_rows), pt(self.loss_dev), pt(b.dNV[BH:]), pt(b.duser), B, C, F, self.loss_kind, ctypes.c_float(1.0 / B), S())
        # user encoder
        if self.type == "ini":
            dhH, dh0 = b.duser, b.dEu  # h0 = long_u: the GRU's initial-state gradient is the user-table gradient
        else:
            Wd = P.view("dense_W")
            gWd = P.g("dense_W")
            call("ebn_gemm_f32", 1, 0, U, U, B, f1, pt(b.Hs[H]), U, pt(b.duser), U, f0, pt(gWd[:U]), U, S())
            call("ebn_gemm_f32", 1, 0, U, U, B, f1, pt(b.Eu), U, pt(b.duser), U, f0, pt(gWd[U:]), U, S())
            call("ebn_gemm_f32", 0, 0, 1, U, B, f1, pt(b.ones), B, pt(b.duser), U, f0, pt(P.g("dense_b")), U, S())
            call("ebn_gemm_f32", 0, 1, B, U, U, f1, pt(b.duser), U, pt(Wd[:U]), U, f0, pt(b.dhH), U, S())
            call("ebn_gemm_f32", 0, 1, B, U, U, f1, pt(b.duser), U, pt(Wd[U:]), U, f0, pt(b.dEu), U, S())
            dhH, dh0 = b.dhH, b.dh0
        his = b.NV[:BH]
        call("ebn_gru_bwd_f32", pt(dhH), pt(his), pt(P.view("gru_r")), pt(b.Hs), pt(b.act), pt(b.dgx), pt(b.dgh), pt(dh0), B, H, F,
             U, S())
        gb = P.g("gru_b")
        call("ebn_gemm_f32_ws", 1, 0, U, 3 * U, BH, f1, pt(b.Hs), U, pt(b.dgh), 3 * U, f0, pt(P.g("gru_r")), 3 * U, ws, wsn, S())
        call("ebn_gemm_f32_ws", 1, 0, F, 3 * U, BH, f1, pt(his), F, pt(b.dgx), 3 * U, f0, pt(P.g("gru_k")), 3 * U, ws, wsn, S())
        call("ebn_gemm_f32_ws", 0, 0, 1, 3 * U, BH, f1, pt(b.ones), BH, pt(b.dgx), 3 * U, f0, pt(gb[0]), 3 * U, ws, wsn, S())
        call("ebn_gemm_f32_ws", 0, 0, 1, 3 * U, BH, f1, pt(b.ones), BH, pt(b.dgh), 3 * U, f0, pt(gb[1]), 3 * U, ws, wsn, S())
        call("ebn_gemm_f32", 0, 1, BH, F, 3 * U, f1, pt(b.dgx), 3 * U, pt(P.view("gru_k")), 3 * U, f0, pt(b.dNV), F, S())
        # news encoder: masked AttLayer2 backward (w == 0 on masked rows: zero gradients there), then the Conv1D
        call("ebn_attpool_bwd_pool_f32", pt(b.Vd), pt(b.w), pt(b.dNV), pt(b.dVd), pt(b.de), N, T, F, S())
        call("ebn_attpool_bwd_dpre_f32", pt(b.Ua), pt(P.view("att_q")), pt(b.de), pt(P.g("att_q")), pt(P.g("att_b")), pt(b.part),
             R, A, 0, S())
        call("ebn_gemm_f32_ws", 1, 0, F, A, R, f1, pt(b.Vd), F, pt(b.Ua), A, f0, pt(P.g("att_W")), A, ws, wsn, S())
        call("ebn_gemm_f32", 0, 1, R, F, A, f1, pt(b.Ua), A, pt(P.view("att_W")), A, f1, pt(b.dVd), F, S())
        self._conv_backward(ConvView(b.ids, b.X, b.Vd, b.dVd, b.dX, b.wpart, b.splits, T, "conv_Wb", SITE_NEWS_IN), N, self.p, 0.0)
        call("ebn_embedding_grad_scatter_fixed", pt(b.uidx), pt(b.dEu), pt(self.user_acc), B, U, self.n_users + 1, None, -1, f0,
             pt(self.range_flag), S())

    # ------------------------------------------------------------------ hooks of the shared host entry points
    def _new_bufs(self, B, n_cand, cand_imp, train):
        return _Bufs(self, B, n_cand, train)

    def _graph_key_extra(self):
        return (self.type,)

    # ------------------------------------------------------------------ scoring from a once-encoded catalogue
    def encode_catalogue(self, tokens, chunk=8192):
        """Everything scorer.predict needs of the articles alone, for the CURRENT weights (build it per predict, never keep it on the
        model): tokens (n_rows, T) -> cache with news_all (n_rows, F), gx_all = news_all . gru_k (n_rows, 3U) -- the GRU's input
        projection is per article -- and live (n_rows,) int32 = any(news_all != 0), the GRU's Masking(0.0) step mask.  Encoded in
        chunks: the scratch is that of `chunk` titles whatever n_rows is."""
        tokens = np.asarray(tokens)
        if tokens.ndim != 2 or tokens.shape[1] != self.T:
            raise ValueError(f"catalogue tokens must be (n_rows, {self.T}), got {tuple(tokens.shape)}")
        self._host_ranges(np.zeros(0, np.int64), tokens)
        n_rows = tokens.shape[0]
        F, U = self.F, self.U
        news_all = torch.empty(n_rows, F, device=self.device)
        b = _Bufs(self, 0, min(chunk, n_rows), train=False) if n_rows else None
        for s in range(0, n_rows, chunk):
            n = min(chunk, n_rows - s)
            if n != b.N:
                b = _Bufs(self, 0, n, train=False)  # the short last chunk
            self._put(b.ids, tokens[s:s + n])
            self._encode_news(b, False, users=False)
            news_all[s:s + n].copy_(b.NV)
        gx_all = torch.empty(n_rows, 3 * U, device=self.device)
        if n_rows:
            _hip.call("ebn_gemm_f32", 0, 0, n_rows, 3 * U, F, ctypes.c_float(1.0), _hip.ptr(news_all), F, _hip.ptr(self.params.view("gru_k")),
                      3 * U, ctypes.c_float(0.0), _hip.ptr(gx_all), 3 * U, _hip.stream_handle())
        live = (news_all != 0).any(dim=1).to(torch.int32).contiguous()
        self._check_oob()
        return SimpleNamespace(news_all=news_all, gx_all=gx_all, live=live, n_rows=n_rows)

    def _user_vectors_indexed(self, cache, user, his_idx):
        """The user half of the cached scorer, launches only: user (b,) user indexes, his_idx (b, H) rows of the cache -> (b, F).
        User-table gather -> indexed GRU over the cached input projections -> ("con") Dense."""
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        B, H, U = his_idx.shape[0], his_idx.shape[1], self.U
        dev = self.device
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        uidx, hi = i32(user), i32(his_idx.reshape(-1))
        Eu, h_work, h_out = (torch.empty(B, U, device=dev) for _ in range(3))
        call("ebn_gather_rows_f32", pt(uidx), pt(self.user_table), pt(Eu), B, U, self.n_users + 1, None, -1, ctypes.c_float(0.0),
             pt(self.user_oob_flag), S())
        call("ebn_gru_infer_indexed_f32", pt(cache.gx_all), pt(cache.live), cache.n_rows, pt(hi), pt(self.params.view("gru_r")),
             pt(self.params.view("gru_b")), pt(Eu) if self.type == "ini" else None, pt(h_work), pt(h_out), B, H, U,
             pt(self.row_oob_flag), S())
        user_vec = h_out
        if self.type == "con":
            user_vec = torch.empty(B, U, device=dev)
            self._con_dense(h_out, Eu, user_vec, torch.ones(max(B, 1), device=dev), B)
        return user_vec

    def _indexed_users_args(self, user, his_idx):
        user = self._uidx(user)
        his_idx = np.asarray(his_idx)
        if his_idx.ndim != 2 or user.shape[0] != his_idx.shape[0]:
            raise ValueError(f"indexed batches need user (b,) and his_idx (b, H), got {tuple(user.shape)} {tuple(his_idx.shape)}")
        self._host_ranges(user)
        return user, his_idx

    def user_vectors_cached(self, cache, user, his_idx):
        """user vectors (b, F) of one indexed batch from the cache (recommend): the user half of ``score_cached``."""
        user, his_idx = self._indexed_users_args(user, his_idx)
        user_vec = self._user_vectors_indexed(cache, user, his_idx)
        self._check_oob()
        return user_vec

    def score_cached(self, cache, user, his_idx, cand_idx, cand_imp, sigmoid=True):
        """act(news_all[cand_i] . user[cand_imp[i]]) of one indexed batch: user (b,) user indexes, his_idx (b, H) / cand_idx (n,) rows
        of the cache, cand_imp (n,) the impression of each candidate.  User-table gather -> indexed GRU over the cached input
        projections -> ("con") Dense -> ragged pair dot against the cached news vectors."""
        user, his_idx = self._indexed_users_args(user, his_idx)
        cand_idx = np.asarray(cand_idx).reshape(-1)
        if cand_idx.size and (cand_idx.min() < 0 or cand_idx.max() >= cache.n_rows):
            raise IndexError(f"article row out of range [0, {cache.n_rows}) for the encoded catalogue")
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
        user_vec = self._user_vectors_indexed(cache, user, his_idx)
        ci, ui = i32(cand_idx), i32(np.asarray(cand_imp).reshape(-1))
        out = pair_score_tail(user_vec, cache.news_all, ui, ci, self.F, sigmoid)
        self._check_oob()
        return out
