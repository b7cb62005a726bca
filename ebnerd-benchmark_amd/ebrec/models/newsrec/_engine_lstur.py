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
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from ebrec import _hip

from ._engine import ADAM_EPS, BETA1, BETA2, FlatParams, glorot_uniform_np, loss_kind_of, require_gpu
from ._engine_npa import conv_glorot_np

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


class LSTUREngine:
    def __init__(self, table: np.ndarray, n_users: int, title_size: int, history_size: int, filter_num: int, window_size: int,
                 attention_hidden_dim: int, gru_unit: int, user_type: str, dropout: float, learning_rate: float, loss: str,
                 seed=None, train_embedding: bool = True, device=None, process_group=None, bce_on: str = "logits"):
        if process_group is not None and torch.distributed.get_world_size(process_group) > 1:
            raise ValueError("LSTURModel runs on one rank: multi-rank LSTUR is not implemented (build it without a process group "
                             "of more than one rank)")
        if user_type not in TYPES:
            raise ValueError(f"LSTUR type must be 'ini' or 'con', got {user_type!r}")
        if int(filter_num) != int(gru_unit):
            raise ValueError(f"filter_num ({filter_num}) must equal gru_unit ({gru_unit}): the score is cand . user")
        self.device = require_gpu() if device is None else torch.device(device)
        table = np.asarray(table, dtype=np.float32)
        self.V, self.E = table.shape
        self.n_users, self.type = int(n_users), user_type
        self.T, self.H, self.F, self.A, self.window = int(title_size), int(history_size), int(filter_num), int(attention_hidden_dim), int(window_size)
        self.U = int(gru_unit)
        if self.E % 4 or self.F % 4:
            raise ValueError(f"word_emb_dim ({self.E}) and filter_num ({self.F}) must be multiples of 4 for the HIP Conv1D and GRU")
        self.p = float(dropout)
        self.loss, self.bce_on = loss, bce_on
        loss_kind_of(loss, bce_on)
        self.train_embedding = bool(train_embedding)
        self.seed = seed
        dev = self.device
        W, E, F, A, U = self.window, self.E, self.F, self.A, self.U
        shapes = {"conv_Wb": (W * E + 1, F), "att_W": (F, A), "att_b": (A,), "att_q": (A,), "gru_k": (F, 3 * U),
                  "gru_r": (U, 3 * U), "gru_b": (2, 3 * U)}
        if self.type == "con":
            shapes.update({"dense_W": (2 * U, U), "dense_b": (U,)})
        self.params = FlatParams(shapes, dev)
        self.table = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
        self.user_table = torch.zeros(self.n_users + 1, U, device=dev)  # embeddings_initializer="zeros" (lstur.py:71-76)
        self.table_acc = torch.zeros(self.table.numel(), dtype=torch.int64, device=dev)
        self.table_m, self.table_v = torch.zeros_like(self.table), torch.zeros_like(self.table)
        self.user_acc = torch.zeros(self.user_table.numel(), dtype=torch.int64, device=dev)
        self.user_m, self.user_v = torch.zeros_like(self.user_table), torch.zeros_like(self.user_table)
        self.oob_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.user_oob_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.range_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.row_oob_flag = torch.zeros(1, dtype=torch.int32, device=dev)  # a history row outside an encoded catalogue
        self.loss_dev = torch.zeros(1, device=dev)
        st = _hip.StepState()
        st.step, st.seed, st.lr, st.adam_alpha = 0, (0 if seed is None else int(seed)) & 0xFFFFFFFF, learning_rate, 0.0
        self.state = torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).to(dev)
        self._lr = float(learning_rate)
        self._bufs, self._graphs = {}, {}
        self.use_graph = True
        self.article_matrix = None
        self._article_matrix_src = None
        self._init_weights(seed)

    # ------------------------------------------------------------------ parameters
    def _init_weights(self, seed):
        pv = self.params.view
        W, E, F, A, U = self.window, self.E, self.F, self.A, self.U
        with torch.no_grad():
            pv("conv_Wb")[: W * E].copy_(torch.from_numpy(conv_glorot_np(W, E, F, seed).reshape(W * E, F)))
            pv("conv_Wb")[W * E].zero_()
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
        W, E, F, A = self.window, self.E, self.F, self.A
        wb = pv("conv_Wb")
        out = [self.table.cpu().numpy(), self.user_table.cpu().numpy(), wb[: W * E].reshape(W, E, F).copy(), wb[W * E].copy()]
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
            pv("conv_Wb")[: W * E].copy_(t(w[2].reshape(W * E, F)))
            pv("conv_Wb")[W * E].copy_(t(w[3]))
            for name, a in zip(self._dense_names(), w[4:]):
                pv(name).copy_(t(a.reshape(pv(name).shape)))

    def count_params(self):
        W, E, F, A, U = self.window, self.E, self.F, self.A, self.U
        n = self.table.numel() + self.user_table.numel() + W * E * F + F + F * A + 2 * A + 3 * U * F + 3 * U * U + 6 * U
        return n + (2 * U * U + U if self.type == "con" else 0)

    @property
    def learning_rate(self):
        return self._lr

    @learning_rate.setter
    def learning_rate(self, lr):
        self._lr = float(lr)
        st = self.read_state()
        st.lr = self._lr
        self.state.copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8))

    def read_state(self):
        return _hip.StepState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    @property
    def loss_kind(self) -> int:
        return loss_kind_of(self.loss, self.bce_on)

    def set_article_matrix(self, matrix) -> None:
        """Keep the loader's (n_articles+1, T) token matrix in HBM: batches can then be given as article-row numbers."""
        m = np.asarray(matrix)
        if m.ndim != 2 or m.shape[1] != self.T or not np.issubdtype(m.dtype, np.integer):
            raise ValueError(f"article matrix must be integer (n_articles+1, {self.T}), got {m.dtype} {m.shape}")
        if m.size and (m.min() < 0 or m.max() >= self.V):
            raise IndexError(f"token id out of range [0, {self.V}) for the embedding table")
        self.article_matrix = torch.from_numpy(np.ascontiguousarray(m.astype(np.int32))).to(self.device)
        self._article_matrix_src = matrix

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
        Wb = P.view("conv_Wb")
        pc, pp = ctypes.c_float(self.p), ctypes.c_float(0.0)
        call("ebn_conv1d_bwd_weight_f32", pt(b.X), pt(b.dVd), pt(b.Vd), pt(b.wpart), b.splits, N, T, E, F, self.window, st, pc, pp,
             S())
        job = (_hip.FinishJob * 1)()
        job[0].kind, job[0].n_parts, job[0].rows, job[0].cols = _hip.FINISH_SPLITK, b.splits, self.window * E + 1, F
        job[0].partials, job[0].out0, job[0].ld, job[0].beta, job[0].scale = b.wpart.data_ptr(), P.g("conv_Wb").data_ptr(), F, 0.0, 1.0
        call("ebn_grad_finish_f32", job, 1, S())
        if self.train_embedding:
            call("ebn_conv1d_bwd_data_f32", pt(b.dVd), pt(b.Vd), pt(Wb), pt(b.dX), N, T, E, F, self.window, st, pc, pp, S())
            call("ebn_embedding_grad_scatter_fixed", pt(b.ids), pt(b.dX), pt(self.table_acc), R, E, self.V, st,
                 SITE_NEWS_IN if self.p > 0 else -1, pc, pt(self.range_flag), S())
        call("ebn_embedding_grad_scatter_fixed", pt(b.uidx), pt(b.dEu), pt(self.user_acc), B, U, self.n_users + 1, None, -1, f0,
             pt(self.range_flag), S())

    def _optimizer_kernels(self):
        """Keras Adam (nrms.py:69-80 form): dense parameters, then both tables straight from their fixed-point accumulators."""
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        P = self.params
        st = pt(self.state)
        f1 = ctypes.c_float(1.0)
        call("ebn_adam_keras_step_f32", pt(P.data), pt(P.grad), pt(P.m), pt(P.v), P.numel, st, BETA1, BETA2, ADAM_EPS, f1, S())
        if self.train_embedding:
            call("ebn_adam_keras_step_fixed_f32", pt(self.table), pt(self.table_acc), pt(self.table_m), pt(self.table_v),
                 self.table.numel(), st, BETA1, BETA2, ADAM_EPS, f1, pt(self.range_flag), S())
        call("ebn_adam_keras_step_fixed_f32", pt(self.user_table), pt(self.user_acc), pt(self.user_m), pt(self.user_v),
             self.user_table.numel(), st, BETA1, BETA2, ADAM_EPS, f1, pt(self.range_flag), S())

    # ------------------------------------------------------------------ host entry points
    def _uidx(self, user):
        u = user if isinstance(user, torch.Tensor) else np.asarray(user)
        return u.reshape(-1)

    def _check(self, user, his):
        if his.ndim != 3 or his.shape[1] != self.H or his.shape[2] != self.T:
            raise ValueError(f"his_input_title must be (B, {self.H}, {self.T}), got {tuple(his.shape)}")
        if user.shape[0] != his.shape[0]:
            raise ValueError(f"user_indexes must hold one id per impression: {tuple(user.shape)} vs {tuple(his.shape)}")

    def _host_ranges(self, user, *tok):
        if not isinstance(user, torch.Tensor) and user.size and (user.min() < 0 or user.max() > self.n_users):
            raise IndexError(f"user index out of range [0, {self.n_users}] for the user embedding table")
        for a in tok:
            if not isinstance(a, torch.Tensor) and a.size and (a.min() < 0 or a.max() >= self.V):
                raise IndexError(f"token id out of range [0, {self.V}) for the embedding table")

    def _put(self, dst: torch.Tensor, src, dtype=torch.int32):
        t = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(src)))
        dst.copy_(t.reshape(-1).to(device=self.device, dtype=dtype), non_blocking=True)

    def _infer(self, user, his, cands):
        """Inference-mode encoders: (user vectors (b, U), candidate news vectors (n, F))."""
        user, his = self._uidx(user), his if isinstance(his, torch.Tensor) else np.asarray(his)
        cands = cands if isinstance(cands, torch.Tensor) else np.asarray(cands)
        self._check(user, his)
        self._host_ranges(user, his, cands)
        B, n = his.shape[0], cands.shape[0]
        b = _Bufs(self, B, n, train=False)
        self._put(b.ids[: B * self.H * self.T], his)
        self._put(b.ids[B * self.H * self.T:], cands)
        self._put(b.uidx, user)
        self._encode(b, False)
        self._check_oob()
        return self._user_vec(b), b.NV[B * self.H:]

    def forward(self, user, his, pred, mode="softmax"):
        """(B,1) users, (B,H,T), (B,C,T) ids -> (probs (B,C), scores (B,C)) device tensors, inference mode."""
        pred = pred if isinstance(pred, torch.Tensor) else np.asarray(pred)
        if pred.ndim != 3 or pred.shape[2] != self.T:
            raise ValueError(f"pred_input_title must be (B, C, {self.T}), got {tuple(pred.shape)}")
        B, C = pred.shape[0], pred.shape[1]
        user_vec, cand = self._infer(user, his, pred.reshape(B * C, self.T))
        scores, probs = torch.empty(B, C, device=self.device), torch.empty(B, C, device=self.device)
        _hip.call("ebn_score_fwd_f32", _hip.ptr(cand), _hip.ptr(user_vec), _hip.ptr(scores), _hip.ptr(probs), B, C, self.F,
                  0 if mode == "softmax" else 1, _hip.stream_handle())
        return probs, scores

    def eval_loss(self, user, his, pred, y):
        """Inference-mode forward + the compiled loss: (loss[1], probs (B,C))."""
        pred = np.asarray(pred) if not isinstance(pred, torch.Tensor) else pred
        B, C = pred.shape[0], pred.shape[1]
        user_vec, cand = self._infer(user, his, pred.reshape(B * C, self.T))
        scores, probs = torch.empty(B, C, device=self.device), torch.empty(B, C, device=self.device)
        S = _hip.stream_handle
        _hip.call("ebn_score_fwd_f32", _hip.ptr(cand), _hip.ptr(user_vec), _hip.ptr(scores), _hip.ptr(probs), B, C, self.F, 0, S())
        labels = torch.as_tensor(np.ascontiguousarray(np.asarray(y, dtype=np.float32))).to(self.device).reshape(B, C).contiguous()
        rows, junk_c, junk_u = torch.empty(B, device=self.device), torch.empty(B * C, self.F, device=self.device), torch.empty(B, self.F, device=self.device)
        loss = torch.empty(1, device=self.device)
        _hip.call("ebn_score_loss_bwd_f32", _hip.ptr(cand), _hip.ptr(user_vec), _hip.ptr(scores), _hip.ptr(labels), _hip.ptr(rows),
                  _hip.ptr(junk_c), _hip.ptr(junk_u), B, C, self.F, self.loss_kind, ctypes.c_float(1.0 / B), S())
        _hip.call("ebn_sum_f32", _hip.ptr(rows), B, ctypes.c_float(1.0), _hip.ptr(loss), 0, S())
        return loss, probs

    def pair_scores(self, user, his, cands, cand_imp, sigmoid=True):
        """act(cand_i . user[cand_imp[i]]) for candidates (n, T) of impressions (user (b,), his (b,H,T)) -- scorer.predict."""
        user_vec, cand = self._infer(user, his, cands)
        n = cand.shape[0]
        out = torch.empty(n, device=self.device)
        ui = torch.from_numpy(np.ascontiguousarray(cand_imp, dtype=np.int32)).to(self.device)
        ni = torch.arange(n, dtype=torch.int32, device=self.device)
        _hip.call("ebn_pair_score_f32", _hip.ptr(user_vec), _hip.ptr(cand), _hip.ptr(ui), _hip.ptr(ni), _hip.ptr(out), n, self.F,
                  1 if sigmoid else 0, _hip.stream_handle())
        return out

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
        n = cand_idx.shape[0]
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
        user_vec = self._user_vectors_indexed(cache, user, his_idx)
        ci, ui = i32(cand_idx), i32(np.asarray(cand_imp).reshape(-1))
        out = torch.empty(n, device=self.device)
        _hip.call("ebn_pair_score_f32", _hip.ptr(user_vec), _hip.ptr(cache.news_all), _hip.ptr(ui), _hip.ptr(ci), _hip.ptr(out), n,
                  self.F, 1 if sigmoid else 0, _hip.stream_handle())
        self._check_oob()
        return out

    def _check_oob(self):
        flags = torch.cat([self.oob_flag, self.user_oob_flag, self.range_flag, self.row_oob_flag])
        oob, uoob, rng_bad, row_bad = (int(v) for v in flags.cpu().tolist())
        if oob or uoob or rng_bad or row_bad:
            self.oob_flag.zero_()
            self.user_oob_flag.zero_()
            self.range_flag.zero_()
            self.row_oob_flag.zero_()
        if row_bad:
            raise IndexError("article row out of range for the encoded catalogue")
        if uoob:
            raise IndexError(f"user index out of range [0, {self.n_users}] for the user embedding table")
        if oob:
            raise IndexError(f"token id out of range [0, {self.V}) for the embedding table")
        if rng_bad:
            raise FloatingPointError("embedding gradient left the range of the deterministic fixed-point accumulator: the run has "
                                     "diverged")

    def check_oob(self):
        """One host read of the device flags (fit() calls it once per epoch): ids outside a table raise IndexError."""
        self._check_oob()

    def train_step(self, user, his, pred, y, return_probs=False, indexed=False):
        """One optimizer step; returns the batch loss as a 1-element device tensor (no host sync).  The launch sequence of a
        (B, C) shape is captured once into one hipGraph on the current stream and replayed (step-dependent scalars live in
        the device step state).  indexed: his (B,H) / pred (B,C) are article-row numbers of set_article_matrix()'s matrix."""
        user = self._uidx(user)
        his = his if isinstance(his, torch.Tensor) else np.asarray(his)
        pred = pred if isinstance(pred, torch.Tensor) else np.asarray(pred)
        B, C = his.shape[0], pred.shape[1]
        if user.shape[0] != B or pred.shape[0] != B:
            raise ValueError(f"batch sizes differ: user {tuple(user.shape)}, his {tuple(his.shape)}, pred {tuple(pred.shape)}")
        if indexed:
            if self.article_matrix is None:
                raise ValueError("indexed batches need set_article_matrix() first")
            if his.ndim != 2 or his.shape[1] != self.H or pred.ndim != 2:
                raise ValueError(f"indexed batches must be (B, {self.H}) and (B, C), got {tuple(his.shape)} {tuple(pred.shape)}")
            self._host_ranges(user)
        else:
            self._check(user, his)
            if pred.ndim != 3 or pred.shape[2] != self.T:
                raise ValueError(f"pred_input_title must be (B, C, {self.T}), got {tuple(pred.shape)}")
            self._host_ranges(user, his, pred)
        b, expand = self._stage(user, his, pred, y, indexed)
        key = (B, C, bool(indexed), self.type, self.loss_kind, self.train_embedding)
        if self.use_graph:
            g = self._graphs.get(key)
            if g is None:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with _hip.capture(g):
                    self._train_kernels(b, C, expand)
                self._graphs[key] = g
            g.replay()
        else:
            self._train_kernels(b, C, expand)
        if return_probs:
            return self.loss_dev, b.probs.view(B, C), b.labels.view(B, C)
        return self.loss_dev

    def _stage(self, user, his, pred, y, indexed):
        """The step's static buffers for (B, C), filled with the batch: (buffers, article rows to expand or None)."""
        B, C = his.shape[0], pred.shape[1]
        b = self._bufs.get((B, C))
        if b is None:
            b = self._bufs[(B, C)] = _Bufs(self, B, B * C, train=True)
            b.art = torch.empty(b.N, dtype=torch.int32, device=self.device)
        if indexed:
            self._put(b.art[: B * self.H], his)
            self._put(b.art[B * self.H:], pred)
        else:
            self._put(b.ids[: B * self.H * self.T], his)
            self._put(b.ids[B * self.H * self.T:], pred)
        self._put(b.uidx, user)
        self._put(b.labels, y, torch.float32)
        return b, (b.art if indexed else None)
