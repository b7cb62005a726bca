"""Device engine of the MI355X NPA path (reference npa.py, layers.py:312-339), one rank.

Per impression b with user index u_b (npa.py:60-190):
  e_b = user_emb[u_b];  qn_b = e_b.Wn + bn (the news encoder's Dense, shared by history and candidate titles);  qu_b = e_b.Wu + bu
  title of impression b:  X = Dropout(p)(emb[tokens]) -> Vd = Dropout(0.2)(Dropout(p)(relu(conv1d_same(X) + b_c)))
                          -> U = tanh(Vd.Wa + ba), w = softmax_l(qn_b . U_l), news = sum_l w_l Vd_l
  user_b = PAP_u(Dropout(0.2)(news of the H history titles), qu_b);  scores = cand . user_b -> softmax + compiled loss
Candidates are encoded with their impression's query, so a training step encodes every title per impression.  At inference
the user reaches a title only through the logits qn_b . U_l: Vd and U are per article, and scorer.predict keeps them per row of
the loader's article matrix (encode_catalogue) and pools each (impression, article) pair from them (score_cached).

Data layout in HBM (fp32 row-major):
  table        (V, E)              word embeddings (trainable: fixed-point gradient accumulator + fused Adam sweep)
  user_table   (n_users + 1, Du)   zeros-initialised user embeddings (same gradient path, dropout-free)
  dense        flat buffer         conv_Wb (window*E + 1, F) = Conv1D kernel rows | bias row, then n_Wa, n_ba, n_Wq, n_bq,
                                   u_Wa, u_ba, u_Wq, u_bq -> one Adam launch per step
  titles       N = B*(H+C) per step, history titles first (b*H + h), then candidates (B*H + b*C + c); q_idx[n] = impression

Shared with the other engines and defined in _engine_base.py: constructor scaffolding, step state, flags (_check_oob), staging and
train_step, forward / eval_loss / pair_scores, the Adam launches, the Conv1D backward block (UserTableEngine <- ConvEngineBase).  Here:
buffers, shapes, weight order, the encoder, the backward up to the Conv1D, and scoring from an encoded catalogue.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from ebrec import _hip

from ._engine_base import BETA1, BETA2, ConvView, UserTableEngine, glorot_uniform_np

SITE_NEWS_IN, SITE_CONV, SITE_NEWS_PAP, SITE_USER_PAP = 0, 2, 3, 4
PAP_DROPOUT = 0.2  # layers.py:324: a fixed rate, not hparams.dropout

WEIGHT_NAMES = ["news.emb", "user.emb", "news.conv.W", "news.conv.b", "news.query.W", "news.query.b", "news.pap.W", "news.pap.b",
                "user.query.W", "user.query.b", "user.pap.W", "user.pap.b"]


class _Bufs:
    """Activations and backward scratch of one (B, H, n_cand) shape."""

    def __init__(self, eng, B, n_cand, cand_imp, train):
        dev, H, T, E, F, A, Du = eng.device, eng.H, eng.T, eng.E, eng.F, eng.A, eng.Du
        f = lambda *s: torch.empty(*s, device=dev)
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
        N = B * H + n_cand
        R = N * T
        self.B, self.n_cand, self.N, self.R = B, n_cand, N, R
        self.ids, self.uidx = i32(R), i32(B)
        q = np.concatenate([np.repeat(np.arange(B), H), np.asarray(cand_imp).reshape(-1)]).astype(np.int32)
        self.q_idx = torch.from_numpy(q).to(dev)
        self.iota = torch.arange(B, dtype=torch.int32, device=dev)
        self.X, self.Vd, self.U, self.w = f(R, E), f(R, F), f(R, A), f(R)
        self.NV, self.NVd_h = f(N, F), f(B * H, F)
        self.Eu, self.Qn, self.Qu = f(B, Du), f(B, A), f(B, A)
        self.Uu, self.wu, self.user = f(B * H, A), f(B * H), f(B, F)
        self.ones = torch.ones(max(R, B * H, B), device=dev)
        if train:
            self.labels, self.scores, self.probs = f(n_cand), f(n_cand), f(n_cand)
            self.loss_rows = f(B)
            self.dNV, self.duser, self.dQu, self.dQn = f(N, F), f(B, F), f(B, A), f(B, A)
            self.dq_seq, self.dVd, self.dX, self.dEu = f(N, A), f(R, F), f(R, E), f(B, Du)
            lib = _hip.lib()
            self.splits = int(lib.ebn_conv1d_wgrad_splits(N, T, E, F, eng.window))
            self.wpart = f(max(int(lib.ebn_conv1d_wgrad_workspace_floats(N, T, E, F, eng.window, self.splits)), 1))
            wsf = lib.ebn_gemm_workspace_floats
            self.ws = f(max(int(wsf(F, A, R)), int(wsf(1, A, R)), int(wsf(R, F, A)), int(wsf(F, A, B * H)),
                            int(wsf(B * H, F, A)), 1))


class NPAEngine(UserTableEngine):
    MODEL = "NPA"

    def __init__(self, table: np.ndarray, n_users: int, title_size: int, history_size: int, filter_num: int, window_size: int,
                 attention_hidden_dim: int, user_emb_dim: int, dropout: float, learning_rate: float, loss: str, seed=None,
                 train_embedding: bool = True, device=None, process_group=None, bce_on: str = "logits"):
        self._require_one_rank(process_group)
        self._init_table(table, device)
        self.n_users, self.Du = int(n_users), int(user_emb_dim)
        self.T, self.H, self.F, self.A, self.window = int(title_size), int(history_size), int(filter_num), int(attention_hidden_dim), int(window_size)
        if self.E % 4 or self.F % 4:
            raise ValueError(f"word_emb_dim ({self.E}) and filter_num ({self.F}) must be multiples of 4 for the HIP Conv1D")
        W, E, F, A, Du = self.window, self.E, self.F, self.A, self.Du
        shapes = {"conv_Wb": (W * E + 1, F), "n_Wa": (F, A), "n_ba": (A,), "n_Wq": (Du, A), "n_bq": (A,),
                  "u_Wa": (F, A), "u_ba": (A,), "u_Wq": (Du, A), "u_bq": (A,)}
        self._init_state(shapes, Du, dropout, learning_rate, loss, seed, train_embedding, bce_on)  # user table: npa.py:180-185
        self._init_weights(seed)

    # ------------------------------------------------------------------ parameters
    def _init_weights(self, seed):
        pv = self.params.view
        F, A, Du = self.F, self.A, self.Du
        self._conv_init("conv_Wb", seed)
        with torch.no_grad():
            for name, shape in (("n_Wa", (F, A)), ("n_Wq", (Du, A)), ("u_Wa", (F, A)), ("u_Wq", (Du, A))):
                pv(name).copy_(torch.from_numpy(glorot_uniform_np(shape, seed)))
            for name in ("n_ba", "n_bq", "u_ba", "u_bq"):
                pv(name).zero_()

    def weight_names(self):
        return list(WEIGHT_NAMES)

    def get_weights(self):
        pv = lambda n: self.params.view(n).cpu().numpy()
        return ([self.table.cpu().numpy(), self.user_table.cpu().numpy()] + self._conv_get("conv_Wb")
                + [pv(n) for n in ("n_Wq", "n_bq", "n_Wa", "n_ba", "u_Wq", "u_bq", "u_Wa", "u_ba")])

    def set_weights(self, weights):
        if len(weights) != len(WEIGHT_NAMES):
            raise ValueError(f"expected {len(WEIGHT_NAMES)} weight arrays ({', '.join(WEIGHT_NAMES)}), got {len(weights)}")
        w = [np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in weights]
        W, E, F = self.window, self.E, self.F
        want = [tuple(self.table.shape), tuple(self.user_table.shape), (W, E, F), (F,)]
        for a, s, n in zip(w[:4], want, WEIGHT_NAMES):
            if a.shape != s:
                raise ValueError(f"{n}: shape {a.shape} != {s}")
        t = lambda a: torch.from_numpy(a)
        with torch.no_grad():
            self.table.copy_(t(w[0]))
            self.user_table.copy_(t(w[1]))
            pv = self.params.view
            self._conv_set("conv_Wb", w[2], w[3])
            for name, a in zip(("n_Wq", "n_bq", "n_Wa", "n_ba", "u_Wq", "u_bq", "u_Wa", "u_ba"), w[4:]):
                pv(name).copy_(t(a.reshape(pv(name).shape)))

    def count_params(self):
        W, E, F, A, Du = self.window, self.E, self.F, self.A, self.Du
        return self.table.numel() + self.user_table.numel() + W * E * F + F + 2 * (F * A + A + Du * A + A)

    # ------------------------------------------------------------------ kernels
    def _encode(self, b: _Bufs, train: bool, expand=None):
        """Forward of every title and user of the buffers' batch (ids / uidx already staged); training: dropout on."""
        S = _hip.stream_handle
        lib_call = _hip.call
        P, pt = self.params, _hip.ptr
        st = pt(self.state) if train else None
        B, N, R, T, E, F, A, Du, H = b.B, b.N, b.R, self.T, self.E, self.F, self.A, self.Du, self.H
        p_in = self.p if train else 0.0
        p_pap = PAP_DROPOUT if train else 0.0
        if expand is not None:  # article-row numbers -> token ids on the device (dataloader.py:169-179)
            lib_call("ebn_expand_titles_i32", pt(expand), pt(self.article_matrix), pt(b.ids), N, T, self.article_matrix.shape[0],
                     pt(self.oob_flag), S())
        lib_call("ebn_gather_rows_f32", pt(b.ids), pt(self.table), pt(b.X), R, E, self.V, st, SITE_NEWS_IN if p_in > 0 else -1,
                 ctypes.c_float(p_in), pt(self.oob_flag), S())
        lib_call("ebn_gather_rows_f32", pt(b.uidx), pt(self.user_table), pt(b.Eu), B, Du, self.n_users + 1, None, -1,
                 ctypes.c_float(0.0), pt(self.user_oob_flag), S())
        for Q, Wq, bq in ((b.Qn, "n_Wq", "n_bq"), (b.Qu, "u_Wq", "u_bq")):  # Dense(A)(u_emb) = 1.bq + e.Wq
            lib_call("ebn_gemm_f32", 0, 0, B, A, 1, ctypes.c_float(1.0), pt(b.ones), 1, pt(P.view(bq)), A, ctypes.c_float(0.0),
                     pt(Q), A, S())
            lib_call("ebn_gemm_f32", 0, 0, B, A, Du, ctypes.c_float(1.0), pt(b.Eu), Du, pt(P.view(Wq)), A, ctypes.c_float(1.0),
                     pt(Q), A, S())
        Wb = P.view("conv_Wb")
        lib_call("ebn_conv1d_fwd_f32", pt(b.X), pt(Wb), pt(Wb[self.window * E]), pt(b.Vd), N, T, E, F, self.window, st,
                 SITE_CONV if p_in > 0 else -1, ctypes.c_float(p_in), SITE_NEWS_PAP, ctypes.c_float(p_pap), S())
        lib_call("ebn_gemm_f32", 0, 0, R, A, F, ctypes.c_float(1.0), pt(b.Vd), F, pt(P.view("n_Wa")), A, ctypes.c_float(0.0),
                 pt(b.U), A, S())
        lib_call("ebn_pap_fwd_f32", pt(b.U), pt(P.view("n_ba")), pt(b.Qn), pt(b.q_idx), B, pt(b.Vd), pt(b.NV), pt(b.w),
                 pt(b.NVd_h), B * H, N, T, F, A, st, SITE_USER_PAP, ctypes.c_float(p_pap), S())
        lib_call("ebn_gemm_f32", 0, 0, B * H, A, F, ctypes.c_float(1.0), pt(b.NVd_h), F, pt(P.view("u_Wa")), A,
                 ctypes.c_float(0.0), pt(b.Uu), A, S())
        lib_call("ebn_pap_fwd_f32", pt(b.Uu), pt(P.view("u_ba")), pt(b.Qu), pt(b.iota), B, pt(b.NVd_h), pt(b.user), pt(b.wu),
                 None, 0, B, H, F, A, None, -1, ctypes.c_float(0.0), S())

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
        B, N, R, T, E, F, A, Du, H = b.B, b.N, b.R, self.T, self.E, self.F, self.A, self.Du, self.H
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        call("ebn_step_advance", st, BETA1, BETA2, S())
        self._encode(b, True, expand)
        cand = b.NV[B * H:]
        call("ebn_score_loss_train_f32", pt(cand), pt(b.user), pt(b.labels), pt(b.scores), pt(b.probs), pt(b.loss_rows),
             pt(self.loss_dev), pt(b.dNV[B * H:]), pt(b.duser), B, C, F, self.loss_kind, ctypes.c_float(1.0 / B), S())
        # user-level pooling backward: Uu <- d(pre-tanh), dQu (one sequence per impression)
        call("ebn_pap_bwd_f32", pt(b.Uu), pt(b.Qu), pt(b.iota), B, pt(b.NVd_h), pt(b.wu), pt(b.duser), None, pt(b.dQu), 0, B, H,
             F, A, None, -1, f0, S())
        ws, wsn = pt(b.ws), b.ws.numel()
        call("ebn_gemm_f32_ws", 1, 0, F, A, B * H, f1, pt(b.NVd_h), F, pt(b.Uu), A, f0, pt(P.g("u_Wa")), A, ws, wsn, S())
        call("ebn_gemm_f32_ws", 0, 0, 1, A, B * H, f1, pt(b.ones), B * H, pt(b.Uu), A, f0, pt(P.g("u_ba")), A, ws, wsn, S())
        # d(history news vectors, after the user pooling's dropout) = dpre_u.Wu_a^T + wu (x) duser
        call("ebn_gemm_f32_rank1", B * H, F, A, f1, pt(b.Uu), A, pt(P.view("u_Wa")), A, pt(b.dNV), F, pt(b.wu), pt(b.duser), F, H,
             ws, wsn, S())
        # news-level pooling backward (the user pooling's input dropout is undone on the history rows in place)
        call("ebn_pap_bwd_f32", pt(b.U), pt(b.Qn), pt(b.q_idx), B, pt(b.Vd), pt(b.w), pt(b.dNV), None, pt(b.dq_seq), B * H, N, T,
             F, A, st, SITE_USER_PAP, ctypes.c_float(PAP_DROPOUT), S())
        call("ebn_pap_dq_reduce_f32", pt(b.dq_seq), pt(b.q_idx), N, pt(b.dQn), B, A, S())
        call("ebn_gemm_f32_ws", 1, 0, F, A, R, f1, pt(b.Vd), F, pt(b.U), A, f0, pt(P.g("n_Wa")), A, ws, wsn, S())
        call("ebn_gemm_f32_ws", 0, 0, 1, A, R, f1, pt(b.ones), R, pt(b.U), A, f0, pt(P.g("n_ba")), A, ws, wsn, S())
        call("ebn_gemm_f32_rank1", R, F, A, f1, pt(b.U), A, pt(P.view("n_Wa")), A, pt(b.dVd), F, pt(b.w), pt(b.dNV), F, T, ws, wsn,
             S())
        self._conv_backward(ConvView(b.ids, b.X, b.Vd, b.dVd, b.dX, b.wpart, b.splits, T, "conv_Wb", SITE_NEWS_IN), N, self.p, PAP_DROPOUT)
        # the two query Dense layers and the user embedding
        for dQ, Wq, bq in ((b.dQn, "n_Wq", "n_bq"), (b.dQu, "u_Wq", "u_bq")):
            call("ebn_gemm_f32", 1, 0, Du, A, B, f1, pt(b.Eu), Du, pt(dQ), A, f0, pt(P.g(Wq)), A, S())
            call("ebn_gemm_f32", 0, 0, 1, A, B, f1, pt(b.ones), B, pt(dQ), A, f0, pt(P.g(bq)), A, S())
        call("ebn_gemm_f32", 0, 1, B, Du, A, f1, pt(b.dQn), A, pt(P.view("n_Wq")), A, f0, pt(b.dEu), Du, S())
        call("ebn_gemm_f32", 0, 1, B, Du, A, f1, pt(b.dQu), A, pt(P.view("u_Wq")), A, f1, pt(b.dEu), Du, S())
        call("ebn_embedding_grad_scatter_fixed", pt(b.uidx), pt(b.dEu), pt(self.user_acc), B, Du, self.n_users + 1, None, -1, f0,
             pt(self.range_flag), S())

    # ------------------------------------------------------------------ hooks of the shared host entry points
    def _new_bufs(self, B, n_cand, cand_imp, train):
        return _Bufs(self, B, n_cand, cand_imp, train)

    def _user_vec(self, b: _Bufs):
        return b.user

    # ------------------------------------------------------------------ scoring from a once-encoded catalogue
    def catalogue_bytes(self, n_rows) -> int:
        """HBM bytes of encode_catalogue()'s two arrays for n_rows titles: n_rows * T * (F + A) fp32."""
        return int(n_rows) * self.T * (self.F + self.A) * 4

    def encode_catalogue(self, tokens, chunk=4096):
        """Everything the news encoder computes from the article alone, for the CURRENT weights (build it per predict, never keep it
        on the model): tokens (n_rows, T) -> cache with Vd_all (n_rows, T, F) = relu(conv1d_same(emb[tokens]) + b_c) and
        Ua_all (n_rows, T, A) = tanh(Vd.Wa + ba), inference mode (no dropout).  The user enters the news vector only through the
        logits q . Ua_l, which score_cached computes.  Encoded in chunks: the gathered-token scratch is that of `chunk` titles
        whatever n_rows is; the conv and the attention GEMM write straight into the chunk's slices."""
        tokens = np.asarray(tokens)
        if tokens.ndim != 2 or tokens.shape[1] != self.T:
            raise ValueError(f"catalogue tokens must be (n_rows, {self.T}), got {tuple(tokens.shape)}")
        self._host_ranges(np.zeros(0, np.int64), tokens)
        S = _hip.stream_handle
        call, pt, P = _hip.call, _hip.ptr, self.params
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        n_rows, T, E, F, A = tokens.shape[0], self.T, self.E, self.F, self.A
        dev = self.device
        Vd_all, Ua_all = torch.empty(n_rows, T, F, device=dev), torch.empty(n_rows, T, A, device=dev)
        chunk = max(1, min(int(chunk), n_rows))
        ids, X = torch.empty(chunk * T, dtype=torch.int32, device=dev), torch.empty(chunk * T, E, device=dev)
        Wb = P.view("conv_Wb")
        for s in range(0, n_rows, chunk):
            n = min(chunk, n_rows - s)
            R = n * T
            self._put(ids[:R], tokens[s:s + n])
            call("ebn_gather_rows_f32", pt(ids), pt(self.table), pt(X), R, E, self.V, None, -1, f0, pt(self.oob_flag), S())
            call("ebn_conv1d_fwd_f32", pt(X), pt(Wb), pt(Wb[self.window * E]), pt(Vd_all[s]), n, T, E, F, self.window, None, -1, f0,
                 SITE_NEWS_PAP, f0, S())
            call("ebn_gemm_f32", 0, 0, R, A, F, f1, pt(Vd_all[s]), F, pt(P.view("n_Wa")), A, f0, pt(Ua_all[s]), A, S())
            call("ebn_bias_tanh_rows_f32", pt(Ua_all[s]), pt(P.view("n_ba")), R, A, S())
        self._check_oob()
        return SimpleNamespace(Vd_all=Vd_all, Ua_all=Ua_all, n_rows=n_rows)

    def _indexed_users(self, user, his_idx):
        """(user (b,) indexes, his_idx (b, H) rows) of an indexed batch, checked on the host"""
        user = self._uidx(user)
        his_idx = np.asarray(his_idx)
        if his_idx.ndim != 2 or his_idx.shape[1] != self.H or user.shape[0] != his_idx.shape[0]:
            raise ValueError(f"indexed batches need user (b,) and his_idx (b, {self.H}), got {tuple(user.shape)} {tuple(his_idx.shape)}")
        self._host_ranges(user)
        return user, his_idx

    def _user_state(self, cache, user, his_idx):
        """The launches of user_state_cached() on checked arguments; the flags are left for the caller to read."""
        S = _hip.stream_handle
        call, pt, P = _hip.call, _hip.ptr, self.params
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        B, T, F, A, Du, H = his_idx.shape[0], self.T, self.F, self.A, self.Du, self.H
        dev = self.device
        f = lambda *s: torch.empty(*s, device=dev)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        uidx, hi = i32(user), i32(his_idx.reshape(-1))
        q_his = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(H)
        iota = torch.arange(B, dtype=torch.int32, device=dev)
        Eu, Qn, Qu, ones = f(B, Du), f(B, A), f(B, A), torch.ones(max(B, 1), device=dev)
        NV_h, Uu, wu, user_vec = f(B * H, F), f(B * H, A), f(B * H), f(B, F)
        call("ebn_gather_rows_f32", pt(uidx), pt(self.user_table), pt(Eu), B, Du, self.n_users + 1, None, -1, f0,
             pt(self.user_oob_flag), S())
        for Q, Wq, bq in ((Qn, "n_Wq", "n_bq"), (Qu, "u_Wq", "u_bq")):  # Dense(A)(u_emb) = 1.bq + e.Wq, as _encode
            call("ebn_gemm_f32", 0, 0, B, A, 1, f1, pt(ones), 1, pt(P.view(bq)), A, f0, pt(Q), A, S())
            call("ebn_gemm_f32", 0, 0, B, A, Du, f1, pt(Eu), Du, pt(P.view(Wq)), A, f1, pt(Q), A, S())
        call("ebn_pap_indexed_f32", pt(cache.Ua_all), pt(cache.Vd_all), cache.n_rows, pt(hi), pt(Qn), pt(q_his), B, pt(NV_h), None,
             None, 0, pt(self.row_oob_flag), B * H, T, F, A, S())
        call("ebn_gemm_f32", 0, 0, B * H, A, F, f1, pt(NV_h), F, pt(P.view("u_Wa")), A, f0, pt(Uu), A, S())
        call("ebn_pap_fwd_f32", pt(Uu), pt(P.view("u_ba")), pt(Qu), pt(iota), B, pt(NV_h), pt(user_vec), pt(wu), None, 0, B, H, F, A,
             None, -1, f0, S())
        return user_vec, Qn

    def user_state_cached(self, cache, user, his_idx):
        """Everything of an indexed batch that depends on the impression alone -> (user_vec (b, F), Qn (b, A)): user (b,) user
        indexes, his_idx (b, H) rows of the cache.  User-table gather -> the two query Dense -> indexed pooling of the b*H history
        slots -> the user stage of _encode, unchanged.  Qn is the news-level query a candidate of the impression is pooled with."""
        user, his_idx = self._indexed_users(user, his_idx)
        out = self._user_state(cache, user, his_idx)
        self._check_oob()
        return out

    def score_cached(self, cache, user, his_idx, cand_idx, cand_imp, sigmoid=True):
        """act(news(cand_i | user[cand_imp[i]]) . user_vec[cand_imp[i]]) of one indexed batch: user (b,) user indexes, his_idx (b, H) /
        cand_idx (n,) rows of the cache, cand_imp (n,) the impression of each candidate.  user_state_cached()'s launches -> indexed
        pooling of the candidates fused with the score (the candidate vectors are not written)."""
        user, his_idx = self._indexed_users(user, his_idx)
        cand_idx, cand_imp = np.asarray(cand_idx).reshape(-1), np.asarray(cand_imp).reshape(-1)
        if cand_idx.shape != cand_imp.shape:
            raise ValueError(f"one impression per candidate: {cand_idx.shape} vs {cand_imp.shape}")
        if cand_imp.size and (cand_imp.min() < 0 or cand_imp.max() >= his_idx.shape[0]):
            raise IndexError(f"candidate impression out of range [0, {his_idx.shape[0]})")
        call, pt = _hip.call, _hip.ptr
        B, n = his_idx.shape[0], cand_idx.shape[0]
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
        ci, rows, out = i32(cand_idx), i32(cand_imp), torch.empty(n, device=self.device)
        user_vec, Qn = self._user_state(cache, user, his_idx)
        if n:
            call("ebn_pap_indexed_f32", pt(cache.Ua_all), pt(cache.Vd_all), cache.n_rows, pt(ci), pt(Qn), pt(rows), B, None, pt(user_vec),
                 pt(out), 1 if sigmoid else 0, pt(self.row_oob_flag), n, self.T, self.F, self.A, _hip.stream_handle())
        self._check_oob()
        return out
