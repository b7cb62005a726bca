"""Device engine of the MI355X NAML path (reference naml.py, layers.py:55-81), one rank.

Per article (naml.py _build_newsencoder):
  title:    Xt = Dropout(p)(emb[title]) -> Vt = Dropout(p)(relu(conv1d_same(Xt; title conv) + bt)) -> AttLayer2 -> [F]
  body:     the same on the body tokens with its own Conv1D and AttLayer2 weights (the word table is shared)
  vert:     relu(vert_emb[vert].Wv + bv) -> [F]  (no dropout);  subvert: the same with its own table and Dense
  news    = AttLayer2 over the 4 views [title, body, vert, subvert]
Per impression: user = AttLayer2 over the H history news vectors (encoded with dropout in training);
  train: softmax(cand . user) + compiled loss;  scorer: sigmoid(cand_one . user).
The news encoder does not depend on the user, and neither does the user encoder's logit of a history item (an unmasked
AttLayer2: a = exp(tanh(x.W + b).q) per article): scorer.predict over an eval loader encodes the loader's article catalogue
once (encode_catalogue) and scores each batch with one indexed pooling-and-scoring launch (score_cached).

Data layout in HBM (fp32 row-major):
  table      (V, E)           word embeddings (trainable: fixed-point gradient accumulator + fused Adam sweep)
  dense      flat buffer      t_conv / b_conv (window*E + 1, F) = Conv1D kernel rows | bias row, t_aW, t_ab, t_aq, b_aW, b_ab,
                              b_aq, v_emb (vert_num, Kv), v_Wb (Kv + 1, F), s_emb, s_Wb, va_W, va_b, va_q, u_W, u_b, u_q
                              -> one Adam launch per step (the two small tables included: Keras' dense Adam on an Embedding)
  articles   N = B*(H+C) per step, history first (b*H + h), then candidates (B*H + b*C + c)
  views      Vw (4, N, F) view-major: the title / body poolings write Vw[0] / Vw[1] contiguously, the view x.W is one GEMM

Shared with the other engines and defined in _engine_base.py (ConvEngineBase): constructor scaffolding, step state, the flag read
(_check_oob over this engine's FLAGS), capture-or-replay of a step, the Adam launches, the Conv1D weight-gradient / finishing block and
the eval_loss / pair_scores launch tails.  Here: buffers, shapes, weight order, the encoders, the backward, staging of the eight input
arrays, and scoring from an encoded catalogue.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from ebrec import _hip

from ._engine_base import (BETA1, BETA2, RANGE_FLAG, ROW_FLAG, TOKEN_FLAG, ConvEngineBase, ConvView, glorot_uniform_np, pair_score_tail,
                           score_loss_tail)

SITE_TITLE_IN, SITE_TITLE_CONV, SITE_BODY_IN, SITE_BODY_CONV = 0, 2, 5, 6
N_VIEWS = 4

WEIGHT_NAMES = ["news.emb", "news.title.conv.W", "news.title.conv.b", "news.title.att.W", "news.title.att.b", "news.title.att.q",
                "news.body.conv.W", "news.body.conv.b", "news.body.att.W", "news.body.att.b", "news.body.att.q", "news.vert.emb",
                "news.vert.dense.W", "news.vert.dense.b", "news.subvert.emb", "news.subvert.dense.W", "news.subvert.dense.b",
                "news.view_att.W", "news.view_att.b", "news.view_att.q", "user.att.W", "user.att.b", "user.att.q"]
# (flat-buffer name of each AttLayer2 / Dense weight after the word table and the two convolutions, in WEIGHT_NAMES order)
_ATT = {"t": ("t_aW", "t_ab", "t_aq"), "b": ("b_aW", "b_ab", "b_aq"), "va": ("va_W", "va_b", "va_q"), "u": ("u_W", "u_b", "u_q")}


class _Bufs:
    """Activations and backward scratch of one (B, n_cand) shape."""

    def __init__(self, eng, B, n_cand, train):
        dev, H, T, Tb, E, F, A = eng.device, eng.H, eng.T, eng.Tb, eng.E, eng.F, eng.A
        f = lambda *s: torch.empty(*s, device=dev)
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
        N = B * H + n_cand
        BH = B * H
        Rt, Rb = N * T, N * Tb
        self.B, self.n_cand, self.N, self.Rt, self.Rb = B, n_cand, N, Rt, Rb
        self.ids_t, self.ids_b, self.cat_v, self.cat_s = i32(Rt), i32(Rb), i32(N), i32(N)
        self.Xt, self.Vt, self.Ut, self.wt = f(Rt, E), f(Rt, F), f(Rt, A), f(Rt)
        self.Xb, self.Vb, self.Ub, self.wb = f(Rb, E), f(Rb, F), f(Rb, A), f(Rb)
        self.Vw, self.Uv, self.wv, self.NV = f(N_VIEWS, N, F), f(N_VIEWS * N, A), f(N_VIEWS * N), f(N, F)
        self.Uu, self.wu, self.user = f(BH, A), f(BH), f(B, F)
        if train:
            lib = _hip.lib()
            self.labels, self.scores, self.probs = f(n_cand), f(n_cand), f(n_cand)
            self.loss_rows = f(B)
            self.dNV, self.duser, self.deu = f(N, F), f(B, F), f(BH)
            self.dVw, self.dew = f(N_VIEWS, N, F), f(N_VIEWS * N)
            self.dVt, self.det, self.dXt = f(Rt, F), f(Rt), f(Rt, E)
            self.dVb, self.deb, self.dXb = f(Rb, F), f(Rb), f(Rb, E)
            apl = lib.ebn_attpool_partials_len
            self.part = f(max(int(apl(Rt, A)), int(apl(Rb, A)), int(apl(N_VIEWS * N, A)), int(apl(BH, A)), 1))
            self.head_partials = f(max(int(lib.ebn_user_head_partials_len(B, A)), 1))
            self.cpart = f(max(int(lib.ebn_naml_catview_partials_len(N, eng.Kv, eng.Ks, F)), 1))
            self.splits_t = int(lib.ebn_conv1d_wgrad_splits(N, T, E, F, eng.window))
            self.splits_b = int(lib.ebn_conv1d_wgrad_splits(N, Tb, E, F, eng.window))
            self.wpart_t = f(max(int(lib.ebn_conv1d_wgrad_workspace_floats(N, T, E, F, eng.window, self.splits_t)), 1))
            self.wpart_b = f(max(int(lib.ebn_conv1d_wgrad_workspace_floats(N, Tb, E, F, eng.window, self.splits_b)), 1))
            wsf = lib.ebn_gemm_workspace_floats
            self.ws = f(max(int(wsf(F, A, Rt)), int(wsf(F, A, Rb)), int(wsf(F, A, N_VIEWS * N)), int(wsf(F, A, BH)),
                            int(wsf(Rt, F, A)), int(wsf(Rb, F, A)), int(wsf(BH, F, A)), int(wsf(N_VIEWS * N, F, A)), 1))


class NAMLEngine(ConvEngineBase):
    MODEL = "NAML"
    FLAGS = (ROW_FLAG, TOKEN_FLAG, ("cat_oob_flag", IndexError, "category id out of range: vert ids must lie in [0, {e.n_vert}), "
                                    "subvert ids in [0, {e.n_sub})"), RANGE_FLAG)

    def __init__(self, table: np.ndarray, title_size: int, body_size: int, history_size: int, filter_num: int, window_size: int,
                 attention_hidden_dim: int, vert_num: int, vert_emb_dim: int, subvert_num: int, subvert_emb_dim: int,
                 dropout: float, learning_rate: float, loss: str, seed=None, train_embedding: bool = True, device=None,
                 process_group=None, bce_on: str = "logits"):
        self._require_one_rank(process_group)
        self._init_table(table, device)
        self.T, self.Tb, self.H = int(title_size), int(body_size), int(history_size)
        self.F, self.A, self.window = int(filter_num), int(attention_hidden_dim), int(window_size)
        self.n_vert, self.Kv, self.n_sub, self.Ks = int(vert_num), int(vert_emb_dim), int(subvert_num), int(subvert_emb_dim)
        if self.E % 4 or self.F % 4 or self.A % 4:
            raise ValueError(f"word_emb_dim ({self.E}), filter_num ({self.F}) and attention_hidden_dim ({self.A}) must be "
                             "multiples of 4 for the HIP Conv1D and pooling kernels")
        if min(self.n_vert, self.n_sub, self.Kv, self.Ks) < 1 or max(self.Kv, self.Ks) > 256:
            raise ValueError(f"vert/subvert tables must be non-empty with an embedding width in [1, 256], got "
                             f"({self.n_vert}, {self.Kv}) and ({self.n_sub}, {self.Ks})")
        W, E, F, A = self.window, self.E, self.F, self.A
        shapes = {"t_conv": (W * E + 1, F), "t_aW": (F, A), "t_ab": (A,), "t_aq": (A,),
                  "b_conv": (W * E + 1, F), "b_aW": (F, A), "b_ab": (A,), "b_aq": (A,),
                  "v_emb": (self.n_vert, self.Kv), "v_Wb": (self.Kv + 1, F), "s_emb": (self.n_sub, self.Ks), "s_Wb": (self.Ks + 1, F),
                  "va_W": (F, A), "va_b": (A,), "va_q": (A,), "u_W": (F, A), "u_b": (A,), "u_q": (A,)}
        self._init_state(shapes, dropout, learning_rate, loss, seed, train_embedding, bce_on)
        self.fuse_user_head = True  # False: the user pooling + loss as separate launches (validation of the fused head)
        self._init_weights(seed)

    # ------------------------------------------------------------------ parameters
    def _init_weights(self, seed):
        pv = self.params.view
        F, A = self.F, self.A
        rng = np.random.default_rng(seed)
        for conv in ("t_conv", "b_conv"):
            self._conv_init(conv, seed)
        with torch.no_grad():
            for aW, ab, aq in _ATT.values():
                pv(aW).copy_(torch.from_numpy(glorot_uniform_np((F, A), seed)))
                pv(ab).zero_()
                pv(aq).copy_(torch.from_numpy(glorot_uniform_np((A, 1), seed).reshape(A)))
            for emb, Wb, K, n in (("v_emb", "v_Wb", self.Kv, self.n_vert), ("s_emb", "s_Wb", self.Ks, self.n_sub)):
                # Keras' default Embedding initializer: RandomUniform(-0.05, 0.05)
                pv(emb).copy_(torch.from_numpy(rng.uniform(-0.05, 0.05, (n, K)).astype(np.float32)))
                pv(Wb)[:K].copy_(torch.from_numpy(glorot_uniform_np((K, F), seed)))
                pv(Wb)[K].zero_()

    def weight_names(self):
        return list(WEIGHT_NAMES)

    def _flat_order(self):
        """(flat-buffer name, row slice or None) of every entry of WEIGHT_NAMES after news.emb."""
        W, E = self.window, self.E
        conv = lambda n: [(n, slice(0, W * E)), (n, W * E)]
        att = lambda k: [(_ATT[k][0], None), (_ATT[k][1], None), (_ATT[k][2], None)]
        return (conv("t_conv") + att("t") + conv("b_conv") + att("b") + [("v_emb", None), ("v_Wb", slice(0, self.Kv)),
                ("v_Wb", self.Kv), ("s_emb", None), ("s_Wb", slice(0, self.Ks)), ("s_Wb", self.Ks)] + att("va") + att("u"))

    def _shapes(self):
        W, E, F, A = self.window, self.E, self.F, self.A
        conv = [(W, E, F), (F,)]
        att = [(F, A), (A,), (A, 1)]
        return ([tuple(self.table.shape)] + conv + att + conv + att + [(self.n_vert, self.Kv), (self.Kv, F), (F,),
                (self.n_sub, self.Ks), (self.Ks, F), (F,)] + att + att)

    def get_weights(self):
        out = [self.table.cpu().numpy()]
        for (name, rows), shape in zip(self._flat_order(), self._shapes()[1:]):
            v = self.params.view(name)
            v = v if rows is None else v[rows]
            out.append(v.cpu().numpy().reshape(shape).copy())
        return out

    def set_weights(self, weights):
        if len(weights) != len(WEIGHT_NAMES):
            raise ValueError(f"expected {len(WEIGHT_NAMES)} weight arrays ({', '.join(WEIGHT_NAMES)}), got {len(weights)}")
        w = [np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in weights]
        for a, s, n in zip(w, self._shapes(), WEIGHT_NAMES):
            if a.size != int(np.prod(s)) or (a.ndim > 1 and a.shape != s and a.shape != s[:-1]):
                raise ValueError(f"{n}: shape {a.shape} != {s}")
        with torch.no_grad():
            self.table.copy_(torch.from_numpy(w[0].reshape(self.table.shape)))
            for (name, rows), a in zip(self._flat_order(), w[1:]):
                v = self.params.view(name)
                v = v if rows is None else v[rows]
                v.copy_(torch.from_numpy(a.reshape(v.shape)))

    def count_params(self):
        W, E, F, A = self.window, self.E, self.F, self.A
        return (self.table.numel() + 2 * (W * E * F + F) + 4 * (F * A + 2 * A) + self.n_vert * self.Kv + self.n_sub * self.Ks
                + (self.Kv + self.Ks) * F + 2 * F)

    # ------------------------------------------------------------------ kernels
    def _encode(self, b: _Bufs, train: bool, user: bool = True):
        """Forward of every article of the buffers' batch (ids already staged); training: dropout on.  user: also the user
        pooling (inference; a training step runs it inside the fused head)."""
        self._encode_news(b, train)
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        P = self.params
        B, F, A, H = b.B, self.F, self.A, self.H
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        his = b.NV[: B * H]
        call("ebn_gemm_f32", 0, 0, B * H, A, F, f1, pt(his), F, pt(P.view("u_W")), A, f0, pt(b.Uu), A, S())
        if user:
            call("ebn_attpool_fwd_f32", pt(b.Uu), pt(P.view("u_b")), pt(P.view("u_q")), pt(his), pt(b.user), pt(b.wu), B, H, F, A, S())

    def _encode_news(self, b: _Bufs, train: bool):
        """The news encoder over the buffers' N articles (four views, view attention) -> b.NV."""
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        P = self.params
        st = pt(self.state) if train else None
        N, E, F, A, W = b.N, self.E, self.F, self.A, self.window
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        p = self.p if train else 0.0
        on = p > 0
        for ids, X, Vd, U, w, L, conv, (aW, ab, aq), s_in, s_conv, v in (
                (b.ids_t, b.Xt, b.Vt, b.Ut, b.wt, self.T, "t_conv", _ATT["t"], SITE_TITLE_IN, SITE_TITLE_CONV, 0),
                (b.ids_b, b.Xb, b.Vb, b.Ub, b.wb, self.Tb, "b_conv", _ATT["b"], SITE_BODY_IN, SITE_BODY_CONV, 1)):
            R = N * L
            call("ebn_gather_rows_f32", pt(ids), pt(self.table), pt(X), R, E, self.V, st, s_in if on else -1, ctypes.c_float(p),
                 pt(self.oob_flag), S())
            Wb = P.view(conv)
            call("ebn_conv1d_fwd_f32", pt(X), pt(Wb), pt(Wb[W * E]), pt(Vd), N, L, E, F, W, st, s_conv if on else -1,
                 ctypes.c_float(p), -1, f0, S())
            call("ebn_gemm_f32", 0, 0, R, A, F, f1, pt(Vd), F, pt(P.view(aW)), A, f0, pt(U), A, S())
            call("ebn_attpool_fwd_f32", pt(U), pt(P.view(ab)), pt(P.view(aq)), pt(Vd), pt(b.Vw[v]), pt(w), N, L, F, A, S())
        call("ebn_naml_catview_fwd_f32", pt(b.cat_v), pt(P.view("v_emb")), self.n_vert, self.Kv, pt(P.view("v_Wb")), pt(b.Vw[2]),
             pt(b.cat_s), pt(P.view("s_emb")), self.n_sub, self.Ks, pt(P.view("s_Wb")), pt(b.Vw[3]), N, F, pt(self.cat_oob_flag), S())
        call("ebn_gemm_f32", 0, 0, N_VIEWS * N, A, F, f1, pt(b.Vw), F, pt(P.view("va_W")), A, f0, pt(b.Uv), A, S())
        call("ebn_naml_viewatt_fwd_f32", pt(b.Uv), pt(P.view("va_b")), pt(P.view("va_q")), pt(b.Vw), pt(b.wv), pt(b.NV), N, N_VIEWS,
             F, A, S())

    def _train_kernels(self, b: _Bufs, C: int):
        """One optimizer step on the staged batch: step advance, forward, loss, backward, Adam (dense buffer, word table)."""
        self._grad_kernels(b, C)
        self._optimizer_kernels()

    def _grad_kernels(self, b: _Bufs, C: int):
        """Step advance, forward, loss and backward: the dense gradients land in params.grad, the word-table gradient in the
        fixed-point accumulator table_acc."""
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        P, g = self.params, self.params.g
        st = pt(self.state)
        B, N, F, A, H = b.B, b.N, self.F, self.A, self.H
        BH = B * H
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        ws, wsn = pt(b.ws), b.ws.numel()
        inv_b = ctypes.c_float(1.0 / B)
        call("ebn_step_advance", st, BETA1, BETA2, S())
        self._encode(b, True, user=False)
        his, cand = b.NV[:BH], b.NV[BH:]
        # user AttLayer2 + Dot + softmax + loss and their backward: U_u <- d(pre-tanh), dcand, duser, dq_u, db_u
        if self.fuse_user_head and int(_hip.lib().ebn_user_head_supported(H, C, F, A)):
            call("ebn_user_head_train_f32", pt(b.Uu), pt(P.view("u_b")), pt(P.view("u_q")), pt(his), pt(cand), pt(b.labels),
                 pt(b.wu), pt(b.user), pt(b.scores), pt(b.probs), pt(b.loss_rows), pt(self.loss_dev), pt(b.dNV[BH:]), pt(b.duser),
                 pt(b.deu), pt(g("u_q")), pt(g("u_b")), pt(b.head_partials), B, H, C, F, A, self.loss_kind, inv_b, S())
        else:
            call("ebn_attpool_fwd_f32", pt(b.Uu), pt(P.view("u_b")), pt(P.view("u_q")), pt(his), pt(b.user), pt(b.wu), B, H, F, A, S())
            call("ebn_score_loss_train_f32", pt(cand), pt(b.user), pt(b.labels), pt(b.scores), pt(b.probs), pt(b.loss_rows),
                 pt(self.loss_dev), pt(b.dNV[BH:]), pt(b.duser), B, C, F, self.loss_kind, inv_b, S())
            call("ebn_attpool_bwd_pool_f32", pt(his), pt(b.wu), pt(b.duser), None, pt(b.deu), B, H, F, S())
            call("ebn_attpool_bwd_dpre_f32", pt(b.Uu), pt(P.view("u_q")), pt(b.deu), pt(g("u_q")), pt(g("u_b")), pt(b.part), BH, A,
                 0, S())
        call("ebn_gemm_f32_ws", 1, 0, F, A, BH, f1, pt(his), F, pt(b.Uu), A, f0, pt(g("u_W")), A, ws, wsn, S())
        # d(history news vectors) = dpre_u.Wu^T + wu (x) duser
        call("ebn_gemm_f32_rank1", BH, F, A, f1, pt(b.Uu), A, pt(P.view("u_W")), A, pt(b.dNV), F, pt(b.wu), pt(b.duser), F, H,
             ws, wsn, S())
        # view attention: dVw = wv (x) dnews + dpre_v.Wva^T
        R4 = N_VIEWS * N
        call("ebn_naml_viewatt_bwd_f32", pt(b.Vw), pt(b.wv), pt(b.dNV), pt(b.dVw), pt(b.dew), N, N_VIEWS, F, S())
        call("ebn_attpool_bwd_dpre_f32", pt(b.Uv), pt(P.view("va_q")), pt(b.dew), pt(g("va_q")), pt(g("va_b")), pt(b.part), R4, A,
             0, S())
        call("ebn_gemm_f32_ws", 1, 0, F, A, R4, f1, pt(b.Vw), F, pt(b.Uv), A, f0, pt(g("va_W")), A, ws, wsn, S())
        call("ebn_gemm_f32", 0, 1, R4, F, A, f1, pt(b.Uv), A, pt(P.view("va_W")), A, f1, pt(b.dVw), F, S())
        # categorical views: Dense kernel / bias and the dense gradients of both small tables
        call("ebn_naml_catview_bwd_f32", pt(b.cat_v), pt(P.view("v_emb")), self.n_vert, self.Kv, pt(P.view("v_Wb")), pt(b.Vw[2]),
             pt(b.dVw[2]), pt(g("v_Wb")), pt(g("v_emb")), pt(b.cat_s), pt(P.view("s_emb")), self.n_sub, self.Ks, pt(P.view("s_Wb")),
             pt(b.Vw[3]), pt(b.dVw[3]), pt(g("s_Wb")), pt(g("s_emb")), pt(b.cpart), b.cpart.numel(), N, F, S())
        # title and body: AttLayer2 backward, then the Conv1D
        views = ((ConvView(b.ids_t, b.Xt, b.Vt, b.dVt, b.dXt, b.wpart_t, b.splits_t, self.T, "t_conv", SITE_TITLE_IN), b.Ut, b.wt, b.det,
                  _ATT["t"], 0),
                 (ConvView(b.ids_b, b.Xb, b.Vb, b.dVb, b.dXb, b.wpart_b, b.splits_b, self.Tb, "b_conv", SITE_BODY_IN), b.Ub, b.wb, b.deb,
                  _ATT["b"], 1))
        for cv, U, w, de, (aW, ab, aq), v in views:
            R = N * cv.L
            call("ebn_attpool_bwd_pool_f32", pt(cv.Vd), pt(w), pt(b.dVw[v]), None, pt(de), N, cv.L, F, S())
            call("ebn_attpool_bwd_dpre_f32", pt(U), pt(P.view(aq)), pt(de), pt(g(aq)), pt(g(ab)), pt(b.part), R, A, 0, S())
            call("ebn_gemm_f32_ws", 1, 0, F, A, R, f1, pt(cv.Vd), F, pt(U), A, f0, pt(g(aW)), A, ws, wsn, S())
            call("ebn_gemm_f32_rank1", R, F, A, f1, pt(U), A, pt(P.view(aW)), A, pt(cv.dVd), F, pt(w), pt(b.dVw[v]), F, cv.L, ws, wsn, S())
            self._conv_wgrad(cv, N, self.p, 0.0)
        self._conv_finish([view[0] for view in views], N, self.p, 0.0)  # both weight gradients in one finishing launch

    # ------------------------------------------------------------------ host entry points
    def _arrays(self, xs, what):
        """(title, body, vert, subvert) of one side as numpy arrays or device tensors, checked: (B, K, T), (B, K, Tb), (B, K, 1)."""
        t, bo, v, s = (a if isinstance(a, torch.Tensor) else np.asarray(a) for a in xs)
        if t.ndim != 3 or t.shape[2] != self.T:
            raise ValueError(f"{what}_input_title must be (B, n, {self.T}), got {tuple(t.shape)}")
        lead = tuple(t.shape[:2])
        if tuple(bo.shape) != lead + (self.Tb,):
            raise ValueError(f"{what}_input_body must be {lead + (self.Tb,)}, got {tuple(bo.shape)}")
        for a, n in ((v, "vert"), (s, "subvert")):
            if tuple(a.shape) not in (lead + (1,), lead):
                raise ValueError(f"{what}_input_{n} must be {lead + (1,)}, got {tuple(a.shape)}")
        for a in (t, bo):
            if not isinstance(a, torch.Tensor) and a.size and (a.min() < 0 or a.max() >= self.V):
                raise IndexError(f"token id out of range [0, {self.V}) for the embedding table")
        return t, bo, v, s

    def _fill(self, b: _Bufs, his, cands):
        """Stage the token and category ids: history articles first, then the candidates."""
        BH = b.B * self.H
        for dst, width, h, c in ((b.ids_t, self.T, his[0], cands[0]), (b.ids_b, self.Tb, his[1], cands[1]),
                                 (b.cat_v, 1, his[2], cands[2]), (b.cat_s, 1, his[3], cands[3])):
            self._put(dst[: BH * width], h)
            self._put(dst[BH * width:], c)

    def _infer(self, his, cands, cand_imp):
        """Inference-mode encoders: (user vectors (b, F), candidate news vectors (n, F))."""
        his = self._arrays(his, "his")
        if his[0].shape[1] != self.H:
            raise ValueError(f"his_input_title must be (B, {self.H}, {self.T}), got {tuple(his[0].shape)}")
        cands = self._arrays(cands, "pred")
        B, n = his[0].shape[0], cands[0].shape[0] * cands[0].shape[1]
        b = _Bufs(self, B, n, train=False)
        self._fill(b, his, cands)
        self._encode(b, False)
        self._check_oob()
        return b.user, b.NV[B * self.H:]

    def forward(self, *xs, mode="softmax"):
        """The 8 input arrays (his_title, his_body, his_vert, his_subvert, pred_title, pred_body, pred_vert, pred_subvert) ->
        (probs (B,C), scores (B,C)) device tensors, inference mode."""
        B, C = np.shape(xs[4])[:2]
        user_vec, cand = self._infer(xs[:4], xs[4:8], None)
        scores, probs = torch.empty(B, C, device=self.device), torch.empty(B, C, device=self.device)
        _hip.call("ebn_score_fwd_f32", _hip.ptr(cand), _hip.ptr(user_vec), _hip.ptr(scores), _hip.ptr(probs), B, C, self.F,
                  0 if mode == "softmax" else 1, _hip.stream_handle())
        return probs, scores

    def eval_loss(self, *xs):
        """Inference-mode forward + the compiled loss: (loss[1], probs (B,C)); xs = the 8 input arrays and y."""
        y = xs[8]
        B, C = np.shape(xs[4])[:2]
        user_vec, cand = self._infer(xs[:4], xs[4:8], None)
        return score_loss_tail(cand, user_vec, y, B, C, self.F, self.loss_kind)[:2]

    def pair_scores(self, his, cands, cand_imp, sigmoid=True):
        """act(cand_i . user[cand_imp[i]]) for the candidates (title (n,T), body (n,Tb), vert (n,), subvert (n,)) of the impressions
        whose history is his = (title (b,H,T), body (b,H,Tb), vert (b,H,1), subvert (b,H,1)) -- scorer.predict."""
        cands = tuple(np.asarray(a) if not isinstance(a, torch.Tensor) else a for a in cands)
        n = cands[0].shape[0]
        cands = (cands[0].reshape(n, 1, self.T), cands[1].reshape(n, 1, self.Tb), cands[2].reshape(n, 1, 1), cands[3].reshape(n, 1, 1))
        user_vec, cand = self._infer(his, cands, cand_imp)
        ui = torch.from_numpy(np.ascontiguousarray(cand_imp, dtype=np.int32)).to(self.device)
        ni = torch.arange(n, dtype=torch.int32, device=self.device)
        return pair_score_tail(user_vec, cand, ui, ni, self.F, sigmoid)

    # ------------------------------------------------------------------ scoring from a once-encoded catalogue
    def encode_catalogue(self, title, body, vert, subvert, chunk=4096):
        """Everything scorer.predict needs of the articles alone, for the CURRENT weights (build it per predict, never keep it on the
        model): four aligned arrays -- title tokens (n_rows, T), body tokens (n_rows, Tb), vert (n_rows,), subvert (n_rows,) -> cache
        with news_all (n_rows, F) and a_all (n_rows,) = exp(tanh(news_all.Wu + bu).qu), the user AttLayer2's logit of each article.
        Encoded in chunks: the scratch is that of `chunk` articles whatever n_rows is."""
        n_rows = int(np.shape(title)[0])
        if n_rows == 0:
            return SimpleNamespace(news_all=torch.empty(0, self.F, device=self.device), a_all=torch.empty(0, device=self.device), n_rows=0)
        t, bo, v, s_ = self._arrays((np.asarray(title).reshape(n_rows, 1, -1), np.asarray(body).reshape(n_rows, 1, -1),
                                     np.asarray(vert).reshape(n_rows, 1, 1), np.asarray(subvert).reshape(n_rows, 1, 1)), "catalogue")
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        F, A, P = self.F, self.A, self.params
        f1, f0 = ctypes.c_float(1.0), ctypes.c_float(0.0)
        news_all, a_all = torch.empty(n_rows, F, device=self.device), torch.empty(n_rows, device=self.device)
        b = _Bufs(self, 0, min(chunk, n_rows), train=False)
        for s in range(0, n_rows, chunk):
            n = min(chunk, n_rows - s)
            if n != b.N:
                b = _Bufs(self, 0, n, train=False)  # the short last chunk
            for dst, src in ((b.ids_t, t), (b.ids_b, bo), (b.cat_v, v), (b.cat_s, s_)):
                self._put(dst, src[s:s + n])
            self._encode_news(b, False)
            news_all[s:s + n].copy_(b.NV)
        Uu = torch.empty(n_rows, A, device=self.device)
        call("ebn_gemm_f32", 0, 0, n_rows, A, F, f1, pt(news_all), F, pt(P.view("u_W")), A, f0, pt(Uu), A, S())
        call("ebn_att_logit_rows_f32", pt(Uu), pt(P.view("u_b")), pt(P.view("u_q")), pt(a_all), n_rows, A, S())
        self._check_oob()
        return SimpleNamespace(news_all=news_all, a_all=a_all, n_rows=n_rows)

    def score_cached(self, cache, his_idx, cand_idx, cand_imp, sigmoid=True, return_user=False):
        """act(news_all[cand_i] . user[cand_imp[i]]) of one indexed batch in ONE launch: his_idx (b, H) / cand_idx (n,) rows of the
        cache, cand_imp (n,) the impression of each candidate, ascending (an impression's candidates are contiguous)."""
        his_idx, cand_idx, cand_imp = np.asarray(his_idx), np.asarray(cand_idx).reshape(-1), np.asarray(cand_imp).reshape(-1)
        if his_idx.ndim != 2 or cand_imp.shape != cand_idx.shape:
            raise ValueError(f"indexed batches need his_idx (b, H) and one impression per candidate, got {tuple(his_idx.shape)}, "
                             f"{tuple(cand_idx.shape)}, {tuple(cand_imp.shape)}")
        if cand_imp.size > 1 and (np.diff(cand_imp) < 0).any():
            raise ValueError("the candidates of an impression must be contiguous (impression numbers ascending)")
        B, H, n = his_idx.shape[0], his_idx.shape[1], cand_idx.shape[0]
        dev = self.device
        offsets = torch.from_numpy(np.searchsorted(cand_imp, np.arange(B + 1)).astype(np.int64)).to(dev)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        hi, ci = i32(his_idx.reshape(-1)), i32(cand_idx)
        out = torch.empty(n, device=dev)
        user = torch.empty(B, self.F, device=dev) if return_user else None
        _hip.call("ebn_indexed_attpool_score_f32", _hip.ptr(cache.news_all), _hip.ptr(cache.a_all), cache.n_rows, _hip.ptr(hi),
                  _hip.ptr(ci), _hip.ptr(offsets), n, _hip.ptr(out), _hip.ptr(user), _hip.ptr(self.row_oob_flag), B, H, self.F,
                  1 if sigmoid else 0, _hip.stream_handle())
        self._check_oob()
        return (out, user) if return_user else out

    def train_step(self, *xs, return_probs=False):
        """One optimizer step on (the 8 input arrays, y); returns the batch loss as a 1-element device tensor (no host sync).  The
        launch sequence of a (B, C) shape is captured once into one hipGraph on the current stream (one stream, no parallel
        branches) and replayed; step-dependent scalars live in the device step state."""
        if len(xs) != 9:
            raise ValueError(f"train_step takes the 8 NAML input arrays and y, got {len(xs)} arguments")
        his, pred, y = self._arrays(xs[:4], "his"), self._arrays(xs[4:8], "pred"), xs[8]
        B, C = pred[0].shape[0], pred[0].shape[1]
        if his[0].shape[0] != B or his[0].shape[1] != self.H:
            raise ValueError(f"his_input_title must be ({B}, {self.H}, {self.T}), got {tuple(his[0].shape)}")
        b = self._stage(his, pred, y)
        key = (B, C, self.loss_kind, self.train_embedding, self.fuse_user_head)
        self._run_step(key, lambda: self._train_kernels(b, C))
        if return_probs:
            return self.loss_dev, b.probs.view(B, C), b.labels.view(B, C)
        return self.loss_dev

    def _stage(self, his, pred, y):
        """The step's static buffers for (B, C), filled with the batch (checked input arrays, see _arrays)."""
        B, C = pred[0].shape[0], pred[0].shape[1]
        b = self._bufs.get((B, C))
        if b is None:
            b = self._bufs[(B, C)] = _Bufs(self, B, B * C, train=True)
        self._fill(b, his, pred)
        self._put(b.labels, y, torch.float32)
        return b
