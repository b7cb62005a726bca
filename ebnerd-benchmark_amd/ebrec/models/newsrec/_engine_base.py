"""What the device engines share (imports nothing from _engine.py, which re-exports the small pieces):

  * the small host pieces: Adam constants, loss_kind_of, require_gpu, the Glorot initialisers, FlatParams, set_article_matrix;
  * StepStateOwner -- the device step state (step, seed, lr) of all five engines: learning_rate, read_state, loss_kind;
  * score_loss_tail / pair_score_tail -- the launches every engine's eval_loss / pair_scores ends in;
  * ConvEngineBase -- the one-rank engines over a Conv1D title encoder (LSTUR, NPA, NAML): word table with its fixed-point
    gradient accumulator, the sticky device flags and their one host read, capture-or-replay of a step, the Adam launches, the
    Conv1D backward block and the (window, E, F) kernel | bias packing of a conv_Wb-style parameter;
  * UserTableEngine -- on top of it, the two engines with a trainable user table (LSTUR, NPA): host checks, staging, train_step
    and the inference entry points.
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from ebrec import _hip

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-7  # tf.keras.optimizers.Adam defaults (nrms.py:77)
_ALIGN = 64  # floats; keeps every parameter 256-byte aligned inside the flat buffer

LOSS_KIND = {"cross_entropy_loss": 0, "log_loss": 1}
BCE_ON = ("logits", "probs")


def loss_kind_of(loss: str, bce_on: str) -> int:
    """C-ABI loss_kind: 0 categorical CE on the softmax logits; 1 log_loss as sigmoid-CE on the logits Keras caches on the
    output of Activation("softmax") (bce_on="logits", the default); 2 log_loss as BCE on the clipped softmax outputs
    (bce_on="probs", SURVEY.md A.5's reading).  Which of the two TF 2.12-2.15 runs at nrms.py:54,61-62 is settled by the TF
    dump (tools/dump_tf_golden.py); until then both are implemented and tested, and switching is this one argument."""
    if bce_on not in BCE_ON:
        raise ValueError(f"bce_on must be one of {BCE_ON}, got {bce_on}")
    return 0 if loss == "cross_entropy_loss" else (1 if bce_on == "logits" else 2)


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("the MI355X NRMS path needs a visible GPU (no CPU fallback); "
                           "torch.cuda.is_available() is False")
    _hip.lib()
    return torch.device("cuda", torch.cuda.current_device())


def glorot_uniform_np(shape, seed):
    """[KERAS-SEMANTICS] GlorotUniform(seed): the same (seed, shape) gives the same draw, which is
    why WQ, WK and WV of one layer start identical in the reference (layers.py:155-172)."""
    rng = np.random.default_rng(seed)
    lim = math.sqrt(6.0 / (shape[0] + shape[-1]))
    return rng.uniform(-lim, lim, size=shape).astype(np.float32)


def conv_glorot_np(window, E, F, seed):
    """GlorotUniform of a Conv1D kernel (window, E, F): fan_in = window*E, fan_out = window*F (Keras' receptive-field rule)."""
    rng = np.random.default_rng(seed)
    lim = math.sqrt(6.0 / (window * E + window * F))
    return rng.uniform(-lim, lim, size=(window, E, F)).astype(np.float32)


class FlatParams:
    """Named fp32 parameters carved out of one flat device buffer (plus grad / Adam moments)."""

    def __init__(self, shapes: dict, device):
        self.shapes = dict(shapes)
        self.offsets = {}
        off = 0
        for name, shp in shapes.items():
            self.offsets[name] = off
            off += -(-int(np.prod(shp)) // _ALIGN) * _ALIGN
        self.numel = off
        self.data = torch.zeros(off, device=device)
        self.grad = torch.zeros(off, device=device)
        self.m = torch.zeros(off, device=device)
        self.v = torch.zeros(off, device=device)

    def view(self, name, buf=None):
        buf = self.data if buf is None else buf
        n = int(np.prod(self.shapes[name]))
        return buf[self.offsets[name]: self.offsets[name] + n].view(*self.shapes[name])

    def g(self, name):
        return self.view(name, self.grad)


class StepStateOwner:
    """The device step state of an engine (ebn_step_state: step, seed, lr, Adam step size) and what reads it on the host."""

    def _init_step_state(self, seed, learning_rate):
        st = _hip.StepState()
        st.step, st.seed, st.lr, st.adam_alpha = 0, (0 if seed is None else int(seed)) & 0xFFFFFFFF, learning_rate, 0.0
        self.state = torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).to(self.device)
        self._lr = float(learning_rate)

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
    """Keep the loader's (n_articles+1, T) token matrix in HBM; batches can then be given as article-row
    numbers (``train_step(..., indexed=True)``) and expanded to token ids on the device."""
    m = np.asarray(matrix)
    if m.ndim != 2 or m.shape[1] != self.T or not np.issubdtype(m.dtype, np.integer):
        raise ValueError(f"article matrix must be integer (n_articles+1, {self.T}), got {m.dtype} {m.shape}")
    if m.size and (m.min() < 0 or m.max() >= self.V):
        raise IndexError(f"token id out of range [0, {self.V}) for the embedding table")
    self.article_matrix = torch.from_numpy(np.ascontiguousarray(m.astype(np.int32))).to(self.device)
    self._article_matrix_src = matrix


def score_loss_tail(cand, user_vec, y, B, C, F, loss_kind):
    """Scorer + compiled loss over encoded vectors: cand (B*C, F), user_vec (B, F), labels y (B, C) ->
    (loss[1], probs (B,C), scores (B,C)).  Softmax scores, the loss rows (its gradients are discarded), their sum."""
    dev = cand.device
    S = _hip.stream_handle
    scores, probs = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev)
    _hip.call("ebn_score_fwd_f32", _hip.ptr(cand), _hip.ptr(user_vec), _hip.ptr(scores), _hip.ptr(probs), B, C, F, 0, S())
    labels = y if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(y, dtype=np.float32)))
    labels = labels.to(device=dev, dtype=torch.float32).reshape(B, C).contiguous()
    rows, junk_c, junk_u = torch.empty(B, device=dev), torch.empty(B * C, F, device=dev), torch.empty(B, F, device=dev)
    loss = torch.empty(1, device=dev)
    _hip.call("ebn_score_loss_bwd_f32", _hip.ptr(cand), _hip.ptr(user_vec), _hip.ptr(scores), _hip.ptr(labels), _hip.ptr(rows),
              _hip.ptr(junk_c), _hip.ptr(junk_u), B, C, F, loss_kind, ctypes.c_float(1.0 / B), S())
    _hip.call("ebn_sum_f32", _hip.ptr(rows), B, ctypes.c_float(1.0), _hip.ptr(loss), 0, S())
    return loss, probs, scores


def pair_score_tail(user_vec, news, u_idx, n_idx, F, sigmoid=True):
    """act(news[n_idx[i]] . user_vec[u_idx[i]]) of the n (u_idx, n_idx) int32 device pairs -> (n,)."""
    n = n_idx.numel()
    out = torch.empty(n, device=user_vec.device)
    _hip.call("ebn_pair_score_f32", _hip.ptr(user_vec), _hip.ptr(news), _hip.ptr(u_idx), _hip.ptr(n_idx), _hip.ptr(out), n, F,
              1 if sigmoid else 0, _hip.stream_handle())
    return out


TOKEN_FLAG = ("oob_flag", IndexError, "token id out of range [0, {e.V}) for the embedding table")
ROW_FLAG = ("row_oob_flag", IndexError, "article row out of range for the encoded catalogue")
RANGE_FLAG = ("range_flag", FloatingPointError, "embedding gradient left the range of the deterministic fixed-point accumulator: "
              "the run has diverged")

# one Conv1D over L-token sequences, as the backward block sees it: token ids, gathered rows X, conv output Vd, its gradient dVd,
# dX, the split-K partials of the weight gradient and their count, the conv_Wb-style parameter, the dropout site of the gather
ConvView = namedtuple("ConvView", "ids X Vd dVd dX wpart splits L conv site_in")


class ConvEngineBase(StepStateOwner):
    """One-rank engine over a Conv1D title encoder.  A subclass declares MODEL (for messages) and FLAGS -- its sticky device
    flags as (attribute, exception type, message formatted with e=the engine), in the order they are raised."""

    MODEL = ""
    FLAGS = ()
    user_table = None  # UserTableEngine: the (n_users + 1, width) table, trained like the word table

    def _require_one_rank(self, process_group):
        if process_group is not None and torch.distributed.get_world_size(process_group) > 1:
            raise ValueError(f"{self.MODEL}Model runs on one rank: multi-rank {self.MODEL} is not implemented (build it without a "
                             "process group of more than one rank)")

    def _init_table(self, table, device):
        self.device = require_gpu() if device is None else torch.device(device)
        table = np.asarray(table, dtype=np.float32)
        self.V, self.E = table.shape
        self.table = torch.from_numpy(np.ascontiguousarray(table)).to(self.device)

    def _init_state(self, shapes, dropout, learning_rate, loss, seed, train_embedding, bce_on):
        """Everything but the model's own weights: flat dense parameters, the word table's accumulator and moments, the flags,
        the step state, the per-shape buffer and graph caches."""
        dev = self.device
        self.p = float(dropout)
        self.loss, self.bce_on = loss, bce_on
        loss_kind_of(loss, bce_on)
        self.train_embedding = bool(train_embedding)
        self.seed = seed
        self.params = FlatParams(shapes, dev)
        self.table_acc = torch.zeros(self.table.numel(), dtype=torch.int64, device=dev)
        self.table_m, self.table_v = torch.zeros_like(self.table), torch.zeros_like(self.table)
        for attr, _exc, _msg in self.FLAGS:
            setattr(self, attr, torch.zeros(1, dtype=torch.int32, device=dev))
        self.loss_dev = torch.zeros(1, device=dev)
        self._init_step_state(seed, learning_rate)
        self._bufs, self._graphs = {}, {}
        self.use_graph = True

    # ------------------------------------------------------------------ (window, E, F) kernel | bias  <->  conv_Wb rows
    def _conv_get(self, name):
        n = self.window * self.E
        wb = self.params.view(name).cpu().numpy()
        return [wb[:n].reshape(self.window, self.E, self.F).copy(), wb[n].copy()]

    def _conv_set(self, name, kernel, bias):
        n = self.window * self.E
        wb = self.params.view(name)
        with torch.no_grad():
            wb[:n].copy_(torch.from_numpy(kernel.reshape(n, self.F)))
            wb[n].copy_(torch.from_numpy(bias))

    def _conv_init(self, name, seed):
        self._conv_set(name, conv_glorot_np(self.window, self.E, self.F, seed), np.zeros(self.F, np.float32))

    # ------------------------------------------------------------------ kernels
    def _conv_wgrad(self, v: ConvView, N, p_conv, p_post):
        """Split-K partials of d(conv_Wb) of one Conv1D over N sequences; p_conv / p_post: the rates of the two dropouts behind it."""
        pt = _hip.ptr
        _hip.call("ebn_conv1d_bwd_weight_f32", pt(v.X), pt(v.dVd), pt(v.Vd), pt(v.wpart), v.splits, N, v.L, self.E, self.F, self.window,
                  pt(self.state), ctypes.c_float(p_conv), ctypes.c_float(p_post), _hip.stream_handle())

    def _conv_finish(self, views, N, p_conv, p_post):
        """Behind _conv_wgrad of every view: ONE finishing launch sums their partials into the gradients; with a trainable word
        table, then d(X) of each view and its scatter into the fixed-point accumulator."""
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        st, E, F, W = pt(self.state), self.E, self.F, self.window
        pc, pp = ctypes.c_float(p_conv), ctypes.c_float(p_post)
        jobs = (_hip.FinishJob * len(views))()
        for j, v in zip(jobs, views):
            j.kind, j.n_parts, j.rows, j.cols = _hip.FINISH_SPLITK, v.splits, W * E + 1, F
            j.partials, j.out0, j.ld, j.beta, j.scale = v.wpart.data_ptr(), self.params.g(v.conv).data_ptr(), F, 0.0, 1.0
        call("ebn_grad_finish_f32", jobs, len(views), S())
        if self.train_embedding:
            for v in views:
                call("ebn_conv1d_bwd_data_f32", pt(v.dVd), pt(v.Vd), pt(self.params.view(v.conv)), pt(v.dX), N, v.L, E, F, W, st, pc, pp,
                     S())
                call("ebn_embedding_grad_scatter_fixed", pt(v.ids), pt(v.dX), pt(self.table_acc), N * v.L, E, self.V, st,
                     v.site_in if self.p > 0 else -1, pc, pt(self.range_flag), S())

    def _conv_backward(self, v: ConvView, N, p_conv, p_post):
        """The Conv1D backward of an engine with one convolution: weight gradient, its finishing launch, the table gradient."""
        self._conv_wgrad(v, N, p_conv, p_post)
        self._conv_finish((v,), N, p_conv, p_post)

    def _optimizer_kernels(self):
        """Keras Adam (nrms.py:69-80 form): dense parameters, then the word table (and the user table of an engine that has one)
        straight from their fixed-point accumulators."""
        S = _hip.stream_handle
        call, pt = _hip.call, _hip.ptr
        P = self.params
        st = pt(self.state)
        f1 = ctypes.c_float(1.0)
        call("ebn_adam_keras_step_f32", pt(P.data), pt(P.grad), pt(P.m), pt(P.v), P.numel, st, BETA1, BETA2, ADAM_EPS, f1, S())
        if self.train_embedding:
            call("ebn_adam_keras_step_fixed_f32", pt(self.table), pt(self.table_acc), pt(self.table_m), pt(self.table_v),
                 self.table.numel(), st, BETA1, BETA2, ADAM_EPS, f1, pt(self.range_flag), S())
        if self.user_table is not None:
            call("ebn_adam_keras_step_fixed_f32", pt(self.user_table), pt(self.user_acc), pt(self.user_m), pt(self.user_v),
                 self.user_table.numel(), st, BETA1, BETA2, ADAM_EPS, f1, pt(self.range_flag), S())

    def _run_step(self, key, kernels):
        """Launch a step's kernel sequence: eagerly, or (use_graph) captured once per key into one hipGraph on the current stream
        and replayed -- step-dependent scalars live in the device step state."""
        if not self.use_graph:
            return kernels()
        g = self._graphs.get(key)
        if g is None:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with _hip.capture(g):
                kernels()
            self._graphs[key] = g
        g.replay()

    # ------------------------------------------------------------------ host side
    def _put(self, dst: torch.Tensor, src, dtype=torch.int32):
        t = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(src)))
        dst.copy_(t.reshape(-1).to(device=self.device, dtype=dtype), non_blocking=True)

    def _check_oob(self):
        """One host read of every flag in FLAGS; all are cleared when any is set, the first set one (in FLAGS order) raises."""
        flags = torch.cat([getattr(self, attr) for attr, _exc, _msg in self.FLAGS]).cpu().tolist()
        if any(flags):
            for attr, _exc, _msg in self.FLAGS:
                getattr(self, attr).zero_()
        for v, (_attr, exc, msg) in zip(flags, self.FLAGS):
            if v:
                raise exc(msg.format(e=self))

    def check_oob(self):
        """One host read of the device flags (fit() calls it once per epoch): ids outside a table raise IndexError."""
        self._check_oob()


class UserTableEngine(ConvEngineBase):
    """LSTUR and NPA: (user index, history titles, candidate titles) batches and a zeros-initialised trainable user table.
    A subclass supplies _new_bufs, _user_vec, _encode, _train_kernels and, where its graphs depend on more, _graph_key_extra."""

    FLAGS = (ROW_FLAG, ("user_oob_flag", IndexError, "user index out of range [0, {e.n_users}] for the user embedding table"),
             TOKEN_FLAG, RANGE_FLAG)
    set_article_matrix = set_article_matrix

    def _init_state(self, shapes, user_dim, *args):
        super()._init_state(shapes, *args)
        self.user_table = torch.zeros(self.n_users + 1, user_dim, device=self.device)  # embeddings_initializer="zeros"
        self.user_acc = torch.zeros(self.user_table.numel(), dtype=torch.int64, device=self.device)
        self.user_m, self.user_v = torch.zeros_like(self.user_table), torch.zeros_like(self.user_table)
        self.article_matrix = None
        self._article_matrix_src = None

    def _graph_key_extra(self):
        return ()

    def _new_bufs(self, B, n_cand, cand_imp, train):
        """The engine's _Bufs of one shape; cand_imp (n_cand,): the impression of each candidate."""
        raise NotImplementedError

    def _cand_imp(self, B, C):
        """The impression of each of a (B, C) batch's candidates."""
        return np.repeat(np.arange(B), C)

    # ------------------------------------------------------------------ host checks
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

    # ------------------------------------------------------------------ inference
    def _infer(self, user, his, cands, cand_imp=None):
        """Inference-mode encoders: (user vectors (b, F), candidate news vectors (n, F)); cand_imp[i]: the impression of
        candidate i, for an engine whose title encoder depends on it."""
        user, his = self._uidx(user), his if isinstance(his, torch.Tensor) else np.asarray(his)
        cands = cands if isinstance(cands, torch.Tensor) else np.asarray(cands)
        self._check(user, his)
        self._host_ranges(user, his, cands)
        B, n = his.shape[0], cands.shape[0]
        b = self._new_bufs(B, n, cand_imp, train=False)
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
        user_vec, cand = self._infer(user, his, pred.reshape(B * C, self.T), self._cand_imp(B, C))
        scores, probs = torch.empty(B, C, device=self.device), torch.empty(B, C, device=self.device)
        _hip.call("ebn_score_fwd_f32", _hip.ptr(cand), _hip.ptr(user_vec), _hip.ptr(scores), _hip.ptr(probs), B, C, self.F,
                  0 if mode == "softmax" else 1, _hip.stream_handle())
        return probs, scores

    def eval_loss(self, user, his, pred, y):
        """Inference-mode forward + the compiled loss: (loss[1], probs (B,C))."""
        pred = np.asarray(pred) if not isinstance(pred, torch.Tensor) else pred
        B, C = pred.shape[0], pred.shape[1]
        user_vec, cand = self._infer(user, his, pred.reshape(B * C, self.T), self._cand_imp(B, C))
        return score_loss_tail(cand, user_vec, y, B, C, self.F, self.loss_kind)[:2]

    def pair_scores(self, user, his, cands, cand_imp, sigmoid=True):
        """act(cand_i . user[cand_imp[i]]) for candidates (n, T) of impressions (user (b,), his (b,H,T)) -- scorer.predict."""
        user_vec, cand = self._infer(user, his, cands, cand_imp)
        ui = torch.from_numpy(np.ascontiguousarray(cand_imp, dtype=np.int32)).to(self.device)
        ni = torch.arange(cand.shape[0], dtype=torch.int32, device=self.device)
        return pair_score_tail(user_vec, cand, ui, ni, self.F, sigmoid)

    # ------------------------------------------------------------------ training
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
        key = (B, C, bool(indexed)) + self._graph_key_extra() + (self.loss_kind, self.train_embedding)
        self._run_step(key, lambda: self._train_kernels(b, C, expand))
        if return_probs:
            return self.loss_dev, b.probs.view(B, C), b.labels.view(B, C)
        return self.loss_dev

    def _stage(self, user, his, pred, y, indexed):
        """The step's static buffers for (B, C), filled with the batch: (buffers, article rows to expand or None)."""
        B, C = his.shape[0], pred.shape[1]
        b = self._bufs.get((B, C))
        if b is None:
            b = self._bufs[(B, C)] = self._new_bufs(B, B * C, self._cand_imp(B, C), train=True)
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
