"""Fastformer_wu and StandardFastformerEncoder (reference models/fastformer/fastformer_wu.py) on the MI355X.

``StandardFastformerEncoder(config, pooler_count=1)`` is the Fastformer encoder as Wu et al. wrote it: one token sequence per sample,
EACH TOKEN WITH ITS OWN POSITION EMBEDDING (``Fastformer``'s encoder only ever reads row 0).  ``Fastformer_wu(config, word_embedding)``
is a 4-way text classifier over it: ``forward(input_ids, targets) -> (loss, score)`` with ``score`` the ``[N, 4]`` logits and ``loss``
their mean cross-entropy.  Both are ``torch.nn.Module``s whose parameters carry exactly the reference's ``state_dict()`` names and
shapes (52 entries at two layers), so a reference checkpoint loads with ``strict=True``.  Each forward is ONE
``torch.autograd.Function`` over the C ABI and shares ``fastformer.py``'s engine: the Linear layers run on the exact-fp32 GEMM, the
layer stack on the kernels ``Fastformer`` runs, the embedding block on ``ebn_ff_ln_pos_fwd_f32`` and the head on the
``ebn_ff_cls_fwd_f32`` / ``ebn_ff_cls_bwd_f32`` pair.  There is no CPU fallback: construction, ``state_dict`` and ``load_state_dict``
work anywhere, ``forward`` without the library and a GPU raises ``RuntimeError``.

What the reference computes, reproduced on purpose:

* mask = ``input_ids != 0``; ``x = drop(LN(embedding_transform(word_embedding(ids)) + position_embeddings[t]))``, ``t`` the token's
  index; then the layers and the ``AttentionPooling`` of ``Fastformer`` (``exp`` without max-subtraction, times the mask, over
  ``sum + 1e-8``): a sequence that is all padding pools to an exact zero vector and its logits are ``output_layer.bias``;
* a sequence longer than ``config.max_position_embeddings`` raises ``IndexError`` (the reference's embedding lookup fails there);
* a passed ``word_embedding`` is re-initialised like every other Embedding (``reset_parameters``).

The loss is ``nn.CrossEntropyLoss()`` with its defaults: mean over the batch, stable log-softmax.  ``ignore_index`` is NOT supported:
every target must lie in ``[0, 4)``, and ``-100`` raises ``IndexError`` like any other value outside it (reported through a device flag
read at the forward's one host synchronisation, together with the token-id flag of the gather).  No class weights.

Dropout draws from the build's counter stream with ``Fastformer``'s site numbering: site 0 the embedding dropout, sites ``1 + 2 l`` and
``2 + 2 l`` layer ``l``; the mask of element ``(n, t, c)`` is that of flat index ``(n * T + t) * D + c``.  ``seed`` and ``dropout_step``
work as in ``Fastformer`` (each module keeps its own counter, advanced by every training-mode forward with dropout).

``attention="auto"`` is the default here: a sequence is a whole text, and the resident attention pair stops at 47 tokens when training
at hidden 256.  ``"resident"`` and ``"streamed"`` force a pair and raise ``fastformer.py``'s ``ValueError`` with that pair's limits, in
the forward.  The autograd limits are ``Fastformer``'s: a second backward through one forward, or a parameter changed in place between
forward and backward, raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from .fastformer import ATTENTIONS, AttentionPooling, Fastformer, FastformerLayer, _Engine, _f, dropout_key

N_CLASSES = 4  # fastformer_wu.py: output_layer = nn.Linear(hidden_size, 4)


def _check_config(config, attention):
    if getattr(config, "hidden_act", "gelu") != "gelu":
        raise ValueError(f"hidden_act = {config.hidden_act!r}: only 'gelu' (the exact erf form) has a kernel")
    if getattr(config, "pooler_type", "weightpooler") != "weightpooler":
        raise ValueError(f"pooler_type = {config.pooler_type!r}: only 'weightpooler' is supported")
    if attention not in ATTENTIONS:
        raise ValueError(f"attention = {attention!r}: one of {ATTENTIONS}")


def _check_device(what, module, *tensors):
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what}.forward needs the MI355X HIP library and a GPU: there is no CPU fallback")
    for t in list(tensors) + list(module.parameters()):
        if not t.is_cuda:
            raise RuntimeError(f"{what}.forward: parameters and inputs must be on the GPU (there is no CPU fallback)")
        if isinstance(t, nn.Parameter) and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError(f"{what}.forward: parameters must be contiguous float32")


# ---- the engine: fastformer.py's launches around the positional embedding block ------------------------------------------------------
class _WuEngine(_Engine):
    """`_Engine` over a StandardFastformerEncoder (self.m): the encoder's forward / backward from the embedding sum on."""

    def encode_fwd(self, Z, bias, mask, n_seq, T, p, keys, keep, pooler_index):
        """Z [n_seq*T, D] (embeddings before the position rows; bias [D] or None is added to them), mask [n_seq, T] float
        -> out [n_seq, D], what encode_bwd needs."""
        from ebrec._hip import ptr, stream_handle

        enc = self.m
        self.T = T
        R, D = Z.shape
        kind = self.attention_kind(T, keep)  # both directions' shape rules before anything runs
        h = torch.empty_like(Z)
        xhat0 = torch.empty_like(Z) if keep else None
        rstd0 = torch.empty(R, device=Z.device) if keep else None
        self.call("ebn_ff_ln_pos_fwd_f32", ptr(Z), ptr(bias), ptr(enc.position_embeddings.weight), ptr(enc.LayerNorm.weight),
                  ptr(enc.LayerNorm.bias), _f(self.eps), keys[0], _f(p), ptr(h), ptr(xhat0), ptr(rstd0), n_seq, T, D, stream_handle())
        attn_fwd = "ebn_ff_attn_fwd_f32" if kind == "resident" else "ebn_ff_attn_streamed_fwd_f32"
        h, layers = self.layers_fwd(enc.encoders, h, mask, n_seq, T, p, keys, keep, attn_fwd)
        out, sv_tok = self.pool_fwd(h, enc.poolers[pooler_index], mask, n_seq, T)
        saved = None
        if keep:
            saved = dict(n_seq=n_seq, T=T, xhat0=xhat0, rstd0=rstd0, layers=layers, hL=h, sv_tok=sv_tok, p=p, keys=keys, attention=kind,
                         pooler=pooler_index)
        return out, saved

    def encode_bwd(self, sv, dout, g, pre, need):
        """From dout [n_seq, D]: the encoder's parameter gradients into g under the prefix `pre`
        -> (dZ [n_seq*T, D], its column sum = the gradient of encode_fwd's `bias`)."""
        from ebrec._hip import ptr, stream_handle

        enc = self.m
        n_seq, T, p, keys = sv["n_seq"], sv["T"], sv["p"], sv["keys"]
        self.T = T
        D = self.D
        dh = torch.empty(n_seq * T, D, device=dout.device)
        self.pool_bwd(sv["hL"], enc.poolers[sv["pooler"]], sv["sv_tok"], dout, dh, n_seq, T, g, f"{pre}poolers.{sv['pooler']}.", need)
        dh = self.layers_bwd(enc.encoders, sv["layers"], dh, n_seq, T, p, keys, sv["attention"], g, pre + "encoders.", need)
        dZ, _, (dg, dbt, dbias) = self.ln_bwd(dh, sv["xhat0"], sv["rstd0"], enc.LayerNorm, 0, keys[0], p)
        g[pre + "LayerNorm.weight"], g[pre + "LayerNorm.bias"] = dg, dbt
        if need(pre + "position_embeddings.weight"):
            # dpos[t] = sum_n dX[n, t]: dX as n_seq "partials" of T * D floats, finished in ascending n; rows >= T are never read
            dpos = torch.zeros_like(enc.position_embeddings.weight)
            self.call("ebn_ff_colsum_finish_f32", ptr(dZ), n_seq, T * D, T * D, ptr(dpos), stream_handle())
            g[pre + "position_embeddings.weight"] = dpos
        return dZ, dbias


def _stale_check(ctx, what):
    if ctx.spent:
        raise RuntimeError(f"{what}: a second backward through the same forward; the first one released (and partly overwrote) the "
                           "saved activations, retain_graph=True is not supported: run the forward again")
    if ctx.saved is None:
        raise RuntimeError(f"{what}: backward through a forward that kept no activations")
    for n, t, v in zip(ctx.names, ctx.params, ctx.versions):  # the backward reads the parameters themselves: they must be unchanged
        if t._version != v:
            raise RuntimeError(f"{what}: parameter {n} was modified in place between forward and backward (version {v} -> "
                               f"{t._version}); call backward() before optimizer.step()")


def _remember(ctx, module, saved, names, keep, params):
    ctx.module, ctx.saved, ctx.names = module, saved, names
    ctx.versions = [t._version for t in params] if keep else None
    ctx.params = params if keep else None
    ctx.spent = False
    ctx.req = [t.requires_grad for t in params]


def _grads(ctx, g):
    out = [g[n].view_as(ctx.module.get_parameter(n)) if (r and n in g) else None for n, r in zip(ctx.names, ctx.req)]
    ctx.saved, ctx.params, ctx.spent = None, None, True
    return out


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, mask, pooler_index, p, keys, names, keep, x, *params):
        n_seq, T, D = x.shape
        out, saved = enc._engine.encode_fwd(x.reshape(n_seq * T, D), None, mask, n_seq, T, p, keys, keep, pooler_index)
        _remember(ctx, enc, saved, names, keep, params)
        ctx.x_shape, ctx.x_req = x.shape, x.requires_grad
        return out

    @staticmethod
    def backward(ctx, dout):
        _stale_check(ctx, "StandardFastformerEncoder")
        req = dict(zip(ctx.names, ctx.req))
        g = {}
        dZ, _ = ctx.module._engine.encode_bwd(ctx.saved, dout.contiguous().to(torch.float32), g, "", lambda n: req.get(n, False))
        grads = _grads(ctx, g)
        return (None, None, None, None, None, None, None, dZ.view(ctx.x_shape) if ctx.x_req else None, *grads)


class _WuFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, ids, targets, p, keys, names, keep, *params):
        from ebrec._hip import ptr, stream_handle

        enc = model.fastformer_model
        eng = enc._engine
        N, T = ids.shape
        D, C = eng.D, N_CLASSES
        dev = ids.device
        table = model.word_embedding.weight
        V, E = table.shape
        R = N * T
        mask = (ids != 0).to(torch.float32).contiguous()
        eng.T = T
        eng.attention_kind(T, keep)  # a shape no attention pair takes is an error before the first launch
        X0 = torch.empty(R, E, device=dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)  # [token id outside the table, target outside the classes]
        eng.call("ebn_gather_rows_f32", ptr(ids), ptr(table), ptr(X0), R, E, V, None, -1, _f(0), ptr(flags), stream_handle())
        Z = eng.linear(X0, model.embedding_transform.weight, torch.empty(R, D, device=dev))
        TV, saved = eng.encode_fwd(Z, model.embedding_transform.bias, mask, N, T, p, keys, keep, 0)
        del Z
        score, prob = torch.empty(N, C, device=dev), torch.empty(N, C, device=dev)
        rowloss, loss = torch.empty(N, device=dev), torch.empty(1, device=dev)
        out = model.output_layer
        eng.call("ebn_ff_cls_fwd_f32", ptr(TV), ptr(out.weight), ptr(out.bias), ptr(targets), ptr(score), ptr(prob), ptr(rowloss), ptr(loss),
                 ptr(flags[1:]), N, D, C, stream_handle())
        bad_id, bad_target = flags.tolist()  # the forward's one host synchronisation
        if bad_id:
            raise IndexError(f"token id outside the word table [0, {V})")
        if bad_target:
            raise IndexError(f"target outside the classes [0, {C}) (ignore_index is not supported)")
        if keep:
            saved.update(ids=ids, X0=X0, TV=TV, prob=prob, targets=targets)
        _remember(ctx, model, saved, names, keep, params)
        ctx.set_materialize_grads(False)
        return loss.view(()), score

    @staticmethod
    def backward(ctx, dloss, dscore):
        from ebrec import _hip
        from ebrec._hip import ptr, stream_handle

        _stale_check(ctx, "Fastformer_wu")
        model, sv = ctx.module, ctx.saved
        eng = model.fastformer_model._engine
        req = dict(zip(ctx.names, ctx.req))
        need = lambda n: req.get(n, False)
        TV = sv["TV"]
        N, D = TV.shape
        C = N_CLASSES
        dev = TV.device
        dloss = None if dloss is None else dloss.contiguous().to(torch.float32)
        dscore = None if dscore is None else dscore.contiguous().to(torch.float32)
        g = {}
        out = model.output_layer
        dTV = torch.empty(N, D, device=dev)
        part = torch.empty(int(_hip.lib().ebn_ff_cls_partials_len(N, D, C)), device=dev)
        n = ctypes.c_int32(0)
        eng.call("ebn_ff_cls_bwd_f32", ptr(TV), ptr(out.weight), ptr(sv["prob"]), ptr(sv["targets"]), ptr(dloss), ptr(dscore), ptr(dTV),
                 ptr(part), ctypes.byref(n), N, D, C, stream_handle())
        s = eng.finish(part, n.value, C * D + C, C * D + C)
        g["output_layer.weight"], g["output_layer.bias"] = s[:C * D], s[C * D:]
        dZ, dbias = eng.encode_bwd(sv, dTV, g, "fastformer_model.", need)
        g["embedding_transform.bias"] = dbias
        X0 = sv["X0"]
        if need("embedding_transform.weight"):
            g["embedding_transform.weight"] = eng.back_weight(dZ, X0)
        if need("word_embedding.weight"):  # a frozen table: no scatter launch
            g["word_embedding.weight"] = eng.table_grad(model.word_embedding.weight, sv["ids"], dZ, model.embedding_transform.weight, X0)
        grads = _grads(ctx, g)
        return (None, None, None, None, None, None, None, *grads)


# ---- the modules --------------------------------------------------------------------------------------------------------------------
class _DropoutStream:
    """seed / dropout_step as Fastformer keeps them."""

    def _draw(self):
        """-> (p, keys) of this forward; a training-mode forward with dropout advances the step counter"""
        p = float(self.config.hidden_dropout_prob) if self.training else 0.0
        if p > 0.0:
            self.dropout_step += 1
        return p, tuple(dropout_key(self.seed, self.dropout_step, s) for s in range(1 + 2 * self.config.num_hidden_layers))


class StandardFastformerEncoder(_DropoutStream, nn.Module):
    """See the module docstring.  ``forward(input_embs [N, T, D] float32, attention_mask [N, T], pooler_index=0) -> [N, D]``,
    differentiable with respect to the parameters and ``input_embs``."""

    def __init__(self, config, pooler_count: int = 1, *, seed: int = 0, attention: str = "auto"):
        super().__init__()
        _check_config(config, attention)
        self.config = config
        self.attention = attention
        self.seed = int(seed)
        self.dropout_step = 0
        self.encoders = nn.ModuleList([FastformerLayer(config) for _ in range(config.num_hidden_layers)])
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.poolers = nn.ModuleList([AttentionPooling(config) for _ in range(pooler_count)])
        self.reset_parameters()
        self._engine = _WuEngine(self)

    reset_parameters = Fastformer.reset_parameters  # the reference's init_weights: it is the same in both files

    def _check_length(self, T):
        if T > self.position_embeddings.weight.shape[0]:
            raise IndexError(f"a sequence of {T} tokens is longer than max_position_embeddings = {self.position_embeddings.weight.shape[0]}")

    def forward(self, input_embs, attention_mask, pooler_index: int = 0) -> torch.Tensor:
        from ebrec import _hip

        if input_embs.dim() != 3 or input_embs.shape[2] != self.config.hidden_size or tuple(attention_mask.shape) != tuple(input_embs.shape[:2]):
            raise ValueError(f"input_embs (N, T, {self.config.hidden_size}) and attention_mask (N, T) expected, got {tuple(input_embs.shape)} and "
                             f"{tuple(attention_mask.shape)}")
        if not 0 <= pooler_index < len(self.poolers):
            raise IndexError(f"pooler_index = {pooler_index}: the encoder has {len(self.poolers)} pooler(s)")
        self._check_length(input_embs.shape[1])
        _check_device("StandardFastformerEncoder", self, input_embs, attention_mask)
        _hip.lib()
        if input_embs.dtype != torch.float32:
            raise RuntimeError("StandardFastformerEncoder.forward: input_embs must be float32")
        p, keys = self._draw()
        names, params = zip(*self.named_parameters())
        x = input_embs.contiguous()
        keep = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in params))
        mask = attention_mask.to(torch.float32).contiguous()
        return _EncoderFn.apply(self, mask, pooler_index, p, keys, names, keep, x, *params)


class Fastformer_wu(_DropoutStream, nn.Module):
    """See the module docstring.  ``config``: a ``BertConfig`` or any object with ``hidden_size``, ``num_attention_heads``,
    ``num_hidden_layers``, ``intermediate_size``, ``max_position_embeddings``, ``hidden_dropout_prob``, ``layer_norm_eps``,
    ``initializer_range``, ``hidden_act``, ``pooler_type``.  ``forward(input_ids [N, T] int, targets [N] int64) -> (loss, score)``;
    every target must lie in [0, 4): ``ignore_index`` (-100) is not supported and raises ``IndexError``."""

    def __init__(self, config, word_embedding: nn.Embedding, *, seed: int = 0, attention: str = "auto"):
        super().__init__()
        _check_config(config, attention)
        self.config = config
        self.seed = int(seed)
        self.dropout_step = 0
        self.word_embedding = word_embedding
        self.embedding_transform = nn.Linear(word_embedding.weight.shape[1], config.hidden_size)
        self.output_layer = nn.Linear(config.hidden_size, N_CLASSES)
        self.fastformer_model = StandardFastformerEncoder(config, seed=seed, attention=attention)
        self.reset_parameters()

    @property
    def attention(self):
        return self.fastformer_model.attention

    reset_parameters = Fastformer.reset_parameters  # a passed word_embedding too; a padding row, if the table declares one, zeroed

    def forward(self, input_ids, targets):
        from ebrec import _hip

        if input_ids.dim() != 2 or targets.dim() != 1 or targets.shape[0] != input_ids.shape[0]:
            raise ValueError(f"input_ids (N, T) and targets (N,) expected, got {tuple(input_ids.shape)} and {tuple(targets.shape)}")
        self.fastformer_model._check_length(input_ids.shape[1])
        _check_device("Fastformer_wu", self, input_ids, targets)
        _hip.lib()
        p, keys = self._draw()
        names, params = zip(*self.named_parameters())
        keep = torch.is_grad_enabled() and any(t.requires_grad for t in params)  # decided here: grad mode is off inside Function.forward
        ids = input_ids.to(torch.int32).contiguous()
        return _WuFn.apply(self, ids, targets.to(torch.int64).contiguous(), p, keys, names, keep, *params)
