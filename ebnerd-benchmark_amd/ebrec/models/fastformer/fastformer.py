"""Fastformer (reference models/fastformer/fastformer.py) on the MI355X.

``Fastformer(config, word_embedding=None)`` is a ``torch.nn.Module`` whose parameters carry exactly the reference's
``state_dict()`` names and shapes, so a reference checkpoint loads with ``strict=True``.  The whole forward is ONE
``torch.autograd.Function`` over the C ABI: the Linear layers run on the exact-fp32 MFMA GEMM, everything between them on
the kernels of ``csrc/ebn_fastformer.hip``; torch does the loss and the optimizer.  There is no CPU fallback: construction,
``state_dict`` and ``load_state_dict`` work anywhere, ``forward`` without the library and a GPU raises ``RuntimeError``.

What the reference computes, reproduced on purpose:

* only row 0 of ``position_embeddings`` is ever used (the encoder sees one article at a time), for every token;
* ``query_att`` / ``key_att`` read the whole D-wide row for each head's logit, not the head's slice;
* ``AttentionPooling`` is ``exp`` without max-subtraction, times the mask, over ``sum + 1e-8``;
* in ``user_encoder`` the token mask of history slot 0 is applied to ALL history slots of that sample, and the history mask
  is ``token 0 != 0`` per slot.  With left-padded histories a user whose first slot is padding gets an all-zero user vector.
  ``token_mask="per_slot"`` (keyword-only; default ``"first_slot"``) uses each slot's own token mask instead;
* a passed ``word_embedding`` is re-initialised like every other Embedding (``reset_parameters``).

The reference also runs the news encoder twice per history slot and drops the first result; that has no numerical effect and
is not reproduced.  Dropout draws from this build's counter-based stream (statistical parity with torch only): site 0 is the
embedding dropout, sites ``1 + 2 l`` and ``2 + 2 l`` the two dropouts of layer ``l``; the module keeps the step counter
(``dropout_step``, advanced by every training-mode forward).  The logit biases ``query_att.bias`` / ``key_att.bias`` have
identically zero gradients (a softmax does not see a shift of its logits) and get exact zeros.

The attention core has two kernel pairs (keyword-only ``attention``):

* ``"resident"`` (default) keeps a sequence's Q rows in LDS: ``heads * hidden_size <= 4096`` and 64 KiB of LDS for ``T * (hidden_size
  + 4)`` floats plus the rest, i.e. hidden 256 / 16 heads with at most 47 tokens per title when training;
* ``"streamed"`` (``csrc/ebn_fastformer_streamed.hip``) re-reads Q and K from global memory and leaves the logit weights' gradients
  to the split-K GEMM: ``hidden_size <= 1024`` with any number of heads, LDS ``4 * (heads * T + T + 2 * hidden_size)`` bytes forward
  and ``4 * (2 * heads * T + 4 * hidden_size)`` backward (hidden 768 / 12 heads: 554 tokens when training);
* ``"auto"`` takes the resident pair wherever it accepts the shape (for both directions when the forward keeps activations) -- then
  bit-identical to the default -- and the streamed pair otherwise.

The option changes no parameter.  Limits of the autograd Function: the backward reads the parameters themselves and releases (and partly overwrites) the saved
activations, so a parameter changed in place between forward and backward, or a second backward through the same forward
(``retain_graph=True``), raises ``RuntimeError``.  The shape rules of both directions are checked at the start of a forward that
keeps activations.  An eager step synchronises with the host twice (the out-of-range flags of the gather and of the fixed-point
scatter).
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn

_M32 = 0xFFFFFFFF
TOKEN_MASKS = ("first_slot", "per_slot")
ATTENTIONS = ("resident", "streamed", "auto")


def _lowbias32(x: int) -> int:
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def dropout_key(seed: int, step: int, site: int) -> int:
    """The 32-bit key of (seed, step, call site) of the build's counter-based dropout stream (csrc/ebn_common.h)."""
    k = _lowbias32((seed & _M32) ^ 0x9E3779B9)
    k = (k + (step & _M32) * 0x85EBCA6B + (site & _M32) * 0xC2B2AE35) & _M32
    return _lowbias32(k)


# ---- parameter containers with the reference's names ------------------------------------------------------------------------
class AttentionPooling(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.att_fc1 = nn.Linear(config.hidden_size, config.hidden_size)
        self.att_fc2 = nn.Linear(config.hidden_size, 1)


class FastSelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        D, h = config.hidden_size, config.num_attention_heads
        if D % h != 0:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)" % (D, h))
        self.query = nn.Linear(D, D)
        self.query_att = nn.Linear(D, h)
        self.key = nn.Linear(D, D)
        self.key_att = nn.Linear(D, h)
        self.transform = nn.Linear(D, D)


class _DenseNorm(nn.Module):
    """BertSelfOutput / BertOutput: dense, dropout, LayerNorm(h + input)."""

    def __init__(self, d_in, d_out, eps):
        super().__init__()
        self.dense = nn.Linear(d_in, d_out)
        self.LayerNorm = nn.LayerNorm(d_out, eps=eps)


class _Dense(nn.Module):
    def __init__(self, d_in, d_out):
        super().__init__()
        self.dense = nn.Linear(d_in, d_out)


class FastAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.self = FastSelfAttention(config)
        self.output = _DenseNorm(config.hidden_size, config.hidden_size, config.layer_norm_eps)


class FastformerLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.attention = FastAttention(config)
        self.intermediate = _Dense(config.hidden_size, config.intermediate_size)
        self.output = _DenseNorm(config.intermediate_size, config.hidden_size, config.layer_norm_eps)


class SequenceFastformerEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.encoders = nn.ModuleList([FastformerLayer(config) for _ in range(config.num_hidden_layers)])
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.poolers = nn.ModuleList([AttentionPooling(config)])


# ---- the engine: launches only ---------------------------------------------------------------------------------------------------
def _f(x):
    return ctypes.c_float(float(x))


class _Engine:
    """One forward / backward of the model as C-ABI launches on the current stream."""

    def __init__(self, model):
        self.m = model
        cfg = model.config
        self.D, self.heads, self.layers, self.I = cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers, cfg.intermediate_size
        self.eps = float(cfg.layer_norm_eps)
        self._ws = {}

    # -- plumbing
    def call(self, name, *args):
        from ebrec import _hip

        rc = getattr(_hip.lib(), name)(*args)
        if rc == -2:
            shape = (f"hidden_size = {self.D}, heads = {self.heads}, intermediate_size = {self.I}, tokens per title = "
                     f"{getattr(self, 'T', '?')}")
            if name.startswith("ebn_ff_attn_streamed"):
                raise ValueError(
                    f"{name}: shape outside what the streamed Fastformer attention kernels are built for ({shape}).  Limits: hidden_size % 4 "
                    "== 0, hidden_size <= 1024, T <= 4096, and per sequence 4 * (heads * T + T + 2 * hidden_size) bytes (forward) and 4 * (2 * "
                    "heads * T + 4 * hidden_size) bytes (backward) <= 64 KiB of LDS")
            if name.startswith("ebn_ff_attn"):
                raise ValueError(
                    f"{name}: shape outside what the Fastformer attention kernels are built for ({shape}).  Limits: hidden_size % 4 == 0, "
                    "hidden_size <= 1024, heads * hidden_size <= 4096, and per sequence 4 * (T * (hidden_size + 4) + 6 * hidden_size + "
                    "heads * T + T) bytes (forward) and 4 * (T * (hidden_size + 4) + 4 * hidden_size + 4 * heads * T) bytes (backward) "
                    "<= 64 KiB of LDS.  Fastformer(..., attention=\"auto\") takes the streamed kernels, which keep no sequence in LDS, for "
                    "such shapes")
            raise ValueError(f"{name}: shape outside the kernel's supported range ({shape}); LayerNorm needs hidden_size <= 1024, "
                             "the pooling a history size <= 4096 (see include/ebnerd_hip.h)")
        if rc != 0:
            msg = _hip.lib().ebn_error_string(rc)
            raise _hip.HipError(f"{name} failed with code {rc}: {msg.decode() if msg else '?'}")

    def linear(self, x, W, out, beta=0.0):
        """out [R, n_out] = x [R, n_in] . W^T (+ beta * out), W [n_out, n_in] as torch keeps it."""
        from ebrec._hip import ptr, stream_handle

        n_out, n_in = W.shape
        self.call("ebn_gemm_f32", 0, 1, x.shape[0], n_out, n_in, _f(1), ptr(x), n_in, ptr(W), n_in, _f(beta), ptr(out), n_out, stream_handle())
        return out

    def back_data(self, dy, W, out, beta=0.0):
        """out [R, n_in] = dy [R, n_out] . W (+ beta * out)."""
        from ebrec._hip import ptr, stream_handle

        n_out, n_in = W.shape
        self.call("ebn_gemm_f32", 0, 0, dy.shape[0], n_in, n_out, _f(1), ptr(dy), n_out, ptr(W), n_in, _f(beta), ptr(out), n_in, stream_handle())
        return out

    def back_weight(self, dy, x, alpha=1.0):
        """dW [n_out, n_in] = alpha * dy^T . x with deterministic split-K over the rows."""
        from ebrec import _hip
        from ebrec._hip import ptr, stream_handle

        R, n_out, n_in = dy.shape[0], dy.shape[1], x.shape[1]
        n_ws = int(_hip.lib().ebn_gemm_workspace_floats(n_out, n_in, R))
        ws = self._ws.get((dy.device, n_ws))
        if ws is None:
            ws = self._ws[(dy.device, n_ws)] = torch.empty(max(n_ws, 1), device=dy.device)
        dW = torch.empty(n_out, n_in, device=dy.device)
        self.call("ebn_gemm_f32_ws", 1, 0, n_out, n_in, R, _f(alpha), ptr(dy), n_out, ptr(x), n_in, _f(0), ptr(dW), n_in, ptr(ws), n_ws, stream_handle())
        return dW

    def finish(self, partials, n_parts, stride, width):
        from ebrec._hip import ptr, stream_handle

        out = torch.empty(width, device=partials.device)
        self.call("ebn_ff_colsum_finish_f32", ptr(partials), n_parts, stride, width, ptr(out), stream_handle())
        return out

    def ln_fwd(self, X, bias, res, ln, mode, key, p, keep):
        from ebrec._hip import ptr, stream_handle

        R, D = X.shape
        Y = torch.empty_like(X)
        xhat = torch.empty_like(X) if keep else None
        rstd = torch.empty(R, device=X.device) if keep else None
        self.call("ebn_ff_ln_fwd_f32", ptr(X), ptr(bias), ptr(res), ptr(ln.weight), ptr(ln.bias), _f(self.eps), mode, key, _f(p), ptr(Y),
                  ptr(xhat), ptr(rstd), R, D, stream_handle())
        return Y, xhat, rstd

    def ln_bwd(self, dY, xhat, rstd, ln, mode, key, p):
        """-> dX, dres (mode 1), (dgamma, dbeta, dbias)"""
        from ebrec import _hip
        from ebrec._hip import ptr, stream_handle

        R, D = dY.shape
        dX = torch.empty_like(dY)
        dres = torch.empty_like(dY) if mode == 1 else None
        part = torch.empty(int(_hip.lib().ebn_ff_ln_partials_len(R, D)), device=dY.device)
        n = ctypes.c_int32(0)
        self.call("ebn_ff_ln_bwd_f32", ptr(dY), ptr(xhat), ptr(rstd), ptr(ln.weight), mode, key, _f(p), ptr(dX), ptr(dres), ptr(part),
                  ctypes.byref(n), R, D, stream_handle())
        s = self.finish(part, n.value, 3 * D, 3 * D)
        return dX, dres, (s[:D], s[D:2 * D], s[2 * D:])

    def pool_fwd(self, X, pool, mask, n_seq, L):
        from ebrec._hip import ptr, stream_handle

        D = self.D
        U = self.linear(X, pool.att_fc1.weight, torch.empty(n_seq * L, D, device=X.device))
        out, w, sinv = torch.empty(n_seq, D, device=X.device), torch.empty(n_seq, L, device=X.device), torch.empty(n_seq, device=X.device)
        self.call("ebn_ff_pool_fwd_f32", ptr(U), ptr(pool.att_fc1.bias), ptr(pool.att_fc2.weight), ptr(pool.att_fc2.bias), ptr(X), ptr(mask),
                  ptr(out), ptr(w), ptr(sinv), n_seq, L, D, stream_handle())
        return out, (U, w, sinv)

    def pool_bwd(self, X, pool, saved, dout, dX, n_seq, L, grads, prefix, need):
        """dX (a [n_seq*L, D] buffer or view) <- dL/dX; parameter gradients into `grads`."""
        from ebrec import _hip
        from ebrec._hip import ptr, stream_handle

        D = self.D
        U, w, sinv = saved
        dev = X.device
        de, db2n = torch.empty(n_seq * L, device=dev), torch.empty(n_seq, device=dev)
        self.call("ebn_ff_pool_bwd_f32", ptr(X), ptr(w), ptr(sinv), ptr(dout), ptr(dX), ptr(de), ptr(db2n), n_seq, L, D, stream_handle())
        part = torch.empty(int(_hip.lib().ebn_attpool_partials_len(n_seq * L, D)), device=dev)
        dw2, db1, db2 = torch.empty(1, D, device=dev), torch.empty(D, device=dev), torch.empty(1, device=dev)
        _hip.call("ebn_attpool_bwd_dpre_f32", ptr(U), ptr(pool.att_fc2.weight), ptr(de), ptr(dw2), ptr(db1), ptr(part), n_seq * L, D, 0,
                  stream_handle())  # U is d(pre-tanh) now
        _hip.call("ebn_sum_f32", ptr(db2n), n_seq, _f(1), ptr(db2), 0, stream_handle())
        grads[prefix + "att_fc2.weight"], grads[prefix + "att_fc1.bias"], grads[prefix + "att_fc2.bias"] = dw2, db1, db2
        if need(prefix + "att_fc1.weight"):
            grads[prefix + "att_fc1.weight"] = self.back_weight(U, X)
        self.back_data(U, pool.att_fc1.weight, dX, beta=1.0)

    def attention_kind(self, T, keep):
        """"resident" or "streamed" for sequences of T tokens, by the model's `attention` option; raises ValueError with the limits of
        the pair it settles on when that pair does not take the shape (both directions when `keep`: a training step must not learn its
        limit inside loss.backward())."""
        from ebrec import _hip

        want, both = self.m.attention, 1 if keep else 0
        if want == "auto":
            want = "resident" if _hip.lib().ebn_ff_attn_supported(T, self.D, self.heads, both) == 0 else "streamed"
        self.call("ebn_ff_attn_supported" if want == "resident" else "ebn_ff_attn_streamed_supported", T, self.D, self.heads, both)
        return want

    # -- the model
    def masks(self, hist, cand, token_mask):
        N, H, T = hist.shape
        tok = hist != 0
        hmask = tok[:, :, 0].to(torch.float32).contiguous()
        if token_mask == "first_slot":
            tok = tok[:, 0:1, :].expand(N, H, T)
        mask = torch.cat([tok.reshape(N * H, T), (cand != 0).reshape(N, T)], 0).to(torch.float32).contiguous()
        return mask, hmask

    def forward(self, hist, cand, p, keys, keep, token_mask):
        from ebrec._hip import ptr, stream_handle

        m = self.m
        N, H, T = hist.shape
        self.T = T
        D = self.D
        dev = hist.device
        table = m.word_embedding.weight
        V, E = table.shape
        n_seq = N * (H + 1)
        R = n_seq * T
        ids = torch.cat([hist.reshape(N * H, T), cand.reshape(N, T)], 0).to(torch.int32).contiguous()
        mask, hmask = self.masks(hist, cand, token_mask)
        S = stream_handle
        # both directions' shape rules before anything runs: a training step must not learn its limit inside loss.backward()
        kind = self.attention_kind(T, keep)
        attn_fwd = "ebn_ff_attn_fwd_f32" if kind == "resident" else "ebn_ff_attn_streamed_fwd_f32"
        X0 = torch.empty(R, E, device=dev)
        oob = torch.zeros(1, dtype=torch.int32, device=dev)
        self.call("ebn_gather_rows_f32", ptr(ids), ptr(table), ptr(X0), R, E, V, None, -1, _f(0), ptr(oob), S())
        Z = self.linear(X0, m.embedding_transform.weight, torch.empty(R, D, device=dev))
        enc = m.news_encoder
        h, xhat0, rstd0 = self.ln_fwd(Z, m.embedding_transform.bias, enc.position_embeddings.weight, enc.LayerNorm, 0, keys[0], p, keep)
        del Z
        h, saved_layers = self.layers_fwd(enc.encoders, h, mask, n_seq, T, p, keys, keep, attn_fwd)
        NV, sv_tok = self.pool_fwd(h, enc.poolers[0], mask, n_seq, T)
        HV = NV[:N * H]
        user, sv_user = self.pool_fwd(HV, m.user_attention_polling, hmask, N, H)
        CV = NV[N * H:]
        score = torch.empty(N, device=dev)
        self.call("ebn_ff_head_fwd_f32", ptr(user), ptr(CV), ptr(m.output_layer.weight), ptr(m.output_layer.bias), ptr(score), N, D, S())
        if int(oob.item()) != 0:
            raise IndexError(f"token id outside the word table [0, {V})")
        saved = None
        if keep:
            saved = dict(N=N, H=H, T=T, ids=ids, X0=X0, xhat0=xhat0, rstd0=rstd0, layers=saved_layers, hL=h, NV=NV, sv_tok=sv_tok,
                         user=user, sv_user=sv_user, score=score, p=p, keys=keys, attention=kind)
        return score, saved, (user, NV)

    def layers_fwd(self, encoders, h, mask, n_seq, T, p, keys, keep, attn_fwd):
        """The FastformerLayer stack over h [n_seq*T, D] (shared with fastformer_wu.py) -> (h, what the backward needs per layer)."""
        from ebrec._hip import ptr, stream_handle

        D, heads, I = self.D, self.heads, self.I
        dev = h.device
        R = n_seq * T
        S = stream_handle
        saved_layers = []
        for l, layer in enumerate(encoders):
            at = layer.attention.self
            Q = self.linear(h, at.query.weight, torch.empty(R, D, device=dev))
            K = self.linear(h, at.key.weight, torch.empty(R, D, device=dev))
            AO, SV = torch.empty(R, D, device=dev), torch.empty(R, D, device=dev)
            qw, kw = torch.empty(n_seq, heads, T, device=dev), torch.empty(n_seq, heads, T, device=dev)
            pq, pk = torch.empty(n_seq, D, device=dev), torch.empty(n_seq, D, device=dev)
            self.call(attn_fwd, ptr(Q), ptr(K), ptr(at.query.bias), ptr(at.key.bias), ptr(at.transform.bias), ptr(at.query_att.weight),
                      ptr(at.query_att.bias), ptr(at.key_att.weight), ptr(at.key_att.bias), ptr(mask), ptr(AO), ptr(SV), ptr(qw), ptr(kw),
                      ptr(pq), ptr(pk), n_seq, T, D, heads, S())
            self.linear(AO, at.transform.weight, SV, beta=1.0)  # SV = transform(AO) + mixed_query_layer
            so = layer.attention.output
            Y1 = self.linear(SV, so.dense.weight, torch.empty(R, D, device=dev))
            A1, xh1, rs1 = self.ln_fwd(Y1, so.dense.bias, h, so.LayerNorm, 1, keys[1 + 2 * l], p, keep)
            del Y1
            I1 = self.linear(A1, layer.intermediate.dense.weight, torch.empty(R, I, device=dev))
            G = torch.empty(R, I, device=dev)
            self.call("ebn_ff_gelu_fwd_f32", ptr(I1), ptr(layer.intermediate.dense.bias), ptr(G), R, I, S())
            O = self.linear(G, layer.output.dense.weight, torch.empty(R, D, device=dev))
            hn, xh2, rs2 = self.ln_fwd(O, layer.output.dense.bias, A1, layer.output.LayerNorm, 1, keys[2 + 2 * l], p, keep)
            del O
            if keep:
                saved_layers.append((h, Q, K, AO, SV, qw, kw, pq, pk, xh1, rs1, A1, I1, G, xh2, rs2))
            h = hn
        return h, saved_layers

    def backward(self, sv, dscore, need):
        """-> {parameter name: gradient}"""
        from ebrec._hip import ptr, stream_handle

        m = self.m
        N, H, T, p, keys = sv["N"], sv["H"], sv["T"], sv["p"], sv["keys"]
        self.T = T
        D = self.D
        n_seq = N * (H + 1)
        R = n_seq * T
        NV = sv["NV"]
        dev = NV.device
        S = stream_handle
        g = {}
        enc = m.news_encoder
        HV, CV = NV[:N * H], NV[N * H:]
        dNV, duser = torch.empty(n_seq, D, device=dev), torch.empty(N, D, device=dev)
        dW, db = torch.empty(1, 2 * D, device=dev), torch.empty(1, device=dev)
        self.call("ebn_ff_head_bwd_f32", ptr(sv["user"]), ptr(CV), ptr(m.output_layer.weight), ptr(sv["score"]), ptr(dscore), ptr(duser),
                  ptr(dNV[N * H:]), ptr(dW), ptr(db), N, D, S())
        g["output_layer.weight"], g["output_layer.bias"] = dW, db
        self.pool_bwd(HV, m.user_attention_polling, sv["sv_user"], duser, dNV[:N * H], N, H, g, "user_attention_polling.", need)
        dh = torch.empty(R, D, device=dev)
        self.pool_bwd(sv["hL"], enc.poolers[0], sv["sv_tok"], dNV, dh, n_seq, T, g, "news_encoder.poolers.0.", need)
        dh = self.layers_bwd(enc.encoders, sv["layers"], dh, n_seq, T, p, keys, sv["attention"], g, "news_encoder.encoders.", need)
        dZ, _, (dg, dbt, dbias) = self.ln_bwd(dh, sv["xhat0"], sv["rstd0"], enc.LayerNorm, 0, keys[0], p)
        g["news_encoder.LayerNorm.weight"], g["news_encoder.LayerNorm.bias"], g["embedding_transform.bias"] = dg, dbt, dbias
        if need("news_encoder.position_embeddings.weight"):
            dpos = torch.zeros_like(enc.position_embeddings.weight)
            dpos[0].copy_(dbias)  # only row 0 is ever read
            g["news_encoder.position_embeddings.weight"] = dpos
        X0 = sv["X0"]
        if need("embedding_transform.weight"):
            g["embedding_transform.weight"] = self.back_weight(dZ, X0)
        if need("word_embedding.weight"):
            g["word_embedding.weight"] = self.table_grad(m.word_embedding.weight, sv["ids"], dZ, m.embedding_transform.weight, X0)
        return g

    def table_grad(self, table, ids, dZ, Wt, X0):
        """The word table's gradient from dZ [R, D] behind embedding_transform (weight Wt): dX0 = dZ . Wt into X0's buffer (not needed
        any more), then the fixed-point scatter by ids [R]."""
        from ebrec import _hip
        from ebrec._hip import ptr, stream_handle

        V, E = table.shape
        R, dev = X0.shape[0], X0.device
        dX0 = self.back_data(dZ, Wt, X0)
        acc = getattr(self, "_acc", None)
        if acc is None or acc.numel() != V * E or acc.device != dev:
            acc = self._acc = torch.zeros(V * E, dtype=torch.int64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        dT = torch.empty(V, E, device=dev)
        _hip.call("ebn_embedding_grad_scatter_fixed", ptr(ids), ptr(dX0), ptr(acc), R, E, V, None, -1, _f(0), ptr(flag), stream_handle())
        _hip.call("ebn_fixed_to_f32", ptr(acc), ptr(dT), V * E, ptr(flag), stream_handle())  # re-zeroes the accumulator
        if int(flag.item()) != 0:
            raise FloatingPointError("word-table gradient outside the fixed-point accumulator's range")
        return dT

    def layers_bwd(self, encoders, saved_layers, dh, n_seq, T, p, keys, kind, g, prefix, need):
        """The backward of layers_fwd from dh [n_seq*T, D]: parameter gradients into g under `prefix`, -> dL/d(the stack's input)."""
        from ebrec import _hip
        from ebrec._hip import ptr, stream_handle

        D, heads = self.D, self.heads
        R = n_seq * T
        dev = dh.device
        S = stream_handle
        for l in range(len(saved_layers) - 1, -1, -1):
            layer = encoders[l]
            at, so = layer.attention.self, layer.attention.output
            h, Q, K, AO, SV, qw, kw, pq, pk, xh1, rs1, A1, I1, G, xh2, rs2 = saved_layers[l]
            pre = f"{prefix}{l}."
            dO, dA1, (dg, dbt, dbias) = self.ln_bwd(dh, xh2, rs2, layer.output.LayerNorm, 1, keys[2 + 2 * l], p)
            g[pre + "output.LayerNorm.weight"], g[pre + "output.LayerNorm.bias"], g[pre + "output.dense.bias"] = dg, dbt, dbias
            if need(pre + "output.dense.weight"):
                g[pre + "output.dense.weight"] = self.back_weight(dO, G)
            dG = self.back_data(dO, layer.output.dense.weight, torch.empty_like(G))
            dbi = torch.empty(self.I, device=dev)
            part = torch.empty(int(_hip.lib().ebn_colsum_partials_len(R, self.I)), device=dev)
            self.call("ebn_ff_gelu_bwd_f32", ptr(I1), ptr(layer.intermediate.dense.bias), ptr(dG), ptr(dG), ptr(dbi), ptr(part), R, self.I, S())
            g[pre + "intermediate.dense.bias"] = dbi
            if need(pre + "intermediate.dense.weight"):
                g[pre + "intermediate.dense.weight"] = self.back_weight(dG, A1)
            self.back_data(dG, layer.intermediate.dense.weight, dA1, beta=1.0)
            del dG, dO
            dY1, dh_in, (dg, dbt, dbias) = self.ln_bwd(dA1, xh1, rs1, so.LayerNorm, 1, keys[1 + 2 * l], p)
            g[pre + "attention.output.LayerNorm.weight"], g[pre + "attention.output.LayerNorm.bias"] = dg, dbt
            g[pre + "attention.output.dense.bias"] = dbias
            if need(pre + "attention.output.dense.weight"):
                g[pre + "attention.output.dense.weight"] = self.back_weight(dY1, SV)
            dSV = self.back_data(dY1, so.dense.weight, torch.empty(R, D, device=dev))
            if need(pre + "attention.self.transform.weight"):
                g[pre + "attention.self.transform.weight"] = self.back_weight(dSV, AO)
            dAO = self.back_data(dSV, at.transform.weight, dY1)  # dY1's buffer is free again
            dQ, dK = torch.empty(R, D, device=dev), torch.empty(R, D, device=dev)
            n = ctypes.c_int32(0)
            a = pre + "attention.self."
            if kind == "resident":
                width = 2 * heads * D + 3 * D
                part = torch.empty(int(_hip.lib().ebn_ff_attn_partials_len(n_seq, D, heads)), device=dev)
                self.call("ebn_ff_attn_bwd_f32", ptr(Q), ptr(K), ptr(at.query_att.weight), ptr(at.key_att.weight), ptr(qw), ptr(kw), ptr(pq), ptr(pk),
                          ptr(dAO), ptr(dSV), ptr(dQ), ptr(dK), ptr(part), ctypes.byref(n), n_seq, T, D, heads, S())
                s = self.finish(part, n.value, width, width)
                HD = heads * D
                g[a + "query_att.weight"], g[a + "key_att.weight"] = s[:HD].view(heads, D), s[HD:2 * HD].view(heads, D)
                s = s[2 * HD:]
            else:  # the streamed pair leaves the logit gradients and the K * pooled_query rows: the logit weights' gradients are GEMMs
                lib = _hip.lib()
                part = torch.empty(int(lib.ebn_ff_attn_streamed_partials_len(n_seq, D)), device=dev)
                n_dl = int(lib.ebn_ff_attn_streamed_dlogits_len(n_seq, T, heads))
                d1, d2 = torch.empty(n_dl, device=dev).view(R, heads), torch.empty(n_dl, device=dev).view(R, heads)
                KP = torch.empty(int(lib.ebn_ff_attn_streamed_kp_len(n_seq, T, D)), device=dev).view(R, D)
                self.call("ebn_ff_attn_streamed_bwd_f32", ptr(Q), ptr(K), ptr(at.query_att.weight), ptr(at.key_att.weight), ptr(qw), ptr(kw), ptr(pq),
                          ptr(pk), ptr(dAO), ptr(dSV), ptr(dQ), ptr(dK), ptr(d1), ptr(d2), ptr(KP), ptr(part), ctypes.byref(n), n_seq, T, D, heads, S())
                s = self.finish(part, n.value, 3 * D, 3 * D)
                inv = 1.0 / math.sqrt(D // heads)
                g[a + "query_att.weight"], g[a + "key_att.weight"] = self.back_weight(d1, Q, inv), self.back_weight(d2, KP, inv)
                del d1, d2, KP
            g[a + "query.bias"], g[a + "key.bias"], g[a + "transform.bias"] = s[:D], s[D:2 * D], s[2 * D:]
            g[a + "query_att.bias"] = torch.zeros(heads, device=dev)
            g[a + "key_att.bias"] = torch.zeros(heads, device=dev)
            if need(a + "query.weight"):
                g[a + "query.weight"] = self.back_weight(dQ, h)
            if need(a + "key.weight"):
                g[a + "key.weight"] = self.back_weight(dK, h)
            self.back_data(dQ, at.query.weight, dh_in, beta=1.0)
            self.back_data(dK, at.key.weight, dh_in, beta=1.0)
            dh = dh_in
        return dh


class _FastformerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, hist, cand, p, keys, names, keep, *params):
        score, saved, _ = model._engine.forward(hist, cand, p, keys, keep, model.token_mask)
        ctx.model, ctx.saved, ctx.names = model, saved, names
        ctx.versions = [t._version for t in params] if keep else None
        ctx.params = params if keep else None
        ctx.spent = False
        ctx.req = [t.requires_grad for t in params]
        return score.view(-1, 1)

    @staticmethod
    def backward(ctx, dscore):
        if ctx.spent:
            raise RuntimeError("Fastformer: a second backward through the same forward; the first one released (and partly overwrote) the "
                               "saved activations, retain_graph=True is not supported: run the forward again")
        if ctx.saved is None:
            raise RuntimeError("Fastformer: backward through a forward that kept no activations")
        for n, t, v in zip(ctx.names, ctx.params, ctx.versions):  # the backward reads the parameters themselves: they must be unchanged
            if t._version != v:
                raise RuntimeError(f"Fastformer: parameter {n} was modified in place between forward and backward (version {v} -> "
                                   f"{t._version}); call backward() before optimizer.step()")
        req = dict(zip(ctx.names, ctx.req))
        g = ctx.model._engine.backward(ctx.saved, dscore.contiguous().view(-1).to(torch.float32), lambda n: req.get(n, False))
        ctx.saved, ctx.params, ctx.spent = None, None, True
        grads = [g[n].view_as(ctx.model._param(n)) if (r and n in g) else None for n, r in zip(ctx.names, ctx.req)]
        return (None, None, None, None, None, None, None, *grads)


class Fastformer(nn.Module):
    """See the module docstring.  ``config``: a ``BertConfig`` or any object with ``hidden_size``, ``num_attention_heads``,
    ``num_hidden_layers``, ``intermediate_size``, ``max_position_embeddings``, ``hidden_dropout_prob``, ``layer_norm_eps``,
    ``initializer_range``, ``hidden_act``, ``pooler_type``, ``vocab_size``."""

    def __init__(self, config, word_embedding: nn.Embedding = None, *, token_mask: str = "first_slot", seed: int = 0,
                 attention: str = "resident"):
        super().__init__()
        if getattr(config, "hidden_act", "gelu") != "gelu":
            raise ValueError(f"hidden_act = {config.hidden_act!r}: only 'gelu' (the exact erf form) has a kernel")
        if getattr(config, "pooler_type", "weightpooler") != "weightpooler":
            raise ValueError(f"pooler_type = {config.pooler_type!r}: only 'weightpooler' is supported")
        if token_mask not in TOKEN_MASKS:
            raise ValueError(f"token_mask = {token_mask!r}: one of {TOKEN_MASKS}")
        if attention not in ATTENTIONS:
            raise ValueError(f"attention = {attention!r}: one of {ATTENTIONS}")
        self.config = config
        self.token_mask = token_mask
        self.attention = attention
        self.seed = int(seed)
        self.dropout_step = 0
        self.word_embedding = nn.Embedding(config.vocab_size, config.hidden_size) if word_embedding is None else word_embedding
        self.embedding_transform = nn.Linear(self.word_embedding.weight.shape[1], config.hidden_size)
        self.output_layer = nn.Linear(config.hidden_size * 2, 1)
        self.news_encoder = SequenceFastformerEncoder(config)
        self.user_attention_polling = AttentionPooling(config)
        self.reset_parameters()
        self._engine = _Engine(self)

    def reset_parameters(self):
        """The reference's initial state: every Linear / Embedding weight ~ N(0, initializer_range) (a passed word_embedding too; a
        padding row, if the table declares one, zeroed), zero Linear biases, LayerNorm at (1, 0)."""
        std = float(self.config.initializer_range)
        with torch.no_grad():
            for mod in self.modules():
                if isinstance(mod, nn.LayerNorm):
                    nn.init.ones_(mod.weight)
                    nn.init.zeros_(mod.bias)
                elif isinstance(mod, nn.Linear):
                    nn.init.normal_(mod.weight, 0.0, std)
                    if mod.bias is not None:
                        nn.init.zeros_(mod.bias)
                elif isinstance(mod, nn.Embedding):
                    nn.init.normal_(mod.weight, 0.0, std)
                    if mod.padding_idx is not None:
                        mod.weight[mod.padding_idx].zero_()

    def _param(self, name):
        return self.get_parameter(name)

    def _keys(self, step):
        return tuple(dropout_key(self.seed, step, s) for s in range(1 + 2 * self.config.num_hidden_layers))

    def _check_device(self, *tensors):
        if not torch.cuda.is_available():
            raise RuntimeError("Fastformer.forward needs the MI355X HIP library and a GPU: there is no CPU fallback")
        for t in list(tensors) + list(self.parameters()):
            if not t.is_cuda:
                raise RuntimeError("Fastformer.forward: parameters and inputs must be on the GPU (there is no CPU fallback)")
            if isinstance(t, nn.Parameter) and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise RuntimeError("Fastformer.forward: parameters must be contiguous float32")

    def _run(self, hist, cand):
        from ebrec import _hip

        _hip.lib()
        self._check_device(hist, cand)
        if hist.dim() != 3 or cand.dim() != 3 or cand.shape[1] != 1 or cand.shape[0] != hist.shape[0] or cand.shape[2] != hist.shape[2]:
            raise ValueError(f"history_input (N, H, T) and candidate_input (N, 1, T) expected, got {tuple(hist.shape)} and {tuple(cand.shape)}")
        p = float(self.config.hidden_dropout_prob) if self.training else 0.0
        if p > 0.0:
            self.dropout_step += 1
        names, params = zip(*self.named_parameters())
        keep = torch.is_grad_enabled() and any(t.requires_grad for t in params)  # decided here: grad mode is off inside Function.forward
        return _FastformerFn.apply(self, hist, cand, p, self._keys(self.dropout_step), names, keep, *params)

    def forward(self, history_input, candidate_input) -> torch.Tensor:
        """history_input (N, H, T) int, candidate_input (N, 1, T) int -> (N, 1) sigmoid scores."""
        return self._run(history_input, candidate_input)

    def user_encoder(self, history_input: torch.Tensor) -> torch.Tensor:
        """(N, H, T) int -> the (N, hidden_size) user vectors (inference path: no gradient)."""
        from ebrec import _hip

        _hip.lib()
        self._check_device(history_input)
        N, H, T = history_input.shape
        with torch.no_grad():
            cand = torch.zeros(N, 1, T, dtype=history_input.dtype, device=history_input.device)
            p = float(self.config.hidden_dropout_prob) if self.training else 0.0
            _, _, (user, _) = self._engine.forward(history_input, cand, p, self._keys(self.dropout_step), False, self.token_mask)
            return user
