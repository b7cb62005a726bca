"""Float64-capable torch restatement of the reference's Fastformer_wu and StandardFastformerEncoder (models/fastformer/fastformer_wu.py),
written from its formulas over a dict of tensors with the reference's state_dict names; the building blocks are those of
tests/fastformer_oracle.py.  Differentiable by autograd (the tensors of P and the encoder's input may require grad).  Dropout masks
come from the build's counter-based stream: the mask of element (n, t, c) of an [n_seq, T, D] activation is that of flat index
(n * T + t) * D + c; site 0 the embedding dropout, sites 1 + 2 l and 2 + 2 l the two dropouts of layer l."""
import math

import torch

from tests.fastformer_oracle import drop_mult, fast_attention, layer_norm, linear, pooling


def encoder(x, mask, P, heads, eps, pre="", pooler_index=0, drop=None):
    """StandardFastformerEncoder.forward: x [n, T, D] input embeddings, mask [n, T] (1 = token) -> [n, D].  Token t gets row t of the
    position table.  `pre`: the prefix of the encoder's names in P; drop = (p, seed, step) or None."""
    n, T, D = x.shape
    dt, dev = x.dtype, x.device
    mask = mask.to(dt)
    x = layer_norm(x + P[pre + "position_embeddings.weight"][:T], P[pre + "LayerNorm.weight"], P[pre + "LayerNorm.bias"], eps)
    dm = (lambda site: drop_mult((n, T, D), drop[1], drop[2], site, drop[0], dt, dev)) if drop and drop[0] > 0 else (lambda site: 1.0)
    x = x * dm(0)
    add_mask = (1.0 - mask) * -10000.0
    l = 0
    while f"{pre}encoders.{l}.intermediate.dense.weight" in P:
        lp = f"{pre}encoders.{l}."
        sv = fast_attention(x, add_mask, P, lp + "attention.self", heads)
        a1 = layer_norm(linear(sv, P, lp + "attention.output.dense") * dm(1 + 2 * l) + x, P[lp + "attention.output.LayerNorm.weight"],
                        P[lp + "attention.output.LayerNorm.bias"], eps)
        v = linear(a1, P, lp + "intermediate.dense")
        gl = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
        x = layer_norm(linear(gl, P, lp + "output.dense") * dm(2 + 2 * l) + a1, P[lp + "output.LayerNorm.weight"],
                       P[lp + "output.LayerNorm.bias"], eps)
        l += 1
    return pooling(x, mask, P, f"{pre}poolers.{pooler_index}")


def cross_entropy(score, targets):
    """nn.CrossEntropyLoss() with its defaults: the mean of -log softmax(score)[n, targets[n]], stable."""
    m = score.max(1, keepdim=True).values
    lse = (score - m).exp().sum(1).log() + m.squeeze(1)
    return (lse - score.gather(1, targets.view(-1, 1)).squeeze(1)).mean()


def forward(P, ids, targets, heads, eps, drop=None):
    """Fastformer_wu.forward: ids [N, T] integer, targets [N] integer -> (loss, score [N, C])."""
    ids = ids.long()
    dt = P["embedding_transform.weight"].dtype
    mask = (ids != 0).to(dt)
    x = linear(P["word_embedding.weight"][ids], P, "embedding_transform")
    vec = encoder(x, mask, P, heads, eps, "fastformer_model.", 0, drop)
    score = linear(vec, P, "output_layer")
    return cross_entropy(score, targets.long()), score
