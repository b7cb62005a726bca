"""Float64-capable torch restatement of the reference's Fastformer (models/fastformer/fastformer.py), written from its formulas:
``forward(P, hist, cand, heads, eps, ...)`` over a dict of tensors with the reference's state_dict names.  Differentiable by
autograd (the tensors of P may require grad).  Dropout masks come from the build's counter-based stream (oracle.nrms_numpy), the
mask of element (r, c) of an [R, D] activation being that of flat index r * D + c: site 0 the embedding dropout, sites 1 + 2 l and
2 + 2 l the two dropouts of layer l."""
import math

import numpy as np
import torch

from oracle import nrms_numpy as on


def drop_mult(shape, seed, step, site, p, dtype, device):
    """Inverted-dropout multipliers (0 or 1 / (1 - p), the scale rounded in float32 as the kernels do)."""
    n = int(np.prod(shape))
    keep = on.dropout_keep_mask(on.dropout_key(seed, step, site), n, p).reshape(shape)
    scale = float(np.float32(1.0) / np.float32(1.0 - np.float32(p)))
    return torch.as_tensor(keep.astype(np.float64) * scale, dtype=dtype, device=device)


def layer_norm(z, g, b, eps):
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    return (z - mu) / torch.sqrt(var + eps) * g + b


def linear(x, P, name):
    return x @ P[name + ".weight"].T + P[name + ".bias"]


def pooling(x, mask, P, name):
    """AttentionPooling: x [n, L, D], mask [n, L] -> [n, D]; exp without max-subtraction, times mask, over sum + 1e-8."""
    e = torch.tanh(linear(x, P, name + ".att_fc1"))
    a = torch.exp(linear(e, P, name + ".att_fc2")) * mask.unsqueeze(2)
    a = a / (a.sum(1, keepdim=True) + 1e-8)
    return (x * a).sum(1)


def fast_attention(x, add_mask, P, name, heads):
    """FastSelfAttention: x [n, T, D], add_mask [n, T] = (1 - mask) * -10000."""
    n, T, D = x.shape
    hs = D // heads
    q, k = linear(x, P, name + ".query"), linear(x, P, name + ".key")
    s = linear(q, P, name + ".query_att") / math.sqrt(hs) + add_mask.unsqueeze(2)  # [n, T, heads]: each head reads the whole row
    a = torch.softmax(s, dim=1)
    pq = (a.unsqueeze(3) * q.view(n, T, heads, hs)).sum(1).reshape(n, 1, D)
    kp = k * pq
    s2 = linear(kp, P, name + ".key_att") / math.sqrt(hs) + add_mask.unsqueeze(2)
    b = torch.softmax(s2, dim=1)
    pk = (b.unsqueeze(3) * kp.view(n, T, heads, hs)).sum(1).reshape(n, 1, D)
    return linear(pk * q, P, name + ".transform") + q


def news_encoder(ids, mask, P, heads, eps, drop=None):
    """ids [n, T] int64, mask [n, T] (1 = token) -> [n, D].  drop = (p, seed, step) or None."""
    n, T = ids.shape
    dt, dev = P["embedding_transform.weight"].dtype, ids.device
    x = linear(P["word_embedding.weight"][ids], P, "embedding_transform")
    D = x.shape[-1]
    x = layer_norm(x + P["news_encoder.position_embeddings.weight"][0], P["news_encoder.LayerNorm.weight"], P["news_encoder.LayerNorm.bias"], eps)
    dm = (lambda site: drop_mult((n, T, D), drop[1], drop[2], site, drop[0], dt, dev)) if drop and drop[0] > 0 else (lambda site: 1.0)
    x = x * dm(0)
    add_mask = (1.0 - mask) * -10000.0
    l = 0
    while f"news_encoder.encoders.{l}.intermediate.dense.weight" in P:
        pre = f"news_encoder.encoders.{l}."
        sv = fast_attention(x, add_mask, P, pre + "attention.self", heads)
        a1 = layer_norm(linear(sv, P, pre + "attention.output.dense") * dm(1 + 2 * l) + x, P[pre + "attention.output.LayerNorm.weight"],
                        P[pre + "attention.output.LayerNorm.bias"], eps)
        v = linear(a1, P, pre + "intermediate.dense")
        gl = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
        x = layer_norm(linear(gl, P, pre + "output.dense") * dm(2 + 2 * l) + a1, P[pre + "output.LayerNorm.weight"],
                       P[pre + "output.LayerNorm.bias"], eps)
        l += 1
    return pooling(x, mask, P, "news_encoder.poolers.0")


def forward(P, hist, cand, heads, eps, token_mask="first_slot", drop=None, parts=False):
    """hist [N, H, T], cand [N, 1, T] integer -> scores [N, 1] (and the user / candidate vectors with parts=True).  History and
    candidates run as ONE batch of N (H + 1) sequences, history first, so that dropout element indices match the kernels'."""
    N, H, T = hist.shape
    dt = P["embedding_transform.weight"].dtype
    hist, cand = hist.long(), cand.long()
    tok = (hist != 0).to(dt)
    hmask = tok[:, :, 0]
    if token_mask == "first_slot":
        tok = tok[:, 0:1, :].expand(N, H, T)
    ids = torch.cat([hist.reshape(N * H, T), cand.reshape(N, T)], 0)
    mask = torch.cat([tok.reshape(N * H, T), (cand != 0).to(dt).reshape(N, T)], 0)
    nv = news_encoder(ids, mask, P, heads, eps, drop)
    user = pooling(nv[:N * H].view(N, H, -1), hmask, P, "user_attention_polling")
    cv = nv[N * H:]
    score = torch.sigmoid(linear(torch.cat([user, cv], 1), P, "output_layer"))
    return (score, user, cv) if parts else score


def measure(got, ref, G):
    """max|got - ref| / max(max|ref|, 1e-4 G), G the largest gradient magnitude over all tensors of the run."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-4 * G))
