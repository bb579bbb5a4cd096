"""The causal attention layer of the stage-2 prior stated in plain torch, for any dtype (tests use float64 as the
yardstick).  Written from the formula, not from the reference's code:

    w = g * v / ||v||_2 per output row                      (weight-normed linear layers, with a bias)
    Q = w_q x_q + b_q,  K = w_k x_k + b_k,  V = w_v x_k + b_v      per pixel; head h owns channels h*dh .. (h+1)*dh-1
    S = Q K^T / sqrt(dh);  position i sees positions j < i only (strict: the diagonal is masked)
    P = softmax over the visible positions; a row that sees nothing (row 0) is all zero
    O = (P * keep / (1 - p)) V          with an explicit keep mask [B, n_head, L, L] when dropout is checked
"""
import math

import torch


def weight_norm(v, g):
    return torch._weight_norm(v, g, 0)      # g * v / ||v||_2 per output row, as one torch operation


def attention_core(q, k, v, n_head, keep=None, p=0.0, fill=None):
    """q, k, v [B, L, C] -> O [B, L, C].  fill=None masks properly (excluded scores); fill=-1e4 is the other way to
    write it: masked scores are SET to `fill`, the softmax runs over the whole row and row 0 is zeroed afterwards."""
    b, l, c = q.shape
    dh = c // n_head
    qh, kh, vh = (t.reshape(b, l, n_head, dh).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(2, 3) / math.sqrt(dh)
    vis = torch.ones(l, l, dtype=torch.bool, device=q.device).tril(-1)          # [i, j]: j < i
    # One softmax routine (torch's) for both ways of masking, so that they can be compared bit for bit.  A row that sees
    # nothing would be a row of -inf: it gets scores of 0 instead and is zeroed afterwards, like every masked entry.
    some = vis.any(-1, keepdim=True)
    s = s.masked_fill(~vis, -math.inf if fill is None else fill)
    if fill is None:
        s = torch.where(some, s, torch.zeros_like(s))
        pr = torch.softmax(s, -1) * vis.to(s.dtype)
    else:
        pr = torch.softmax(s, -1) * some.to(s.dtype)
    if keep is not None:
        pr = pr * keep.to(pr.dtype) / (1.0 - p)
    return (pr @ vh).transpose(1, 2).reshape(b, l, c)


def causal_attention(query, key, sd, n_head, keep=None, p=0.0, fill=None, taps=None):
    """query [B,Cq,H,W], key [B,Ck,H,W], sd: {query,key,value}.{bias,weight_g,weight_v} -> [B,channel,H,W].
    taps: a dict that receives the projected Q, K, V [B, L, channel] (with retain_grad) for a caller that wants them."""
    b, _, h, w = query.shape
    xq = query.reshape(b, query.shape[1], h * w).transpose(1, 2)
    xk = key.reshape(b, key.shape[1], h * w).transpose(1, 2)

    def lin(x, name):
        return torch.nn.functional.linear(x, weight_norm(sd[name + ".weight_v"], sd[name + ".weight_g"]), sd[name + ".bias"])

    q, k, v = lin(xq, "query"), lin(xk, "key"), lin(xk, "value")
    if taps is not None:
        for n, t in (("q", q), ("k", k), ("v", v)):
            if t.requires_grad:
                t.retain_grad()
            taps[n] = t
    o = attention_core(q, k, v, n_head, keep, p, fill)
    return o.reshape(b, h, w, -1).permute(0, 3, 1, 2)


PARAM_NAMES = tuple(f"{m}.{n}" for m in ("query", "key", "value") for n in ("bias", "weight_g", "weight_v"))
