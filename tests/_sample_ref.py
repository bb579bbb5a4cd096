"""The row-incremental evaluation of the stage-2 prior stated in plain torch, for any dtype: what vqvae2_amd.PriorSampler
computes, built on the layer statements of _pixelsnail_ref.py / _pixelsnail_model_ref.py.

For pixel (i, j) the reference's sampling loop needs model(row[:, :i + 1])[..., i, j].  Every layer is causal in raster order,
so row i of every layer is computed from row i of its inputs plus

    a history of earlier input rows    for every conv whose kernel has more than one row (it ends at the output row),
    the keys and values of earlier rows   for the attention (a query at raster position p sees positions < p),

and nothing else.  logits_given() steps through the map with the given codes written where a sampler would draw: entry (i, j)
of its result is what step (i, j) saw, with columns > j of the code row still 0.

Also here: the draw rule (draw), in numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import _pixelsnail_model_ref as M
import _pixelsnail_ref as R


def draw(p, u):
    """The smallest class c with p_0 + .. + p_c > u, or the last class if rounding leaves none (p: probabilities, 1-D)."""
    hit = np.nonzero(np.cumsum(p) > u)[0]
    return int(hit[0]) if hit.size else len(p) - 1


class _Stepper:
    def __init__(self, sd, n_class, attention, batch, rows, width, condition):
        self.sd, self.n_class, self.attention = sd, n_class, attention
        self.b, self.h, self.w = batch, rows, width
        self.hist = {}          # name -> list of input rows [B,C,1,W] of a multi-row conv
        self.kv = {}            # name -> (list of key rows, list of value rows), each [B, W, C]
        self.weights = {}
        self.cond = None
        if condition is not None:
            self.cond = M.upsample2(M.cond_resnet(condition, M.sub(sd, "cond_resnet."), n_class))[:, :, :rows, :]

    def weight(self, prefix, mode):
        """The effective weight, formed once (the 'causal' zeroing on a copy, before the norm)."""
        if prefix not in self.weights:
            v = self.sd[prefix + "weight_v"].clone()
            if mode == "causal":
                v[:, :, -1, v.shape[3] // 2:] = 0
            self.weights[prefix] = R.weight_norm(v, self.sd[prefix + "weight_g"])
        return self.weights[prefix]

    def conv_row(self, i, x, prefix, mode):
        """Row i of the conv from row i of its input x [B,C,1,W]; earlier rows come from the conv's history."""
        w = self.weight(prefix, mode)
        kh, kw = w.shape[2:]
        pad_top, pad_left = R.geometry(mode, kh, kw)
        bias = self.sd.get(prefix + "bias")
        if kh == 1:
            return R.conv_at(x, w, bias, 0, pad_left)
        assert pad_top == kh - 1
        rows = self.hist.setdefault(prefix, [])
        del rows[i:]                    # step (i, j) replaces what step (i, j - 1) left for row i
        rows.append(x)
        band = torch.cat(rows[max(0, i - kh + 1):], 2)
        band = F.pad(band, [pad_left, kw - 1 - pad_left, kh - band.shape[2], 0])        # rows above the image are 0
        return F.conv2d(band, w, bias)

    def gated(self, i, x, prefix, conv="wnconv2d", aux=None, condition=None):
        pre = prefix + ("conv1." if conv == "wnconv2d" else "conv1.conv.")
        pre2 = prefix + ("conv2." if conv == "wnconv2d" else "conv2.conv.")
        h = self.conv_row(i, F.elu(x), pre + "conv.", conv)
        if aux is not None:
            h = h + self.conv_row(i, F.elu(aux), prefix + "aux_conv.conv.", "wnconv2d")
        t = self.conv_row(i, F.elu(h), pre2 + "conv.", conv)
        if condition is not None:
            t = t + self.conv_row(i, condition, prefix + "condition.conv.", "wnconv2d")
        return F.glu(t, 1) + x

    def attention_row(self, i, query, key, prefix, n_head=8):
        def lin(x, name):
            w = R.weight_norm(self.sd[prefix + name + ".weight_v"], self.sd[prefix + name + ".weight_g"])
            return F.linear(x[:, :, 0].transpose(1, 2), w, self.sd[prefix + name + ".bias"])      # [B, W, C]

        q, k, v = lin(query, "query"), lin(key, "key"), lin(key, "value")
        ks, vs = self.kv.setdefault(prefix, ([], []))
        del ks[i:], vs[i:]
        ks.append(k)
        vs.append(v)
        kk, vv = torch.cat(ks, 1), torch.cat(vs, 1)                 # positions 0 .. (i + 1) * W - 1
        b, w, c = q.shape
        dh = c // n_head
        qh = q.reshape(b, w, n_head, dh).transpose(1, 2)
        kh = kk.reshape(b, -1, n_head, dh).transpose(1, 2)
        vh = vv.reshape(b, -1, n_head, dh).transpose(1, 2)
        s = qh @ kh.transpose(2, 3) / math.sqrt(dh)
        pos_q = i * w + torch.arange(w).view(w, 1)
        vis = torch.arange(kk.shape[1]).view(1, -1) < pos_q         # [query, key]: key position < query position
        some = vis.any(-1, keepdim=True)
        s = s.masked_fill(~vis, -math.inf)
        s = torch.where(some, s, torch.zeros_like(s))
        pr = torch.softmax(s, -1) * vis.to(s.dtype)
        o = (pr @ vh).transpose(1, 2).reshape(b, w, c)
        return o.transpose(1, 2).unsqueeze(2)                       # [B, C, 1, W]

    def input_row(self, i, codes):
        """Row i of shift_down(horizontal(one_hot)) + shift_right(vertical(one_hot)) from the code rows that end at row i."""
        sd, dtype = self.sd, self.sd["horizontal.conv.conv.weight_v"].dtype
        vert = R.wn_conv(M.one_hot(codes[:, :i + 1], self.n_class, dtype), sd, "vertical.conv.conv.", "downright")
        out = R.shift_right(vert[:, :, i:i + 1])
        if i > 0:       # the row a shift brings in at the top is 0, without the bias
            hor = R.wn_conv(M.one_hot(codes[:, :i], self.n_class, dtype), sd, "horizontal.conv.conv.", "down")
            out = out + hor[:, :, i - 1:i]
        return out

    def row(self, i, codes):
        """Logits of row i [B, n_class, W] from the code map as it stands."""
        sd = self.sd
        x = self.input_row(i, codes)
        bg = sd["background"][:, :, i:i + 1, :].expand(self.b, 2, 1, self.w)
        cond = None if self.cond is None else self.cond[:, :, i:i + 1]
        for bi in range(M._count(sd, "blocks.{}.resblocks.0.conv1.conv.conv.weight_v")):
            p = f"blocks.{bi}."
            out = x
            for k in range(M._count(sd, p + "resblocks.{}.conv1.conv.conv.weight_v")):
                out = self.gated(i, out, f"{p}resblocks.{k}.", "causal", condition=cond)
            if self.attention:
                key = self.gated(i, torch.cat([x, out, bg], 1), p + "key_resblock.")
                query = self.gated(i, torch.cat([out, bg], 1), p + "query_resblock.")
                attn = self.attention_row(i, query, key, p + "causal_attention.")
                x = self.gated(i, out, p + "out_resblock.", aux=attn)
            else:
                x = self.conv_row(i, torch.cat([out, bg], 1), p + "out.conv.", "wnconv2d")
        n = M._count(sd, "out.{}.conv1.conv.weight_v")
        for k in range(n):
            x = self.gated(i, x, f"out.{k}.")
        return self.conv_row(i, F.elu(x), f"out.{n + 1}.conv.", "wnconv2d")[:, :, 0]


def logits_given(codes, sd, n_class, attention, condition=None):
    """codes [B,H,W] int64, sd in the dtype to compute in -> [B, n_class, H, W]; entry (i, j) is what step (i, j) of the
    sampling loop sees when every earlier draw gave the code in `codes`."""
    b, h, w = codes.shape
    st = _Stepper(sd, n_class, attention, b, h, w, condition)
    row = torch.zeros_like(codes)
    out = torch.zeros((b, n_class, h, w), dtype=sd["horizontal.conv.conv.weight_v"].dtype)
    with torch.no_grad():
        for i in range(h):
            for j in range(w):
                out[:, :, i, j] = st.row(i, row)[:, :, j]
                row[:, i, j] = codes[:, i, j]
    return out
