"""The pixel-incremental evaluation of the stage-2 prior stated in plain torch, for any dtype: what
vqvae2_amd.PriorSampler(model, stepping='pixel') computes.

Step (i, j) computes column j of row i of every layer and nothing else.  A layer's value at (i, j) is a [B, C] column buffer;
what earlier steps left is kept in

    a history [B, C, H, W] of the input of every conv whose kernel has more than one row (all of them 'causal': the last
        kernel row stops before its centre column, so at step (i, j) such a conv reads rows < i and, of row i, columns < j
        plus nothing of what later steps will write),
    the keys and values [B, H * W, C] of the attention (the one query at raster position p = i * W + j sees positions < p).

Histories start as NaN: a read of a cell that no earlier step wrote would show in the logits.  Taps outside the image are
skipped, which is reading 0.  The input stage runs the two one-hot convs over the code rows as row stepping does and takes
column j of the result."""
import math

import torch
import torch.nn.functional as F

import _pixelsnail_model_ref as M
import _pixelsnail_ref as R
import _sample_ref as S


class _PixelStepper(S._Stepper):
    def __init__(self, sd, n_class, attention, batch, rows, width, condition):
        super().__init__(sd, n_class, attention, batch, rows, width, condition)
        self.dtype = sd["horizontal.conv.conv.weight_v"].dtype

    def conv_col(self, i, j, x, prefix, mode):
        """Pixel (i, j) of the conv from column buffer x [B, C]; everything else comes from the conv's history."""
        w = self.weight(prefix, mode)
        kh, kw = w.shape[2:]
        bias = self.sd.get(prefix + "bias")
        if kh == 1:
            assert kw == 1
            return F.linear(x, w[:, :, 0, 0], bias)
        assert mode == "causal"
        pad_top, pad_left = R.geometry(mode, kh, kw)
        assert pad_top == kh - 1
        hist = self.hist.get(prefix)
        if hist is None:
            hist = self.hist[prefix] = torch.full((self.b, x.shape[1], self.h, self.w), float("nan"), dtype=self.dtype)
        hist[:, :, i, j] = x
        out = torch.zeros((self.b, w.shape[0]), dtype=self.dtype)
        for a in range(kh):
            for c in range(kw):
                if a == kh - 1 and c >= kw // 2:
                    continue                                # the taps a 'causal' layer zeroes: never read
                r, q = i - (kh - 1) + a, j - pad_left + c
                if r < 0 or q < 0 or q >= self.w:
                    continue                                # outside the image: 0
                out = out + F.linear(hist[:, :, r, q], w[:, :, a, c])
        return out if bias is None else out + bias

    def gated_col(self, i, j, x, prefix, conv="wnconv2d", aux=None, condition=None):
        pre = prefix + ("conv1." if conv == "wnconv2d" else "conv1.conv.")
        pre2 = prefix + ("conv2." if conv == "wnconv2d" else "conv2.conv.")
        h = self.conv_col(i, j, F.elu(x), pre + "conv.", conv)
        if aux is not None:
            h = h + self.conv_col(i, j, F.elu(aux), prefix + "aux_conv.conv.", "wnconv2d")
        t = self.conv_col(i, j, F.elu(h), pre2 + "conv.", conv)
        if condition is not None:
            t = t + self.conv_col(i, j, condition, prefix + "condition.conv.", "wnconv2d")
        return F.glu(t, 1) + x

    def attention_col(self, i, j, query, key, prefix, n_head=8):
        def lin(x, name):
            w = R.weight_norm(self.sd[prefix + name + ".weight_v"], self.sd[prefix + name + ".weight_g"])
            return F.linear(x, w, self.sd[prefix + name + ".bias"])         # [B, C]

        q, k, v = lin(query, "query"), lin(key, "key"), lin(key, "value")
        kv = self.kv.get(prefix)
        if kv is None:
            kv = self.kv[prefix] = tuple(torch.full((self.b, self.h * self.w, k.shape[1]), float("nan"), dtype=self.dtype)
                                         for _ in range(2))
        p = i * self.w + j
        kv[0][:, p], kv[1][:, p] = k, v
        b, c = q.shape
        if p == 0:
            return torch.zeros_like(q)                      # position 0 sees nothing
        dh = c // n_head
        qh = q.view(b, n_head, 1, dh)
        kh = kv[0][:, :p].reshape(b, p, n_head, dh).transpose(1, 2)
        vh = kv[1][:, :p].reshape(b, p, n_head, dh).transpose(1, 2)
        pr = torch.softmax(qh @ kh.transpose(2, 3) / math.sqrt(dh), -1)
        return (pr @ vh).reshape(b, c)

    def pixel(self, i, j, codes):
        """Logits of pixel (i, j) [B, n_class] from the code map as it stands."""
        sd = self.sd
        x = self.input_row(i, codes)[:, :, 0, j]
        bg = sd["background"][:, :, i, j].expand(self.b, 2)
        cond = None if self.cond is None else self.cond[:, :, i, j]
        for bi in range(M._count(sd, "blocks.{}.resblocks.0.conv1.conv.conv.weight_v")):
            p = f"blocks.{bi}."
            out = x
            for k in range(M._count(sd, p + "resblocks.{}.conv1.conv.conv.weight_v")):
                out = self.gated_col(i, j, out, f"{p}resblocks.{k}.", "causal", condition=cond)
            if self.attention:
                key = self.gated_col(i, j, torch.cat([x, out, bg], 1), p + "key_resblock.")
                query = self.gated_col(i, j, torch.cat([out, bg], 1), p + "query_resblock.")
                attn = self.attention_col(i, j, query, key, p + "causal_attention.")
                x = self.gated_col(i, j, out, p + "out_resblock.", aux=attn)
            else:
                x = self.conv_col(i, j, torch.cat([out, bg], 1), p + "out.conv.", "wnconv2d")
        n = M._count(sd, "out.{}.conv1.conv.weight_v")
        for k in range(n):
            x = self.gated_col(i, j, x, f"out.{k}.")
        return self.conv_col(i, j, F.elu(x), f"out.{n + 1}.conv.", "wnconv2d")


def logits_given(codes, sd, n_class, attention, condition=None):
    """codes [B,H,W] int64, sd in the dtype to compute in -> [B, n_class, H, W]; entry (i, j) is what step (i, j) of the
    pixel-stepping loop sees when every earlier draw gave the code in `codes`."""
    b, h, w = codes.shape
    st = _PixelStepper(sd, n_class, attention, b, h, w, condition)
    row = torch.zeros_like(codes)
    out = torch.zeros((b, n_class, h, w), dtype=st.dtype)
    with torch.no_grad():
        for i in range(h):
            for j in range(w):
                out[:, :, i, j] = st.pixel(i, j, row)
                row[:, i, j] = codes[:, i, j]
    return out
