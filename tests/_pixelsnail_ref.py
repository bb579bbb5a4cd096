"""The weight-normed convs and the gated residual block of the stage-2 prior stated in plain torch, for any dtype (tests
use float64 as the yardstick).  Written from the formula, not from the reference's code:

    w = g * v / ||v||_2 per output channel (norm over in * kh * kw), with a bias unless stated
    conv at geometry (pad_top, pad_left): y[h, w] = b + sum_{kh, kw} w[kh, kw] x[h - pad_top + kh, w - pad_left + kw], zeros
        outside the image, output the size of the input
        'wnconv2d'   ((KH - 1) / 2, (KW - 1) / 2)        'downright'   (KH - 1, KW - 1)
        'down', 'causal'   (KH - 1, KW // 2);  'causal' also has v[:, :, -1, KW // 2:] = 0 (the caller's dict is edited in
        place, as the layer edits its parameter)
    block:  h = conv1(ELU(x)) [+ aux_conv(ELU(aux))];  h = ELU(h) * keep / (1 - p);  t = conv2(h) [+ condition(cond)];
            out = t[:, :C] * sigmoid(t[:, C:]) + x
"""
import torch
import torch.nn.functional as F


def weight_norm(v, g):
    return torch._weight_norm(v, g, 0)      # g * v / ||v||_2 per output row, as one torch operation


def geometry(mode, kh, kw):
    if mode == "wnconv2d":
        return (kh - 1) // 2, (kw - 1) // 2
    if mode in ("downright", "causal_downright"):
        return kh - 1, kw - 1
    if mode in ("down", "causal"):
        return kh - 1, kw // 2
    raise ValueError(mode)


def conv_at(x, w, b, pad_top, pad_left):
    """x [N,C,H,W], w [O,C,KH,KW]: the conv that reads from (h - pad_top, w - pad_left) on, output the size of x."""
    kh, kw = w.shape[2:]
    return F.conv2d(F.pad(x, [pad_left, kw - 1 - pad_left, pad_top, kh - 1 - pad_top]), w, b)


def wn_conv(x, sd, prefix, mode):
    """prefix + {weight_v, weight_g[, bias]} of sd; mode as in geometry()."""
    v, g = sd[prefix + "weight_v"], sd[prefix + "weight_g"]
    kh, kw = v.shape[2:]
    if mode == "causal":
        with torch.no_grad():
            v[:, :, -1, kw // 2:].zero_()
    return conv_at(x, weight_norm(v, g), sd.get(prefix + "bias"), *geometry(mode, kh, kw))


def gated_resblock(x, sd, conv="wnconv2d", aux=None, condition=None, keep=None, p=0.0):
    """x [N,C,H,W]; sd: the block's state_dict (conv1 / conv2 / aux_conv / condition); keep: bool [N,channel,H,W] or None."""
    pre = "conv1." if conv == "wnconv2d" else "conv1.conv."
    pre2 = "conv2." if conv == "wnconv2d" else "conv2.conv."
    h = wn_conv(F.elu(x), sd, pre + "conv.", conv)
    if aux is not None:
        h = h + wn_conv(F.elu(aux), sd, "aux_conv.conv.", "wnconv2d")
    h = F.elu(h)
    if keep is not None:
        h = h * keep.to(h.dtype) / (1.0 - p)
    t = wn_conv(h, sd, pre2 + "conv.", conv)
    if condition is not None:
        t = t + wn_conv(condition, sd, "condition.conv.", "wnconv2d")
    return F.glu(t, 1) + x


def shift_right(x, size=1):
    """x [N,C,H,W] moved `size` columns to the right, zeros entering on the left."""
    return F.pad(x, [size, 0, 0, 0])[:, :, :, :x.shape[3]]
