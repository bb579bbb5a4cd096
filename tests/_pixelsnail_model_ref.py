"""The whole stage-2 prior stated in plain torch, for any dtype (tests use float64 as the yardstick), on top of the layer
statements in _pixelsnail_ref.py (weight-normed convs, gated block) and _attention_ref.py (causal attention).  Written from
the formula, not from the reference's code:

    x0 = shift_down(conv_down(one_hot(codes))) + shift_right(conv_downright(one_hot(codes)))
         kernels [k // 2, k] and [(k + 1) // 2, k // 2]; a shift moves the conv OUTPUT by one pixel, zeros (not the bias) enter
    background = the two coordinate planes (a buffer), first `height` rows, repeated over the batch
    condition  = nearest x2 upsample of cond_resnet(one_hot(top codes)), first `height` rows
    block:  out = n_res_block 'causal' gated blocks (each with the condition);
            attention:  key = gated1x1([x, out, background]), query = gated1x1([out, background]),
                        out = gated1x1(out, aux = causal_attention(query, key), 8 heads)
            otherwise:  out = conv1x1([out, background])
    logits = conv1x1(ELU(n_out_res_block gated 1x1 blocks(x)))
    loss = mean over pixels of -log_softmax(logits)[target];  accuracy = mean of (argmax(logits) == target)

Also here: how tests/golden/pixelsnail_model*.npz store their tensors (load, golden_pair), shared by the CPU and the GPU
tests.
"""
import glob
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import _attention_ref as A
import _pixelsnail_ref as R


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def one_hot(codes, n_class, dtype):
    return F.one_hot(codes, n_class).permute(0, 3, 1, 2).to(dtype)


def shift_down(x, size=1):
    """x [N,C,H,W] moved `size` rows down, zeros entering at the top."""
    return F.pad(x, [0, 0, size, 0])[:, :, :x.shape[2], :]


def input_stage(codes, sd, n_class):
    """The two input convs with their shifts: [N,channel,H,W]."""
    dtype = sd["horizontal.conv.conv.weight_v"].dtype
    x = one_hot(codes, n_class, dtype)
    return shift_down(R.wn_conv(x, sd, "horizontal.conv.conv.", "down")) + \
        R.shift_right(R.wn_conv(x, sd, "vertical.conv.conv.", "downright"))


def _count(sd, pattern):
    n = 0
    while pattern.format(n) in sd:
        n += 1
    return n


def pixel_block(x, background, sd, attention, condition=None):
    """sd: the block's own state_dict."""
    out = x
    for i in range(_count(sd, "resblocks.{}.conv1.conv.conv.weight_v")):
        out = R.gated_resblock(out, sub(sd, f"resblocks.{i}."), "causal", condition=condition)
    if attention:
        key = R.gated_resblock(torch.cat([x, out, background], 1), sub(sd, "key_resblock."))
        query = R.gated_resblock(torch.cat([out, background], 1), sub(sd, "query_resblock."))
        attn = A.causal_attention(query, key, sub(sd, "causal_attention."), 8)
        return R.gated_resblock(out, sub(sd, "out_resblock."), aux=attn)
    return R.wn_conv(torch.cat([out, background], 1), sd, "out.conv.", "wnconv2d")


def cond_resnet(codes, sd, n_class):
    dtype = sd["blocks.0.conv.weight_v"].dtype
    v = sd["blocks.0.conv.weight_v"]
    x = F.conv2d(one_hot(codes, n_class, dtype), R.weight_norm(v, sd["blocks.0.conv.weight_g"]), sd["blocks.0.conv.bias"],
                 padding=v.shape[2] // 2)
    def conv(t, pre):
        w = R.weight_norm(sd[pre + "weight_v"], sd[pre + "weight_g"])
        return F.conv2d(t, w, sd[pre + "bias"], padding=w.shape[2] // 2)

    i = 1
    while f"blocks.{i}.conv1.conv.weight_v" in sd:      # plain gated blocks, the padding left to the conv itself
        t = conv(F.elu(conv(F.elu(x), f"blocks.{i}.conv1.conv.")), f"blocks.{i}.conv2.conv.")
        x = F.glu(t, 1) + x
        i += 1
    return x


def upsample2(x):
    return F.interpolate(x, scale_factor=2)         # nearest: every pixel becomes a 2x2 block


def head(x, sd):
    """sd: the state_dict of `out` (gated 1x1 blocks, ELU, 1x1 conv)."""
    n = _count(sd, "{}.conv1.conv.weight_v")
    for i in range(n):
        x = R.gated_resblock(x, sub(sd, f"{i}."))
    # in place, as the model's nn.ELU(inplace=True): torch then forms the derivative from the OUTPUT (y + 1), which rounds
    # differently from the out-of-place exp(x) -- every gradient upstream carries that choice
    return R.wn_conv(F.elu(x, inplace=True), sd, f"{n + 1}.conv.", "wnconv2d")


def pixelsnail(codes, sd, n_class, attention, condition=None):
    """codes [B,H,W] int64, sd: the model's state_dict in the dtype to compute in -> logits [B,n_class,H,W]."""
    b, h, w = codes.shape
    x = input_stage(codes, sd, n_class)
    background = sd["background"][:, :, :h, :].expand(b, 2, h, w)
    cond = None
    if condition is not None:
        cond = upsample2(cond_resnet(condition, sub(sd, "cond_resnet."), n_class))[:, :, :h, :]
    for i in range(_count(sd, "blocks.{}.resblocks.0.conv1.conv.conv.weight_v")):
        x = pixel_block(x, background, sub(sd, f"blocks.{i}."), attention, cond)
    return head(x, sub(sd, "out."))


def cross_entropy(logits, target):
    """(mean loss, accuracy); the lowest index wins an arg-max tie."""
    loss = F.cross_entropy(logits, target)          # the mean of -log_softmax(logits)[target], as one torch operation
    best = logits.max(1, keepdim=True)[0]
    classes = torch.arange(logits.shape[1]).view(1, -1, 1, 1).expand_as(logits)
    pred = torch.where(logits == best, classes, torch.full_like(classes, logits.shape[1])).min(1)[0]
    return loss, (pred == target).to(torch.float32).sum() / target.numel()


# ----------------------------------------------------------------------------- the golden files
class _Merged:
    """Several .npz files read as one (the gradients of the two 64-channel cases are files of their own: one file with
    everything would pass the size limit for a committed file)."""

    def __init__(self, parts):
        self.parts = parts
        self.where = {k: p for p in parts for k in p.files}
        self.files = list(self.where)

    def __getitem__(self, key):
        return self.where[key][key]


_LOADED = []


def load():
    if not _LOADED:
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        paths = [os.path.join(here, "pixelsnail_model.npz")] + sorted(glob.glob(os.path.join(here, "pixelsnail_model_grads*.npz")))
        _LOADED.append(_Merged([np.load(p) for p in paths]))
    return _LOADED[0]


def cases(g):
    return json.loads(str(g["cases"]))


def golden_pair(g, key):
    """(float64 run, float32 run as float64) of the tensor `key` ('c0.logits', 'c0.grad.<parameter>', ...).  Logits and
    losses are stored from both runs in full.  Gradients are stored as the float64 run in full plus the float32 run's
    DIFFERENCE from it as float16 in units of its largest magnitude (`.d16`, `.s`): the gap between the runs, which is all
    the float32 run is used for, is kept to 3 digits, and the file stays under its size limit."""
    f64 = g[key + ".f64"]
    if key + ".f32" in g.files:
        return f64, g[key + ".f32"].astype(np.float64)
    return f64, f64 + g[key + ".d16"].astype(np.float64) * float(g[key + ".s"])


def state_dict(g, ci):
    """The case's state_dict; a case may point at another one's (`sd_of`)."""
    c = cases(g)[ci]
    t = f"c{c.get('sd_of', ci)}.sd."
    return {k[len(t):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(t)}


def grad_names(g, ci):
    t = f"c{ci}.grad."
    return sorted(k[len(t):-4] for k in g.files if k.startswith(t) and k.endswith(".f64"))


def run_case(g, ci, dtype):
    """The yardstick on case ci in `dtype`: {'logits' | 'out', 'loss', 'accuracy', 'grad.<name>'}."""
    c = cases(g)[ci]
    t = f"c{ci}."
    sd = {k: (v.to(dtype) if v.is_floating_point() else v).clone() for k, v in state_dict(g, ci).items()}
    params = [k for k in sd if k != "background"]
    for k in params:
        sd[k].requires_grad_(True)
    res = {}
    if c["kind"] == "model":
        codes = torch.from_numpy(g[t + "in.input"])
        cond = torch.from_numpy(g[t + "in.condition"]) if t + "in.condition" in g.files else None
        logits = pixelsnail(codes, sd, c["n_class"], c["attention"], cond)
        loss, acc = cross_entropy(logits, codes)
        res.update(logits=logits.detach(), loss=loss.detach(), accuracy=acc)
    else:
        x = torch.from_numpy(g[t + "in.input"]).to(dtype)
        bg = torch.from_numpy(g[t + "in.background"]).to(dtype)
        cond = torch.from_numpy(g[t + "in.condition"]).to(dtype) if t + "in.condition" in g.files else None
        out = pixel_block(x, bg, sd, c["attention"], cond)
        loss = (out * torch.from_numpy(g[t + "in.gout"]).to(dtype)).sum()
        res.update(out=out.detach(), loss=loss.detach())
    loss.backward()
    for k in params:
        res["grad." + k] = sd[k].grad
    return res
