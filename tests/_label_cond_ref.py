"""The class-conditional stage-2 prior stated in plain torch, for any dtype (tests use float64 as the yardstick), on top of
_pixelsnail_model_ref.py and _pixelsnail_ref.py.  TEST INFRASTRUCTURE, CPU only.  The rule, written from its formula:

    'causal' gated block with a table E = label_embed [n_label, 2 * C]:
        t   = conv2(dropout(ELU(conv1(ELU(x))))) [+ condition(condition)]             as without a label
        out = a * sigmoid(b) + x,   [a | b] = t + E[label[image]]                      one row per image, every pixel
    a label outside [0, n_label) adds nothing (and so receives no gradient).

Every other layer is the unlabelled model's.  Also here: the three label kernels as formulas over [pixels, C] rows
(glu_label_fwd, glu_label_bwd, label_embed_grad), usable in float64 and float32.
"""
import torch
import torch.nn.functional as F

import _attention_ref as A
import _pixelsnail_model_ref as M
import _pixelsnail_ref as R


def label_rows(embed, label):
    """[B, 2 C]: row label[b] of the table, zeros for a label outside [0, n_label)."""
    n_label = embed.shape[0]
    ok = (label >= 0) & (label < n_label)
    rows = embed[label.clamp(0, n_label - 1)]
    return rows * ok.to(embed.dtype).unsqueeze(1)


def gated_resblock_label(x, sd, condition=None, label=None):
    """The 'causal' gated block of a PixelBlock (eval mode: no dropout); sd: the block's state_dict."""
    h = F.elu(R.wn_conv(F.elu(x), sd, "conv1.conv.conv.", "causal"))
    t = R.wn_conv(h, sd, "conv2.conv.conv.", "causal")
    if condition is not None:
        t = t + R.wn_conv(condition, sd, "condition.conv.", "wnconv2d")
    if "label_embed" in sd:
        t = t + label_rows(sd["label_embed"], label)[:, :, None, None]
    return F.glu(t, 1) + x


def pixel_block(x, background, sd, attention, condition=None, label=None):
    out = x
    for i in range(M._count(sd, "resblocks.{}.conv1.conv.conv.weight_v")):
        out = gated_resblock_label(out, M.sub(sd, f"resblocks.{i}."), condition, label)
    if attention:
        key = R.gated_resblock(torch.cat([x, out, background], 1), M.sub(sd, "key_resblock."))
        query = R.gated_resblock(torch.cat([out, background], 1), M.sub(sd, "query_resblock."))
        attn = A.causal_attention(query, key, M.sub(sd, "causal_attention."), 8)
        return R.gated_resblock(out, M.sub(sd, "out_resblock."), aux=attn)
    return R.wn_conv(torch.cat([out, background], 1), sd, "out.conv.", "wnconv2d")


def pixelsnail(codes, sd, n_class, attention, condition=None, label=None):
    """M.pixelsnail with the label; sd may hold blocks.<i>.resblocks.<k>.label_embed tables (none: the unlabelled model)."""
    b, h, w = codes.shape
    x = M.input_stage(codes, sd, n_class)
    background = sd["background"][:, :, :h, :].expand(b, 2, h, w)
    cond = None
    if condition is not None:
        cond = M.upsample2(M.cond_resnet(condition, M.sub(sd, "cond_resnet."), n_class))[:, :, :h, :]
    for i in range(M._count(sd, "blocks.{}.resblocks.0.conv1.conv.conv.weight_v")):
        x = pixel_block(x, background, M.sub(sd, f"blocks.{i}."), attention, cond, label)
    return M.head(x, M.sub(sd, "out."))


def table_names(sd):
    return sorted(k for k in sd if k.endswith("label_embed"))


def add_tables(sd, n_label, seed, scale=0.05):
    """sd plus one seeded table normal(0, scale) per 'causal' block (float32, as the model holds them)."""
    out = dict(sd)
    gen = torch.Generator().manual_seed(seed)
    for k in sorted(sd):
        if ".resblocks." in k and k.endswith(".conv2.conv.conv.weight_g"):
            name = k[:-len("conv2.conv.conv.weight_g")] + "label_embed"
            out[name] = torch.randn(n_label, sd[k].shape[0], generator=gen) * scale
    return out


def run(sd, codes, n_class, attention, condition, label, dtype):
    """{'logits', 'loss', 'grad.<name>'} of the labelled model in `dtype` (the loss is the mean cross-entropy of the codes)."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v).clone() for k, v in sd.items()}
    params = [k for k in sd if k != "background"]
    for k in params:
        sd[k].requires_grad_(True)
    logits = pixelsnail(codes, sd, n_class, attention, condition, label)
    loss, _ = M.cross_entropy(logits, codes)
    loss.backward()
    res = {"logits": logits.detach(), "loss": loss.detach()}
    res.update({"grad." + k: sd[k].grad for k in params})
    return res


# ----------------------------------------------------------------------------- the kernels as formulas over rows
def _bias(embed, label, ppi, pixels):
    """[pixels, 2 Ch]: what each pixel's row of t gets (pixel p belongs to image p // ppi)."""
    return label_rows(embed, label).repeat_interleave(ppi, 0)[:pixels]


def glu_label_fwd(t, res, embed, label, ppi):
    ch = res.shape[1]
    s = t + _bias(embed, label, ppi, t.shape[0])
    return s[:, :ch] * torch.sigmoid(s[:, ch:]) + res


def glu_label_bwd(dout, t, embed, label, ppi):
    """dt [pixels, 2 Ch]: the existing backward's formulas with the row added to a and b."""
    ch = dout.shape[1]
    s = t + _bias(embed, label, ppi, t.shape[0])
    a, sg = s[:, :ch], torch.sigmoid(s[:, ch:])
    return torch.cat([dout * sg, dout * a * sg * (1 - sg)], 1)


def label_embed_grad(dt, label, ppi, n_label):
    """dE [n_label, C2]: images ascending, each image's pixel sum first; rows of unused labels 0."""
    images = label.shape[0]
    per_image = dt.view(images, ppi, dt.shape[1]).sum(1)
    dE = torch.zeros(n_label, dt.shape[1], dtype=dt.dtype)
    for b in range(images):
        l = int(label[b])
        if 0 <= l < n_label:
            dE[l] = dE[l] + per_image[b]
    return dE
