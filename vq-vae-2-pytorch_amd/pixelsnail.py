"""The stage-2 prior (drop-in for the reference's pixelsnail.py): WNConv2d, CausalConv2d and GatedResBlock
(pixelsnail.py:21-179), CausalAttention (pixelsnail.py:195-234), and PixelBlock, CondResNet and PixelSNAIL
(pixelsnail.py:237-431) assembled from them.  Inside a model everything stays NHWC; the integer codes enter through the
one-hot convolution kernels and the logits leave as a channels-last view."""
import math

import torch
from torch import nn

from . import ops
from ._lib import lib, check
from .ops import ConvSpec

BQ = ops.ATTN_BQ   # query and key tile lengths of the attention kernels
BK = ops.ATTN_BK


class _WNLinear(nn.Module):
    """weight_norm(nn.Linear(in_dim, out_dim)) applied per pixel: parameters bias [out], weight_g [out, 1], weight_v
    [out, in] as torch.nn.utils.weight_norm names and initialises them.  Runs as a 1x1 convolution over NHWC."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.spec = ConvSpec(False, in_dim, out_dim, 1, 1, 0)
        weight = torch.empty(out_dim, in_dim)
        nn.init.kaiming_uniform_(weight, a=math.sqrt(5))           # nn.Linear.reset_parameters
        bound = 1 / math.sqrt(in_dim)
        self.bias = nn.Parameter(torch.empty(out_dim).uniform_(-bound, bound))
        self.weight_g = nn.Parameter(weight.norm(2, dim=1, keepdim=True))   # weight_norm: g = ||w|| per row, v = w
        self.weight_v = nn.Parameter(weight)

    def nhwc(self, x):
        # the effective weight is a non-leaf tensor made each forward: its packed panels are cached on that tensor object
        # and die with it, and its gradient takes the immediate (not the deferred) weight-gradient path of conv_wgrad
        # (a trainer's WeightNormPlan, while it is active and current, hands out its prepared view instead: no launch)
        w = ops.planned_weight(self.weight_v, self.weight_g)
        if w is None:
            w = ops.WeightNormFn.apply(self.weight_v, self.weight_g).view(self.spec.cout, self.spec.cin, 1, 1)
        return ops.conv_op(x, w, self.bias, self.spec)


class CausalAttention(nn.Module):
    """CausalAttention(query_channel, key_channel, channel, n_head=8, dropout=0.1) of the reference: position i of the
    H * W raster attends to positions j < i.  forward(query [B,Cq,H,W], key [B,Ck,H,W]) -> [B,channel,H,W] (a
    channels-last view, as the reference returns).  Masked scores are excluded where the reference fills in -1e4: equal
    to the last bit of every exponential while all unmasked scores of a row are above about -9,896.
    `bf16` (a plain attribute, default False, no parameter or buffer; set_attention_precision sets it) is the permission
    of ops.CausalAttnFn: bf16 operands in the attention core where dim_head is a multiple of 16.  The three projections
    stay fp32, and so does PriorSampler's attention (vq2_causal_attn_fwd_rows), whatever this says."""

    def __init__(self, query_channel, key_channel, channel, n_head=8, dropout=0.1):
        super().__init__()
        self.dim_head = ops.attn_check_geometry(channel, n_head)
        if not 0.0 <= dropout < 1.0:
            raise NotImplementedError(f"vqvae2_amd.CausalAttention: dropout must be in [0, 1), got {dropout}")
        self.n_head = n_head
        self.channel = channel
        self.p = float(dropout)
        self.bf16 = False
        self.query = _WNLinear(query_channel, channel)
        self.key = _WNLinear(key_channel, channel)
        self.value = _WNLinear(key_channel, channel)

    def extra_repr(self):
        return f"channel={self.channel}, n_head={self.n_head}, dropout={self.p}" + (", bf16" if self.bf16 else "")

    def forward(self, query, key):
        ops._require_cuda(query, "query")
        ops._require_cuda(key, "key")
        if query.dim() != 4 or key.dim() != 4 or query.shape[0] != key.shape[0] or query.shape[2:] != key.shape[2:]:
            raise RuntimeError("CausalAttention: query [B,Cq,H,W] and key [B,Ck,H,W] of one batch and size expected")
        qx, kx = ops.to_nhwc(query), ops.to_nhwc(key)
        q, k, v = self.query.nhwc(qx), self.key.nhwc(kx), self.value.nhwc(kx)
        p = self.p if self.training else 0.0
        # one integer per call from torch's default CPU generator: torch.manual_seed makes a run repeatable
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0
        o = ops.CausalAttnFn.apply(q, k, v, self.n_head, p, seed, self.bf16)
        return ops.from_nhwc(o, self.channel)

    def nhwc(self, qx, kx):
        """forward() on NHWC operands [B,H,W,ceil4(Cq)] and [B,H,W,ceil4(Ck)] -> NHWC [B,H,W,channel]: what PixelBlock
        calls, without the layout round trip at the module boundary."""
        kx1, kx2 = ops.FanOutFn.apply(kx)        # the key and value projections read one tensor: their gradients meet in a library kernel
        q, k, v = self.query.nhwc(qx), self.key.nhwc(kx1), self.value.nhwc(kx2)
        p = self.p if self.training else 0.0
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0
        return ops.CausalAttnFn.apply(q, k, v, self.n_head, p, seed, self.bf16)


# ----------------------------------------------------------------------------- weight-normed convs and the gated block
def _pair(v, what):
    if isinstance(v, int):
        return v, v
    v = tuple(int(a) for a in v)
    if len(v) != 2:
        raise NotImplementedError(f"vqvae2_amd: {what} must be an int or a pair, got {v}")
    return v


def _elu_or_none(activation, who):
    """None, or True for ELU with alpha 1 (the class, or an instance with or without inplace); anything else is refused."""
    if activation is None:
        return False
    if activation is nn.ELU or (isinstance(activation, nn.ELU) and activation.alpha == 1.0):
        return True
    raise NotImplementedError(f"vqvae2_amd.{who}: activation must be None or nn.ELU (alpha 1), got {activation!r}")


class _WNConvParams(nn.Module):
    """The parameters of weight_norm(nn.Conv2d(...)) under its names and with its initialisation: weight_v = the conv's
    kaiming-uniform weight, weight_g [out,1,1,1] = its norm per output row (so the effective weight starts as weight_v),
    bias uniform in +-1/sqrt(fan_in)."""

    def __init__(self, in_channel, out_channel, kh, kw, bias):
        super().__init__()
        weight = torch.empty(out_channel, in_channel, kh, kw)
        nn.init.kaiming_uniform_(weight, a=math.sqrt(5))           # nn.Conv2d.reset_parameters
        if bias:
            bound = 1 / math.sqrt(in_channel * kh * kw)
            self.bias = nn.Parameter(torch.empty(out_channel).uniform_(-bound, bound))
        else:
            self.register_parameter("bias", None)
        self.weight_g = nn.Parameter(weight.flatten(1).norm(2, dim=1).view(out_channel, 1, 1, 1))
        self.weight_v = nn.Parameter(weight)


class WNConv2d(nn.Module):
    """WNConv2d(in_channel, out_channel, kernel_size, stride=1, padding=0, bias=True, activation=None) of the reference
    (pixelsnail.py:21-60): a weight-normed conv.  Stride 1 and a padding that keeps the size (2 * pad == k - 1 per axis,
    so 0 for 1x1) only; activation None or ELU.  `_geometry` = (pad_top, pad_left) is how CausalConv2d places the kernel
    (the reference pads with nn.ZeroPad2d and runs this layer unpadded)."""

    def __init__(self, in_channel, out_channel, kernel_size, stride=1, padding=0, bias=True, activation=None, *,
                 _geometry=None):
        super().__init__()
        kh, kw = _pair(kernel_size, "kernel_size")
        if stride != 1 and tuple(_pair(stride, "stride")) != (1, 1):
            raise NotImplementedError(f"vqvae2_amd.WNConv2d: stride 1 only, got {stride}")
        if not (1 <= kh <= 7 and 1 <= kw <= 7 and kh * kw <= 32):
            raise NotImplementedError(f"vqvae2_amd.WNConv2d: kernel sides in 1..7 with at most 32 taps, got {kh} x {kw}")
        if _geometry is None:
            ph, pw = _pair(padding, "padding")
            if 2 * ph != kh - 1 or 2 * pw != kw - 1:
                raise NotImplementedError(f"vqvae2_amd.WNConv2d: padding must keep the size (2 * pad == k - 1 per axis); got "
                                          f"kernel {kh} x {kw}, padding {ph}, {pw}")
        else:
            ph, pw = _geometry
        self.elu = _elu_or_none(activation, "WNConv2d")
        self.activation = activation
        self.out_channel = out_channel
        self.kernel_size = [kh, kw]
        self.spec = ConvSpec.geom(in_channel, out_channel, kh, kw, ph, pw)
        self.conv = _WNConvParams(in_channel, out_channel, kh, kw, bias)

    def _weight(self):
        """The effective weight [out, in, kh, kw]: a non-leaf tensor made each forward (see _WNLinear.nhwc)."""
        c = self.conv
        s = self.spec
        w = ops.planned_weight(c.weight_v, c.weight_g)
        if w is None:
            w = ops.WeightNormFn.apply(c.weight_v.view(s.cout, -1), c.weight_g).view(s.cout, s.cin, s.k, s.kw)
        return w

    def nhwc(self, x, residual=None):
        """x [N,H,W,ceil4(in)] -> [N,H,W,ceil4(out)] (+ residual, added in the conv's epilogue)."""
        c = self.conv
        s = self.spec
        y = ops.conv_op(x, self._weight(), c.bias, s, residual=residual)
        return ops.EluFn.apply(y, s.cout) if self.elu else y

    def onehot(self, codes, shift=(0, 0), acc=None):
        """This layer applied to one_hot(codes) (codes int64 [N,H,W], in_channel classes) -> NHWC [N,H,W,ceil4(out)], the
        result moved shift = (down, right) pixels and `acc` added, all in ops.OneHotConvFn's one launch."""
        c = self.conv
        s = self.spec
        y = ops.onehot_conv(codes, self._weight(), c.bias, (s.k, s.kw, s.pad_top, s.pad_left), shift, acc)
        return ops.EluFn.apply(y, s.cout) if self.elu else y

    def forward(self, input):
        return ops.from_nhwc(self.nhwc(ops.to_nhwc(input)), self.out_channel)


class CausalConv2d(nn.Module):
    """CausalConv2d(in_channel, out_channel, kernel_size, stride=1, padding='downright', activation=None) of the reference
    (pixelsnail.py:71-119).  'downright': the kernel ends at the output pixel (pad_top = KH - 1, pad_left = KW - 1);
    'down' and 'causal': it ends at the output row and is centred on the column (pad_left = KW // 2, odd KW only: with an
    even KW the reference's output is one column wider than its input).  'causal' also zeroes weight_v[:, :, -1, KW // 2:]
    in place on every forward, as the reference does: the centre pixel and everything right of it in the last row."""

    def __init__(self, in_channel, out_channel, kernel_size, stride=1, padding='downright', activation=None):
        super().__init__()
        kh, kw = _pair(kernel_size, "kernel_size")
        self.kernel_size = [kh, kw]
        if padding == 'downright':
            geometry = (kh - 1, kw - 1)
        elif padding in ('down', 'causal'):
            if kw % 2 == 0:
                raise NotImplementedError(f"vqvae2_amd.CausalConv2d: padding={padding!r} needs an odd kernel width, got {kw}")
            geometry = (kh - 1, kw // 2)
        else:
            raise NotImplementedError(f"vqvae2_amd.CausalConv2d: padding must be 'downright', 'down' or 'causal', got {padding!r}")
        self.causal = kw // 2 if padding == 'causal' else 0
        self.padding = padding
        self.conv = WNConv2d(in_channel, out_channel, [kh, kw], stride=stride, padding=0, activation=activation,
                             _geometry=geometry)

    def extra_repr(self):
        return f"padding={self.padding!r}"

    def _mask(self):
        # (a parameter edit, not part of the graph: the reference's own statement; a trainer's WeightNormPlan has already
        # made it, for every layer at once, when it formed this step's weights)
        if self.padding == 'causal' and ops.plan_ready(self.conv.conv.weight_v) is None:
            self.conv.conv.weight_v.data[:, :, -1, self.causal:].zero_()

    def nhwc(self, x, residual=None):
        self._mask()
        return self.conv.nhwc(x, residual)

    def onehot(self, codes, shift=(0, 0), acc=None):
        self._mask()
        return self.conv.onehot(codes, shift, acc)

    def forward(self, input):
        return ops.from_nhwc(self.nhwc(ops.to_nhwc(input)), self.conv.out_channel)


class GatedResBlock(nn.Module):
    """GatedResBlock(in_channel, channel, kernel_size, conv='wnconv2d', activation=nn.ELU, dropout=0.1,
    auxiliary_channel=0, condition_dim=0) of the reference (pixelsnail.py:122-179), and n_label=0 as a last argument:

        h = conv1(ELU(input)) [+ aux_conv(ELU(aux_input))]       the add is conv1's residual epilogue
        h = dropout(ELU(h))                                       one kernel
        t = conv2(h) [+ condition(condition)]                     again the residual epilogue
        out = t[:, :in_channel] * sigmoid(t[:, in_channel:]) + input       one kernel

    n_label > 0 makes the block class-conditional, the way PixelCNN++ puts a class vector into a gate: the fp32 parameter
    label_embed [n_label, 2 * in_channel] (normal(0, 0.05)) exists, nhwc() / forward() need `label` (int64 [N] on the device)
    and the last line reads [a | b] = t + label_embed[label[image]], out = a * sigmoid(b) + input: still one kernel, t in
    memory stays the conv output.  A label outside [0, n_label) adds nothing and receives no gradient.  n_label == 0: no
    such parameter, `label` is refused, and every launch is what it is without this argument.

    forward takes and returns NCHW-shaped tensors; nhwc() the internal [N,H,W,ceil4(C)] ones, so that blocks chain
    without layout changes.  Kept for the backward: ELU(input) (and ELU(aux_input)), conv1's output, the dropped-out
    activation, conv2's output t (and `condition`), plus one dropout seed -- no mask, no sigmoid, no separate copy of the
    input."""

    def __init__(self, in_channel, channel, kernel_size, conv='wnconv2d', activation=nn.ELU, dropout=0.1,
                 auxiliary_channel=0, condition_dim=0, n_label=0):
        super().__init__()
        if n_label < 0:
            raise ValueError(f"vqvae2_amd.GatedResBlock: n_label must be >= 0, got {n_label}")
        if activation is not nn.ELU:
            raise NotImplementedError(f"vqvae2_amd.GatedResBlock: activation must be nn.ELU, got {activation!r}")
        if not 0.0 <= dropout < 1.0:
            raise NotImplementedError(f"vqvae2_amd.GatedResBlock: dropout must be in [0, 1), got {dropout}")
        if conv == 'wnconv2d':
            if not isinstance(kernel_size, int):
                raise NotImplementedError("vqvae2_amd.GatedResBlock: conv='wnconv2d' takes an int kernel_size")

            def conv_module(i, o, k):
                return WNConv2d(i, o, k, padding=k // 2)
        elif conv == 'causal_downright':
            def conv_module(i, o, k):
                return CausalConv2d(i, o, k, padding='downright')
        elif conv == 'causal':
            def conv_module(i, o, k):
                return CausalConv2d(i, o, k, padding='causal')
        else:
            raise NotImplementedError(f"vqvae2_amd.GatedResBlock: conv must be 'wnconv2d', 'causal_downright' or 'causal', "
                                      f"got {conv!r}")
        self.in_channel, self.channel = in_channel, channel
        self.auxiliary_channel, self.condition_dim = auxiliary_channel, condition_dim
        self.p = float(dropout)
        self.conv1 = conv_module(in_channel, channel, kernel_size)
        if auxiliary_channel > 0:
            self.aux_conv = WNConv2d(auxiliary_channel, channel, 1)
        self.conv2 = conv_module(channel, in_channel * 2, kernel_size)
        if condition_dim > 0:
            self.condition = WNConv2d(condition_dim, in_channel * 2, 1, bias=False)
        self.n_label = int(n_label)
        if self.n_label > 0:
            self.label_embed = nn.Parameter(torch.empty(self.n_label, in_channel * 2).normal_(0.0, 0.05))

    def extra_repr(self):
        return f"dropout={self.p}"

    def nhwc(self, x, aux=None, condition=None, label=None):
        if (label is not None) != (self.n_label > 0):
            raise RuntimeError("GatedResBlock: a block built with n_label > 0 needs `label`" if label is None else
                               "GatedResBlock: label given to a block built with n_label=0")
        r = None
        if aux is not None:
            if self.auxiliary_channel <= 0:
                raise RuntimeError("GatedResBlock: aux_input given to a block built with auxiliary_channel=0")
            r = self.aux_conv.nhwc(ops.EluFn.apply(aux, self.auxiliary_channel))
        # the input feeds the first ELU and the skip connection: its two gradients are summed by a library kernel
        x, skip = ops.FanOutFn.apply(x)
        h = self.conv1.nhwc(ops.EluFn.apply(x, self.in_channel), residual=r)
        p = self.p if self.training else 0.0
        # one integer per call from torch's default CPU generator (as CausalAttention); nothing is drawn without dropout
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0
        h = ops.EluDropoutFn.apply(h, self.channel, p, seed)
        r = None
        if condition is not None:
            if self.condition_dim <= 0:
                raise RuntimeError("GatedResBlock: condition given to a block built with condition_dim=0")
            r = self.condition.nhwc(condition)
        t = self.conv2.nhwc(h, residual=r)
        if label is not None:
            return ops.GluResLabelFn.apply(t, skip, self.in_channel, self.label_embed, label)
        return ops.GluResFn.apply(t, skip, self.in_channel)

    def forward(self, input, aux_input=None, condition=None, label=None):
        x = ops.to_nhwc(input)
        aux = ops.to_nhwc(aux_input) if aux_input is not None else None
        cond = ops.to_nhwc(condition) if condition is not None else None
        return ops.from_nhwc(self.nhwc(x, aux, cond, label), self.in_channel)


# ----------------------------------------------------------------------------- PixelBlock, CondResNet, PixelSNAIL
def _fan(x, k):
    """k aliases of x whose gradients are summed by library kernels (chained ops.FanOutFn), not by autograd's own adds."""
    outs = []
    for _ in range(k - 1):
        a, x = ops.FanOutFn.apply(x)
        outs.append(a)
    outs.append(x)
    return outs


def _repeat_batch(x1, batch):
    """NHWC [1,H,W,C] -> [batch,H,W,C], one slice copy per image (the coordinate planes: made once and cached)."""
    _, h, w, c = x1.shape
    out = torch.empty((batch, h, w, c), device=x1.device, dtype=torch.float32)
    for b in range(batch):
        check(lib.vq2_slice_copy(ops._p(x1), c, ops._p(out[b]), c, h * w, c, 0, ops._stream()), "slice_copy")
    return out


class PixelBlock(nn.Module):
    """PixelBlock(in_channel, channel, kernel_size, n_res_block, attention=True, dropout=0.1, condition_dim=0) of the
    reference (pixelsnail.py:237-308), and n_label=0 as a last argument (the 'causal' blocks take the class label, the
    attention branch does not): n_res_block 'causal' GatedResBlocks, then either the attention branch (key and query
    blocks over the concatenations with the two coordinate planes, CausalAttention, and a block that takes the attention
    output as its auxiliary input) or a 1x1 WNConv2d over [out, background].  in_channel must be a multiple of 4 (the
    concatenations are slice copies of whole 16-byte groups) and kernel_size odd."""

    def __init__(self, in_channel, channel, kernel_size, n_res_block, attention=True, dropout=0.1, condition_dim=0,
                 n_label=0):
        super().__init__()
        if in_channel % 4 != 0:
            raise NotImplementedError(f"vqvae2_amd.PixelBlock: in_channel must be a multiple of 4, got {in_channel}")
        if not isinstance(kernel_size, int) or kernel_size % 2 == 0:
            raise NotImplementedError(f"vqvae2_amd.PixelBlock: kernel_size must be an odd int, got {kernel_size} (the "
                                      "reference's 'causal' blocks change the width with an even one)")
        if attention:
            ops.attn_check_geometry(in_channel // 2, 8)
        self.in_channel = in_channel
        self.resblocks = nn.ModuleList([
            GatedResBlock(in_channel, channel, kernel_size, conv='causal', dropout=dropout, condition_dim=condition_dim,
                          n_label=n_label)
            for _ in range(n_res_block)])
        self.n_label = int(n_label)
        self.attention = attention
        if attention:
            self.key_resblock = GatedResBlock(in_channel * 2 + 2, in_channel, 1, dropout=dropout)
            self.query_resblock = GatedResBlock(in_channel + 2, in_channel, 1, dropout=dropout)
            self.causal_attention = CausalAttention(in_channel + 2, in_channel * 2 + 2, in_channel // 2, dropout=dropout)
            self.out_resblock = GatedResBlock(in_channel, in_channel, 1, auxiliary_channel=in_channel // 2, dropout=dropout)
        else:
            self.out = WNConv2d(in_channel + 2, in_channel, 1)

    def nhwc(self, x, background, conditions=None, label=None):
        """x [N,H,W,in_channel], background [N,H,W,4] (two real channels); conditions: None or one NHWC alias of the
        condition per res block; label: int64 [N] on the device for a block built with n_label > 0, else None."""
        if (label is not None) != (self.n_label > 0):
            raise RuntimeError("PixelBlock: a block built with n_label > 0 needs `label`" if label is None else
                               "PixelBlock: label given to a block built with n_label=0")
        if self.attention:
            x, x_key = ops.FanOutFn.apply(x)
        out = x
        for i, resblock in enumerate(self.resblocks):
            out = resblock.nhwc(out, condition=None if conditions is None else conditions[i], label=label)
        if self.attention:
            out_key, out_query, out = _fan(out, 3)
            key = self.key_resblock.nhwc(ops.CatNFn.apply(x_key, out_key, background))
            query = self.query_resblock.nhwc(ops.CatNFn.apply(out_query, background))
            attn_out = self.causal_attention.nhwc(query, key)
            return self.out_resblock.nhwc(out, aux=attn_out)
        return self.out.nhwc(ops.CatNFn.apply(out, background))

    def forward(self, input, background, condition=None, label=None):
        cond = None
        if condition is not None:
            cond = _fan(ops.to_nhwc(condition), len(self.resblocks)) if len(self.resblocks) else None
        return ops.from_nhwc(self.nhwc(ops.to_nhwc(input), ops.to_nhwc(background), cond, label), self.in_channel)


class CondResNet(nn.Module):
    """CondResNet(in_channel, channel, kernel_size, n_res_block) of the reference (pixelsnail.py:311-323): a size-preserving
    WNConv2d and n_res_block plain GatedResBlocks.  forward takes what the reference takes (a float [B,in_channel,H,W]
    tensor, one-hot there) or the int64 codes [B,H,W] themselves, which go through the one-hot convolution kernel."""

    def __init__(self, in_channel, channel, kernel_size, n_res_block):
        super().__init__()
        if not isinstance(kernel_size, int) or kernel_size % 2 == 0:
            raise NotImplementedError(f"vqvae2_amd.CondResNet: kernel_size must be an odd int, got {kernel_size}")
        self.channel = channel
        blocks = [WNConv2d(in_channel, channel, kernel_size, padding=kernel_size // 2)]
        for _ in range(n_res_block):
            blocks.append(GatedResBlock(channel, channel, kernel_size))
        self.blocks = nn.Sequential(*blocks)

    def nhwc(self, input):
        first = self.blocks[0]
        x = first.onehot(input) if input.dtype == torch.int64 else first.nhwc(ops.to_nhwc(input))
        for block in list(self.blocks)[1:]:
            x = block.nhwc(x)
        return x

    def forward(self, input):
        return ops.from_nhwc(self.nhwc(input), self.channel)


class PixelSNAIL(nn.Module):
    """PixelSNAIL(shape, n_class, channel, kernel_size, n_block, n_res_block, res_channel, attention=True, dropout=0.1,
    n_cond_res_block=0, cond_res_channel=0, cond_res_kernel=3, n_out_res_block=0) of the reference (pixelsnail.py:326-431),
    with its parameter and buffer names, and n_label=0 as a last argument: with n_label > 0 the prior is class-conditional,
    every 'causal' GatedResBlock of every PixelBlock holds a table blocks.<i>.resblocks.<k>.label_embed [n_label, 2 * channel]
    and forward needs label, int64 [B] on the device (see GatedResBlock; a label outside [0, n_label) adds nothing).  With
    n_label == 0 the state_dict keys and every launch are those of the reference's model, and a label is refused.

    forward(input [B,H,W] int64, condition=None [B,H/2,W/2] int64, cache=None, label=None) -> (out, cache): out is a channels-last view
    of shape [B,n_class,H,W] (a copy when n_class is no multiple of 4); cache['condition'] is a detached clone of the
    upsampled condition features and is used instead of running cond_resnet when present; an input of fewer rows than
    shape[0] uses the first rows of the coordinate planes and of the condition.  A code outside [0, n_class) contributes
    nothing (the reference raises).  Refused at construction: channel % 4 != 0, an even kernel_size or cond_res_kernel,
    and with attention a channel whose half the 8-head attention kernels do not take."""

    def __init__(self, shape, n_class, channel, kernel_size, n_block, n_res_block, res_channel, attention=True,
                 dropout=0.1, n_cond_res_block=0, cond_res_channel=0, cond_res_kernel=3, n_out_res_block=0, n_label=0):
        super().__init__()
        height, width = shape
        if n_label < 0:
            raise ValueError(f"vqvae2_amd.PixelSNAIL: n_label must be >= 0, got {n_label}")
        if n_label > 0 and n_res_block < 1:
            raise ValueError("vqvae2_amd.PixelSNAIL: n_label > 0 needs n_res_block >= 1 (the label enters the 'causal' blocks)")
        self.n_label = int(n_label)
        if channel % 4 != 0:
            raise NotImplementedError(f"vqvae2_amd.PixelSNAIL: channel must be a multiple of 4, got {channel}")
        if not isinstance(kernel_size, int) or kernel_size % 2 == 0:
            raise NotImplementedError(f"vqvae2_amd.PixelSNAIL: kernel_size must be an odd int, got {kernel_size} (the "
                                      "reference's 'causal' blocks change the width with an even one)")
        if not isinstance(cond_res_kernel, int) or cond_res_kernel % 2 == 0:
            raise NotImplementedError(f"vqvae2_amd.PixelSNAIL: cond_res_kernel must be an odd int, got {cond_res_kernel}")
        if attention:
            ops.attn_check_geometry(channel // 2, 8)
        kernel = kernel_size
        ops.onehot_check_geometry(n_class, (kernel + 1) // 2, kernel)
        self.n_class = n_class
        self.channel = channel
        self.cond_res_channel = cond_res_channel
        self.horizontal = CausalConv2d(n_class, channel, [kernel // 2, kernel], padding='down')
        self.vertical = CausalConv2d(n_class, channel, [(kernel + 1) // 2, kernel // 2], padding='downright')
        coord_x = (torch.arange(height).float() - height / 2) / height
        coord_x = coord_x.view(1, 1, height, 1).expand(1, 1, height, width)
        coord_y = (torch.arange(width).float() - width / 2) / width
        coord_y = coord_y.view(1, 1, 1, width).expand(1, 1, height, width)
        self.register_buffer('background', torch.cat([coord_x, coord_y], 1))
        self.blocks = nn.ModuleList([
            PixelBlock(channel, res_channel, kernel_size, n_res_block, attention=attention, dropout=dropout,
                       condition_dim=cond_res_channel, n_label=n_label) for _ in range(n_block)])
        if n_cond_res_block > 0:
            self.cond_resnet = CondResNet(n_class, cond_res_channel, cond_res_kernel, n_cond_res_block)
        out = [GatedResBlock(channel, res_channel, 1) for _ in range(n_out_res_block)]
        out.extend([nn.ELU(inplace=True), WNConv2d(channel, n_class, 1)])
        self.out = nn.Sequential(*out)
        self._bg = None      # (key, NHWC coordinate planes repeated over the batch)

    def _background(self, batch, height):
        bg = self.background
        key = (batch, height, bg.data_ptr(), bg._version)
        if self._bg is None or self._bg[0] != key:
            planes = ops.to_nhwc(bg[:, :, :height, :].contiguous())            # [1, height, W, 4], two real channels
            self._bg = (key, _repeat_batch(planes, batch))
        return self._bg[1]

    def forward(self, input, condition=None, cache=None, label=None):
        if cache is None:
            cache = {}
        if input.dim() != 3:
            raise RuntimeError("PixelSNAIL: input [B,H,W] of int64 codes expected")
        batch, height, width = input.shape
        if label is None and self.n_label > 0:
            raise RuntimeError(f"PixelSNAIL: a model built with n_label={self.n_label} needs `label` (int64 [B])")
        if label is not None:
            if self.n_label <= 0:
                raise RuntimeError("PixelSNAIL: label given to a model built with n_label=0")
            label = ops.require_labels(label, batch, input.device)
        if height > self.background.shape[2] or width != self.background.shape[3]:
            raise RuntimeError(f"PixelSNAIL: input of {height} x {width} does not fit shape "
                               f"{tuple(self.background.shape[2:])} (fewer rows are allowed, other widths are not)")
        horizontal = self.horizontal.onehot(input, shift=(1, 0))                # shift_down(horizontal(one_hot))
        out = self.vertical.onehot(input, shift=(0, 1), acc=horizontal)         # + shift_right(vertical(one_hot))
        background = self._background(batch, height)
        conditions = None
        if condition is not None:
            if 'condition' in cache:
                cond = ops.to_nhwc(cache['condition'])
            else:
                # (through the module's __call__, so that forward hooks see it; the NCHW-shaped view comes back without a copy)
                cond = ops.Upsample2Fn.apply(ops.to_nhwc(self.cond_resnet(condition)), self.cond_res_channel)
                cache['condition'] = ops.from_nhwc(cond, self.cond_res_channel).detach().clone()
            if height < cond.shape[1]:
                cond = cond[:, :height]
            n_use = sum(len(b.resblocks) for b in self.blocks)
            conditions = _fan(cond, n_use) if n_use else None
        for block in self.blocks:
            n = len(block.resblocks)
            mine = None
            if conditions is not None:
                mine, conditions = conditions[:n], conditions[n:]
            out = block.nhwc(out, background, mine, label)
        for layer in self.out:
            if isinstance(layer, nn.ELU):
                out = ops.EluFn.apply(out, self.channel)       # nn.ELU(inplace=True) of the reference
            else:
                out = layer.nhwc(out)
        return ops.from_nhwc(out, self.n_class), cache


# ----------------------------------------------------------------------------- conv precision (--precision bf16)
def set_conv_precision(module, precision):
    """Give every WNConv2d under `module` (those inside CausalConv2d, GatedResBlock, PixelBlock, CondResNet and PixelSNAIL
    included) the conv precision 'bf16', 'bf16_wgrad' or 'fp32' by replacing its `spec`; returns (eligible_layers,
    total_layers).

    'bf16' is a permission (ConvSpec.bf16): where ops.conv_bf16_eligible holds -- forward with input channels a multiple of
    16, data gradient with output channels a multiple of 16 -- the launch rounds both operands to bfloat16 (nearest even) and
    accumulates in fp32; every other launch, the weight gradient, and every tensor in memory stay fp32.  A layer counts as
    eligible when its forward or its data gradient is.  'bf16_wgrad' sets that permission and ConvSpec.bf16_wgrad: where
    ops.conv_wgrad_bf16_eligible holds -- input and output channels both multiples of 16 -- the weight gradient rounds x and
    dy to bfloat16 as well (the bias gradient stays the fp32 sum of the unrounded dy); 'bf16' and 'fp32' clear it.
    Parameters, buffers and state_dict are untouched.  A PixelSNAIL's
    two one-hot input convs never run a conv kernel and are left out; attention projections (_WNLinear), the cross-entropy
    head and stage 1 have no such layers."""
    import dataclasses
    if precision not in ("bf16", "bf16_wgrad", "fp32"):
        raise ValueError(f"set_conv_precision: precision must be 'bf16', 'bf16_wgrad' or 'fp32', got {precision!r}")
    skip = set()
    for m in module.modules():
        if isinstance(m, PixelSNAIL):
            skip.update(id(c) for c in (m.horizontal.conv, m.vertical.conv))
    eligible = total = 0
    for m in module.modules():
        if isinstance(m, WNConv2d) and id(m) not in skip:
            m.spec = dataclasses.replace(m.spec, bf16=precision != "fp32", bf16_wgrad=precision == "bf16_wgrad")
            total += 1
            eligible += bool(ops.conv_bf16_eligible(m.spec) or ops.conv_bf16_eligible(m.spec, dgrad=True))
    return eligible, total


def conv_precision(module):
    """'bf16_wgrad' if any WNConv2d under `module` carries the bf16 weight-gradient permission, else 'bf16' if any carries
    the bf16 permission, else 'fp32'."""
    specs = [m.spec for m in module.modules() if isinstance(m, WNConv2d)]
    return "bf16_wgrad" if any(s.bf16_wgrad for s in specs) else "bf16" if any(s.bf16 for s in specs) else "fp32"


# ----------------------------------------------------------------------------- attention precision (--precision bf16_attn)
def set_attention_precision(module, precision):
    """Give every CausalAttention under `module` the attention precision 'bf16' or 'fp32' (its `bf16` attribute); returns
    (eligible_layers, total_layers).  'bf16' is a permission: where ops.attn_bf16_eligible holds (dim_head 16, 32, 48 or 64)
    the core's four matrix products round their operands to bfloat16 (nearest even) and accumulate in fp32; softmax, the
    three projections, every tensor in memory and every other geometry stay fp32.  Parameters, buffers and state_dict are
    untouched.  PriorSampler's attention is fp32 whatever this says."""
    if precision not in ("bf16", "fp32"):
        raise ValueError(f"set_attention_precision: precision must be 'bf16' or 'fp32', got {precision!r}")
    eligible = total = 0
    for m in module.modules():
        if isinstance(m, CausalAttention):
            m.bf16 = precision == "bf16"
            total += 1
            eligible += ops.attn_bf16_eligible(m.channel, m.n_head)
    return eligible, total


def attention_precision(module):
    """'bf16' if any CausalAttention under `module` carries the bf16 permission, else 'fp32'."""
    return "bf16" if any(m.bf16 for m in module.modules() if isinstance(m, CausalAttention)) else "fp32"
