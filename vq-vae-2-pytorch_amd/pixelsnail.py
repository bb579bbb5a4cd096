"""Stage-2 prior pieces (drop-in for the reference's pixelsnail.py).  So far: WNConv2d, CausalConv2d and GatedResBlock
(pixelsnail.py:21-179) and CausalAttention (pixelsnail.py:195-234); PixelBlock and PixelSNAIL are assembled from these in
later work."""
import math

import torch
from torch import nn

from . import ops
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
        w = ops.WeightNormFn.apply(self.weight_v, self.weight_g)
        return ops.conv_op(x, w.view(self.spec.cout, self.spec.cin, 1, 1), self.bias, self.spec)


class CausalAttention(nn.Module):
    """CausalAttention(query_channel, key_channel, channel, n_head=8, dropout=0.1) of the reference: position i of the
    H * W raster attends to positions j < i.  forward(query [B,Cq,H,W], key [B,Ck,H,W]) -> [B,channel,H,W] (a
    channels-last view, as the reference returns).  Masked scores are excluded where the reference fills in -1e4: equal
    to the last bit of every exponential while all unmasked scores of a row are above about -9,896."""

    def __init__(self, query_channel, key_channel, channel, n_head=8, dropout=0.1):
        super().__init__()
        self.dim_head = ops.attn_check_geometry(channel, n_head)
        if not 0.0 <= dropout < 1.0:
            raise NotImplementedError(f"vqvae2_amd.CausalAttention: dropout must be in [0, 1), got {dropout}")
        self.n_head = n_head
        self.channel = channel
        self.p = float(dropout)
        self.query = _WNLinear(query_channel, channel)
        self.key = _WNLinear(key_channel, channel)
        self.value = _WNLinear(key_channel, channel)

    def extra_repr(self):
        return f"channel={self.channel}, n_head={self.n_head}, dropout={self.p}"

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
        o = ops.CausalAttnFn.apply(q, k, v, self.n_head, p, seed)
        return ops.from_nhwc(o, self.channel)


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

    def nhwc(self, x, residual=None):
        """x [N,H,W,ceil4(in)] -> [N,H,W,ceil4(out)] (+ residual, added in the conv's epilogue)."""
        c = self.conv
        s = self.spec
        # the effective weight is a non-leaf tensor made each forward (see _WNLinear.nhwc)
        w = ops.WeightNormFn.apply(c.weight_v.view(s.cout, -1), c.weight_g).view(s.cout, s.cin, s.k, s.kw)
        y = ops.conv_op(x, w, c.bias, s, residual=residual)
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

    def nhwc(self, x, residual=None):
        if self.padding == 'causal':
            # (a parameter edit, not part of the graph: the reference's own statement)
            self.conv.conv.weight_v.data[:, :, -1, self.causal:].zero_()
        return self.conv.nhwc(x, residual)

    def forward(self, input):
        return ops.from_nhwc(self.nhwc(ops.to_nhwc(input)), self.conv.out_channel)


class GatedResBlock(nn.Module):
    """GatedResBlock(in_channel, channel, kernel_size, conv='wnconv2d', activation=nn.ELU, dropout=0.1,
    auxiliary_channel=0, condition_dim=0) of the reference (pixelsnail.py:122-179):

        h = conv1(ELU(input)) [+ aux_conv(ELU(aux_input))]       the add is conv1's residual epilogue
        h = dropout(ELU(h))                                       one kernel
        t = conv2(h) [+ condition(condition)]                     again the residual epilogue
        out = t[:, :in_channel] * sigmoid(t[:, in_channel:]) + input       one kernel

    forward takes and returns NCHW-shaped tensors; nhwc() the internal [N,H,W,ceil4(C)] ones, so that blocks chain
    without layout changes.  Kept for the backward: ELU(input) (and ELU(aux_input)), conv1's output, the dropped-out
    activation, conv2's output t (and `condition`), plus one dropout seed -- no mask, no sigmoid, no separate copy of the
    input."""

    def __init__(self, in_channel, channel, kernel_size, conv='wnconv2d', activation=nn.ELU, dropout=0.1,
                 auxiliary_channel=0, condition_dim=0):
        super().__init__()
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

    def extra_repr(self):
        return f"dropout={self.p}"

    def nhwc(self, x, aux=None, condition=None):
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
        return ops.GluResFn.apply(t, skip, self.in_channel)

    def forward(self, input, aux_input=None, condition=None):
        x = ops.to_nhwc(input)
        aux = ops.to_nhwc(aux_input) if aux_input is not None else None
        cond = ops.to_nhwc(condition) if condition is not None else None
        return ops.from_nhwc(self.nhwc(x, aux, cond), self.in_channel)
