"""Stage-2 prior pieces (drop-in for the reference's pixelsnail.py).  So far: CausalAttention (pixelsnail.py:195-234);
the rest of PixelSNAIL is assembled from the conv kernels plus this layer in later work."""
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
