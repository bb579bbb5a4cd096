"""Cases, inputs and fp64 references of the bf16-operand weight gradient (tests/test_gpu_wgrad_bf16.py runs them on the GPU,
tests/test_wgrad_bf16_cpu.py checks on the CPU that their tolerance bites).  No GPU and no library needed here.

The contract (include/vq2.h, VQ2_ALLOW_BF16 in the flags of vq2_conv_wgrad):
    dw[o][i][kh][kw] = sum over (n,h,w) of bf16(dy[n,h,w,o]) * bf16(a[n, h-pad_top+kh, w-pad_left+kw, i]),  a = x or relu(x),
accumulated in fp32; db = the fp32 sum of the UNROUNDED dy.  The references are therefore the fp64 weight gradient of the
bf16-ROUNDED operands (ReLU first, then the rounding) and the fp64 column sums of the unrounded dy: against them only the
accumulation differs and the project's weight-gradient tolerance applies unchanged; against the fp64 gradient of the
unrounded operands dw must MISS it.

A case is (name, cin, cout, kh, kw, pad_top, pad_left, n, h, w); inputs are scaled as tests/_conv_bf16_cases.py make_inputs."""
import torch

from _conv_bf16_cases import bf16, ceil4, conv, make_inputs  # noqa: F401  (re-exported for the tests)

CASES = [
    ("a", 16, 48, 5, 5, 4, 2, 2, 5, 7),        # causal; M = 70, ragged; one split
    ("b", 48, 80, 3, 2, 2, 1, 3, 4, 9),        # downright; K = 288 past a K tile; O past 64
    ("c", 32, 32, 1, 1, 0, 0, 1, 8, 16),       # M = 128; every tile full
    ("d", 16, 16, 7, 4, 6, 3, 2, 3, 3),        # 28 taps; kernel larger than the image; M = 18, less than one chunk
    ("e", 32, 144, 3, 3, 1, 1, 3, 13, 17),     # M = 663: several splits, the last one short; O past 128
    ("f", 64, 16, 3, 3, 1, 1, 1, 6, 10),       # the fp32 plan exchanges roles (sw)
    ("g", 128, 128, 3, 3, 1, 1, 1, 2, 32),     # the fp32 plan is wino
    ("h", 128, 64, 1, 1, 0, 0, 1, 5, 9),       # the 64 x 128 tile, which none of the above plans
    ("i", 128, 128, 1, 1, 0, 0, 2, 17, 16),    # the 128 x 128 tile split three ways: M = 544, the last split short (160 rows);
                                               # the bias partials of all 128 staging threads
]
NOT_ELIGIBLE = ("n", 20, 32, 3, 3, 1, 1, 1, 4, 8)
BY_NAME = {c[0]: c for c in CASES + [NOT_ELIGIBLE]}
MAX_ROWS = 65664     # rows the project's dw / db tolerance was set for (tests/test_gpu_geom_dispatch.py)


def rows(c):
    return c[7] * c[8] * c[9]


def eligible(c):
    """The stated rule on a same_size layer: padded input and output channels both multiples of 16."""
    return ceil4(c[1]) % 16 == 0 and ceil4(c[2]) % 16 == 0


def wgrad(c, a, dy, dtype):
    """dw [cout, cin, kh, kw] of the same_size conv: the full correlation of a (NHWC) with dy (NHWC), computed in `dtype`."""
    name, cin, cout, kh, kw = c[:5]
    wt = torch.zeros(cout, cin, kh, kw, dtype=dtype, requires_grad=True)
    return torch.autograd.grad(conv(c, a.to(dtype), wt), wt, dy.to(dtype))[0]


def dw_ref(c, d, relu_in, dtype=torch.float64, rounded=True, x=None, dy=None):
    x = d["x"] if x is None else x
    dy = d["dy"] if dy is None else dy
    a = torch.relu(x) if relu_in else x
    rnd = bf16 if rounded else (lambda t: t)
    return wgrad(c, rnd(a), rnd(dy), dtype)


def db_ref(c, d, dtype=torch.float64):
    return d["dy"].to(dtype).sum(dim=(0, 1, 2))


def tolerance(c, ref):
    """The project's weight-gradient rule, 1e-5 max|ref| (tests/test_gpu_geom_dispatch.py, set for up to 65,664 rows)."""
    assert rows(c) <= MAX_ROWS
    return 1e-5 * float(ref.abs().max())


def drop_one(c, d, relu_in, dtype=torch.float32):
    """Plain `dtype` dw of the rounded operands with ONE pixel's contribution to one (o, i, tap) removed: the tap that reads
    the output pixel itself (pad_top, pad_left), which lies inside the image for every pixel of every case; the pixel with
    the largest such product, so that the check does not depend on a lucky seed."""
    name, cin, cout, kh, kw, pt, pl = c[:7]
    a = bf16(torch.relu(d["x"]) if relu_in else d["x"])
    g = bf16(d["dy"])
    o, i = cout // 2, cin // 2
    prod = (g[..., o] * a[..., i]).to(dtype)
    bad = wgrad(c, a, g, dtype).clone()
    bad[o, i, pt, pl] -= prod.flatten()[prod.abs().argmax()]
    return bad
