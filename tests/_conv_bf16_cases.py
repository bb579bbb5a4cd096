"""Cases, inputs and fp64 references of the bf16-operand conv tests (tests/test_gpu_conv_bf16.py runs them on the GPU,
tests/test_conv_bf16_cpu.py checks on the CPU that their tolerance bites).  No GPU and no library needed here.

The contract (include/vq2.h, VQ2_ALLOW_BF16): y = sum_k bf16(a_k) * bf16(w_k) accumulated in fp32, then the fp32 epilogue.
The reference is therefore the fp64 conv of the bf16-ROUNDED operands: against it only the accumulation differs, and the
project's fp32 tolerance applies unchanged; against the fp64 conv of the unrounded operands the result must MISS it.

A case is (name, cin, cout, kh, kw, pad_top, pad_left, n, h, w).  The forward runs it as written.  The data gradient's
depth is the OUTPUT channel count, so it runs the case with cin and cout exchanged (`swapped`): the same ragged rows,
columns and depths; as written, the data gradients of (a), (b) and (d) are not eligible and must stay on the fp32 kernel."""
import torch
import torch.nn.functional as Fn

CASES = [
    ("a", 16, 36, 5, 5, 4, 2, 2, 5, 7),     # 5x5 causal: M = 70, ragged rows and columns
    ("b", 48, 68, 3, 2, 2, 1, 3, 4, 9),     # 3x2 downright: depth 288, Co just past a 64 tile
    ("c", 32, 32, 1, 1, 0, 0, 1, 8, 16),    # 1x1: every tile full (M = 128, 128 x 64 tile)
    ("d", 16, 4, 7, 4, 6, 3, 2, 3, 3),      # 28 taps, kernel larger than the image
    ("m129", 16, 68, 1, 1, 0, 0, 1, 3, 43),  # M = 129 = tile + 1 rows; Co > 64 takes the 128 x 128 tile
]
BY_NAME = {c[0]: c for c in CASES}
DEEP_Y = 16 * 256          # reduction depth the project's y / dx tolerance was set for (tests/test_gpu_geom_dispatch.py)


def swapped(c):
    name, cin, cout = c[:3]
    return (name,) + (cout, cin) + tuple(c[3:])


def ceil4(v):
    return (v + 3) // 4 * 4


def bf16(t):
    """Round to nearest even to bfloat16, kept in the input's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def make_inputs(c, seed=0):
    """fp32 NHWC x, dy, residuals and mask, OIHW weight, bias."""
    name, cin, cout, kh, kw, pt, pl, n, h, w = c
    g = torch.Generator().manual_seed(1000 * seed + 17 * cin + cout + 3 * kh + kw)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"x": r(n, h, w, cin), "dy": r(n, h, w, cout), "w": r(cout, cin, kh, kw) / (cin * kh * kw) ** 0.5, "b": r(cout),
            "res_y": r(n, h, w, cout), "res_x": r(n, h, w, cin), "mask": r(n, h, w, cin)}


def conv(c, x, wt, b=None):
    """The same_size conv of vq2_conv_desc on NHWC x, in x's dtype."""
    name, cin, cout, kh, kw, pt, pl, n, h, w = c
    xp = Fn.pad(x.permute(0, 3, 1, 2), (pl, kw - 1 - pl, pt, kh - 1 - pt))
    return Fn.conv2d(xp, wt, b).permute(0, 2, 3, 1).contiguous()


def dgrad(c, dy, wt):
    """dx = sum over taps and co of dy * w (the transpose of conv), in dy's dtype."""
    name, cin, cout, kh, kw, pt, pl, n, h, w = c
    x = torch.zeros(n, h, w, cin, dtype=dy.dtype, requires_grad=True)
    return torch.autograd.grad(conv(c, x, wt), x, dy)[0]


def fwd_ref(c, d, dtype=torch.float64, rounded=True, bias=False, residual=False, w=None):
    rnd = bf16 if rounded else (lambda t: t)
    wt = d["w"] if w is None else w
    y = conv(c, rnd(d["x"]).to(dtype), rnd(wt).to(dtype), d["b"].to(dtype) if bias else None)
    return y + d["res_y"].to(dtype) if residual else y


def dgrad_ref(c, d, dtype=torch.float64, rounded=True, mask=False, residual=False, mask_after=False, w=None):
    rnd = bf16 if rounded else (lambda t: t)
    wt = d["w"] if w is None else w
    dx = dgrad(c, rnd(d["dy"]).to(dtype), rnd(wt).to(dtype))
    keep = (d["mask"] > 0).to(dtype)
    if mask and not mask_after:
        dx = dx * keep
    if residual:
        dx = dx + d["res_x"].to(dtype)
    if mask and mask_after:
        dx = dx * keep
    return dx


def tolerance(c, op, ref, ref32=None):
    """The project's rule (tests/test_gpu_geom_dispatch.py tolerance / deep_tolerance): 5e-6 max|ref|, and past the depth
    that was set for, max(that, 4 x the error of plain fp32 torch on the CPU on the same rounded operands)."""
    name, cin, cout, kh, kw = c[:5]
    depth = kh * kw * (ceil4(cin) if op == "fwd" else ceil4(cout))
    tol = 5e-6 * float(ref.abs().max())
    if depth > DEEP_Y:
        tol = max(tol, 4 * float((ref32.double() - ref).abs().max()))
    return tol


def drop_one(c, wt):
    """The weight with one tap of one (co, ci) pair zeroed: the tap that reads the output pixel itself (pad_top, pad_left),
    which lies inside the image for every pixel of every case (the centre tap of case (d) never does)."""
    bad = wt.clone()
    bad[wt.shape[0] // 2, wt.shape[1] // 2, c[5], c[6]] = 0
    return bad
