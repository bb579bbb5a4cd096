"""Plain torch reference of the fused ResBlock family (csrc/vq2_resblock.hip, csrc/vq2_rbwino.hip; vqvae.py:81-96), usable
in float64 (the yardstick) and in float32 (what a plain evaluation costs), with the operands and the case table that
tests/test_resblock_ref_cpu.py and tests/test_gpu_resblock.py share.  TEST INFRASTRUCTURE, CPU only.

    forward     r = relu(conv3x3(relu(x)) + b1)             [N,H,W,32]
                y = [relu](conv1x1(r) + b2 + x)             [N,H,W,128]
    backward    dh = (r > 0) * (g . w2)                     [N,H,W,32]
                dx = (x > 0) * conv3x3^T(dh) + g            [N,H,W,128]
                dw2[co,cm] = sum over pixels g[co] * r[cm]  [128,32,1,1]
                db2 = sum over pixels g                     [128]

The backward takes r and x as INPUTS, as the kernel does: its masks are exact, whatever a forward would have rounded.

Two kinds of operands.  "normal": normal activations, weights scaled as in test_fused_resblock_forward_backward of
tests/test_gpu_edge.py.  "integer": activations and g in {-2..2}, weights in {-1,0,1}, small integer biases: every product and every
partial sum a kernel can form is an integer below 2^23 in magnitude (integer_bounds derives that from the operands, per
output, Winograd domain included), so float32 is exact in any summation order and the tolerance is 0.  The F(2,3)
output transform halves sums of two such integers that are even: exact too."""
import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import rng

C, CM = 128, 32
SEED = 53

# (N, H, W, label family of the forward under VQ2_FORMS=all).  The direct tile is 8 rows x 16 columns, the Winograd tile
# 4 rows x 64 columns; workgroup ids pass through xcd_remap, which deals them over 8 XCDs.
DIRECT, WINO = "resblock_fwd", "resblock_fwd_wino"
CASES = [
    (1, 1, 1, DIRECT),
    (1, 7, 15, DIRECT), (1, 8, 16, DIRECT), (1, 9, 17, DIRECT),     # one pixel below, at and above a tile, both directions
    (2, 8, 33, DIRECT),                                             # a one-column third tile
    (3, 17, 16, DIRECT),                                            # a one-row third tile and image seams, grid 9
    (11, 3, 5, DIRECT),                                             # images smaller than a tile, grid 11 (not a multiple of 8)
    (1, 16, 64, WINO),                                              # direct grid 8; the forward takes the Winograd kernel
    (1, 4, 64, WINO),                                               # grid 1
    (2, 8, 64, WINO),                                               # grid 4: a row seam and an image seam
    (1, 4, 128, WINO),                                              # a column seam between 64-pixel segments
    (3, 12, 64, WINO),                                              # grid 9
    (1, 4, 48, DIRECT), (1, 4, 80, DIRECT), (1, 5, 64, DIRECT), (1, 6, 64, DIRECT),      # near misses of the Winograd gate
]
BWD_CASES = CASES[:8]        # the backward has the direct kernel only: the direct shapes, (1, 16, 64) included
assert max(n * h * w for n, h, w, _ in CASES) == 2304


def case_id(c):
    return "%dx%dx%d" % tuple(c[:3])


def direct_grid(n, h, w):
    return n * ((h + 7) // 8) * ((w + 15) // 16)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _ints(stream, shape, lo, hi):
    """integers lo..hi (inclusive), uniformly, as float32"""
    u = rng.uniform01(SEED, stream, int(np.prod(shape)))
    return (np.floor(u * (hi - lo + 1)) + lo).astype(np.float32).reshape(shape)


def operands(tag, n, h, w, kind):
    """Seeded CPU float32 operands: x, g [N,H,W,128], r [N,H,W,32] (drawn on its own, relu of a draw: about half exact
    zeros -- the backward's saved activation), reference-layout w1 [32,128,3,3], b1 [32], w2 [128,32,1,1], b2 [128].
    Counter-based streams, one per image: image i depends on (tag, H, W, i) alone, not on N."""
    assert kind in ("normal", "integer")
    tag = "%s.%s.%dx%d" % (tag, kind, h, w)

    def act(name, ch):
        if kind == "normal":
            return torch.stack([_t(rng.normal(SEED, "%s.%s.%d" % (tag, name, i), (h, w, ch))) for i in range(n)])
        return torch.stack([_t(_ints("%s.%s.%d" % (tag, name, i), (h, w, ch), -2, 2)) for i in range(n)])

    d = {"x": act("x", C), "g": act("g", C), "r": torch.relu(act("r", CM))}
    if kind == "normal":
        d["w1"] = _t(rng.normal(SEED, tag + ".w1", (CM, C, 3, 3))) * 0.03
        d["b1"] = _t(rng.uniform(SEED, tag + ".b1", (CM,), -0.2, 0.2))
        d["w2"] = _t(rng.normal(SEED, tag + ".w2", (C, CM, 1, 1))) * 0.15
        d["b2"] = _t(rng.uniform(SEED, tag + ".b2", (C,), -0.2, 0.2))
    else:
        d["w1"] = _t(_ints(tag + ".w1", (CM, C, 3, 3), -1, 1))
        d["b1"] = _t(_ints(tag + ".b1", (CM,), -3, 3))
        d["w2"] = _t(_ints(tag + ".w2", (C, CM, 1, 1), -1, 1))
        d["b2"] = _t(_ints(tag + ".b2", (C,), -3, 3))
    return d


def _nchw(a, dtype):
    return a.to(dtype).permute(0, 3, 1, 2)


def _nhwc(a):
    return a.permute(0, 2, 3, 1).contiguous()


def fwd(x, w1, b1, w2, b2, relu_out, dtype=torch.float64):
    """-> r [N,H,W,32], y [N,H,W,128]"""
    xc = _nchw(x, dtype)
    r = Fn.relu(Fn.conv2d(Fn.relu(xc), w1.to(dtype), b1.to(dtype), padding=1))
    y = Fn.conv2d(r, w2.to(dtype), b2.to(dtype)) + xc
    if relu_out:
        y = Fn.relu(y)
    return _nhwc(r), _nhwc(y)


def bwd(g, r, x, w1, w2, dtype=torch.float64):
    """-> dh [N,H,W,32], dx [N,H,W,128], dw2 [128,32,1,1], db2 [128]; the masks are (r > 0) and (x > 0) of the arguments"""
    g, r = g.to(dtype), r.to(dtype)
    dh = torch.einsum("nhwo,om->nhwm", g, w2.to(dtype)[:, :, 0, 0]) * (r > 0).to(dtype)
    dx = _nhwc(Fn.conv_transpose2d(_nchw(dh, dtype), w1.to(dtype), padding=1)) * (x > 0).to(dtype) + g
    dw2 = torch.einsum("nhwo,nhwm->om", g, r)[:, :, None, None]
    db2 = g.sum((0, 1, 2))
    return dh, dx, dw2, db2


RULE = {"r": 5e-6, "y": 5e-6, "dh": 5e-6, "dx": 5e-6, "dw2": 1e-5, "db2": 1e-5}


def tolerances(ref, kind="normal"):
    """{name: atol} for a dict of float64 references: the project's rule (rtol 0; 5e-6 * max|ref| for activations,
    1e-5 * max|ref| for weight and bias gradients); 0 for "integer" operands."""
    return {k: (0.0 if kind == "integer" else RULE[k] * float(v.abs().max())) for k, v in ref.items()}


def differs(got, ref, tol):
    return bool(((got.double() - ref).abs() > tol).any())


def integer_bounds(d):
    """For "integer" operands: per output, the largest sum of |products| (|bias| and |skip| included) that any element
    accumulates, from the operands themselves -- float32 is exact in any order while it stays below 2^23 (one bit is
    left for the sums of two that the Winograd output transform halves).  Inputs of a second stage (r for y, dh for dx)
    are the exact first-stage values, which the first-stage bound makes representable."""
    f8 = torch.float64
    x, g, r = d["x"].to(f8), d["g"].to(f8), d["r"].to(f8)
    w1, b1, w2, b2 = (d[k].to(f8) for k in ("w1", "b1", "w2", "b2"))
    ax = _nchw(Fn.relu(x), f8)
    out = {}
    out["r"] = float((Fn.conv2d(ax, w1.abs(), b1.abs(), padding=1)).max())
    # F(2,3) along the rows: a transformed tap is at most |g0| + |g1| + |g2| of its kernel row, a transformed input at
    # most the sum of the four columns of its window; every Winograd-domain sum is below this (3 x 4)-window sum
    rowsum = w1.abs().sum(3, keepdim=True).expand(-1, -1, -1, 4).contiguous()
    out["r_wino"] = float((Fn.conv2d(Fn.pad(ax, (2, 2, 1, 1)), rowsum) + b1.abs()[None, :, None, None]).max())
    r_f, _ = fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], False)
    out["y"] = float((torch.einsum("nhwm,om->nhwo", r_f.abs(), w2.abs()[:, :, 0, 0]) + b2.abs() + x.abs()).max())
    out["dh"] = float(torch.einsum("nhwo,om->nhwm", g.abs(), w2.abs()[:, :, 0, 0]).max())
    dh = bwd(d["g"], d["r"], d["x"], d["w1"], d["w2"])[0]
    out["dx"] = float((_nhwc(Fn.conv_transpose2d(_nchw(dh.abs(), f8), w1.abs(), padding=1)) + g.abs()).max())
    out["dw2"] = float(torch.einsum("nhwo,nhwm->om", g.abs(), r.abs()).max())
    out["db2"] = float(g.abs().sum((0, 1, 2)).max())
    return out
