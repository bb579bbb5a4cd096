"""The same_size form of vq2_conv_desc (rectangular kernels with top / left padding, output the size of the input) on
every kernel the stage-2 prior trains with, against fp64 at the shape boundaries of plan_conv (csrc/vq2_conv.hip),
plan_wgrad with its kernel-family test (csrc/vq2_wgrad.hip).  tests/test_gpu_dispatch.py is that table for the other form; this
module is its counterpart and shares its helpers (counter-based inputs, launched / short_label / conv_labels, sliced /
guarded / untouched, the label syntax "<family>|<variant>") unchanged.  The geometries (KH, KW, pad_top, pad_left) are
KERNELS of tests/test_gpu_gated_resblock.py, whose own fp64 test stops at 144 rows and 8-pixel rows: every label here is
one that test cannot reach.

Every operand is a channel slice at offset 4 of a buffer 8 channels wider; outputs land in such a slice of a sentinel-filled
buffer with 64 guard pixels on both ends; guards and neighbouring channels must be untouched and the zero pad lanes
(channels cout .. ceil4(cout) of y, cin .. ceil4(cin) of dx) must be 0.  The reference is tests/_pixelsnail_ref.conv_at in
fp64 (autograd for the gradients) on the values the GPU sees.

What each section of GEOM_CASES straddles (8x16 images: wgs128 = N * ceil(Co / 128)):
    causal 5x5 (5,5,4,2), 25 taps    wgs128 399 | 400: `half`, 64x128x32 | 128x128x32, forward (pads 4, 2) and data gradient
                                     (pads 0, 2: the window hangs below and to the right)
    (3,2,2,1), 6 taps                wgs128 512 | 513 and 1024 | 1025: 128x128x32 | the four-per-CU 128x128x16 | 128x128x32,
                                     forward and data gradient, one data-gradient row with VQ2_MASK_AFTER_RESIDUAL
    the other 128-row tiles          Co 64 (128x64x16), Co 32 (128x32x32, 28 taps, pad_top 6, both directions);
                                     Ci % BK: 48 on BK 32 -> var, 48 on BK 16 -> uni (occ4), Ci = 32 -> uni (not tap: Ci > 32 fails)
    workload channel counts, 1x1     516 stored input channels (Ci % 16 != 0: 128x128x32 var), 516 stored output channels
                                     (last column tile: 4 stored, 2 real), the data gradient of 514 -> 256 (the same tile,
                                     mask and residual on 516 channels), 260 stored with 258 real
    weight gradient, W % 32 == 0     wgrad_fast_kernel on all six tiles of plan_wgrad with KH != KW, pad_top up to 6 (negative
                                     xbase; pad_top > H at 2x3x32), pad_left != pad_top, images shorter than the kernel, two
                                     chunks per row (W = 64), ragged O and K (36 -> 132), 516 stored channels, the M >= 65536 rule
                                     of the 128x96 tile (N 171 | 170 on 4x96), a ragged last split (M % rows-per-split != 0);
                                     W = 40: wgrad_kernel (gen)
    exchanged roles                  (3,3,1,1) 128 -> 32 takes them (sw); (3,3,2,1) (pad_h != pad_w) and (3,2,2,1) (KH != KW) do not

(tile, instantiation, geometry) products without a case, and why:
  - every product is not enumerated: each 128-row tile has a rectangular, asymmetrically padded case in each direction it
    trains in, and tap / uni / var each have one on a BK = 32 and (tap, uni) on a BK = 16 tile; 128x64x16 and 128x32x32 run
    `tap` only here (their uni / var instantiations differ from the cases of tests/test_gpu_dispatch.py in the tap decomposition alone,
    which `tap` exercises with more taps);
  - 64x192x16 and 64x128x16 (K <= 64) need KH * KW * Ci <= 64 with Co > 128: no stage-2 layer has that shape;
  - the 64-row tiles other than 64x128x32 with these geometries are what tests/test_gpu_gated_resblock.py runs (M <= 144);
  - conv1x1_k64, the Winograd, sub-pixel, k4s2 and conv-transpose families take square centred kernels only: the same_size
    form reaches the first three as (3,3,1,1) / (1,1,0,0), checked bit for bit against the other form in
    test_old_and_new_descriptor_agree_bitwise_on_the_winograd_shapes;
  - the non-uniform instantiation of 128x128x16 cannot exist (see tests/test_gpu_dispatch.py);
  - tensors of 1 GiB and more: the kernels are shared with the other form, test_tensors_of_one_gib_and_more covers them.

Tolerances are the project's: rtol 0, atol 5e-6 * max|ref| for y and dx, 1e-5 * max|ref| for dw and db.  A case deeper than
they were set for (y / dx depth above 4096, dw of more than 65,664 rows) would use max(project tolerance, 4 x the error of
plain fp32 torch on the CPU against fp64), measured and printed on every run.  No row of GEOM_CASES is that deep:

    case                                   depth    fp32-vs-fp64 max err / max|ref|   tolerance used / max|ref|
    (none: the deepest y / dx row is 7x4 x 64 = 1792, the longest dw row count is 65,664)

That the tolerance bites (_bites: one tap of one (co, ci) pair of the weights dropped, for weight gradients one pixel of one
channel of dy; plain fp32 on the CPU then misses the tolerance, intact fp32 meets it) was run on the CPU for EVERY row of
GEOM_CASES when the table was written: it held for every row, none needed the deep-tolerance rule.
tests/test_host_cpu.py runs it for the cheapest case of every label.

Batch invariance (GEOM_SWITCH_PAIRS): image 0 is bitwise the same on both sides of 399 | 400 (5x5) and of 512 | 513 and
1024 | 1025 ((3,2,2,1)), forward and data gradient.

Peak device memory of the table is 0.30 GiB (the census test asserts that it stays below 1 GiB)."""
import os
import subprocess
import sys
import time

import pytest
import torch
import torch.nn.functional as Fn

import _pixelsnail_ref as R
from oracle import rng
from test_gpu_dispatch import (COL, DEEP_Y, FORMS, _t, ceil4, conv_labels, differs, guarded, launched, sliced, untouched)

C5, K32, K25, K74, K13, K11 = (5, 5, 4, 2), (3, 2, 2, 1), (2, 5, 1, 2), (7, 4, 6, 3), (1, 3, 0, 1), (1, 1, 0, 0)
DEEP_DW = 65664            # rows the project's dw / db tolerance was set for

GEOM_CASES = [
    # op, cin, cout, (KH, KW, pad_top, pad_left), N, H, W, flags, label under VQ2_FORMS = all, direct, general
    # flags -- fwd: i ReLU-in, b bias, r residual, o ReLU-out; dgrad: m mask, r residual, a VQ2_MASK_AFTER_RESIDUAL;
    #          wgrad: i ReLU-in, b bias (every wgrad case also runs without ReLU-in)
    # ---- the causal 5x5 across wgs128 399 | 400
    ('fwd', 64, 128, C5, 399, 8, 16, 'ibr',       'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('fwd', 64, 128, C5, 400, 8, 16, 'ibr',       'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', 128, 64, C5, 399, 8, 16, 'mr',      'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', 128, 64, C5, 400, 8, 16, 'mr',      'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    # ---- (3,2,2,1) across 512 | 513 and 1024 | 1025: the four-per-CU tile of the top prior
    ('fwd', 64, 128, K32, 512, 8, 16, 'ibr',      'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('fwd', 64, 128, K32, 513, 8, 16, 'ibr',      'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x32>|gen'),
    ('fwd', 64, 128, K32, 1024, 8, 16, 'ibr',     'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x32>|gen'),
    ('fwd', 64, 128, K32, 1025, 8, 16, 'ibr',     'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', 128, 64, K32, 512, 8, 16, 'mr',     'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', 128, 64, K32, 513, 8, 16, 'mr',     'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', 128, 64, K32, 1024, 8, 16, 'mr',    'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', 128, 64, K32, 1024, 8, 16, 'mra',   'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', 128, 64, K32, 1025, 8, 16, 'mr',    'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    # ---- the other 128-row tiles; Ci % BK
    ('fwd', 64, 64, K25, 400, 8, 16, 'ibr',       'conv_gemm<128x64x16>|tap', 'conv_gemm<128x64x16>|tap', 'conv_gemm<128x64x16>|gen'),
    ('fwd', 64, 32, K74, 400, 8, 16, '',          'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x16>|gen'),
    ('dgrad', 32, 64, K74, 400, 8, 16, 'mra',     'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x16>|gen'),
    ('fwd', 48, 128, C5, 400, 8, 16, 'ibr',       'conv_gemm<128x128x32>|var', 'conv_gemm<128x128x32>|var', 'conv_gemm<128x128x32>|gen'),
    ('fwd', 48, 128, K32, 600, 8, 16, '',         'conv_gemm<128x128x16>|uni', 'conv_gemm<128x128x16>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', 32, 128, K13, 400, 8, 16, '',         'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|gen'),
    # ---- the workload's channel counts as 1x1 geometry convs: 514 real in 516 stored, 258 real in 260 stored
    ('fwd', 514, 256, K11, 200, 8, 16, 'ibr',     'conv_gemm<128x128x32>|var', 'conv_gemm<128x128x32>|var', 'conv_gemm<128x128x32>|gen'),
    ('fwd', 256, 514, K11, 80, 8, 16, 'ibr',      'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', 514, 256, K11, 80, 8, 16, 'mr',     'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', 258, 256, K11, 200, 8, 16, '',        'conv_gemm<128x128x32>|var', 'conv_gemm<128x128x32>|var', 'conv_gemm<128x128x32>|gen'),
    # ---- weight gradients: wgrad_fast_kernel (W % 32 == 0) on the six tiles, then wgrad_kernel (W = 40)
    ('wgrad', 128, 128, C5, 4, 3, 32, 'ib',       'wgrad<128x128>|fast', 'wgrad<128x128>|fast', 'wgrad<128x128>|gen'),   # M=384 S=2 rows/split=192; H < KH
    ('wgrad', 64, 128, K25, 4, 3, 32, 'ib',       'wgrad<128x128>|fast', 'wgrad<128x128>|fast', 'wgrad<128x128>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', 64, 128, K25, 5, 3, 32, 'ib',       'wgrad<128x128>|fast', 'wgrad<128x128>|fast', 'wgrad<128x128>|gen'),   # M=480 S=2 rows/split=256 ragged
    ('wgrad', 64, 36, K32, 2, 3, 64, 'ib',        'wgrad<64x128>|fast', 'wgrad<64x128>|fast', 'wgrad<64x128>|gen'),   # M=384 S=2 rows/split=192; two chunks per row
    ('wgrad', 16, 40, K74, 2, 8, 32, 'ib',        'wgrad<64x64>|fast', 'wgrad<64x64>|fast', 'wgrad<64x64>|gen'),   # M=512 S=2 rows/split=256
    ('wgrad', 16, 40, K74, 2, 3, 32, 'ib',        'wgrad<64x64>|fast', 'wgrad<64x64>|fast', 'wgrad<64x64>|gen'),   # M=192 S=1 rows/split=192; pad_top 6 > H
    ('wgrad', 256, 32, K13, 4, 3, 32, 'ib',       'wgrad<32x256>|fast', 'wgrad<32x256>|fast', 'wgrad<32x256>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', 36, 132, C5, 4, 3, 32, 'ib',        'wgrad<32x256>|fast', 'wgrad<32x256>|fast', 'wgrad<32x256>|gen'),   # M=384 S=2 rows/split=192; O, K ragged
    ('wgrad', 514, 256, K11, 4, 3, 32, 'ib',      'wgrad<128x32>|fast', 'wgrad<128x32>|fast', 'wgrad<128x32>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', 32, 128, K13, 171, 4, 96, 'ib',     'wgrad<128x96>|fast', 'wgrad<128x96>|fast', 'wgrad<128x96>|gen'),   # M=65664 S=257 rows/split=256 ragged
    ('wgrad', 32, 128, K13, 170, 4, 96, 'ib',     'wgrad<128x32>|fast', 'wgrad<128x32>|fast', 'wgrad<128x32>|gen'),   # M=65280 S=255 rows/split=256
    ('wgrad', 128, 128, C5, 4, 3, 40, 'ib',       'wgrad<128x128>|gen', 'wgrad<128x128>|gen', 'wgrad<128x128>|gen'),   # M=480 S=2 rows/split=256 ragged
    ('wgrad', 64, 36, K32, 3, 5, 40, 'ib',        'wgrad<64x128>|gen', 'wgrad<64x128>|gen', 'wgrad<64x128>|gen'),   # M=600 S=3 rows/split=224 ragged
    # ---- the gate of the exchanged-roles form: pad_h == pad_w && 2 * pad_h == KH - 1 && KH == KW
    ('wgrad', 128, 32, (3, 3, 1, 1), 4, 3, 32, 'ib', 'wgrad<128x32>sw|fast', 'wgrad<128x32>sw|fast', 'wgrad<32x256>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', 128, 32, (3, 3, 2, 1), 4, 3, 32, 'ib', 'wgrad<32x256>|fast', 'wgrad<32x256>|fast', 'wgrad<32x256>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', 128, 32, K32, 4, 3, 32, 'ib',       'wgrad<32x256>|fast', 'wgrad<32x256>|fast', 'wgrad<32x256>|gen'),   # M=384 S=2 rows/split=192
]

EXPECTED_GEOM_LABELS = {
    "all": {
        'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|uni', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|uni',
        'conv_gemm<128x128x32>|var', 'conv_gemm<128x32x32>|tap', 'conv_gemm<128x64x16>|tap', 'conv_gemm<64x128x32>|tap',
        'wgrad<128x128>|fast', 'wgrad<128x128>|gen', 'wgrad<128x32>sw|fast', 'wgrad<128x32>|fast', 'wgrad<128x96>|fast',
        'wgrad<32x256>|fast', 'wgrad<64x128>|fast', 'wgrad<64x128>|gen', 'wgrad<64x64>|fast'
    },
    "direct": {
        'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|uni', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|uni',
        'conv_gemm<128x128x32>|var', 'conv_gemm<128x32x32>|tap', 'conv_gemm<128x64x16>|tap', 'conv_gemm<64x128x32>|tap',
        'wgrad<128x128>|fast', 'wgrad<128x128>|gen', 'wgrad<128x32>sw|fast', 'wgrad<128x32>|fast', 'wgrad<128x96>|fast',
        'wgrad<32x256>|fast', 'wgrad<64x128>|fast', 'wgrad<64x128>|gen', 'wgrad<64x64>|fast'
    },
    "general": {
        'conv_gemm<128x128x32>|gen', 'conv_gemm<128x32x16>|gen', 'conv_gemm<128x64x16>|gen', 'conv_gemm<64x128x16>|gen',
        'wgrad<128x128>|gen', 'wgrad<128x32>|gen', 'wgrad<128x96>|gen', 'wgrad<32x256>|gen', 'wgrad<64x128>|gen', 'wgrad<64x64>|gen'
    },
}


def case_id(c):
    op, cin, cout, (kh, kw, pt, pl), n, h, w, fl = c[:8]
    return "%s-%d-%dk%dx%dp%d_%d-%dx%dx%d-%s" % (op, cin, cout, kh, kw, pt, pl, n, h, w, fl or "none")


def expected(c):
    return c[8 + COL]


def cost(c):
    """multiply-adds of the fp64 reference of a case (orders the table for the CPU bites test)"""
    op, cin, cout, (kh, kw, pt, pl), n, h, w, fl = c[:8]
    return n * h * w * kh * kw * cin * cout


def make_inputs(c):
    """Seeded operands of a case as CPU fp32 tensors (NHWC activations padded to 4 channels with zeros -- residuals too: the
    pad lanes of every activation of the pipeline are 0 --, reference-layout weights).  Image n of every activation depends
    on (case shape without N, n) alone: counter-based streams."""
    op, cin, cout, (kh, kw, pt, pl), n, h, w, fl = c[:8]
    ci, co = ceil4(cin), ceil4(cout)
    tag = "G%d.%d.%dx%d.%d.%d.%dx%d" % (cin, cout, kh, kw, pt, pl, h, w)
    d = {}
    for name, ch, real in (("x", ci, cin), ("dy", co, cout), ("res_y", co, cout), ("res_x", ci, cin)):
        a = _t(rng.normal(43, tag + "." + name, (n, h, w, ch)))
        a[..., real:] = 0
        d[name] = a
    d["w"] = _t(rng.uniform(43, tag + ".w", (cout, cin, kh, kw), -0.1, 0.1))
    d["b"] = _t(rng.uniform(43, tag + ".b", (cout,), -1, 1))
    return d


def reference(c, d, dtype=torch.float64, relu_in=None):
    """The op of a case through _pixelsnail_ref.conv_at on the CPU (autograd for the gradients).  Returns NHWC /
    reference-layout tensors restricted to the real channels: y | dx | (dw, db)."""
    op, cin, cout, (kh, kw, pt, pl), n, h, w, fl = c[:8]
    x = d["x"][..., :cin].permute(0, 3, 1, 2).to(dtype)
    wt, b = d["w"].to(dtype), d["b"].to(dtype)
    if op == "fwd":
        y = R.conv_at(Fn.relu(x) if "i" in fl else x, wt, b if "b" in fl else None, pt, pl)
        if "r" in fl:
            y = y + d["res_y"][..., :cout].permute(0, 3, 1, 2).to(dtype)
        if "o" in fl:
            y = Fn.relu(y)
        return y.permute(0, 2, 3, 1)
    dy = d["dy"][..., :cout].permute(0, 3, 1, 2).to(dtype)
    if op == "dgrad":
        a = x.clone().requires_grad_(True)
        R.conv_at(a, wt, None, pt, pl).backward(dy)
        g = a.grad
        keep = (x > 0).to(dtype)
        res = d["res_x"][..., :cin].permute(0, 3, 1, 2).to(dtype)
        if "m" in fl and "a" not in fl:
            g = g * keep
        if "r" in fl:
            g = g + res
        if "m" in fl and "a" in fl:
            g = g * keep
        return g.permute(0, 2, 3, 1)
    wr, br = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    R.conv_at(Fn.relu(x) if relu_in else x, wr, br, pt, pl).backward(dy)
    return wr.grad, br.grad


def tolerance(c, ref, what):
    """The project's tolerance; None when the case is deeper than that tolerance was set for (the caller then measures
    plain fp32 against fp64, see the module docstring)."""
    op, cin, cout, (kh, kw, pt, pl), n, h, w, fl = c[:8]
    scale = float(ref.abs().max())
    if what in ("dw", "db"):
        return 1e-5 * scale if n * h * w <= DEEP_DW else None
    depth = kh * kw * (ceil4(cin) if op == "fwd" else ceil4(cout))
    return 5e-6 * scale if depth <= DEEP_Y else None


def deep_tolerance(c, ref, ref32, what):
    """max(project tolerance, 4 x the error of plain fp32 torch on the CPU) for a case past the project's depth."""
    err32 = float((ref32.double() - ref).abs().max())
    scale = float(ref.abs().max())
    tol = max((1e-5 if what in ("dw", "db") else 5e-6) * scale, 4 * err32)
    print("deep case %s %s: fp32-vs-fp64 max err %.3e (%.3e of max|ref|), tolerance %.3e (%.3e of max|ref|)"
          % (case_id(c), what, err32, err32 / scale, tol, tol / scale))
    return tol


def _bites(c):
    """CPU check that the tolerance of a case would catch a kernel that drops ONE product: plain fp32 torch with one tap of
    one (co, ci) pair of the weights zeroed (wgrad: one pixel of one channel of dy) must fail the comparison, and intact
    fp32 must pass it (test_gpu_dispatch._bites for the same_size form)."""
    op, cin, cout, (kh, kw, pt, pl), n, h, w, fl = c[:8]
    d = make_inputs(c)
    bad = dict(d)
    if op == "wgrad":
        bad["dy"] = d["dy"].clone()
        bad["dy"][n - 1, h // 2, w // 2, cout // 2] = 0
        ref = reference(c, d, relu_in=True)[0]
        got = reference(c, bad, torch.float32, relu_in=True)[0]
        good = reference(c, d, torch.float32, relu_in=True)[0]
        what = "dw"
    else:
        bad["w"] = d["w"].clone()
        bad["w"][cout // 2, cin // 2, kh // 2, kw // 2] = 0
        ref = reference(c, d)
        got, good = reference(c, bad, torch.float32), reference(c, d, torch.float32)
        what = "y"
    tol = tolerance(c, ref, what)
    if tol is None:
        tol = deep_tolerance(c, ref, good, what)
    assert not differs(good, ref, tol), case_id(c) + ": plain fp32 itself misses the tolerance"
    assert differs(got, ref, tol), case_id(c) + ": the tolerance does not notice a dropped product"


# ----------------------------------------------------------------------------------------------------------------- GPU side
@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _check(c, name, got, ref, ref32_of, labels):
    tol = tolerance(c, ref, name)
    if tol is None:
        tol = deep_tolerance(c, ref, ref32_of(), name)
    err = float((got.cpu().double() - ref).abs().max())
    print("%s %s: %s  max err %.3e  tolerance %.3e  share %.3f" % (case_id(c), name, labels, err, tol, err / tol if tol else 0.0))
    assert tuple(got.shape) == tuple(ref.shape) and err <= tol, "%s.%s: err %.3e > tolerance %.3e" % (case_id(c), name, err, tol)


_RESULTS = {}


def run_case(amd, c):
    """Run one table case on the GPU against fp64 (cached: the census and the invariance tests reuse it).  Returns
    (labels seen, rows of image 0 as a CPU tensor)."""
    key = case_id(c)
    if key in _RESULTS:
        return _RESULTS[key]
    from vqvae2_amd import ops
    dev = torch.device("cuda:0")
    if not _RESULTS:       # the peak the census asserts is this table's own, whatever ran in the process before
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    op, cin, cout, (kh, kw, pt, pl), n, h, w, fl = c[:8]
    ci, co = ceil4(cin), ceil4(cout)
    d = make_inputs(c)
    spec = ops.ConvSpec.geom(cin, cout, kh, kw, pt, pl)
    wt, b = d["w"].to(dev), d["b"].to(dev)
    _, x = sliced(d["x"], dev)
    first = None
    if op == "fwd":
        flat, wide, out = guarded((n, h, w, co), dev)
        flags = (ops.VQ2_RELU_IN if "i" in fl else 0) | (ops.VQ2_RELU_OUT if "o" in fl else 0)
        res = sliced(d["res_y"], dev)[1] if "r" in fl else None
        y, seen = launched(amd, lambda: ops.conv_forward(spec, x, wt, b if "b" in fl else None, flags, residual=res, out=out))
        untouched(flat, wide, co, key)
        assert float(y[..., cout:].abs().sum()) == 0, key + ": pad lanes of y"
        _check(c, "y", y[..., :cout], reference(c, d), lambda: reference(c, d, torch.float32), conv_labels(seen))
        first = y[0].cpu()
    elif op == "dgrad":
        _, dy = sliced(d["dy"], dev)
        _, res = sliced(d["res_x"], dev)
        flat, wide, out = guarded((n, h, w, ci), dev)
        dx, seen = launched(amd, lambda: ops.conv_dgrad(spec, (n, h, w, ci), dy, wt, mask=x if "m" in fl else None,
                                                        residual=res if "r" in fl else None, out=out, mask_after="a" in fl))
        untouched(flat, wide, ci, key)
        assert float(dx[..., cin:].abs().sum()) == 0, key + ": pad lanes of dx"
        _check(c, "dx", dx[..., :cin], reference(c, d), lambda: reference(c, d, torch.float32), conv_labels(seen))
        first = dx[0].cpu()
    else:
        _, dy = sliced(d["dy"], dev)
        seen = []
        for relu_in in (True, False):
            (dw, db), sn = launched(amd, lambda: ops.conv_wgrad(spec, x, dy, relu_in, wt, b))
            seen += sn
            rw, rb = reference(c, d, relu_in=relu_in)
            r32 = lambda: reference(c, d, torch.float32, relu_in=relu_in)
            _check(c, "dw relu_in=%d" % relu_in, dw, rw, lambda: r32()[0], conv_labels(sn))
            _check(c, "db relu_in=%d" % relu_in, db, rb, lambda: r32()[1], conv_labels(sn))
    _RESULTS[key] = (conv_labels(seen), first)
    return _RESULTS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("c", GEOM_CASES, ids=case_id)
def test_geom_case_runs_its_kernel_and_matches_fp64(amd, c):
    labels, _ = run_case(amd, c)
    assert labels and set(labels) == {expected(c)}, (case_id(c), labels, expected(c))


def _pairs(op, cin, cout, g, fl, sides):
    by = {(c[0], c[1], c[2], c[3], c[7], c[4]): c for c in GEOM_CASES}
    return [(by[(op, cin, cout, g, fl, a)], by[(op, cin, cout, g, fl, b)]) for a, b in sides]


GEOM_SWITCH_PAIRS = (
    _pairs("fwd", 64, 128, C5, "ibr", ((399, 400),)) + _pairs("dgrad", 128, 64, C5, "mr", ((399, 400),)) +
    _pairs("fwd", 64, 128, K32, "ibr", ((512, 513), (1024, 1025))) + _pairs("dgrad", 128, 64, K32, "mr", ((512, 513), (1024, 1025)))
)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", GEOM_SWITCH_PAIRS, ids=lambda pr: case_id(pr[0]) + "~" + str(pr[1][4]))
def test_geom_image_zero_is_bitwise_the_same_on_both_sides_of_a_launch_size_switch(amd, pair):
    a, b = pair
    (la, ya), (lb, yb) = run_case(amd, a), run_case(amd, b)      # each is compared with fp64 inside run_case
    if FORMS == "all":
        assert set(la) != set(lb), (la, lb)                      # the pair does sit on two sides of a switch
    same = torch.equal(ya, yb)
    diff = float((ya.double() - yb.double()).abs().max())
    print("%s ~ N=%d: %s vs %s bitwise=%s max diff %.3e" % (case_id(a), b[4], sorted(set(la)), sorted(set(lb)), same, diff))
    assert same, "image 0 differs between batch %d and batch %d: max diff %.3e" % (a[4], b[4], diff)


@pytest.mark.gpu
def test_geom_census_of_labels_over_the_whole_table(amd):
    """The union of labels over the table, tile and instantiation included, is EXPECTED_GEOM_LABELS -- no more, no less."""
    seen = set()
    for c in GEOM_CASES:
        seen |= set(run_case(amd, c)[0])
    want = EXPECTED_GEOM_LABELS[FORMS]
    assert seen == want, (sorted(seen - want), sorted(want - seen))
    print("peak device memory: %.3f GiB" % (torch.cuda.max_memory_allocated() / 2**30))
    assert torch.cuda.max_memory_allocated() < (1 << 30)


# --------------------------------------------------------------------------------------- the two forms of one layer, bitwise
# cin, cout, N, H, W, labels that must be among those seen under VQ2_FORMS=all (forward, data gradient, weight gradient):
# conv_wino3 at both row widths, narrow and wide (`wide`: Co % 128 == 0 and N * H * W / 128 * (Co / 128) >= 400); Winograd
# weight-gradient mode 1 (O % 128 == 0, I % 128 == 0; W % 64 == 0, or W == 32 with H even) and mode 3 (exchanged roles, I == 32)
WINO_SHAPES = [
    (128, 128, 400, 2, 64, {'conv_wino3<2x64,nt2>|', 'wgrad<128x128>wino|fast'}),
    (128, 128, 3, 2, 64, {'conv_wino3<2x64,nt1>|', 'wgrad<128x128>wino|fast'}),
    (128, 128, 400, 4, 32, {'conv_wino3<4x32,nt2>|', 'wgrad<128x128>wino|fast'}),
    (128, 128, 2, 4, 32, {'conv_wino3<4x32,nt1>|', 'wgrad<128x128>wino|fast'}),
    (128, 32, 3, 2, 64, {'conv_gemm<128x32x32>|tap', 'conv_wino3<2x64,nt1>|', 'wgrad<128x96>swwino|fast'}),
    (128, 32, 2, 4, 32, {'conv_gemm<128x32x32>|tap', 'conv_wino3<4x32,nt1>|', 'wgrad<128x96>swwino|fast'}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,n,h,w,want", WINO_SHAPES, ids=["%d-%d-%dx%dx%d" % s[:5] for s in WINO_SHAPES])
def test_old_and_new_descriptor_agree_bitwise_on_the_winograd_shapes(amd, cin, cout, n, h, w, want):
    """ConvSpec(False, cin, cout, 3, 1, 1) and ConvSpec.geom(cin, cout, 3, 3, 1, 1), one layer in the two forms of
    vq2_conv_desc, give the same bits for y, dx, dw and db on the shapes that reach conv_wino3 and the Winograd
    weight-gradient modes: same_size alone changes no plan (tests/test_gpu_gated_resblock.py has the same test up to 64
    channels, which reaches neither)."""
    from vqvae2_amd import ops
    dev = torch.device("cuda:0")
    old, new = ops.ConvSpec(False, cin, cout, 3, 1, 1), ops.ConvSpec.geom(cin, cout, 3, 3, 1, 1)
    tag = "W%d.%d.%dx%d" % (cin, cout, h, w)
    x = _t(rng.normal(47, tag + ".x", (n, h, w, cin))).to(dev)
    dy = _t(rng.normal(47, tag + ".dy", (n, h, w, cout))).to(dev)
    wt = _t(rng.uniform(47, tag + ".w", (cout, cin, 3, 3), -0.1, 0.1)).to(dev)
    bias = _t(rng.uniform(47, tag + ".b", (cout,), -1, 1)).to(dev)
    outs, labels = [], []
    for spec in (old, new):
        w2 = wt.clone()      # (the packed panels are cached on the weight tensor, per spec)

        def run():
            y = ops.conv_forward(spec, x, w2, bias, ops.VQ2_RELU_IN)
            dx = ops.conv_dgrad(spec, x.shape, dy, w2, mask=x)
            dw, db = ops.conv_wgrad(spec, x, dy, True, w2, bias)
            return y, dx, dw, db
        out, seen = launched(amd, run)
        outs.append(out)
        labels.append(conv_labels(seen))
    print("%s: %s" % (tag, labels[1]))
    assert labels[0] == labels[1], labels
    if FORMS == "all":
        assert want <= set(labels[1]), (sorted(want), labels[1])
    for a, b, name in zip(outs[0], outs[1], ("y", "dx", "dw", "db")):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ deferred weight gradient
DEFERRED = [c for c in GEOM_CASES if c[:7] in (('wgrad', 36, 132, C5, 4, 3, 32), ('wgrad', 64, 36, K32, 3, 5, 40))]


@pytest.mark.gpu
@pytest.mark.parametrize("c", DEFERRED, ids=case_id)
def test_deferred_weight_gradient_equals_the_immediate_one_bitwise(amd, c):
    """vq2_conv_wgrad_partial + vq2_wgrad_job_init + vq2_wgrad_reduce_batched through ops.WgradBatch, the collector
    of the trainers, against the immediate conv_wgrad (itself compared with fp64 in the table): the same bits, on
    wgrad_fast_kernel and on wgrad_kernel."""
    from vqvae2_amd import ops
    dev = torch.device("cuda:0")
    op, cin, cout, (kh, kw, pt, pl), n, h, w, fl = c[:8]
    assert len(DEFERRED) == 2
    d = make_inputs(c)
    spec = ops.ConvSpec.geom(cin, cout, kh, kw, pt, pl)
    _, x = sliced(d["x"], dev)
    _, dy = sliced(d["dy"], dev)
    side = torch.cuda.Stream()
    for relu_in in (True, False):
        wt, b = d["w"].to(dev), d["b"].to(dev)
        (dw, db), seen = launched(amd, lambda: ops.conv_wgrad(spec, x, dy, relu_in, wt, b))
        assert set(conv_labels(seen)) == {expected(c)}, seen
        w2, b2 = d["w"].to(dev), d["b"].to(dev)
        w2._vq2_grad, b2._vq2_grad = torch.full_like(w2, 7.0), torch.full_like(b2, 7.0)      # the slots of a ParamArena
        batch = ops.WgradBatch()

        def deferred():
            out = batch.launch(spec, x, dy, relu_in, w2, b2, True, side)
            torch.cuda.current_stream().wait_stream(side)        # all slabs written
            batch.flush()
            return out
        (dw2, db2), seen = launched(amd, deferred)
        assert set(conv_labels(seen)) == {expected(c)}, seen
        assert dw2.data_ptr() == w2._vq2_grad.data_ptr() and db2.data_ptr() == b2._vq2_grad.data_ptr()
        assert torch.equal(dw, dw2), "dw relu_in=%d" % relu_in
        assert torch.equal(db, db2), "db relu_in=%d" % relu_in


# ------------------------------------------------------------------------------------------------------- the other forms
# Wall time on the MI355X machine when this was written (the fp64 references on the CPU are most of it): the table, the
# census and the invariance tests in one process 35 s under VQ2_FORMS=general, 36 s under =direct (the whole module, both
# children included: about 106 s).  CHILD_SECONDS is that figure rounded up; a child gets three times as long.
CHILD_SECONDS = 40


def _child(forms):
    env = dict(os.environ, VQ2_FORMS=forms)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        "-k", "geom_case or geom_census or geom_image_zero"], env=env, capture_output=True, text=True,
                       timeout=3 * CHILD_SECONDS)
    print("VQ2_FORMS=%s child: %.1f s" % (forms, time.time() - t0))
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, \
        r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_geom_table_on_the_general_kernels():
    """conv_gemm_kernel and wgrad_kernel tiles: the whole table in a child process with VQ2_FORMS=general."""
    _child("general")


@pytest.mark.gpu
def test_geom_table_on_the_direct_forms():
    """The whole table in a child process with VQ2_FORMS=direct (no geometry case takes a Winograd form: the same labels)."""
    _child("direct")
