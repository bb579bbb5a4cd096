"""Every conv dispatch branch against fp64, at its shape boundaries (csrc/vq2_conv.hip plan_conv with its conv_k4s2_c4,
conv1x1_k64, Winograd (plan_wino) and sub-pixel gates and its fast-GEMM instantiation flags, use_convT_small; vq2_wgrad.hip
plan_wgrad: role, kernel family, Winograd mode and the tile out of WGRAD_TILES).  Kernel selection is a function of the layer's shape and strides alone, so the only way to reach a kernel is a
shape on the right side of every threshold: CASES is that list, written down as data, with the profiler label (tile and
instantiation included) each case must produce under VQ2_FORMS = all / direct / general.

Label syntax: "<family>|<variant>".  The family is the text before '|' in the library's label; the variant is its last
comma-separated field: conv_gemm says tap / uni / var (conv_gemm_fast_kernel with uniform chunks and the taps innermost,
uniform chunks, chunks that may straddle taps) or gen (conv_gemm_kernel); wgrad says fast (wgrad_fast_kernel) or gen
(wgrad_kernel).  An empty variant means the family has one instantiation per flag set only.

Every operand goes through a channel slice that starts at channel 4 of a buffer 8 channels wider; outputs land in such a
slice of a buffer pre-filled with a sentinel, with 64 sentinel guard pixels before and after the tensor in the same
allocation: neighbouring channels and guard pixels must be untouched after the run.

Tolerances are the project's (tests/test_gpu_edge.py): atol = 5e-6 * max|ref| for y and dx, 1e-5 * max|ref| for dw and db,
rtol = 0.  They were set for reduction depths up to 16 x 256 (y, dx) and some tens of thousands of rows (dw).  A case deeper
than that allows max(project tolerance, 4 x the error of plain fp32 torch on the CPU against fp64 on the same inputs); the
factor 4 covers the difference in summation ORDER between a blocked MFMA sum and a sequential one, not precision.  The test
measures that error again on every run; the values measured when the table was written:

    case                                   depth    fp32-vs-fp64 max err / max|ref|   tolerance used / max|ref|
    fwd  conv 128 -> 128 k7 p3, 1x12x10    6272     2.43e-6                          9.73e-6 (4 x measured)
    (every other case: depth <= 4096 for y / dx, <= 65,664 rows for dw -- the project's two tolerances)

That the tolerance bites was checked on the CPU for every case of the table: with one tap of one (co, ci) pair of the
reference weights set to zero (for weight gradients, which do not read the weights: one pixel of one channel of dy), the
comparison of the plain fp32 result with the fp64 reference fails in every case (_bites in this module is that check;
tests/test_host_cpu.py runs it for one case of every label family).

Batch invariance (SWITCH_PAIRS): the rows of image 0 computed at batch N equal BITWISE the rows computed at batch N' on the
other side of each launch-size switch -- 400 / 512 / 1024 tiles in plan_conv, `wide` in plan_wino (both row widths,
3x3 and k4s2), M >= 16384 of conv1x1_k64.  No exception was found.

Tensors of 1 GiB and more come last (peak device memory of the module: 5.0 GiB)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import rng

FORMS = os.environ.get("VQ2_FORMS", "all")
COL = {"all": 0, "direct": 1, "general": 2}[FORMS]
F, T = False, True

CASES = [
    # op, transposed, cin, cout, k, stride, pad, N, H, W, flags, label under VQ2_FORMS = all, direct, general
    # flags -- fwd: i ReLU-in, b bias, r residual, o ReLU-out; dgrad: m mask, r residual, a VQ2_MASK_AFTER_RESIDUAL;
    #          wgrad: i ReLU-in, b bias (every wgrad case also runs without ReLU-in)
    # ---- plan_conv: wgs128 = ceil(M / 128) * ceil(Co / 128) * phases at 400 / 512 / 1024 (8x16 images: wgs128 == N)
    ('fwd', F, 64, 128, 3, 1, 1, 399, 8, 16, 'ibro',         'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 64, 128, 3, 1, 1, 400, 8, 16, 'ibro',         'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 64, 128, 3, 1, 1, 400, 8, 16, '',             'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 64, 128, 3, 1, 1, 512, 8, 16, 'ibro',         'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 64, 128, 3, 1, 1, 513, 8, 16, 'ibro',         'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 64, 128, 3, 1, 1, 1024, 8, 16, 'ibro',        'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 64, 128, 3, 1, 1, 1025, 8, 16, 'ibro',        'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 399, 8, 16, 'mr',         'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 400, 8, 16, 'mr',         'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 512, 8, 16, 'mr',         'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 513, 8, 16, 'mr',         'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 1024, 8, 16, 'mr',        'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 1024, 8, 16, 'mra',       'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 1025, 8, 16, 'mr',        'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 64, 64, 3, 1, 1, 399, 8, 16, 'ibro',          'conv_gemm<64x64x32>|tap', 'conv_gemm<64x64x32>|tap', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 64, 64, 3, 1, 1, 400, 8, 16, '',              'conv_gemm<128x64x16>|tap', 'conv_gemm<128x64x16>|tap', 'conv_gemm<128x64x16>|gen'),
    ('fwd', F, 48, 32, 3, 1, 1, 2, 9, 7, 'ibro',             'conv_gemm<128x32x32>|var', 'conv_gemm<128x32x32>|var', 'conv_gemm<128x32x16>|gen'),
    ('fwd', F, 48, 36, 3, 1, 1, 2, 9, 7, '',                 'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 64, 64, 3, 1, 1, 2, 9, 7, '',                 'conv_gemm<64x64x32>|tap', 'conv_gemm<64x64x32>|tap', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 64, 68, 3, 1, 1, 2, 9, 7, 'ibro',             'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', F, 32, 96, 3, 1, 1, 2, 9, 7, 'mr',             'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x16>|gen'),
    ('fwd', F, 40, 32, 3, 1, 1, 400, 8, 16, '',              'conv_gemm<128x32x32>|var', 'conv_gemm<128x32x32>|var', 'conv_gemm<128x32x16>|gen'),
    ('fwd', F, 32, 192, 1, 1, 0, 200, 8, 16, 'ibro',         'conv_gemm<64x192x16>|uni', 'conv_gemm<64x192x16>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 32, 132, 1, 1, 0, 200, 8, 16, '',             'conv_gemm<64x192x16>|uni', 'conv_gemm<64x192x16>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 32, 128, 1, 1, 0, 400, 8, 16, 'ibro',         'conv_gemm<64x128x16>|uni', 'conv_gemm<64x128x16>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 32, 196, 1, 1, 0, 200, 8, 16, '',             'conv_gemm<64x128x16>|uni', 'conv_gemm<64x128x16>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 64, 132, 1, 1, 0, 200, 8, 16, 'ibro',         'conv_gemm<64x192x16>|uni', 'conv_gemm<64x192x16>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 68, 132, 1, 1, 0, 200, 8, 16, '',             'conv_gemm<128x128x32>|var', 'conv_gemm<128x128x32>|var', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 16, 128, 2, 1, 0, 401, 9, 17, 'ibro',         'conv_gemm<64x128x16>|uni', 'conv_gemm<64x128x16>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 72, 128, 3, 1, 1, 600, 8, 16, 'ibro',         'conv_gemm<128x128x32>|var', 'conv_gemm<128x128x32>|var', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 48, 128, 3, 1, 1, 600, 8, 16, '',             'conv_gemm<128x128x16>|uni', 'conv_gemm<128x128x16>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 32, 128, 3, 1, 1, 2, 9, 7, '',                'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 48, 128, 3, 1, 1, 2, 9, 7, 'ibro',            'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 96, 128, 3, 1, 1, 2, 9, 7, '',                'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 64, 128, 1, 1, 0, 2, 9, 7, 'ibro',            'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 40, 64, 3, 1, 1, 400, 8, 16, 'ibro',          'conv_gemm<128x64x16>|var', 'conv_gemm<128x64x16>|var', 'conv_gemm<128x64x16>|gen'),
    ('fwd', F, 48, 64, 3, 1, 1, 400, 8, 16, '',              'conv_gemm<128x64x16>|uni', 'conv_gemm<128x64x16>|uni', 'conv_gemm<128x64x16>|gen'),
    ('fwd', F, 32, 64, 5, 1, 2, 2, 9, 7, 'ibro',             'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 32, 64, 6, 1, 2, 2, 9, 7, 'ibro',             'conv_gemm<64x64x16>|gen', 'conv_gemm<64x64x16>|gen', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 128, 128, 7, 1, 3, 1, 12, 10, '',             'conv_gemm<64x128x16>|gen', 'conv_gemm<64x128x16>|gen', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', F, 64, 32, 6, 1, 3, 2, 9, 7, 'mr',             'conv_gemm<64x64x16>|gen', 'conv_gemm<64x64x16>|gen', 'conv_gemm<64x64x16>|gen'),
    ('dgrad', F, 32, 16, 7, 1, 3, 2, 9, 7, 'mra',            'conv_gemm<128x32x16>|gen', 'conv_gemm<128x32x16>|gen', 'conv_gemm<128x32x16>|gen'),
    ('fwd', F, 3, 64, 4, 2, 1, 3, 20, 36, 'ib',              'conv_k4s2_c4|', 'conv_k4s2_c4|', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 4, 64, 4, 2, 1, 3, 20, 36, '',                'conv_k4s2_c4|', 'conv_k4s2_c4|', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 3, 64, 4, 2, 1, 3, 20, 36, 'ibro',            'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 3, 68, 4, 2, 1, 3, 20, 36, 'ib',              'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 8, 64, 4, 2, 1, 3, 20, 36, 'ib',              'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x16>|gen'),
    ('dgrad', T, 64, 3, 4, 2, 1, 3, 10, 18, 'm',             'conv_k4s2_c4|', 'conv_k4s2_c4|', 'conv_gemm<64x64x16>|gen'),
    ('dgrad', T, 64, 3, 4, 2, 1, 3, 10, 18, '',              'conv_k4s2_c4|', 'conv_k4s2_c4|', 'conv_gemm<64x64x16>|gen'),
    ('dgrad', T, 64, 3, 4, 2, 1, 3, 10, 18, 'mr',            'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x16>|gen'),
    ('dgrad', T, 64, 4, 4, 2, 1, 3, 10, 18, 'm',             'conv_k4s2_c4|', 'conv_k4s2_c4|', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 64, 64, 1, 1, 0, 1, 128, 128, 'ibro',         'conv1x1_k64|', 'conv1x1_k64|', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 64, 128, 1, 1, 0, 128, 8, 16, 'ibro',         'conv1x1_k64|', 'conv1x1_k64|', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 64, 128, 1, 1, 0, 127, 8, 16, 'ibro',         'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', F, 128, 64, 1, 1, 0, 128, 8, 16, 'm',          'conv1x1_k64|', 'conv1x1_k64|', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', F, 128, 64, 1, 1, 0, 127, 8, 16, 'm',          'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 64, 192, 1, 1, 0, 3, 43, 127, 'ibro',         'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 64, 192, 1, 1, 0, 1, 128, 128, '',            'conv1x1_k64|', 'conv1x1_k64|', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 68, 128, 1, 1, 0, 1, 128, 128, '',            'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 64, 80, 1, 1, 0, 1, 128, 128, '',             'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 64, 32, 1, 1, 0, 1, 128, 128, 'ibro',         'conv_gemm<128x32x32>|uni', 'conv_gemm<128x32x32>|uni', 'conv_gemm<128x32x16>|gen'),
    ('fwd', F, 64, 224, 1, 1, 0, 1, 128, 128, '',            'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', F, 96, 64, 1, 1, 0, 1, 128, 128, 'mr',         'conv1x1_k64|', 'conv1x1_k64|', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', F, 96, 64, 1, 1, 0, 3, 43, 127, 'mra',         'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', T, 16, 64, 4, 2, 1, 512, 8, 16, 'ibo',           'subpixel_conv|', 'subpixel_conv|', 'conv_gemm<128x64x16>|gen'),
    ('fwd', T, 16, 64, 4, 2, 1, 511, 8, 16, 'ibo',           'conv_gemm<128x64x16>|uni', 'conv_gemm<128x64x16>|uni', 'conv_gemm<128x64x16>|gen'),
    ('fwd', T, 128, 64, 4, 2, 1, 2, 10, 20, '',              'subpixel_conv|', 'subpixel_conv|', 'conv_gemm<64x64x16>|gen'),
    ('fwd', T, 112, 64, 4, 2, 1, 2, 10, 20, 'ibo',           'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x16>|gen'),
    ('fwd', T, 128, 68, 4, 2, 1, 2, 10, 20, '',              'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('fwd', T, 24, 64, 4, 2, 1, 512, 8, 16, '',              'conv_gemm<128x64x16>|var', 'conv_gemm<128x64x16>|var', 'conv_gemm<128x64x16>|gen'),
    ('dgrad', F, 128, 128, 4, 2, 1, 2, 20, 40, 'mr',         'subpixel_conv|', 'subpixel_conv|', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', F, 64, 16, 4, 2, 1, 512, 16, 32, 'mra',        'subpixel_conv|', 'subpixel_conv|', 'conv_gemm<128x64x16>|gen'),
    ('dgrad', F, 64, 112, 4, 2, 1, 2, 20, 40, 'm',           'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x32>|var', 'conv_gemm<64x64x16>|gen'),
    ('fwd', T, 64, 3, 4, 2, 1, 2, 17, 35, 'ib',              'convT_small|', 'convT_small|', 'convT_small|'),
    ('fwd', T, 16, 1, 4, 2, 1, 65535, 1, 1, 'b',             'convT_small|', 'convT_small|', 'convT_small|'),
    ('fwd', T, 64, 4, 4, 2, 1, 2, 17, 35, 'ib',              'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x16>|gen'),
    ('fwd', T, 24, 3, 4, 2, 1, 2, 17, 35, 'ib',              'conv_gemm<128x32x32>|var', 'conv_gemm<128x32x32>|var', 'conv_gemm<128x32x16>|gen'),
    ('fwd', T, 64, 8, 4, 2, 1, 2, 17, 35, '',                'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x16>|gen'),
    ('fwd', F, 32, 128, 3, 1, 1, 400, 2, 64, 'ibro',         'conv_wino3<2x64,nt2>|', 'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 32, 128, 3, 1, 1, 399, 2, 64, 'ibro',         'conv_wino3<2x64,nt1>|', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 32, 128, 3, 1, 1, 400, 4, 32, '',             'conv_wino3<4x32,nt2>|', 'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 32, 128, 3, 1, 1, 399, 4, 32, '',             'conv_wino3<4x32,nt1>|', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 32, 128, 3, 1, 1, 3, 3, 64, '',               'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 32, 128, 3, 1, 1, 3, 2, 32, 'ibro',           'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 24, 128, 3, 1, 1, 3, 2, 64, '',               'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 36, 128, 3, 1, 1, 3, 2, 64, '',               'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 32, 96, 3, 1, 1, 3, 2, 64, 'ibro',            'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 32, 64, 3, 1, 1, 3, 2, 64, 'ibro',            'conv_wino3<2x64,nt1>|', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 400, 2, 64, 'mra',        'conv_wino3<2x64,nt2>|', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 399, 2, 64, 'mra',        'conv_wino3<2x64,nt1>|', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 400, 4, 32, 'mr',         'conv_wino3<4x32,nt2>|', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', F, 128, 64, 3, 1, 1, 399, 4, 32, 'mr',         'conv_wino3<4x32,nt1>|', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 32, 128, 4, 2, 1, 400, 4, 128, 'ibo',         'conv_wino_k4s2<2x64,nt2>|', 'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 32, 128, 4, 2, 1, 399, 4, 128, 'ibo',         'conv_wino_k4s2<2x64,nt1>|', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 32, 128, 4, 2, 1, 400, 8, 64, '',             'conv_wino_k4s2<4x32,nt2>|', 'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|gen'),
    ('fwd', F, 32, 128, 4, 2, 1, 399, 8, 64, '',             'conv_wino_k4s2<4x32,nt1>|', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 32, 64, 4, 2, 1, 3, 4, 128, '',               'conv_wino_k4s2<2x64,nt1>|', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 32, 64, 4, 2, 1, 3, 8, 64, 'ibo',             'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 24, 128, 4, 2, 1, 3, 4, 128, '',              'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x32>|var', 'conv_gemm<64x128x16>|gen'),
    ('fwd', F, 32, 128, 4, 2, 1, 3, 4, 64, '',               'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', T, 128, 64, 4, 2, 1, 400, 2, 64, 'mr',         'conv_wino_k4s2<2x64,nt2>|', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', T, 128, 64, 4, 2, 1, 399, 2, 64, 'mr',         'conv_wino_k4s2<2x64,nt1>|', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', T, 128, 128, 4, 2, 1, 400, 4, 32, 'm',         'conv_wino_k4s2<4x32,nt2>|', 'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|gen'),
    ('dgrad', T, 128, 128, 4, 2, 1, 399, 4, 32, 'm',         'conv_wino_k4s2<4x32,nt1>|', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('fwd', T, 32, 64, 4, 2, 1, 2, 4, 64, 'ibo',             'conv_wino_subpixel<4x64>|', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('fwd', T, 32, 64, 4, 2, 1, 2, 8, 32, '',                'conv_wino_subpixel<8x32>|', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('fwd', T, 32, 64, 4, 2, 1, 2, 4, 32, '',                'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('dgrad', F, 64, 32, 4, 2, 1, 2, 8, 128, 'm',            'conv_wino_subpixel<4x64>|', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('dgrad', F, 64, 32, 4, 2, 1, 2, 16, 64, 'mr',           'conv_wino_subpixel<8x32>|', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    # VQ2_MASK_AFTER_RESIDUAL on the kernels with an epilogue or a pixel mapping of their own, the forward residual of the
    # stride-2 / conv-transpose families (ReLU-in, bias, residual and ReLU-out together), and 64x192x16 with Ci % 16 != 0
    ('dgrad', F, 96, 64, 1, 1, 0, 1, 128, 128, 'mra',        'conv1x1_k64|', 'conv1x1_k64|', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', T, 128, 64, 4, 2, 1, 3, 2, 64, 'mra',          'conv_wino_k4s2<2x64,nt1>|', 'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x16>|gen'),
    ('dgrad', F, 64, 32, 4, 2, 1, 2, 8, 128, 'mra',          'conv_wino_subpixel<4x64>|', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('dgrad', F, 32, 48, 3, 1, 1, 3, 9, 7, 'mra',            'conv_gemm<128x32x32>|var', 'conv_gemm<128x32x32>|var', 'conv_gemm<128x32x16>|gen'),
    ('fwd', T, 128, 64, 4, 2, 1, 2, 10, 20, 'ibro',          'subpixel_conv|', 'subpixel_conv|', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 32, 64, 4, 2, 1, 3, 4, 128, 'ibro',           'conv_wino_k4s2<2x64,nt1>|', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('fwd', T, 32, 64, 4, 2, 1, 2, 4, 64, 'ibro',            'conv_wino_subpixel<4x64>|', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x16>|gen'),
    ('fwd', F, 12, 192, 2, 1, 0, 401, 9, 17, '',             'conv_gemm<64x192x16>|var', 'conv_gemm<64x192x16>|var', 'conv_gemm<128x128x32>|gen'),
    # weight gradients: the six tiles of plan_wgrad, exchanged roles (sw), the conv-transpose form, rows of whole 32-pixel
    # chunks or not (fast | gen), the M >= 65536 rule of 128x96, ragged last splits (M % rows-per-split != 0)
    ('wgrad', F, 128, 128, 3, 1, 1, 4, 3, 32, 'ib',          'wgrad<128x128>|fast', 'wgrad<128x128>|fast', 'wgrad<128x128>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', F, 128, 64, 1, 1, 0, 4, 3, 32, 'ib',           'wgrad<64x128>|fast', 'wgrad<64x128>|fast', 'wgrad<64x128>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', F, 256, 32, 1, 1, 0, 4, 3, 32, 'ib',           'wgrad<32x256>|fast', 'wgrad<32x256>|fast', 'wgrad<32x256>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', F, 32, 128, 3, 1, 1, 171, 4, 96, 'ib',         'wgrad<128x96>|fast', 'wgrad<128x96>|fast', 'wgrad<128x96>|gen'),   # M=65664 S=158 rows/split=416 ragged
    ('wgrad', F, 32, 128, 3, 1, 1, 170, 4, 96, 'ib',         'wgrad<128x32>|fast', 'wgrad<128x32>|fast', 'wgrad<128x32>|gen'),   # M=65280 S=108 rows/split=608 ragged
    ('wgrad', F, 128, 32, 3, 1, 1, 171, 4, 96, 'ib',         'wgrad<128x96>sw|fast', 'wgrad<128x96>sw|fast', 'wgrad<32x256>|gen'),   # M=65664 S=158 rows/split=416 ragged
    ('wgrad', F, 128, 32, 3, 1, 1, 170, 4, 96, 'ib',         'wgrad<128x32>sw|fast', 'wgrad<128x32>sw|fast', 'wgrad<32x256>|gen'),   # M=65280 S=108 rows/split=608 ragged
    ('wgrad', F, 32, 128, 1, 1, 0, 4, 3, 32, 'ib',           'wgrad<128x32>|fast', 'wgrad<128x32>|fast', 'wgrad<128x32>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', F, 64, 64, 1, 1, 0, 5, 7, 32, 'ib',            'wgrad<64x64>|fast', 'wgrad<64x64>|fast', 'wgrad<64x64>|gen'),   # M=1120 S=5 rows/split=224
    ('wgrad', T, 64, 32, 4, 2, 1, 3, 5, 32, 'ib',            'wgrad<64x128>|fast', 'wgrad<64x128>|fast', 'wgrad<64x128>|gen'),   # M=480 S=2 rows/split=256 ragged
    ('wgrad', F, 128, 128, 3, 1, 1, 4, 3, 40, 'ib',          'wgrad<128x128>|gen', 'wgrad<128x128>|gen', 'wgrad<128x128>|gen'),   # M=480 S=2 rows/split=256 ragged
    ('wgrad', F, 128, 32, 3, 1, 1, 4, 8, 40, 'ib',           'wgrad<128x32>sw|gen', 'wgrad<128x32>sw|gen', 'wgrad<32x256>|gen'),   # M=1280 S=5 rows/split=256
    ('wgrad', F, 64, 32, 3, 1, 1, 4, 3, 32, 'ib',            'wgrad<64x64>sw|fast', 'wgrad<64x64>sw|fast', 'wgrad<32x256>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', F, 60, 32, 3, 1, 1, 4, 3, 32, 'ib',            'wgrad<32x256>|fast', 'wgrad<32x256>|fast', 'wgrad<32x256>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', F, 64, 36, 3, 1, 1, 4, 3, 32, 'ib',            'wgrad<64x64>|fast', 'wgrad<64x64>|fast', 'wgrad<64x64>|gen'),   # M=384 S=2 rows/split=192
    ('wgrad', F, 64, 128, 4, 2, 1, 3, 10, 64, 'ib',          'wgrad<128x128>|fast', 'wgrad<128x128>|fast', 'wgrad<128x128>|gen'),   # M=480 S=2 rows/split=256 ragged
    ('wgrad', T, 32, 3, 4, 2, 1, 2, 9, 32, 'ib',             'wgrad<64x64>|fast', 'wgrad<64x64>|fast', 'wgrad<64x64>|gen'),   # M=576 S=3 rows/split=192
    ('wgrad', F, 16, 40, 7, 1, 3, 2, 8, 32, 'ib',            'wgrad<64x64>|fast', 'wgrad<64x64>|fast', 'wgrad<64x64>|gen'),   # M=512 S=2 rows/split=256
]

# the sections of CASES, in order (read the table against the dispatch functions with these):
#   plan_conv tiles by Co (32 | 36, 64 | 68), K <= 64 (Co 128 | 132 | 192 | 196, K 64 | 68), Ci % 16 in the 512..1024 window;
#   plan_conv's uni / tap_inner: Ci % BK (48 on BK 32: var, on BK 16: uni; 40: var), Ci > 32 and Ci % 32 (32 uni, 96 tap), taps > 1;
#   KH * KW <= 32 (25 fast | 36, 49 general);  the conv_k4s2_c4 gate (Ci 4 | 8, Co 64 | 68, residual, 3 or 4 real channels, mask);
#   the conv1x1_k64 gate (M 16383 | 16384, Ci 64 | 68, Co % 32, Co 32 | 64, 192 | 224);  sub-pixel gate (sp_wgs 511 | 512 at K = 64,
#   K 448 | 512, Co % 64, Ci % 16);  use_convT_small (Cor 3 | 4, Co 4 | 8, Ci % 16; refusals: test_conv_transpose_small_refusals);
#   plan_wino (rows64 | rows32 | neither, Ci 24 | 32 | 36, Co % 64, Co % 128 for k4s2 on 32-pixel rows, wide 399 | 400).
# Branches that cannot be reached through the ABI, by the code (no case can exist):
#   - plan_wgrad's kernel family, `rows_per_split % 32 == 0`: it rounds rows_per_split up to a multiple of 32 just before;
#   - plan_conv's `uni`, `K % BK == 0` once `Ci % BK == 0` holds: K = KH * KW * Ci;
#   - the non-uniform instantiation of the four-per-CU 128x128x16 tile: its gate (Ci % 16 == 0, below 1 GiB) implies `small`,
#     and `occ4` makes `uni` true then;
#   - the conv_k4s2_c4 gate, `H % 2`, `W % 2`, `KH == 4`, `pad == 1` given stride 2, and the conv1x1_k64 gate, `stride == 1` given KH == 1:
#     check_conv_desc admits stride 2 only as k4 p1 on even sizes (phases == 1 with a 4x4 stride-2 kernel is that layer or the
#     data gradient of a conv-transpose, which is k4 s2 p1 by check_conv_desc as well).
# Reachable only with a tensor of 1 GiB: `small == false` inside the 513..1024-tile window (an operand that is a channel slice
# of a buffer 2048 floats wide) -- the first case of test_tensors_of_one_gib_and_more.
# Not every (tile, instantiation) product is enumerated: each tile has a case, and each of tap / uni / var has cases on BK = 16
# and on BK = 32 tiles; e.g. conv_gemm<64x128x16>|var (K <= 64, Co = 128, Ci = 12) has none.  EXPECTED_LABELS lists exactly
# the products that have.

EXPECTED_LABELS = {
    "all": {
        'conv1x1_k64|', 'convT_small|', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|uni',
        'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|var', 'conv_gemm<128x32x16>|gen', 'conv_gemm<128x32x32>|tap',
        'conv_gemm<128x32x32>|uni', 'conv_gemm<128x32x32>|var', 'conv_gemm<128x64x16>|tap', 'conv_gemm<128x64x16>|uni',
        'conv_gemm<128x64x16>|var', 'conv_gemm<64x128x16>|gen', 'conv_gemm<64x128x16>|uni', 'conv_gemm<64x128x32>|tap',
        'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|var', 'conv_gemm<64x192x16>|uni', 'conv_gemm<64x192x16>|var', 'conv_gemm<64x64x16>|gen',
        'conv_gemm<64x64x32>|tap', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x32>|var', 'conv_k4s2_c4|',
        'conv_wino3<2x64,nt1>|', 'conv_wino3<2x64,nt2>|', 'conv_wino3<4x32,nt1>|', 'conv_wino3<4x32,nt2>|',
        'conv_wino_k4s2<2x64,nt1>|', 'conv_wino_k4s2<2x64,nt2>|', 'conv_wino_k4s2<4x32,nt1>|', 'conv_wino_k4s2<4x32,nt2>|',
        'conv_wino_subpixel<4x64>|', 'conv_wino_subpixel<8x32>|', 'subpixel_conv|', 'wgrad<128x128>|fast',
        'wgrad<128x128>|gen', 'wgrad<128x32>sw|fast', 'wgrad<128x32>sw|gen', 'wgrad<128x32>|fast', 'wgrad<128x96>sw|fast',
        'wgrad<128x96>|fast', 'wgrad<32x256>|fast', 'wgrad<64x128>|fast', 'wgrad<64x64>sw|fast', 'wgrad<64x64>|fast'
    },
    "direct": {
        'conv1x1_k64|', 'convT_small|', 'conv_gemm<128x128x16>|tap', 'conv_gemm<128x128x16>|uni',
        'conv_gemm<128x128x32>|tap', 'conv_gemm<128x128x32>|uni', 'conv_gemm<128x128x32>|var', 'conv_gemm<128x32x16>|gen',
        'conv_gemm<128x32x32>|tap', 'conv_gemm<128x32x32>|uni', 'conv_gemm<128x32x32>|var', 'conv_gemm<128x64x16>|tap',
        'conv_gemm<128x64x16>|uni', 'conv_gemm<128x64x16>|var', 'conv_gemm<64x128x16>|gen', 'conv_gemm<64x128x16>|uni',
        'conv_gemm<64x128x32>|tap', 'conv_gemm<64x128x32>|uni', 'conv_gemm<64x128x32>|var', 'conv_gemm<64x192x16>|uni', 'conv_gemm<64x192x16>|var',
        'conv_gemm<64x64x16>|gen', 'conv_gemm<64x64x32>|tap', 'conv_gemm<64x64x32>|uni', 'conv_gemm<64x64x32>|var',
        'conv_k4s2_c4|', 'subpixel_conv|', 'wgrad<128x128>|fast', 'wgrad<128x128>|gen', 'wgrad<128x32>sw|fast',
        'wgrad<128x32>sw|gen', 'wgrad<128x32>|fast', 'wgrad<128x96>sw|fast', 'wgrad<128x96>|fast', 'wgrad<32x256>|fast',
        'wgrad<64x128>|fast', 'wgrad<64x64>sw|fast', 'wgrad<64x64>|fast'
    },
    "general": {
        'convT_small|', 'conv_gemm<128x128x32>|gen', 'conv_gemm<128x32x16>|gen', 'conv_gemm<128x64x16>|gen',
        'conv_gemm<64x128x16>|gen', 'conv_gemm<64x64x16>|gen', 'wgrad<128x128>|gen', 'wgrad<128x32>|gen',
        'wgrad<128x96>|gen', 'wgrad<32x256>|gen', 'wgrad<64x128>|gen', 'wgrad<64x64>|gen'
    },
}

# families with labels of their own that are not conv dispatch branches (their tests: test_gpu_edge.py, test_gpu_parity.py)
OTHER_FAMILIES = {"resblock_fwd_wino", "resblock_fwd", "resblock_bwd_data", "vq_fwd", "vq_stats"}
# labels that only tensors of 1 GiB and more reach (test_tensors_of_one_gib_and_more)
BIG_LABELS = {"conv_gemm<128x128x32>|var", "conv_gemm<128x128x32>|gen", "wgrad<128x128>|gen", "convT_small|"}

SENT, GUARD = 7.0, 64
DEEP_Y = 16 * 256          # reduction depth the project's y / dx tolerance was set for


def case_id(c):
    op, tr, cin, cout, k, s, p, n, h, w, fl = c[:11]
    return "%s-%s%d-%dk%ds%dp%d-%dx%dx%d-%s" % (op, "T" if tr else "C", cin, cout, k, s, p, n, h, w, fl or "none")


def expected(c):
    return c[11 + COL]


def ceil4(c):
    return (c + 3) // 4 * 4


def out_hw(tr, k, s, p, h, w):
    return (2 * h, 2 * w) if tr else ((h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def make_inputs(c):
    """Seeded operands of a case as CPU fp32 tensors (NHWC activations padded to 4 channels with zeros, reference-layout
    weights).  Image n of every activation depends on (case shape without N, n) alone: counter-based streams."""
    op, tr, cin, cout, k, s, p, n, h, w, fl = c[:11]
    ci, co = ceil4(cin), ceil4(cout)
    ho, wo = out_hw(tr, k, s, p, h, w)
    tag = "%s%d.%d.%d.%d.%d.%dx%d" % ("T" if tr else "C", cin, cout, k, s, p, h, w)
    d = {}
    x = _t(rng.normal(41, tag + ".x", (n, h, w, ci)))
    x[..., cin:] = 0
    dy = _t(rng.normal(41, tag + ".dy", (n, ho, wo, co)))
    dy[..., cout:] = 0
    d["x"], d["dy"] = x, dy
    d["w"] = _t(rng.uniform(41, tag + ".w", (cin, cout, k, k) if tr else (cout, cin, k, k), -0.1, 0.1))
    d["b"] = _t(rng.uniform(41, tag + ".b", (cout,), -1, 1))
    d["res_y"] = _t(rng.normal(41, tag + ".ry", (n, ho, wo, co)))
    d["res_x"] = _t(rng.normal(41, tag + ".rx", (n, h, w, ci)))
    return d


def _conv64(tr, a, w, b, s, p):
    fn = Fn.conv_transpose2d if tr else Fn.conv2d
    return fn(a, w, b, stride=s, padding=p)


def reference(c, d, dtype=torch.float64, relu_in=None):
    """The op of a case in plain torch on the CPU (autograd for the gradients).  Returns NHWC / reference-layout tensors
    restricted to the real channels: y | dx | (dw, db)."""
    op, tr, cin, cout, k, s, p, n, h, w, fl = c[:11]
    x = d["x"][..., :cin].permute(0, 3, 1, 2).to(dtype)
    wt, b = d["w"].to(dtype), d["b"].to(dtype)
    if op == "fwd":
        y = _conv64(tr, Fn.relu(x) if "i" in fl else x, wt, b if "b" in fl else None, s, p)
        if "r" in fl:
            y = y + d["res_y"][..., :cout].permute(0, 3, 1, 2).to(dtype)
        if "o" in fl:
            y = Fn.relu(y)
        return y.permute(0, 2, 3, 1)
    dy = d["dy"][..., :cout].permute(0, 3, 1, 2).to(dtype)
    if op == "dgrad":
        a = x.clone().requires_grad_(True)
        _conv64(tr, a, wt, None, s, p).backward(dy)
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
    _conv64(tr, Fn.relu(x) if relu_in else x, wr, br, s, p).backward(dy)
    return wr.grad, br.grad


def tolerance(c, ref, what):
    """The project's tolerance; None when the case is deeper than that tolerance was set for (the caller then measures
    plain fp32 against fp64, see the module docstring)."""
    op, tr, cin, cout, k, s, p = c[:7]
    scale = float(ref.abs().max())
    if what in ("dw", "db"):
        return 1e-5 * scale
    depth = (16 if tr else k * k) * (ceil4(cin) if op == "fwd" else ceil4(cout))
    if tr and op == "fwd":
        depth = 4 * ceil4(cin)
    return 5e-6 * scale if depth <= DEEP_Y else None


def deep_tolerance(c, d, ref):
    """max(project tolerance, 4 x the error of plain fp32 torch on the CPU) for a case past the project's depth."""
    err32 = float((reference(c, d, torch.float32).double() - ref).abs().max())
    scale = float(ref.abs().max())
    tol = max(5e-6 * scale, 4 * err32)
    print("deep case %s: fp32-vs-fp64 max err %.3e (%.3e of max|ref|), tolerance %.3e (%.3e of max|ref|)"
          % (case_id(c), err32, err32 / scale, tol, tol / scale))
    return tol


def differs(got, ref, tol):
    return bool(((got.double() - ref).abs() > tol).any())


def _bites(c):
    """CPU check that the tolerance of a case would catch a kernel that drops ONE product: plain fp32 torch with one tap of
    one (co, ci) pair of the weights zeroed (wgrad: one pixel of one channel of dy) must fail the comparison."""
    op, tr, cin, cout, k, s, p, n, h, w, fl = c[:11]
    d = make_inputs(c)
    bad = dict(d)
    if op == "wgrad":
        bad["dy"] = d["dy"].clone()
        bad["dy"][n - 1, bad["dy"].shape[1] // 2, bad["dy"].shape[2] // 2, cout // 2] = 0
        ref = reference(c, d, relu_in=True)[0]
        got = reference(c, bad, torch.float32, relu_in=True)[0]
        good = reference(c, d, torch.float32, relu_in=True)[0]
        tol = tolerance(c, ref, "dw")
    else:
        bad["w"] = d["w"].clone()
        bad["w"][bad["w"].shape[0] // 2, bad["w"].shape[1] // 2, k // 2, k // 2] = 0
        ref = reference(c, d)
        got, good = reference(c, bad, torch.float32), reference(c, d, torch.float32)
        tol = tolerance(c, ref, "y")
        if tol is None:
            tol = deep_tolerance(c, d, ref)
    assert not differs(good, ref, tol), case_id(c) + ": plain fp32 itself misses the tolerance"
    assert differs(got, ref, tol), case_id(c) + ": the tolerance does not notice a dropped product"


# ----------------------------------------------------------------------------------------------------------------- GPU side
@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def launched(amd, fn):
    """Run fn with every instrumented launch bracketed; returns (result, kernel labels seen).  (test_gpu_edge._launched)"""
    lib = amd._lib.lib
    lib.vq2_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.vq2_prof_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.vq2_prof_report(buf, len(buf))
    return out, [ln.split()[0] for ln in buf.value.decode().splitlines()]


def short_label(full):
    """library label -> "<family>|<variant>" of the table"""
    fam, _, detail = full.partition("|")
    last = detail.rsplit(",", 1)[-1]
    return fam + "|" + (last if last in ("tap", "uni", "var", "gen", "fast") else "")


CONV_FAMILIES = ("conv_gemm", "conv_wino", "conv1x1_k64", "conv_k4s2_c4", "convT_small", "subpixel_conv", "wgrad<")


def conv_labels(seen):
    return [short_label(s) for s in seen if s.startswith(CONV_FAMILIES)]


def sliced(a, dev, pad=8, off=4):
    """NHWC tensor -> the same values as channels [off, off + C) of a device buffer `pad` channels wider (the rest random)"""
    n, h, w, c = a.shape
    wide = torch.randn((n, h, w, c + pad), generator=torch.Generator().manual_seed(c * 131 + w)).to(dev)
    wide[..., off:off + c] = a.to(dev)
    return wide, wide[..., off:off + c]


def guarded(shape, dev, pad=8, off=4):
    """Sentinel-filled allocation holding GUARD pixels, the [n,h,w,c+pad] tensor, GUARD pixels; returns (flat, wide, slice)"""
    n, h, w, c = shape
    ld = c + pad
    flat = torch.full(((n * h * w + 2 * GUARD) * ld,), SENT, device=dev)
    wide = flat[GUARD * ld:(GUARD + n * h * w) * ld].view(n, h, w, ld)
    return flat, wide, wide[..., off:off + c]


def untouched(flat, wide, c, what, pad=8, off=4):
    ld = c + pad
    assert bool((flat[:GUARD * ld] == SENT).all()) and bool((flat[-GUARD * ld:] == SENT).all()), what + ": guard pixels written"
    assert bool((wide[..., :off] == SENT).all()) and bool((wide[..., off + c:] == SENT).all()), what + ": neighbour channels written"


_RESULTS = {}


def run_case(amd, c):
    """Run one table case on the GPU against fp64 (cached: the census and the invariance tests reuse it).  Returns
    (labels seen, rows of image 0 as a CPU tensor)."""
    key = case_id(c)
    if key in _RESULTS:
        return _RESULTS[key]
    from vqvae2_amd import ops
    dev = torch.device("cuda:0")
    op, tr, cin, cout, k, s, p, n, h, w, fl = c[:11]
    ci, co = ceil4(cin), ceil4(cout)
    ho, wo = out_hw(tr, k, s, p, h, w)
    d = make_inputs(c)
    spec = ops.ConvSpec(tr, cin, cout, k, s, p)
    wt, b = d["w"].to(dev), d["b"].to(dev)
    _, x = sliced(d["x"], dev)
    if op == "fwd":
        flat, wide, out = guarded((n, ho, wo, co), dev)
        flags = (ops.VQ2_RELU_IN if "i" in fl else 0) | (ops.VQ2_RELU_OUT if "o" in fl else 0)
        res = sliced(d["res_y"], dev)[1] if "r" in fl else None
        y, seen = launched(amd, lambda: ops.conv_forward(spec, x, wt, b if "b" in fl else None, flags, residual=res, out=out))
        untouched(flat, wide, co, key)
        ref = reference(c, d)
        tol = tolerance(c, ref, "y")
        if tol is None:
            tol = deep_tolerance(c, d, ref)
        got = y[..., :cout].cpu()
        err = float((got.double() - ref).abs().max())
        print("%s: %s  max err %.3e  tolerance %.3e" % (key, conv_labels(seen), err, tol))
        assert err <= tol, key + ".y"
        first = y[0].cpu()
    elif op == "dgrad":
        _, dy = sliced(d["dy"], dev)
        wres, res = sliced(d["res_x"], dev)
        flat, wide, out = guarded((n, h, w, ci), dev)
        dx, seen = launched(amd, lambda: ops.conv_dgrad(spec, (n, h, w, ci), dy, wt, mask=x if "m" in fl else None,
                                                        residual=res if "r" in fl else None, out=out, mask_after="a" in fl))
        untouched(flat, wide, ci, key)
        ref = reference(c, d)
        tol = tolerance(c, ref, "dx")
        if tol is None:
            tol = deep_tolerance(c, d, ref)
        err = float((dx[..., :cin].cpu().double() - ref).abs().max())
        print("%s: %s  max err %.3e  tolerance %.3e" % (key, conv_labels(seen), err, tol))
        assert err <= tol, key + ".dx"
        first = dx[0].cpu()
    else:
        _, dy = sliced(d["dy"], dev)
        seen, first = [], None
        for relu_in in (True, False):
            (dw, db), sn = launched(amd, lambda: ops.conv_wgrad(spec, x, dy, relu_in, wt, b))
            seen += sn
            rw, rb = reference(c, d, relu_in=relu_in)
            for name, got, ref in (("dw", dw, rw), ("db", db, rb)):
                tol = tolerance(c, ref, name)
                err = float((got.cpu().double() - ref).abs().max())
                print("%s relu_in=%d %s: %s  max err %.3e  tolerance %.3e" % (key, relu_in, name, conv_labels(sn), err, tol))
                assert tuple(got.shape) == tuple(ref.shape) and err <= tol, "%s.%s relu_in=%d" % (key, name, relu_in)
    _RESULTS[key] = (conv_labels(seen), first)
    return _RESULTS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_dispatch_case_runs_its_kernel_and_matches_fp64(amd, c):
    labels, _ = run_case(amd, c)
    assert labels and set(labels) == {expected(c)}, (case_id(c), labels, expected(c))


# Launch-size switches: (case on one side, case on the other side), same layer, same flags, same image 0.  Measured on the
# MI355X: every one of them is bitwise invariant (tile height, chunk depth 16 | 32 and the four-per-CU variant all keep the
# order of the sum over (tap, channel) of one output element), so there is no exception to record.
def _sweep(op, tr, cin, cout, k, s, p, h, w, fl, pairs):
    by = {(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[8], c[9], c[10], c[7]): c for c in CASES}
    return [(by[(op, tr, cin, cout, k, s, p, h, w, fl, a)], by[(op, tr, cin, cout, k, s, p, h, w, fl, b)]) for a, b in pairs]


_TILES = ((399, 400), (512, 513), (1024, 1025))
_ONE = ((399, 400),)
SWITCH_PAIRS = (
    _sweep("fwd", F, 64, 128, 3, 1, 1, 8, 16, "ibro", _TILES) +      # plan_conv: 400, 512, 1024 tiles
    _sweep("dgrad", F, 128, 64, 3, 1, 1, 8, 16, "mr", _TILES) +
    _sweep("fwd", F, 32, 128, 3, 1, 1, 2, 64, "ibro", _ONE) + _sweep("fwd", F, 32, 128, 3, 1, 1, 4, 32, "", _ONE) +   # wide, 3x3
    _sweep("dgrad", F, 128, 64, 3, 1, 1, 2, 64, "mra", _ONE) + _sweep("dgrad", F, 128, 64, 3, 1, 1, 4, 32, "mr", _ONE) +
    _sweep("fwd", F, 32, 128, 4, 2, 1, 4, 128, "ibo", _ONE) + _sweep("fwd", F, 32, 128, 4, 2, 1, 8, 64, "", _ONE) +  # wide, k4s2
    _sweep("dgrad", T, 128, 64, 4, 2, 1, 2, 64, "mr", _ONE) + _sweep("dgrad", T, 128, 128, 4, 2, 1, 4, 32, "m", _ONE) +
    _sweep("fwd", F, 64, 128, 1, 1, 0, 8, 16, "ibro", ((127, 128),)) + _sweep("dgrad", F, 128, 64, 1, 1, 0, 8, 16, "m", ((127, 128),))  # M >= 16384
)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", SWITCH_PAIRS, ids=lambda pr: case_id(pr[0]) + "~" + str(pr[1][7]))
def test_image_zero_is_bitwise_the_same_on_both_sides_of_a_launch_size_switch(amd, pair):
    a, b = pair
    (la, ya), (lb, yb) = run_case(amd, a), run_case(amd, b)      # each is compared with fp64 inside run_case
    if FORMS == "all":
        assert set(la) != set(lb), (la, lb)                      # the pair does sit on two sides of a switch
    same = torch.equal(ya, yb)
    diff = float((ya.double() - yb.double()).abs().max())
    print("%s ~ N=%d: %s vs %s bitwise=%s max diff %.3e" % (case_id(a), b[7], sorted(set(la)), sorted(set(lb)), same, diff))
    assert same, "image 0 differs between batch %d and batch %d: max diff %.3e" % (a[7], b[7], diff)


@pytest.mark.gpu
def test_conv_transpose_small_refusals(amd):
    """A conv-transpose to <= 3 channels has its weight panel packed for convT_small alone: a launch that kernel cannot take
    (residual, ReLU-out, more than 65535 images) is refused -- the general kernels would read the panel in another layout."""
    from vqvae2_amd import ops
    dev = torch.device("cuda:0")
    spec = ops.ConvSpec(True, 64, 3, 4, 2, 1)
    wt = torch.zeros((64, 3, 4, 4), device=dev)
    x = torch.zeros((2, 5, 6, 64), device=dev)
    for kw in (dict(flags=ops.VQ2_RELU_OUT), dict(residual=torch.zeros((2, 10, 12, 4), device=dev))):
        with pytest.raises(RuntimeError, match="neither a residual nor ReLU-out"):
            ops.conv_forward(spec, x, wt, None, **kw)
    spec1 = ops.ConvSpec(True, 16, 1, 4, 2, 1)
    with pytest.raises(RuntimeError, match="at most 65535 images"):
        ops.conv_forward(spec1, torch.zeros((65536, 1, 1, 16), device=dev), torch.zeros((16, 1, 4, 4), device=dev), None)


@pytest.mark.gpu
def test_census_of_labels_over_the_whole_table(amd):
    """The union of labels over the table, tile and instantiation included, is EXPECTED_LABELS -- no more, no less."""
    seen = set()
    for c in CASES:
        seen |= set(run_case(amd, c)[0])
    assert seen == EXPECTED_LABELS[FORMS], (sorted(seen - EXPECTED_LABELS[FORMS]), sorted(EXPECTED_LABELS[FORMS] - seen))


def _child(forms):
    env = dict(os.environ, VQ2_FORMS=forms)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        "-k", "dispatch_case or census or bitwise"], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, \
        r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_table_on_the_general_kernels():
    """conv_gemm_kernel and wgrad_kernel tiles: the whole table in a child process with VQ2_FORMS=general."""
    _child("general")


@pytest.mark.gpu
def test_table_on_the_direct_forms():
    """The direct forms of the shapes Winograd takes: the whole table in a child process with VQ2_FORMS=direct."""
    _child("direct")


# ------------------------------------------------------------------------------------------- tensors of 1 GiB and more
def _need(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip("needs %.1f GiB of free device memory, %.1f GiB free" % (nbytes / 2**30, free / 2**30))


def _windows(n, ho, wo, count, seed):
    """(image, oy, ox) of 8x8 output windows: four corners and one interior seam window (across the 64-pixel boundary where
    there is one) of the first and the last image, then `count` seeded random ones over the whole batch."""
    g = torch.Generator().manual_seed(seed)
    wins = []
    for img in (0, n - 1):
        wins += [(img, 0, 0), (img, 0, wo - 8), (img, ho - 8, 0), (img, ho - 8, wo - 8), (img, ho // 2 - 4, min(60, wo - 8))]
    for _ in range(count):
        wins.append((int(torch.randint(0, n, (1,), generator=g)), int(torch.randint(0, ho - 7, (1,), generator=g)),
                     int(torch.randint(0, wo - 7, (1,), generator=g))))
    return wins


def _window_ref_conv3(x, wt64, b64, img, oy, ox):
    """fp64 3x3 s1 p1 conv of one 8x8 output window from the 10x10 input window around it (zeros outside the image)"""
    n, h, w, c = x.shape
    patch = torch.zeros((10, 10, c), dtype=torch.float64)
    y0, y1, x0, x1 = max(oy - 1, 0), min(oy + 9, h), max(ox - 1, 0), min(ox + 9, w)
    patch[y0 - (oy - 1):y1 - (oy - 1), x0 - (ox - 1):x1 - (ox - 1)] = x[img, y0:y1, x0:x1].cpu().double()
    return Fn.conv2d(patch.permute(2, 0, 1)[None], wt64, b64)[0].permute(1, 2, 0)


def _window_ref_convT(x, wt64, b64, img, oy, ox):
    """fp64 k4 s2 p1 conv-transpose of one 8x8 output window (oy, ox even) from the 6x6 input window around it"""
    n, h, w, c = x.shape
    iy, ix = oy // 2 - 1, ox // 2 - 1
    patch = torch.zeros((6, 6, c), dtype=torch.float64)
    y0, y1, x0, x1 = max(iy, 0), min(iy + 6, h), max(ix, 0), min(ix + 6, w)
    patch[y0 - iy:y1 - iy, x0 - ix:x1 - ix] = x[img, y0:y1, x0:x1].cpu().double()
    full = Fn.conv_transpose2d(patch.permute(2, 0, 1)[None], wt64, b64, stride=2, padding=1)[0].permute(1, 2, 0)   # rows 2*iy ..
    return full[2:10, 2:10]


def _check_windows(y, wins, ref_of, cout, what):
    worst, scale = 0.0, 0.0
    for img, oy, ox in wins:
        ref = ref_of(img, oy, ox)
        got = y[img, oy:oy + 8, ox:ox + 8, :cout].cpu().double()
        worst = max(worst, float((got - ref).abs().max()))
        scale = max(scale, float(ref.abs().max()))
    print("%s: %d windows, max err %.3e, tolerance %.3e" % (what, len(wins), worst, 5e-6 * scale))
    assert worst <= 5e-6 * scale, what


@pytest.mark.gpu
def test_tensors_of_one_gib_and_more(amd):
    """3x3 128 -> 128 on 64x64 rows past the byte-size regimes, with a sampled fp64 reference (all four corners and a seam
    window of the first and the LAST image -- where a wrapped offset lands --, 64 random windows, every output channel):
    just above 2^30 bytes Winograd and the uniform instantiation decline (direct tile, var); at 2^29 elements the fast
    kernels decline (conv_gemm_kernel, wgrad_kernel).  Then the reconstruction layer 64 -> 3 just under convT_small's limit.
    The weight gradient at 2^29 elements is compared with the sum of four chunk launches, and a four-image subset with fp64;
    both of those are small enough for the Winograd form (their labels are asserted), so what this test adds for
    wgrad_kernel is its OFFSETS in that regime -- a wrapped offset moves whole rows and is far outside the linearity
    tolerance.  wgrad_kernel's arithmetic against fp64 rests on the |gen weight-gradient rows of CASES."""
    from vqvae2_amd import ops
    dev = torch.device("cuda:0")
    _need(7 << 30)
    g = torch.Generator(device=dev).manual_seed(1234)
    spec = ops.ConvSpec(False, 128, 128, 3, 1, 1)
    wt = torch.empty((128, 128, 3, 3), device=dev).uniform_(-0.1, 0.1, generator=g)
    b = torch.empty((128,), device=dev).uniform_(-1, 1, generator=g)
    w64, b64 = wt.cpu().double(), b.cpu().double()
    # 1024 tiles (inside the four-per-CU window) but the input is a 64-channel slice of a 1 GiB buffer: Winograd and the
    # four-per-CU tile decline by their byte clauses, the 128x128x32 tile runs with chunks that may straddle taps
    spec64 = ops.ConvSpec(False, 64, 128, 3, 1, 1)
    wt64 = torch.empty((128, 64, 3, 3), device=dev).uniform_(-0.1, 0.1, generator=g)
    wide = torch.randn((32, 64, 64, 2048), device=dev, generator=g)
    assert wide.numel() * 4 == 1 << 30
    xs = wide[..., 4:68]
    y, seen = launched(amd, lambda: ops.conv_forward(spec64, xs, wt64, b, 0))
    assert set(conv_labels(seen)) == {"conv_gemm<128x128x32>|gen" if FORMS == "general" else "conv_gemm<128x128x32>|var"}, seen
    w64, b64 = wt64.cpu().double(), b.cpu().double()
    _check_windows(y, _windows(32, 64, 64, 64, 5), lambda i, oy, ox: _window_ref_conv3(xs, w64, b64, i, oy, ox), 128,
                   "fwd 3x3 64->128 out of a 2048-wide buffer, 32 images")
    del wide, xs, y
    torch.cuda.empty_cache()
    w64, b64 = wt.cpu().double(), b.cpu().double()
    x = torch.randn((1024, 64, 64, 128), device=dev, generator=g)           # 2^29 elements, 2 GiB
    for n, want in ((513, "conv_gemm<128x128x32>|var"), (1024, "conv_gemm<128x128x32>|gen")):
        if FORMS == "general":
            want = "conv_gemm<128x128x32>|gen"
        xs = x[:n]
        y, seen = launched(amd, lambda: ops.conv_forward(spec, xs, wt, b, 0))
        assert set(conv_labels(seen)) == {want}, seen
        _check_windows(y, _windows(n, 64, 64, 64, n), lambda i, oy, ox: _window_ref_conv3(xs, w64, b64, i, oy, ox), 128,
                       "fwd 3x3 128->128, %d images" % n)
    # weight gradient at 2^29 elements (y of the last launch serves as dy): wgrad_kernel.  A seeded subset of the batch as
    # its own, smaller launch against fp64; the full-size launch against the sum of per-chunk launches.
    dy = y
    sub = torch.randperm(1024, generator=torch.Generator().manual_seed(7))[:4].to(dev)
    xs, dys = x[sub].contiguous(), dy[sub].contiguous()
    small = {"all": "wgrad<128x128>wino|fast", "direct": "wgrad<128x128>|fast", "general": "wgrad<128x128>|gen"}[FORMS]
    (dw, db), seen = launched(amd, lambda: ops.conv_wgrad(spec, xs, dys, False, wt, b))
    assert set(conv_labels(seen)) == {small}, seen          # NOT wgrad_kernel at this size: see the docstring
    wr, br = w64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
    Fn.conv2d(xs.permute(0, 3, 1, 2).cpu().double(), wr, br, padding=1).backward(dys.permute(0, 3, 1, 2).cpu().double())
    assert float((dw.cpu().double() - wr.grad).abs().max()) <= 1e-5 * float(wr.grad.abs().max()), "dw of the subset"
    assert float((db.cpu().double() - br.grad).abs().max()) <= 1e-5 * float(br.grad.abs().max()), "db of the subset"
    (dw, db), seen = launched(amd, lambda: [t.clone() for t in ops.conv_wgrad(spec, x, dy, False, wt, b)])
    assert set(conv_labels(seen)) == {"wgrad<128x128>|gen"}, seen
    sw, sb = torch.zeros_like(dw), torch.zeros_like(db)
    for i in range(0, 1024, 256):
        (pw, pb), seen = launched(amd, lambda: ops.conv_wgrad(spec, x[i:i + 256], dy[i:i + 256], False, wt, b))
        assert set(conv_labels(seen)) == {small}, seen
        sw += pw
        sb += pb
    for name, got, want_ in (("dw", dw, sw), ("db", db, sb)):       # the tolerance of the batch-linearity tests (test_gpu_parity.py)
        np.testing.assert_allclose(got.cpu().numpy(), want_.cpu().numpy(), rtol=1e-3, atol=2e-4 * float(want_.abs().max()) + 1e-10,
                                   err_msg=name + " of 2^29 elements vs the sum of four chunks")
    del x, y, dy, xs, dys
    torch.cuda.empty_cache()
    # ConvTranspose2d(64 -> 3) at 507 x 128 x 128: the input is 507 * 2^14 * 256 bytes, just under 0x7F000000
    n = 507
    assert n * 128 * 128 * 64 * 4 < 0x7F000000 <= (n + 1) * 128 * 128 * 64 * 4
    tspec = ops.ConvSpec(True, 64, 3, 4, 2, 1)
    wt = torch.empty((64, 3, 4, 4), device=dev).uniform_(-0.1, 0.1, generator=g)
    b = torch.empty((3,), device=dev).uniform_(-1, 1, generator=g)
    x = torch.randn((n, 128, 128, 64), device=dev, generator=g)
    y, seen = launched(amd, lambda: ops.conv_forward(tspec, x, wt, b, 0))
    assert set(conv_labels(seen)) == {"convT_small|"}, seen
    w64, b64 = wt.cpu().double(), b.cpu().double()
    wins = [(i, oy // 2 * 2, ox // 2 * 2) for i, oy, ox in _windows(n, 256, 256, 64, 99)]
    _check_windows(y, wins, lambda i, oy, ox: _window_ref_convT(x, w64, b64, i, oy, ox), 3, "convT 64->3, 507 images")
    print("peak device memory: %.2f GiB" % (torch.cuda.max_memory_allocated() / 2**30))
    assert torch.cuda.max_memory_allocated() < (16 << 30)
