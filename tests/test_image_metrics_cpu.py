"""No GPU: the fp64 reference of the image metrics against an independent 2-D form and against values known in closed
form, PSNR on hand values, and the host layer (the Evaluator's argument check, the new entry points' bindings)."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import _image_metrics_ref as R


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _pairs():
    g = np.random.default_rng(11)
    a = g.integers(0, 256, (2, 23, 31, 3), dtype=np.uint8)
    b = g.integers(0, 256, (2, 23, 31, 3), dtype=np.uint8)
    noisy = np.clip(a.astype(np.int64) + g.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    ramp = (np.arange(23 * 31 * 3, dtype=np.int64).reshape(1, 23, 31, 3) * 7 % 256).astype(np.uint8)
    ramp = np.concatenate([ramp, ramp[:, ::-1]], 0)
    flat = np.full((2, 23, 31, 3), 255, dtype=np.uint8)
    return {"random": (a, b), "noisy copy": (a, noisy), "ramp": (ramp, ramp[::-1].copy()), "255 vs 254": (flat, flat - 1)}


def test_separable_reference_agrees_with_the_two_dimensional_window():
    for name, (a, b) in _pairs().items():
        s, s2 = R.ssim_u8(a, b), R.ssim_u8_2d(a, b)
        print(name, s, np.abs(s - s2).max())
        assert s.shape == (2,) and np.abs(s - s2).max() <= 1e-12, name


def test_known_values():
    shape = (1, 13, 17, 2)
    for p, q in ((0, 0), (255, 254), (10, 200), (255, 0), (128, 128)):
        a, b = np.full(shape, p, dtype=np.uint8), np.full(shape, q, dtype=np.uint8)
        want = (2.0 * p * q + R.C1) / (p * p + q * q + R.C1)
        assert abs(R.ssim_u8(a, b)[0] - want) <= 1e-12, (p, q)
    g = np.random.default_rng(3)
    a = g.integers(0, 256, (3, 19, 12, 3), dtype=np.uint8)
    b = g.integers(0, 256, (3, 19, 12, 3), dtype=np.uint8)
    assert np.all(R.ssim_u8(a, a) == 1.0) and np.all(R.ssim_map_u8(a, a) == 1.0)
    assert np.abs(R.ssim_u8(a, b) - R.ssim_u8(b, a)).max() <= 1e-12
    assert np.array_equal(R.sse_u8(a, b), R.sse_u8(b, a)) and not R.sse_u8(a, a).any()
    one = R.ssim_map_u8(a[:, :11, :11], b[:, :11, :11])
    assert one.shape == (3, 1, 1, 3)                          # an 11x11 image has exactly one window position
    w2 = np.outer(R.gaussian(), R.gaussian())[None, :, :, None]
    x, y = a[:, :11, :11].astype(np.float64), b[:, :11, :11].astype(np.float64)
    mx, my = (w2 * x).sum((1, 2)), (w2 * y).sum((1, 2))
    vx, vy, cxy = (w2 * x * x).sum((1, 2)) - mx * mx, (w2 * y * y).sum((1, 2)) - my * my, (w2 * x * y).sum((1, 2)) - mx * my
    want = ((2 * mx * my + R.C1) * (2 * cxy + R.C2)) / ((mx * mx + my * my + R.C1) * (vx + vy + R.C2))
    assert np.abs(one[:, 0, 0] - want).max() <= 1e-12
    assert abs(R.gaussian().sum() - 1.0) <= 1e-15 and abs(R.C1 - 6.5025) < 1e-12 and abs(R.C2 - 58.5225) < 1e-12
    with pytest.raises(AssertionError):
        R.ssim_u8(a[:, :10], b[:, :10])


def test_psnr_on_hand_values(amd):
    assert R.psnr(0, 100) == math.inf and amd.psnr_from_mse_u8(0.0) == math.inf
    a = np.zeros((1, 11, 11, 3), dtype=np.uint8)
    sse = int(R.sse_u8(a, a + 1)[0])
    assert sse == a.size and R.mse_u8(sse, a.size) == 1.0
    assert abs(R.psnr(sse, a.size) - 20 * math.log10(255)) <= 1e-12
    assert abs(amd.psnr_from_mse_u8(1.0) - 20 * math.log10(255)) <= 1e-12
    assert abs(R.psnr(255 * 255 * 10, 10)) <= 1e-12           # black against white: 0 dB
    assert amd.psnr_from_mse_u8(4.0) == R.psnr(40, 10)


def test_host_layer(amd):
    model = amd.VQVAE()                                       # on the CPU: the constructor check needs no device
    with pytest.raises(TypeError, match="image_metrics"):
        amd.Evaluator(model, None, image_metrics=True)
    ev = amd.Evaluator(model, amd.ImageNormalizer(layout="hwc"), image_metrics=True)
    assert ev.image_metrics and not amd.Evaluator(model).image_metrics
    assert list(inspect.signature(amd.Evaluator.__init__).parameters) == ["self", "model", "normalizer", "image_metrics"]
    assert list(inspect.signature(amd.Stage1Trainer.evaluate_image_metrics).parameters) == ["self", "batches", "sample"]
    x = torch.zeros(1, 11, 11, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        amd.ops.image_metrics(x, x, 3, (2.0,) * 3, (0.5,) * 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        amd.ops.image_metrics_accumulate(torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.float64),
                                         torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.float64))


def test_entry_points_are_bound_and_refuse_bad_arguments(amd):
    P, I32, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t
    FP = ctypes.POINTER(ctypes.c_float)
    want = {"vq2_image_metrics_workspace_bytes": (SZ, [I32, I32, I32, I32]),
            "vq2_image_metrics": (ctypes.c_int, [P, I32, P, I32, I32, I32, I32, I32, FP, FP, P, P, P, SZ, P]),
            "vq2_image_metrics_accumulate": (ctypes.c_int, [P, P, I32, P, P, P])}
    L = amd._lib.lib
    for name, (res, args) in want.items():
        assert name in amd._lib.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert amd._lib.API_VERSION >= 7
    # one (double, int64) pair per 32x32 tile of window positions and image; the tiling does not depend on N
    ws = L.vq2_image_metrics_workspace_bytes
    assert ws(1, 3, 11, 11) == 16 and ws(1, 3, 42, 42) == 16 and ws(1, 3, 43, 42) == 32 and ws(1, 3, 43, 43) == 64
    assert ws(9, 3, 256, 256) == 9 * 64 * 16 and ws(5, 1, 256, 256) == 5 * 64 * 16
    assert ws(1, 3, 10, 64) == 0 and ws(1, 5, 64, 64) == 0 and ws(65536, 3, 64, 64) == 0 and ws(0, 3, 64, 64) == 0
    # refusals come before any launch (no GPU here)
    backing = ctypes.create_string_buffer(4096 + 16)
    dummy = ctypes.c_void_p((ctypes.addressof(backing) + 15) & ~15)
    one = (ctypes.c_float * 4)(2.0, 2.0, 2.0, 2.0)
    zero = (ctypes.c_float * 4)(2.0, 0.0, 2.0, 2.0)

    def call(lda=4, ldb=4, n=1, c=3, h=16, w=16, inv_s=one, nbytes=4096, a=dummy):
        return L.vq2_image_metrics(a, lda, dummy, ldb, n, c, h, w, inv_s, one, dummy, dummy, dummy, nbytes, None)

    assert call(a=None) == 1 and b"null pointer" in L.vq2_last_error()
    assert call(h=10) == 1 and b"10x16" in L.vq2_last_error()
    assert call(w=10) == 1 and b"16x10" in L.vq2_last_error()
    assert call(c=5) == 1 and call(c=0) == 1 and call(n=0) == 1 and call(n=65536) == 1
    assert call(lda=2) == 1 and call(ldb=2) == 1 and b"stride" in L.vq2_last_error()
    assert call(inv_s=zero) == 1 and b"inv_s[1]" in L.vq2_last_error()
    assert call(nbytes=8) == 3                                # VQ2_ERR_WORKSPACE
    assert L.vq2_image_metrics_accumulate(None, None, 1, None, None, None) == 1
    assert L.vq2_image_metrics_accumulate(dummy, dummy, 0, dummy, dummy, None) == 1
