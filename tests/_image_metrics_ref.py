"""fp64 numpy restatement of the image metrics of include/vq2.h (vq2_image_metrics), from bytes: the exact integer
squared error, SSIM after Wang et al. 2004 with an 11x11 Gaussian window of sigma 1.5 over the valid region and data
range 255, and PSNR.  Shared by test_image_metrics_cpu.py and test_gpu_image_metrics.py; the kernel is never its source."""
import math

import numpy as np

WIN = 11
C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2


def gaussian():
    g = np.exp(-(np.arange(WIN, dtype=np.float64) - WIN // 2) ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def sse_u8(a, b):
    """int64 [N]: sum over H, W, C of (a - b)^2 of uint8 [N,H,W,C] arrays."""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return (d * d).reshape(d.shape[0], -1).sum(1)


def _ssim_map(mua, mub, eaa, ebb, eab):
    va, vb, cov = eaa - mua * mua, ebb - mub * mub, eab - mua * mub
    return ((2 * (mua * mub) + C1) * (2 * cov + C2)) / ((mua * mua + mub * mub + C1) * (va + vb + C2))


def _separable(x, g):
    """x float64 [N,H,W,C] -> [N,H-10,W-10,C]: the window along rows (W), then along columns (H)."""
    h, w = x.shape[1], x.shape[2]
    t = sum(g[k] * x[:, :, k:k + w - WIN + 1] for k in range(WIN))
    return sum(g[k] * t[:, k:k + h - WIN + 1] for k in range(WIN))


def ssim_map_u8(a, b):
    a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    assert a.shape == b.shape and a.ndim == 4 and a.shape[1] >= WIN and a.shape[2] >= WIN
    g = gaussian()
    return _ssim_map(_separable(a, g), _separable(b, g), _separable(a * a, g), _separable(b * b, g), _separable(a * b, g))


def ssim_u8(a, b):
    """float64 [N]: mean of the SSIM map over positions and channels, uint8 [N,H,W,C] inputs."""
    m = ssim_map_u8(a, b)
    return m.reshape(m.shape[0], -1).mean(1)


def ssim_u8_2d(a, b):
    """The same from the 2-D window g x g through scipy.signal.correlate2d (valid): independent of _separable."""
    from scipy.signal import correlate2d
    a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    g = gaussian()
    w2 = np.outer(g, g)

    def f(x):
        return np.stack([np.stack([correlate2d(x[n, :, :, c], w2, mode="valid") for c in range(x.shape[3])], -1)
                         for n in range(x.shape[0])])

    m = _ssim_map(f(a), f(b), f(a * a), f(b * b), f(a * b))
    return m.reshape(m.shape[0], -1).mean(1)


def mse_u8(sse_total, elements):
    return float(sse_total) / float(elements)


def psnr(sse_total, elements):
    """10 log10(255^2 / mse) in dB; inf when the images are identical."""
    if int(sse_total) == 0:
        return float("inf")
    return 10.0 * math.log10(255.0 ** 2 / mse_u8(sse_total, elements))
