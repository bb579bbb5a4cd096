"""numpy references for tests/test_gpu_optim_extras.py: the global gradient norm and clip coefficient of vq2_grad_norm, the
clipped / averaged Adam step of vq2_adam_step_ex and the averaging recurrence, each as ONE formula evaluated in the dtype of
its array arguments -- float64 is the reference, float32 (every scalar rounded once, as the kernel receives it) is the
yardstick whose own distance from float64 bounds the kernel's."""
import math

import numpy as np


def grad_norm(g, grad_scale):
    """sqrt(sum (g[i] * grad_scale)^2): the product in float32 as the kernel forms it, squares and sum in float64."""
    a = np.asarray(g, dtype=np.float32) * np.float32(grad_scale)
    a = a.astype(np.float64)
    return math.sqrt(float(np.sum(a * a))) if np.isfinite(a).all() else float("nan")


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient in float64."""
    return min(1.0, max_norm / (norm + 1e-6))


def one_ulp(got, want):
    """|got - want| <= the float32 spacing at want, got a float32 value, want a float64."""
    got, want = float(got), float(want)
    return abs(got - want) <= float(np.spacing(np.float32(abs(want))))


def adam_ex(p, g, m, v, avg, lr, beta1, beta2, eps, step, grad_scale=1.0, coef=1.0, avg_decay=None):
    """One step on (g * grad_scale) * coef in the arrays' dtype -> (p, m, v, avg); avg / avg_decay None: no average."""
    dt = p.dtype
    c = lambda x: dt.type(x)
    gi = (g * c(grad_scale)) * c(coef)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    m = m + c(1.0 - beta1) * (gi - m)
    v = v * c(beta2) + (c(1.0 - beta2) * gi) * gi
    denom = np.sqrt(v) / c(math.sqrt(bc2)) + c(eps)
    p = p + c(-(lr / bc1)) * (m / denom)
    if avg is not None:
        avg = avg + c(1.0 - avg_decay) * (p - avg)
    return p, m, v, avg


def ema(states, start, decay):
    """avg_k = avg_{k-1} + (1 - decay) * (p_k - avg_{k-1}) over the recorded parameter states, in their dtype."""
    dt = start.dtype
    avg = start.copy()
    for p in states:
        avg = avg + dt.type(1.0 - decay) * (p - avg)
    return avg


def bound(name, got, ref64, ref32):
    """The rule of _bound in tests/test_gpu_small_kernels.py: max abs error against float64 <= 4 x the error of the float32
    formula against float64 (0: the formula is exact there and so must the kernel be).  Returns the float32 error."""
    err = float(np.abs(np.asarray(got, dtype=np.float64) - ref64).max())
    err32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    print("%s: err %.3e, fp32 reference %.3e, ratio %.2f" % (name, err, err32, err / err32 if err32 else float("inf") if err else 0.0))
    assert err <= 4 * err32, name
    return err32
