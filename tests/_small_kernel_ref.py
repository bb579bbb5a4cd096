"""Plain torch references of the HBM-bound helper kernels (include/vq2.h: AdaIN, loss + optimizer, the small Quantize
kernels, vq2_colsum), usable in float64 and in float32.  TEST INFRASTRUCTURE, CPU only.

The float64 variant is the yardstick.  The float32 variant is the same formula with every operation rounded to float32 and
every sum taken strictly left to right, so its distance from float64 is what a plain sequential float32 evaluation costs: the
GPU tests allow a kernel 4 x that distance.  Scalars enter the way the entry points form them (a reciprocal or a step size
computed in double on the host, then one float32 factor), so that an elementwise kernel and its float32 reference round at the
same places and the comparison measures summation order and indexing, not the spelling of a constant.

Left to right in float32 is numpy's accumulate.  torch's own CPU cumsum accumulates float32 input in double
(test_small_kernel_ref_cpu.py::test_float32_sum_is_sequential shows both), which would make the float32 reference as good as
float64 and the bound meaningless."""
import math

import numpy as np
import torch


def seq_sum(t, dim):
    """Sum over `dim`: torch.sum in float64; in float32 a running float32 sum in index order."""
    if t.dtype == torch.float64:
        return t.sum(dim)
    assert t.dtype == torch.float32
    run = np.cumsum(t.contiguous().numpy(), axis=dim, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(np.take(run, -1, axis=dim)))


# ------------------------------------------------------------------------------------------------ AdaIN
def instnorm_stats(x, eps):
    """x [N, HW, C] -> mean, rstd [N, C]: biased variance, rstd = 1 / sqrt(var + eps), two passes."""
    inv = 1.0 / x.shape[1]
    mean = seq_sum(x, 1) * inv
    d = x - mean[:, None]
    var = seq_sum(d * d, 1) * inv
    return mean, 1.0 / torch.sqrt(var + eps)


def adain_fwd(x, mean, rstd, h, relu):
    """y = [relu]((1 + gamma) * ((x - mean) * rstd) + beta), h [N, 2C] = (gamma | beta)."""
    c = x.shape[2]
    y = (1.0 + h[:, None, :c]) * ((x - mean[:, None]) * rstd[:, None]) + h[:, None, c:]
    return torch.where(y > 0, y, torch.zeros_like(y)) if relu else y


def adain_bwd(dy, y, x, mean, rstd, h):
    """dz = dy * (y > 0) (y None: no ReLU); dh [N, 2C] = (sum_p dz * xhat | sum_p dz);
    dx = rstd * (1 + gamma) * (dz - mean_p dz - xhat * mean_p(dz * xhat))."""
    c = x.shape[2]
    inv = 1.0 / x.shape[1]
    dz = dy if y is None else torch.where(y > 0, dy, torch.zeros_like(dy))
    xhat = (x - mean[:, None]) * rstd[:, None]
    sb = seq_sum(dz, 1)
    sg = seq_sum(dz * xhat, 1)
    dx = (rstd * (1.0 + h[:, :c]))[:, None] * (dz - (sb * inv)[:, None] - xhat * (sg * inv)[:, None])
    return torch.cat([sg, sb], 1), dx


# ------------------------------------------------------------------------------------------------ loss
def mse(a, b, denom, gscale=None):
    """loss = sum((a - b)^2) / denom over flat operands, grad = gscale * 2 * (a - b) / denom (gscale None: 1)."""
    d = a - b
    loss = seq_sum(d * d, 0) / denom
    coef = torch.tensor(2.0 / denom, dtype=a.dtype)
    if gscale is not None:
        coef = coef * torch.as_tensor(gscale, dtype=a.dtype)
    return loss, coef * d


def stage1_total(recon, latent, weight):
    """recon + weight * latent (train_vqvae.py:85); weight is a float32 argument of the entry point."""
    return recon + torch.tensor(weight, dtype=torch.float32).to(recon.dtype) * latent


# ------------------------------------------------------------------------------------------------ Adam
def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """One step of torch.optim.Adam (single-tensor form: lerp, addcmul, addcdiv; no weight decay, no amsgrad) on
    g * grad_scale.  Returns the new (p, m, v)."""
    g = g * grad_scale
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    m = m + (1.0 - beta1) * (g - m)
    v = v * beta2 + ((1.0 - beta2) * g) * g
    denom = torch.sqrt(v) / math.sqrt(bc2) + eps
    return p + (-(lr / bc1)) * (m / denom), m, v


# ------------------------------------------------------------------------------------------------ Quantize
def vq_bwd(g_out, g_diff, x, e):
    """dx = g_out + (2 / (M * D)) * g_diff * (x - e), e [M, D] the selected code rows; g_out / g_diff None: absent."""
    dx = torch.zeros_like(x) if g_out is None else g_out.clone()
    if g_diff is not None:
        dx = dx + (g_diff * (1.0 / x.numel())) * (2.0 * (x - e))
    return dx


def vq_loss(partials, m, d):
    """diff = sum(partials) / (M * D)."""
    return seq_sum(partials, 0) / float(m * d)


def colsum(x):
    """x [rows, C] -> [C]."""
    return seq_sum(x, 0)
