"""The references of tests/_small_kernel_ref.py against autograd and torch.optim in float64, so that the GPU tests of the
helper kernels (test_gpu_small_kernels.py) rest on checked formulas.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _small_kernel_ref as R

RTOL = 1e-12


def _close(name, got, want):
    err = float((got - want).abs().max())
    scale = max(float(want.abs().max()), 1e-300)
    assert err <= RTOL * scale, f"{name}: err {err:.3e} against a scale of {scale:.3e}"


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def test_float32_sum_is_sequential():
    """seq_sum in float32 is the running float32 sum of an explicit loop, bit for bit, along either axis; torch's CPU cumsum
    is not (it accumulates in double), which is why the reference does not use it."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3001, 5, generator=g)
    acc = np.zeros(5, dtype=np.float32)
    for row in x.numpy():
        acc = (acc + row).astype(np.float32)
    assert np.array_equal(R.seq_sum(x, 0).numpy(), acc)
    assert np.array_equal(R.seq_sum(x.t().contiguous(), 1).numpy(), acc)
    assert np.array_equal(R.seq_sum(x.t(), 1).numpy(), acc)                     # a strided view as well
    exact = x.double().sum(0)
    assert float((R.seq_sum(x, 0).double() - exact).abs().max()) > 4 * float((x.cumsum(0)[-1].double() - exact).abs().max())
    assert torch.equal(R.seq_sum(x.double(), 0), exact)


@pytest.mark.parametrize("n,hw,c", [(1, 1, 4), (3, 17, 8), (2, 64, 12)])
def test_instnorm_stats_matches_instance_norm(n, hw, c):
    g = torch.Generator().manual_seed(hw)
    x = _randn(g, n, hw, c) + 3.0
    mean, rstd = R.instnorm_stats(x, 1e-5)
    _close("mean", mean, x.mean(1))
    _close("rstd", rstd, 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5))
    if hw > 1:                                                                   # F.instance_norm refuses a single pixel
        want = F.instance_norm(x.permute(0, 2, 1), eps=1e-5).permute(0, 2, 1)
        _close("xhat", (x - mean[:, None]) * rstd[:, None], want)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("n,hw,c", [(1, 5, 4), (3, 17, 8), (2, 64, 12)])
def test_adain_closed_form_backward_is_autograd(n, hw, c, relu):
    g = torch.Generator().manual_seed(100 * hw + relu)
    x = (_randn(g, n, hw, c) * 1.5 + 0.5).requires_grad_(True)
    h = (_randn(g, n, 2 * c) * 0.5).requires_grad_(True)
    dy = _randn(g, n, hw, c)
    xhat = F.instance_norm(x.permute(0, 2, 1), eps=1e-5).permute(0, 2, 1)
    y = (1 + h[:, None, :c]) * xhat + h[:, None, c:]
    if relu:
        y = F.relu(y)
    y.backward(dy)
    mean, rstd = R.instnorm_stats(x.detach(), 1e-5)
    yr = R.adain_fwd(x.detach(), mean, rstd, h.detach(), relu)
    _close("y", yr, y.detach())
    dh, dx = R.adain_bwd(dy, yr if relu else None, x.detach(), mean, rstd, h.detach())
    _close("dh", dh, h.grad)
    _close("dx", dx, x.grad)


@pytest.mark.parametrize("numel,denom", [(1, 1), (5, 4), (1027, 771)])
@pytest.mark.parametrize("gscale", [None, 0.37])
def test_mse_gradient_is_autograd(numel, denom, gscale):
    g = torch.Generator().manual_seed(numel)
    a, b = _randn(g, numel).requires_grad_(True), _randn(g, numel)
    loss = ((a - b) ** 2).sum() / denom
    loss.backward(torch.tensor(1.0 if gscale is None else gscale, dtype=torch.float64))
    lr, gr = R.mse(a.detach(), b, denom, gscale)
    _close("loss", lr, loss.detach())
    _close("grad", gr, a.grad)
    total = R.stage1_total(lr, torch.tensor(0.75, dtype=torch.float64), 0.25)
    _close("total", total, loss.detach() + 0.25 * 0.75)


@pytest.mark.parametrize("mode", ["out", "diff", "both"])
def test_vq_backward_is_autograd(mode):
    g = torch.Generator().manual_seed(5)
    m, d, k = 129, 12, 37
    x = _randn(g, m, d).requires_grad_(True)
    embed_t = _randn(g, k, d)
    idx = torch.randint(0, k, (m,), generator=g)
    g_out = _randn(g, m, d) if mode != "diff" else None
    g_diff = _randn(g, 1)[0] if mode != "out" else None
    q = embed_t[idx]
    diff = ((q.detach() - x) ** 2).mean()                                        # vqvae.py:72
    out = x + (q - x).detach()                                                   # vqvae.py:73
    total = (out * g_out).sum() if g_out is not None else 0.0
    if g_diff is not None:
        total = total + diff * g_diff
    total.backward()
    _close("dx", R.vq_bwd(g_out, g_diff, x.detach(), q), x.grad)
    part = ((q - x.detach()) ** 2).sum(1)
    _close("diff", R.vq_loss(part, m, d), diff.detach())


@pytest.mark.parametrize("hyper", [(3e-4, 0.9, 0.999, 1e-8), (1e-2, 0.5, 0.9, 1e-3)])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_adam_is_torch_optim_adam(hyper, grad_scale):
    lr, b1, b2, eps = hyper
    g = torch.Generator().manual_seed(11)
    p0 = _randn(g, 257)
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([param], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(1, 6):
        grad = _randn(g, 257)
        grad[::7] = 0.0
        param.grad = grad * grad_scale
        opt.step()
        p, m, v = R.adam_step(p, grad, m, v, lr, b1, b2, eps, step, grad_scale)
        _close(f"p after step {step}", p, param.detach())
    state = opt.state[param]
    _close("m", m, state["exp_avg"])
    _close("v", v, state["exp_avg_sq"])


def test_colsum_is_sum():
    g = torch.Generator().manual_seed(2)
    x = _randn(g, 257, 12)
    assert torch.equal(R.colsum(x), x.sum(0))
