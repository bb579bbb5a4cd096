"""tests/_resblock_ref.py without a GPU: its explicit-mask backward is the gradient of the module the kernels implement
(vqvae.py:81-96), its "integer" operands are exact in float32, and the tolerance of tests/test_gpu_resblock.py bites -- plain
float32 torch meets it, a computation with one product, one mask bit or one pixel wrong does not."""
import pytest
import torch
import torch.nn.functional as Fn

import _resblock_ref as R

BITE_SHAPES = [(1, 9, 17), (1, 4, 64)]       # one direct, one Winograd-eligible (both in R.CASES)


@pytest.mark.parametrize("shape", [(2, 9, 17), (1, 4, 64)], ids=lambda s: "%dx%dx%d" % s)
def test_backward_formulas_are_the_autograd_of_the_module(shape):
    """relu -> conv3x3 -> relu -> conv1x1 -> + x in float64 autograd against bwd() with r taken from fwd(): 1e-12, away from
    the zeros of the two ReLUs (|pre-activation| > 1e-3)."""
    n, h, w = shape
    d = R.operands("auto", n, h, w, "normal")
    f8 = torch.float64
    x = d["x"].to(f8).permute(0, 3, 1, 2).clone().requires_grad_(True)
    w1, b1, w2, b2 = (d[k].to(f8).clone().requires_grad_(True) for k in ("w1", "b1", "w2", "b2"))
    pre = Fn.conv2d(Fn.relu(x), w1, b1, padding=1)
    pre.retain_grad()
    y = Fn.conv2d(Fn.relu(pre), w2, b2) + x
    y.backward(d["g"].to(f8).permute(0, 3, 1, 2))
    r, y_ref = R.fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], False)
    assert torch.equal(r, Fn.relu(pre).detach().permute(0, 2, 3, 1)) and torch.equal(y_ref, y.detach().permute(0, 2, 3, 1))
    dh, dx, dw2, db2 = R.bwd(d["g"], r, d["x"], d["w1"], d["w2"])
    far_h = (pre.detach().abs() > 1e-3).permute(0, 2, 3, 1)
    far_x = d["x"].abs() > 1e-3
    assert float(far_h.float().mean()) > 0.99 and float(far_x.float().mean()) > 0.99
    for name, got, want, keep in (("dh", dh, pre.grad.permute(0, 2, 3, 1), far_h), ("dx", dx, x.grad.permute(0, 2, 3, 1), far_x),
                                  ("dw2", dw2, w2.grad, None), ("db2", db2, b2.grad, None)):
        err = (got - want).abs()
        err = float((err[keep] if keep is not None else err).max())
        assert tuple(got.shape) == tuple(want.shape) and err <= 1e-12 * max(1.0, float(want.abs().max())), (name, err)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_integer_operands_stay_exact_in_float32(c):
    n, h, w, _ = c
    d = R.operands("rb", n, h, w, "integer")
    for k, v in d.items():
        assert torch.equal(v, v.round()), k
    assert float(d["x"].abs().max()) <= 2 and float(d["g"].abs().max()) <= 2 and float(d["w1"].abs().max()) <= 1
    if n * h * w >= 64:
        assert bool((d["x"] == 0).any()) and 0.3 < float((d["r"] == 0).float().mean()) < 0.8
    bounds = R.integer_bounds(d)
    assert set(bounds) == {"r", "r_wino", "y", "dh", "dx", "dw2", "db2"}
    for k, v in bounds.items():
        assert v < 2 ** 23, (k, v)
    # and plain float32 torch does reproduce float64 bit for bit on them
    r8, y8 = R.fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], True)
    r4, y4 = R.fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], True, torch.float32)
    assert torch.equal(r4.double(), r8) and torch.equal(y4.double(), y8)
    for a, b in zip(R.bwd(d["g"], d["r"], d["x"], d["w1"], d["w2"], torch.float32), R.bwd(d["g"], d["r"], d["x"], d["w1"], d["w2"])):
        assert torch.equal(a.double(), b)


def test_image_n_does_not_depend_on_the_batch_size():
    a, b = R.operands("rb", 2, 3, 5, "normal"), R.operands("rb", 11, 3, 5, "normal")
    for k in ("x", "g", "r"):
        assert torch.equal(a[k], b[k][:2]), k
    for k in ("w1", "b1", "w2", "b2"):
        assert torch.equal(a[k], b[k]), k
    assert 0.4 < float((b["r"] == 0).float().mean()) < 0.6


def _all(d, dtype, relu_out=False):
    r, y = R.fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], relu_out, dtype)
    dh, dx, dw2, db2 = R.bwd(d["g"], d["r"], d["x"], d["w1"], d["w2"], dtype)
    return {"r": r, "y": y, "dh": dh, "dx": dx, "dw2": dw2, "db2": db2}


@pytest.mark.parametrize("shape", BITE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_tolerance_bites(shape):
    """_bites of tests/test_gpu_dispatch.py for this family: intact float32 passes the comparison with float64; each corruption
    fails it on every output it reaches."""
    n, h, w = shape
    assert shape in [c[:3] for c in R.CASES]
    d = R.operands("rb", n, h, w, "normal")
    ref = _all(d, torch.float64)
    tol = R.tolerances(ref)
    good = _all(d, torch.float32)
    for k in ref:
        assert not R.differs(good[k], ref[k], tol[k]), k + ": plain fp32 itself misses the tolerance"

    def corrupted(**changed):
        return _all(dict(d, **changed), torch.float32)

    w1 = d["w1"].clone()
    w1[CM_HALF, C_HALF, 1, 1] = 0                  # one tap of one (co, ci) pair of the 3x3
    w2 = d["w2"].clone()
    w2[C_HALF, CM_HALF, 0, 0] = 0                                    # one (co, cm) of the 1x1
    # a pixel of the first tile's halo (row 8 / column 16 are outside an 8 x 16 tile at the origin), one channel that is 0
    py, px = (8, 16) if h > 8 else (h - 1, 16)
    cm = int((d["r"][0, py, px] == 0).nonzero()[0])
    r = d["r"].clone()
    r[0, py, px, cm] = 1.0                                           # ... treated as positive
    g = d["g"].clone()
    g[n - 1, h // 2, w // 2] = 0                                     # one pixel of g dropped
    for what, bad, reached in (("w1 tap", corrupted(w1=w1), ("r", "y", "dx")), ("w2 entry", corrupted(w2=w2), ("y", "dh")),
                               ("r halo mask", corrupted(r=r), ("dx",)), ("g pixel", corrupted(g=g), ("dw2", "db2"))):
        for k in reached:
            assert R.differs(bad[k], ref[k], tol[k]), "%s: the tolerance of %s does not notice it" % (what, k)


CM_HALF, C_HALF = R.CM // 2, R.C // 2
