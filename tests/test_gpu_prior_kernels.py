"""GPU checks of the kernels at the two ends of the stage-2 prior (csrc/vq2_prior.hip): the one-hot convolution with its
shift and accumulate operand, its weight and bias gradient, the cross-entropy head, and the x2 upsample -- all against float64
torch on the values the GPU sees, bounded by 4 x the error of the same formula in float32 torch (ratios printed).  Where the
float32 formula is exact (a sum of one term), the GPU result has to be exact too."""
import glob
import os
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

import _pixelsnail_model_ref as M
import _pixelsnail_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def ceil4(c):
    return (c + 3) // 4 * 4


def to_dev_nhwc(t):
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, ceil4(c), dtype=torch.float32)
    out[..., :c] = t.permute(0, 2, 3, 1).float()
    return out.cuda()


def from_dev_nhwc(t, c):
    return t[..., :c].permute(0, 3, 1, 2).double().cpu()


def _bound(name, got, ref64, ref32):
    """err <= 4 x the float32 formula's error; returns that error (0: the formula is exact there and so must the GPU be)."""
    err = float((got.double() - ref64).abs().max())
    err32 = float((ref32.double() - ref64).abs().max())
    print("%s: err %.3e, fp32 torch %.3e, ratio %.2f" % (name, err, err32, err / err32 if err32 else float("inf") if err else 0.0))
    assert err <= 4 * err32, name
    return err32


# ----------------------------------------------------------------------------------------------- one-hot conv
GEOMS = [(2, 5, 1, 2, "down"), (3, 2, 2, 1, "right"), (1, 3, 0, 1, "down"), (2, 1, 1, 0, "right"), (3, 3, 1, 1, "none"),
         (7, 4, 6, 3, "none")]
IMAGES = [(2, 1, 1), (2, 3, 2), (2, 9, 8)]
CLASSES = [1, 6, 512, 513]
COUTS = [4, 6, 132, 256]


def _onehot_cases():
    out, i = [], 0
    for geom in GEOMS:
        for img in IMAGES:
            out.append((geom, img, CLASSES[i % 4], COUTS[(i // 2) % 4], i % 2 == 0, i % 3 == 0))
            i += 1
    return out


def _oid(c):
    (kh, kw, pt, pl, sh), (n, h, w), ncls, co, bias, acc = c
    return f"k{kh}x{kw}p{pt}_{pl}{sh}-{n}x{h}x{w}-{ncls}to{co}" + ("-bias" if bias else "") + ("-acc" if acc else "")


def _shift(y, sh):
    return M.shift_down(y) if sh == "down" else R.shift_right(y) if sh == "right" else y


def _onehot_reference(c, d, dtype):
    (kh, kw, pt, pl, sh), _, ncls, co, bias, acc = c
    w = d["w"].to(dtype).clone().requires_grad_(True)
    b = d["b"].to(dtype).clone().requires_grad_(True) if bias else None
    y = _shift(R.conv_at(M.one_hot(d["idx"], ncls, dtype), w, b, pt, pl), sh)
    if acc:
        y = y + d["acc"].to(dtype)
    y.backward(d["dy"].to(dtype))
    return {"y": y.detach(), "dw": w.grad, **({"db": b.grad} if bias else {})}


@pytest.mark.parametrize("case", _onehot_cases(), ids=_oid)
def test_onehot_conv_against_fp64(amd, case):
    ops = amd.ops
    (kh, kw, pt, pl, sh), (n, h, w), ncls, co, bias, acc = case
    g = torch.Generator().manual_seed(zlib.crc32(_oid(case).encode()))
    idx = torch.randint(0, ncls, (n, h, w), generator=g)
    if ncls >= 512:
        idx[0, 0, 0] = ncls - 1                                   # the last class occurs; most of the others do not
    d = {"idx": idx, "w": torch.randn(co, ncls, kh, kw, generator=g), "b": torch.randn(co, generator=g),
         "acc": torch.randn(n, co, h, w, generator=g), "dy": torch.randn(n, co, h, w, generator=g)}
    ref, ref32 = _onehot_reference(case, d, torch.float64), _onehot_reference(case, d, torch.float32)
    shift = (int(sh == "down"), int(sh == "right"))

    def run():
        wt = d["w"].cuda().requires_grad_(True)
        bt = d["b"].cuda().requires_grad_(True) if bias else None
        y = ops.onehot_conv(idx.cuda(), wt, bt, (kh, kw, pt, pl), shift, to_dev_nhwc(d["acc"]) if acc else None)
        y.backward(to_dev_nhwc(d["dy"]))
        torch.cuda.synchronize()
        return y.detach(), wt.grad, (bt.grad if bias else None)

    y, dw, db = run()
    assert y.shape == (n, h, w, ceil4(co)) and dw.shape == (co, ncls, kh, kw)
    assert float(y[..., co:].abs().sum()) == 0                                    # pad lanes
    if not acc:                                                                   # the row / column that entered: bias-free zeros
        assert float((y[:, :shift[0]].abs().sum() + y[:, :, :shift[1]].abs().sum())) == 0
    absent = torch.ones(ncls, dtype=torch.bool)
    absent[idx.unique()] = False
    assert float(dw[:, absent.cuda()].abs().sum()) == 0                           # classes that do not occur: exact zeros
    got = {"y": from_dev_nhwc(y, co), "dw": dw.cpu(), **({"db": db.cpu()} if bias else {})}
    errs = [_bound(f"{_oid(case)} {k}", got[k], ref[k].double(), ref32[k]) for k in got]
    degenerate = (h - shift[0]) * (w - shift[1]) == 0                             # every pixel was shifted in: all zeros
    exact_by_form = n * h * w <= 2 and not bias and not acc                       # single-term sums
    assert degenerate or exact_by_form or max(errs) > 0, "the float32 formula is exact for every tensor: the bound shows nothing"
    y2, dw2, db2 = run()
    assert torch.equal(y, y2) and torch.equal(dw, dw2) and (db is None or torch.equal(db, db2))


def test_onehot_conv_out_of_range_codes_contribute_nothing(amd):
    ops = amd.ops
    g = torch.Generator().manual_seed(9)
    ncls, co = 6, 8
    idx = torch.randint(0, ncls, (2, 5, 4), generator=g)
    bad = idx.clone()
    bad[0, 2, 1], bad[1, 0, 0], bad[1, 4, 3] = -1, ncls, 2 ** 40
    w = torch.randn(co, ncls, 3, 3, generator=g)
    dy = torch.randn(2, co, 5, 4, generator=g)
    oh = M.one_hot(idx, ncls, torch.float64)
    oh[0, :, 2, 1] = 0
    oh[1, :, 0, 0] = 0
    oh[1, :, 4, 3] = 0
    wr = w.double().requires_grad_(True)
    yr = R.conv_at(oh, wr, None, 1, 1)
    yr.backward(dy.double())
    wt = w.cuda().requires_grad_(True)
    y = ops.onehot_conv(bad.cuda(), wt, None, (3, 3, 1, 1))
    y.backward(to_dev_nhwc(dy))
    torch.cuda.synchronize()
    assert float((from_dev_nhwc(y, co) - yr.detach()).abs().max()) <= 1e-5
    assert float((wt.grad.double().cpu() - wr.grad).abs().max()) <= 1e-5


def test_onehot_conv_refusals(amd):
    ops = amd.ops
    idx = torch.zeros(1, 2, 2, dtype=torch.int64, device="cuda")
    for shape, geom in (((4, 2, 8, 1), (8, 1, 0, 0)), ((4, 2, 6, 6), (6, 6, 0, 0)), ((4, 16385, 1, 1), (1, 1, 0, 0))):
        with pytest.raises(NotImplementedError):
            ops.onehot_conv(idx, torch.zeros(shape, device="cuda"), None, geom)
    with pytest.raises(RuntimeError):
        ops.onehot_conv(idx.int(), torch.zeros(4, 2, 1, 1, device="cuda"), None, (1, 1, 0, 0))


# ----------------------------------------------------------------------------------------------- cross-entropy
def _xent_reference(logits, target, dtype):
    x = logits.to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(x, target)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("offset", [0.0, 80.0], ids=["plain", "offset80"])
@pytest.mark.parametrize("ncls", [2, 6, 512, 513])
@pytest.mark.parametrize("m", [1, 3, 257])
def test_cross_entropy_against_fp64(amd, m, ncls, offset):
    g = torch.Generator().manual_seed(1000 * m + ncls + int(offset))
    logits = torch.randn(1, ncls, m, 1, generator=g)
    if offset:
        logits = (logits + offset * (torch.randint(0, 2, (1, 1, m, 1), generator=g) * 2 - 1)).float()
    target = torch.randint(0, ncls, (1, m, 1), generator=g)
    l64, g64 = _xent_reference(logits, target, torch.float64)
    l32, g32 = _xent_reference(logits, target, torch.float32)
    hits = int((M.cross_entropy(logits.double(), target)[1] * m).round())

    def run():
        x = to_dev_nhwc(logits).requires_grad_(True)
        out = amd.ops.from_nhwc(x, ncls)
        ptr = x.data_ptr()
        loss, acc, count = amd.ops.prior_loss(out, target.cuda(), return_count=True)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), acc, count, x.grad, ptr

    loss, acc, count, dx, _ = run()
    assert loss.dim() == 0 and acc.dim() == 0
    assert int(count) == hits and float(acc) == float(torch.tensor(float(hits)) / m)
    assert float(dx[..., ncls:].abs().sum()) == 0
    e1 = _bound(f"xent loss M={m} C={ncls} off={offset}", loss.cpu(), l64, l32)
    e2 = _bound(f"xent dlogits M={m} C={ncls} off={offset}", from_dev_nhwc(dx, ncls), g64, g32)
    assert max(e1, e2) > 0
    loss2, acc2, count2, dx2, _ = run()
    assert torch.equal(loss, loss2) and torch.equal(dx, dx2) and int(count2) == hits


def test_cross_entropy_reads_the_channels_last_view_in_place(amd):
    x = torch.randn(2, 3, 5, 8, device="cuda")                       # NHWC, 8 classes
    out = amd.ops.from_nhwc(x, 8)
    assert out.shape == (2, 8, 3, 5) and out.data_ptr() == x.data_ptr()
    v = amd.ops.to_nhwc(out)
    assert v.data_ptr() == x.data_ptr() and v.shape == x.shape
    loss, acc = amd.prior_loss(out, torch.randint(0, 8, (2, 3, 5), device="cuda"))
    assert bool(torch.isfinite(loss)) and 0.0 <= float(acc) <= 1.0


def test_cross_entropy_tie_goes_to_the_lowest_index(amd):
    logits = torch.zeros(1, 513, 4, 1)
    logits[0, 100, 0] = logits[0, 300, 0] = 2.0            # tie across lanes: 100 wins
    logits[0, 7, 1] = logits[0, 6, 1] = 1.0                # tie inside one lane's group: 6 wins
    logits[0, 512, 2] = logits[0, 256, 2] = 3.0            # tie between a lane's first and a later pass: 256 wins
    target = torch.tensor([[[100], [7], [256], [0]]])      # row 3: all equal, 0 wins
    _, acc, count = amd.ops.prior_loss(amd.ops.from_nhwc(to_dev_nhwc(logits), 513), target.cuda(), return_count=True)
    assert int(count) == 3 and float(acc) == 0.75
    target = torch.tensor([[[300], [6], [512], [1]]])
    _, _, count = amd.ops.prior_loss(amd.ops.from_nhwc(to_dev_nhwc(logits), 513), target.cuda(), return_count=True)
    assert int(count) == 1


def test_cross_entropy_out_of_range_target_is_skipped(amd):
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(1, 6, 5, 1, generator=g)
    target = torch.tensor([[[1], [-1], [6], [3], [2 ** 40]]])
    x = to_dev_nhwc(logits).requires_grad_(True)
    loss, acc = amd.prior_loss(amd.ops.from_nhwc(x, 6), target.cuda())
    loss.backward()
    keep = torch.tensor([0, 3])
    want = F.cross_entropy(logits.double()[:, :, keep], target[:, keep], reduction="sum") / 5
    assert abs(float(loss) - float(want)) <= 1e-6
    assert float(x.grad[0, [1, 2, 4]].abs().sum()) == 0 and float(x.grad[0, [0, 3]].abs().sum()) > 0


# ----------------------------------------------------------------------------------------------- upsample
@pytest.mark.parametrize("c", [4, 6, 132])
@pytest.mark.parametrize("img", [(2, 1, 1), (2, 3, 2)])
def test_upsample(amd, c, img):
    n, h, w = img
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(n, c, h, w, generator=g)
    dy = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    xd = to_dev_nhwc(x).requires_grad_(True)
    y = amd.ops.Upsample2Fn.apply(xd, c)
    y.backward(to_dev_nhwc(dy))
    torch.cuda.synchronize()
    assert y.shape == (n, 2 * h, 2 * w, ceil4(c))
    assert float(y[..., c:].abs().sum()) == 0 and float(xd.grad[..., c:].abs().sum()) == 0
    assert torch.equal(from_dev_nhwc(y, c), F.interpolate(x, scale_factor=2).double())        # a copy: exact
    x64 = x.double().requires_grad_(True)
    F.interpolate(x64, scale_factor=2).backward(dy.double())
    x32 = x.clone().requires_grad_(True)
    F.interpolate(x32, scale_factor=2).backward(dy)
    assert _bound(f"upsample bwd C={c} {img}", from_dev_nhwc(xd.grad, c), x64.grad, x32.grad) > 0


# ----------------------------------------------------------------------------------------------- registers
def test_prior_kernels_do_not_spill():
    """The compiler's resource report of csrc/vq2_prior.hip (written by csrc/build.sh): no spilled register and no scratch
    in any of its kernels."""
    files = glob.glob(os.path.join(ROOT, "vq-vae-2-pytorch_amd", "csrc", "_obj", "vq2_prior.res"))
    assert files, "csrc/_obj/vq2_prior.res is missing: csrc/build.sh lists vq2_prior and writes the report with the object"
    hot = re.compile(r"onehot_pack_kernel|onehot_conv_fwd_kernel|onehot_wgrad_kernel|onehot_bgrad_partial_kernel|"
                     r"onehot_bgrad_final_kernel|xent_rows_kernel|xent_reduce_kernel|xent_bwd_kernel|upsample2_fwd_kernel|"
                     r"upsample2_bwd_kernel")
    seen, name = 0, None
    for line in open(files[0]):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen += bool(hot.search(name))
            continue
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name and hot.search(name):
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
    assert seen == 10, f"{seen} kernels found in the report, expected 10"
