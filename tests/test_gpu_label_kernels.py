"""GPU checks of the three class-label kernels of csrc/vq2_gated.hip (vq2_glu_res_label_fwd, vq2_glu_res_label_bwd,
vq2_label_embed_grad), called through the C entry points against the float64 formulas of _label_cond_ref.py.

The bar is the elementwise kernels' own (test_gpu_gated_resblock.py): the error against float64 is at most 4 x the error of
the same formula in float32 torch; ratios are printed.  Shapes: Ch 3 (unaligned second half), 4 (one 16-byte group), 6, 256
(the real width); 1, 3, 5 images of 1, 3, 1024 pixels (never a multiple of the 256-thread workgroup's items except where the
image is one); pixel strides larger than ceil4; labels that repeat, labels no image has, and -1 / n_label (out of range).
Every cell a kernel must not read holds NaN (table rows of unused labels included), every cell it must not write is checked."""
import ctypes

import pytest
import torch

import _label_cond_ref as LR

pytestmark = pytest.mark.gpu

N_LABEL = 5
LABELS = {1: [1], 3: [-1, 2, 2], 5: [1, -1, 1, N_LABEL, 3]}      # 5 images: 1 repeats, 0 / 2 / 4 unused, two out of range


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def ceil4(c):
    return (c + 3) // 4 * 4


def P(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset * t.element_size())


def _poisoned(vals, extra):
    """[rows, c] values in a device buffer of row stride ceil4(c) + extra; every other lane holds NaN."""
    rows, c = vals.shape
    buf = torch.full((rows, ceil4(c) + extra), float("nan"))
    buf[:, :c] = vals
    return buf.cuda()


def _nan(rows, ld):
    return torch.full((rows, ld), float("nan"), device="cuda")


def _bits(t):
    return t.view(torch.int32).clone()


def _bound(name, got, ref64, ref32):
    err = float((got.double() - ref64).abs().max())
    err32 = float((ref32.double() - ref64).abs().max())
    print("%s: err %.3e, fp32 torch %.3e, ratio %.2f" % (name, err, err32, err / err32 if err32 else float("inf") if err else 0.0))
    assert err <= 4 * err32, name


def _check_rows(buf, c, what):
    """pad lanes are exactly 0, lanes beyond ceil4(c) untouched (NaN)"""
    assert not bool(torch.isnan(buf[:, :c]).any()), what
    assert float(buf[:, c:ceil4(c)].abs().sum()) == 0, what
    assert bool(torch.isnan(buf[:, ceil4(c):]).all()), what


@pytest.mark.parametrize("ppi", [1, 3, 1024])
@pytest.mark.parametrize("images", [1, 3, 5])
@pytest.mark.parametrize("ch", [3, 4, 6, 256])
def test_label_kernels_against_fp64(amd, ch, images, ppi):
    L, check, S = amd._lib.lib, amd._lib.check, amd.ops._stream()
    gen = torch.Generator().manual_seed(1000 * ch + 10 * images + ppi % 7)
    pixels = images * ppi
    labels = [N_LABEL] if (images, ppi) == (1, 3) else LABELS[images]        # one case where nothing is in range
    label = torch.tensor(labels, dtype=torch.int64)
    used = sorted({l for l in labels if 0 <= l < N_LABEL})
    # the label buffer sits between two words no kernel may take for a label
    lbuf = torch.tensor([1 << 40] + labels + [-(1 << 40)], dtype=torch.int64).cuda()
    lp = P(lbuf, 1)
    t32 = torch.empty(pixels, 2 * ch).uniform_(-12, 12, generator=gen)
    t32[0, :min(4, ch)] = torch.tensor([0.0, -0.0, 1e-5, -20.0])[:min(4, ch)]
    r32 = torch.randn(pixels, ch, generator=gen)
    dy32 = torch.randn(pixels, ch, generator=gen)
    e32 = torch.randn(N_LABEL, 2 * ch, generator=gen) * 0.5
    tb, rb, dyb = _poisoned(t32, 8), _poisoned(r32, 4), _poisoned(dy32, 4)
    lde = ceil4(2 * ch) + 4
    eb = torch.full((N_LABEL, lde), float("nan"))
    eb[used, :2 * ch] = e32[used]                                             # rows no image names: NaN, never read
    eb = eb.cuda()
    e32 = torch.where(torch.isnan(eb[:, :2 * ch].cpu()), torch.zeros(()), e32)
    t64, r64, dy64, e64 = t32.double(), r32.double(), dy32.double(), e32.double()
    tag = f"Ch={ch} images={images} ppi={ppi}"

    # forward: t stays the conv output
    t_before = _bits(tb)
    ob = _nan(pixels, ceil4(ch) + 4)
    check(L.vq2_glu_res_label_fwd(P(tb), tb.shape[1], P(rb), rb.shape[1], P(eb), lde, lp, images, ppi, P(ob), ob.shape[1],
                                  pixels, ch, N_LABEL, S), "glu_res_label_fwd")
    _check_rows(ob, ch, "glu_res_label_fwd")
    assert torch.equal(_bits(tb), t_before)
    _bound("glu_res_label_fwd " + tag, ob[:, :ch].cpu(), LR.glu_label_fwd(t64, r64, e64, label, ppi),
           LR.glu_label_fwd(t32, r32, e32, label, ppi))
    if not used:        # nothing in range: the unlabelled kernel's bits
        plain = _nan(pixels, ceil4(ch) + 4)
        check(L.vq2_glu_res_fwd(P(tb), tb.shape[1], P(rb), rb.shape[1], P(plain), plain.shape[1], pixels, ch, S), "glu_res_fwd")
        assert torch.equal(_bits(ob), _bits(plain))

    # backward
    dtb = _nan(pixels, ceil4(2 * ch) + 8)
    check(L.vq2_glu_res_label_bwd(P(dyb), dyb.shape[1], P(tb), tb.shape[1], P(eb), lde, lp, images, ppi, P(dtb), dtb.shape[1],
                                  pixels, ch, N_LABEL, S), "glu_res_label_bwd")
    _check_rows(dtb, 2 * ch, "glu_res_label_bwd")
    want64, want32 = LR.glu_label_bwd(dy64, t64, e64, label, ppi), LR.glu_label_bwd(dy32, t32, e32, label, ppi)
    _bound("glu_res_label_bwd da " + tag, dtb[:, :ch].cpu(), want64[:, :ch], want32[:, :ch])
    _bound("glu_res_label_bwd db " + tag, dtb[:, ch:2 * ch].cpu(), want64[:, ch:], want32[:, ch:])

    # the table's gradient from the kernel's own dt
    nbytes = L.vq2_label_embed_grad_workspace_bytes(images, ppi, 2 * ch)
    assert nbytes > 0
    dt32 = dtb[:, :2 * ch].cpu()
    outs = []
    for _ in range(2):
        ws = torch.full((nbytes // 4 + 4,), float("nan"), device="cuda")
        dE = _nan(N_LABEL + 1, 2 * ch)
        check(L.vq2_label_embed_grad(P(dtb), dtb.shape[1], lp, images, ppi, 2 * ch, N_LABEL, P(dE), P(ws), nbytes, S),
              "label_embed_grad")
        assert bool(torch.isnan(ws[nbytes // 4:]).all()) and bool(torch.isnan(dE[N_LABEL]).all())
        outs.append(dE[:N_LABEL].cpu())
    assert torch.equal(outs[0], outs[1])                                      # fixed order: bit for bit
    for l in range(N_LABEL):
        if l not in used:
            assert float(outs[0][l].abs().sum()) == 0, l                      # exactly 0 (and not NaN)
    _bound("label_embed_grad " + tag, outs[0], LR.label_embed_grad(dt32.double(), label, ppi, N_LABEL),
           LR.label_embed_grad(dt32, label, ppi, N_LABEL))
    torch.cuda.synchronize()


def test_refusals(amd):
    L, S = amd._lib.lib, amd.ops._stream()
    ch, images, ppi = 4, 2, 3
    t, r, e = torch.zeros(6, 8, device="cuda"), torch.zeros(6, 4, device="cuda"), torch.zeros(N_LABEL, 8, device="cuda")
    o = torch.full((6, 4), 7.0, device="cuda")
    dt = torch.full((6, 8), 7.0, device="cuda")
    lab = torch.zeros(3, dtype=torch.int64, device="cuda")       # (three: one call below states three images)
    for pixels in (5, 7):                               # pixels != images * pixels_per_image
        assert L.vq2_glu_res_label_fwd(P(t), 8, P(r), 4, P(e), 8, P(lab), images, ppi, P(o), 4, pixels, ch, N_LABEL, S) == 1
        assert L.vq2_glu_res_label_bwd(P(r), 4, P(t), 8, P(e), 8, P(lab), images, ppi, P(dt), 8, pixels, ch, N_LABEL, S) == 1
    assert L.vq2_glu_res_label_fwd(P(t), 8, P(r), 4, P(e), 8, P(lab), 3, 2, P(o), 4, 6, ch, N_LABEL, S) == 0     # 3 x 2 is 6 too
    torch.cuda.synchronize()
    assert L.vq2_glu_res_label_fwd(P(t), 8, P(r), 4, P(e), 8, P(lab), images, 0, P(o), 4, 6, ch, N_LABEL, S) == 1
    nbytes = L.vq2_label_embed_grad_workspace_bytes(images, ppi, 8)
    ws = torch.zeros(nbytes // 4, device="cuda")
    dE = torch.full((N_LABEL, 8), 7.0, device="cuda")
    assert L.vq2_label_embed_grad(P(dt), 8, P(lab), images, ppi, 8, N_LABEL, P(dE), P(ws), nbytes - 1, S) == 1
    assert L.vq2_label_embed_grad(P(dt), 8, P(lab), images, ppi, 8, 0, P(dE), P(ws), nbytes, S) == 1
    torch.cuda.synchronize()
    assert bool((dE == 7.0).all())
    assert L.vq2_label_embed_grad(P(dt), 8, P(lab), images, ppi, 8, N_LABEL, P(dE), P(ws), nbytes, S) == 0
    torch.cuda.synchronize()
    assert float(dE[0, 0]) == 42.0 and float(dE[1:].abs().sum()) == 0       # 6 pixels of 7 under label 0
