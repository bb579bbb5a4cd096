"""The bf16-operand conv forward and data gradient (VQ2_ALLOW_BF16) through the C ABI, against the fp64 conv of the
bf16-rounded operands (tests/_conv_bf16_cases.py: cases, references and the tolerance rule; tests/test_conv_bf16_cpu.py
shows on the CPU that one dropped product exceeds that tolerance and that the rounding is visible at these seeds).

Per case and op: the label is conv_gemm<tile>|...,bf16, the result is inside the project's fp32 tolerance of the rounded reference and
far outside it against the unrounded one, two runs are bit-equal, and without the flag the call is today's path.  The data
gradient runs each case with cin and cout exchanged (its depth is the output channel count); as written, its layers with
Co % 16 != 0 must stay on the fp32 kernel with the flag set.  Each line prints err / tol."""
import ctypes as C

import pytest
import torch

import _conv_bf16_cases as B
from test_gpu_dispatch import conv_labels, differs, guarded, launched, sliced, untouched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _pad4(t, c4):
    """NHWC tensor with its channels padded by zeros to c4."""
    return torch.cat([t, t.new_zeros(t.shape[:-1] + (c4 - t.shape[-1],))], -1) if c4 != t.shape[-1] else t


def _spec(c):
    from vqvae2_amd import ops
    name, cin, cout, kh, kw, pt, pl = c[:7]
    return ops.ConvSpec.geom(cin, cout, kh, kw, pt, pl)


def _pack(amd, spec, wt, which):
    from vqvae2_amd import ops
    buf = torch.full((spec.ci * spec.co * spec.taps,), float("nan"), device=DEV)
    d = ops._desc(spec, 1, 2, 2, spec.ci, spec.co)
    amd._lib.check(amd._lib.lib.vq2_pack_weight(C.byref(d), which, ops._p(wt), ops._p(buf), ops._stream()), "pack_weight")
    return buf


def fwd(amd, c, d, allow, x=None, out=None, bias=False, res=None):
    """vq2_conv_fwd of case c; returns (y [n,h,w,co] as given or fresh, labels)."""
    from vqvae2_amd import ops
    lib = amd._lib.lib
    spec = _spec(c)
    x = _pad4(d["x"], spec.ci).to(DEV) if x is None else x
    n = x.shape[0]
    h, w = x.shape[1:3]
    out = torch.empty(n, h, w, spec.co, device=DEV) if out is None else out
    elig = allow and ops.conv_bf16_eligible(spec)
    wp = _pack(amd, spec, d["w"].to(DEV), ops.PACK_FWD_BF16 if elig else ops.PACK_FWD)
    b = d["b"].to(DEV) if bias else None
    desc = ops._desc(spec, n, h, w, ops.ld_of(x), ops.ld_of(out))
    flags = ops.VQ2_ALLOW_BF16 if allow else 0
    _, seen = launched(amd, lambda: amd._lib.check(
        lib.vq2_conv_fwd(C.byref(desc), flags, ops._p(x), ops._p(wp), ops._p(b), ops._p(res), ops.ld_of(res) if res is not None else 0,
                         ops._p(out), ops._stream()), "conv_fwd"))
    return out, seen


def dgrad(amd, c, d, allow, dy=None, out=None, mask=None, res=None, mask_after=False):
    from vqvae2_amd import ops
    lib = amd._lib.lib
    spec = _spec(c)
    dy = _pad4(d["dy"], spec.co).to(DEV) if dy is None else dy
    n, h, w = dy.shape[:3]
    out = torch.empty(n, h, w, spec.ci, device=DEV) if out is None else out
    elig = allow and ops.conv_bf16_eligible(spec, dgrad=True)
    wp = _pack(amd, spec, d["w"].to(DEV), ops.PACK_DGRAD_BF16 if elig else ops.PACK_DGRAD)
    desc = ops._desc(spec, n, h, w, spec.ci, ops.ld_of(dy))
    flags = (ops.VQ2_ALLOW_BF16 if allow else 0) | (ops.VQ2_MASK_AFTER_RESIDUAL if mask_after else 0)
    _, seen = launched(amd, lambda: amd._lib.check(
        lib.vq2_conv_dgrad(C.byref(desc), flags, ops._p(dy), ops._p(wp), ops._p(mask), ops.ld_of(mask) if mask is not None else 0,
                           ops._p(res), ops.ld_of(res) if res is not None else 0, ops._p(out), ops.ld_of(out), ops._stream()),
        "conv_dgrad"))
    return out, seen


def _check(what, got, ref, ref32, exact, c, op):
    tol = B.tolerance(c, op, ref, ref32)
    err = float((got.double() - ref).abs().max())
    err32 = float((ref32.double() - ref).abs().max())
    print("%s: err %.3e  tol %.3e  err/tol %.3f  err / (fp32 CPU err) %.2f" % (what, err, tol, err / tol, err / max(err32, 1e-30)))
    assert err <= tol, what
    assert differs(got, exact, B.tolerance(c, op, exact, ref32)), what + ": inside the tolerance of the UNROUNDED reference"


def _bf16_only(seen, what):
    labels = [s for s in seen if s.startswith("conv_")]
    assert labels and all(s.startswith("conv_gemm<128x") and "|" in s and s.endswith(",bf16") for s in labels), "%s: %s" % (what, labels)


@pytest.mark.parametrize("c", B.CASES, ids=lambda c: c[0])
def test_forward_matches_fp64_of_the_rounded_operands(amd, c):
    d = B.make_inputs(c)
    cout = c[2]
    y, seen = fwd(amd, c, d, True, bias=True)
    _bf16_only(seen, c[0])
    _check(c[0] + " fwd", y[..., :cout].cpu(), B.fwd_ref(c, d, bias=True), B.fwd_ref(c, d, torch.float32, bias=True),
           B.fwd_ref(c, d, rounded=False, bias=True), c, "fwd")
    assert bool((y[..., cout:] == 0).all()), "pad channels"
    y2, _ = fwd(amd, c, d, True, bias=True)
    assert torch.equal(y, y2), "two runs differ"
    # without the flag: today's label and today's bits (ops.conv_forward on a spec without the permission)
    from vqvae2_amd import ops
    y0, seen0 = fwd(amd, c, d, False, bias=True)
    assert not any("bf16" in s for s in seen0) and conv_labels(seen0)
    today = ops.conv_forward(_spec(c), _pad4(d["x"], ops.ceil4(c[1])).to(DEV), d["w"].to(DEV), d["b"].to(DEV))
    assert torch.equal(y0, today)


@pytest.mark.parametrize("c", B.CASES, ids=lambda c: c[0])
def test_data_gradient_matches_fp64_of_the_rounded_operands(amd, c):
    from vqvae2_amd import ops
    cs = B.swapped(c)
    d = B.make_inputs(cs)
    cin = cs[1]
    dx, seen = dgrad(amd, cs, d, True)
    _bf16_only(seen, c[0])
    _check(c[0] + " dgrad", dx[..., :cin].cpu(), B.dgrad_ref(cs, d), B.dgrad_ref(cs, d, torch.float32), B.dgrad_ref(cs, d, rounded=False),
           cs, "dgrad")
    assert bool((dx[..., cin:] == 0).all()), "pad channels"
    assert torch.equal(dx, dgrad(amd, cs, d, True)[0]), "two runs differ"
    dx0, seen0 = dgrad(amd, cs, d, False)
    assert not any("bf16" in s for s in seen0) and conv_labels(seen0)
    today = ops.conv_dgrad(_spec(cs), (cs[7], cs[8], cs[9], ops.ceil4(cin)), _pad4(d["dy"], ops.ceil4(cs[2])).to(DEV), d["w"].to(DEV))
    assert torch.equal(dx0, today)
    # as written (not exchanged): a layer whose Co is no multiple of 16 stays on the fp32 kernel with the flag set
    if not ops.conv_bf16_eligible(_spec(c), dgrad=True):
        d = B.make_inputs(c)
        a, sa = dgrad(amd, c, d, True)
        b, sb = dgrad(amd, c, d, False)
        assert sa == sb and not any("bf16" in s for s in sa) and torch.equal(a, b)


def test_case_e_strides_guards_bias_and_epilogues(amd):
    """Case (a) on a sliced input, a guarded output, a strided residual and bias; the data gradient with mask and residual
    in both orders.  Guard pixels and neighbour channels keep their sentinel."""
    from vqvae2_amd import ops
    c = B.BY_NAME["a"]
    d = B.make_inputs(c)
    name, cin, cout, kh, kw, pt, pl, n, h, w = c
    _, x = sliced(_pad4(d["x"], ops.ceil4(cin)), DEV)
    _, res = sliced(_pad4(d["res_y"], ops.ceil4(cout)), DEV)
    flat, wide, out = guarded((n, h, w, ops.ceil4(cout)), DEV)
    y, seen = fwd(amd, c, d, True, x=x, out=out, bias=True, res=res)
    _bf16_only(seen, "e fwd")
    untouched(flat, wide, ops.ceil4(cout), "e fwd")
    kw_ = dict(bias=True, residual=True)
    _check("e fwd", y[..., :cout].cpu(), B.fwd_ref(c, d, **kw_), B.fwd_ref(c, d, torch.float32, **kw_), B.fwd_ref(c, d, rounded=False, **kw_), c, "fwd")
    cs = B.swapped(c)
    d = B.make_inputs(cs)
    cin, cout = cs[1], cs[2]
    for mask_after in (False, True):
        _, dy = sliced(_pad4(d["dy"], ops.ceil4(cout)), DEV)
        _, res = sliced(_pad4(d["res_x"], ops.ceil4(cin)), DEV)
        _, mask = sliced(_pad4(d["mask"], ops.ceil4(cin)), DEV)
        flat, wide, out = guarded((n, h, w, ops.ceil4(cin)), DEV)
        dx, seen = dgrad(amd, cs, d, True, dy=dy, out=out, mask=mask, res=res, mask_after=mask_after)
        _bf16_only(seen, "e dgrad")
        untouched(flat, wide, ops.ceil4(cin), "e dgrad")
        kw_ = dict(mask=True, residual=True, mask_after=mask_after)
        _check("e dgrad after=%d" % mask_after, dx[..., :cin].cpu(), B.dgrad_ref(cs, d, **kw_), B.dgrad_ref(cs, d, torch.float32, **kw_),
               B.dgrad_ref(cs, d, rounded=False, **kw_), cs, "dgrad")


def test_relu_flags_on_the_bf16_path(amd):
    """VQ2_RELU_IN is applied before the rounding, VQ2_RELU_OUT in the epilogue."""
    from vqvae2_amd import ops
    c = B.BY_NAME["b"]
    d = B.make_inputs(c)
    spec = _spec(c)
    x = _pad4(d["x"], spec.ci).to(DEV)
    wt = d["w"].to(DEV)
    wp = _pack(amd, spec, wt, ops.PACK_FWD_BF16)
    out = torch.empty(c[7], c[8], c[9], spec.co, device=DEV)
    desc = ops._desc(spec, c[7], c[8], c[9], spec.ci, spec.co)
    flags = ops.VQ2_ALLOW_BF16 | ops.VQ2_RELU_IN | ops.VQ2_RELU_OUT
    amd._lib.check(amd._lib.lib.vq2_conv_fwd(C.byref(desc), flags, ops._p(x), ops._p(wp), None, None, 0, ops._p(out), ops._stream()), "conv_fwd")
    dd = dict(d, x=d["x"].clamp(min=0))
    ref, ref32 = B.fwd_ref(c, dd).clamp(min=0), B.fwd_ref(c, dd, torch.float32).clamp(min=0)
    err, tol = float((out[..., :c[2]].cpu().double() - ref).abs().max()), B.tolerance(c, "fwd", ref, ref32)
    print("relu in/out: err %.3e tol %.3e err/tol %.3f" % (err, tol, err / tol))
    assert err <= tol


def test_an_ineligible_layer_keeps_the_fp32_kernel_with_the_flag_set(amd):
    """Ci = 20: the label is the fp32 one and the output is bit-equal to the call without the flag; the bf16 panel of such
    a layer is refused."""
    from vqvae2_amd import ops
    c = ("ci20", 20, 36, 5, 5, 4, 2, 2, 5, 7)
    d = B.make_inputs(c)
    a, sa = fwd(amd, c, d, True)
    b, sb = fwd(amd, c, d, False)
    assert sa == sb and conv_labels(sa) and all(s.startswith("conv_gemm<") and "bf16" not in s for s in sa if s.startswith("conv_"))
    assert torch.equal(a, b)
    spec = _spec(c)
    desc = ops._desc(spec, 1, 2, 2, spec.ci, spec.co)
    buf = torch.empty(spec.ci * spec.co * spec.taps, device=DEV)
    rc = amd._lib.lib.vq2_pack_weight(C.byref(desc), ops.PACK_FWD_BF16, ops._p(d["w"].to(DEV)), ops._p(buf), ops._stream())
    assert rc == 2      # VQ2_ERR_UNSUPPORTED


def test_an_image_does_not_depend_on_its_batch(amd):
    """Image 1 of a batch of 3 is bit-equal to the same image run alone, forward and data gradient."""
    c = B.BY_NAME["b"]
    d = B.make_inputs(c)
    y3, _ = fwd(amd, c, d, True, bias=True)
    y1, _ = fwd(amd, c, dict(d, x=d["x"][1:2]), True, bias=True)
    assert torch.equal(y3[1:2], y1)
    cs = B.swapped(c)
    d = B.make_inputs(cs)
    g3, _ = dgrad(amd, cs, d, True)
    g1, _ = dgrad(amd, cs, dict(d, dy=d["dy"][1:2]), True)
    assert torch.equal(g3[1:2], g1)
