"""Host side of the bf16-operand weight gradient (--precision bf16_wgrad), and the CPU checks that the tolerance of
tests/test_gpu_wgrad_bf16.py bites.  No GPU."""
import ctypes as C
import dataclasses
import importlib.util
import os

import pytest
import torch

import _wgrad_bf16_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = W.CASES + [W.NOT_ELIGIBLE]


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _example(name):
    spec = importlib.util.spec_from_file_location(name + "_example", os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ----------------------------------------------------------------------------- the GPU tests' tolerance, checked on the CPU
@pytest.mark.parametrize("c", ALL, ids=lambda c: c[0])
def test_the_tolerance_bites(c):
    """For dw of every case, with and without ReLU: plain fp32 torch on the rounded operands passes; the same with one
    pixel's contribution to one (o, i, tap) dropped fails; the fp64 gradient of the unrounded operands fails.  For db: the
    fp32 sum passes and the sum without one pixel fails."""
    assert W.rows(c) < W.MAX_ROWS // 50
    d = W.make_inputs(c)
    for relu_in in (False, True):
        ref = W.dw_ref(c, d, relu_in)
        tol = W.tolerance(c, ref)
        good = W.dw_ref(c, d, relu_in, torch.float32)
        bad = W.drop_one(c, d, relu_in)
        exact = W.dw_ref(c, d, relu_in, rounded=False)
        errs = [float((t.double() - ref).abs().max()) for t in (good, bad, exact)]
        print("%s relu_in=%d: tol %.3e  fp32 %.3e  one product dropped %.3e  unrounded %.3e" % ((c[0], relu_in, tol) + tuple(errs)))
        assert errs[0] <= tol, "plain fp32 misses the tolerance"
        assert errs[1] > tol, "a dropped product goes unnoticed"
        assert errs[2] > 20 * tol, "the rounding is not visible"
    rb = W.db_ref(c, d)
    tol = W.tolerance(c, rb)
    assert float((W.db_ref(c, d, torch.float32).double() - rb).abs().max()) <= tol
    short = dict(d, dy=d["dy"].clone())
    short["dy"][-1, -1, -1, :] = 0
    assert float((W.db_ref(c, short) - rb).abs().max()) > tol
    # db of the ROUNDED dy would miss it too: the bias gradient must come from the unrounded values
    assert float((W.bf16(d["dy"]).double().sum(dim=(0, 1, 2)) - rb).abs().max()) > tol


def test_the_reference_is_the_full_correlation():
    """wgrad() by autograd against the contract's formula written out, on the case whose kernel is larger than the image."""
    c = W.BY_NAME["d"]
    name, cin, cout, kh, kw, pt, pl, n, h, w = c
    d = W.make_inputs(c)
    x, dy = d["x"].double(), d["dy"].double()
    want = torch.zeros(cout, cin, kh, kw, dtype=torch.float64)
    for a in range(kh):
        for b in range(kw):
            for hh in range(h):
                for ww in range(w):
                    ih, iw = hh - pt + a, ww - pl + b
                    if 0 <= ih < h and 0 <= iw < w:
                        want[:, :, a, b] += torch.einsum("no,ni->oi", dy[:, hh, ww], x[:, ih, iw])
    assert float((W.wgrad(c, x, dy, torch.float64) - want).abs().max()) < 1e-12


# ----------------------------------------------------------------------------- eligibility, plans, ABI
def test_host_mirror_of_the_eligibility_rule(amd):
    from vqvae2_amd import ops
    lib = amd._lib.lib
    for c in ALL:
        spec = ops.ConvSpec.geom(*c[1:7])
        assert ops.conv_wgrad_bf16_eligible(spec) == W.eligible(c) == (c[0] != "n"), c[0]
    for cin in (4, 12, 16, 20, 32, 48, 256, 258, 514):
        for cout in (4, 16, 36, 64, 256, 258, 514):
            for spec in (ops.ConvSpec.geom(cin, cout, 3, 3, 2, 1), ops.ConvSpec(False, cin, cout, 3, 1, 1)):
                want = bool(spec.same_size) and ops.ceil4(cin) % 16 == 0 and ops.ceil4(cout) % 16 == 0
                d = ops._desc(spec, 2, 8, 8, spec.ci, spec.co)
                assert ops.conv_wgrad_bf16_eligible(spec) == want
                assert bool(lib.vq2_conv_wgrad_bf16_eligible(C.byref(d))) == want
    assert not ops.conv_wgrad_bf16_eligible(ops.ConvSpec.geom(514, 256, 1, 1, 0, 0))    # padded 516
    assert not ops.conv_wgrad_bf16_eligible(ops.ConvSpec.geom(256, 258, 1, 1, 0, 0))    # padded 260
    assert not lib.vq2_conv_wgrad_bf16_eligible(None)


def _plan(amd, c, flags, n=None):
    from vqvae2_amd import ops
    lib = amd._lib.lib
    spec = ops.ConvSpec.geom(*c[1:7])
    d = ops._desc(spec, n or c[7], c[8], c[9], spec.ci, spec.co)
    job = amd._lib.WgradJob()
    backing = C.create_string_buffer(64)
    dummy = C.c_void_p((C.addressof(backing) + 15) & ~15)
    assert lib.vq2_wgrad_job_init_ex(C.byref(d), flags, dummy, dummy, dummy, C.byref(job)) == 0
    return lib.vq2_conv_wgrad_workspace_bytes_ex(C.byref(d), flags), job, d, dummy


def test_the_ex_entry_points_with_flag_zero_are_the_old_ones(amd):
    lib = amd._lib.lib
    for c in ALL:
        for flags in (0, 1):       # VQ2_RELU_IN does not change a plan
            nbytes, job, d, dummy = _plan(amd, c, flags)
            old = amd._lib.WgradJob()
            assert lib.vq2_wgrad_job_init(C.byref(d), dummy, dummy, dummy, C.byref(old)) == 0
            assert bytes(job) == bytes(old), c[0]
            assert nbytes == lib.vq2_conv_wgrad_workspace_bytes(C.byref(d)) > 0


def test_the_bf16_plan_is_plain_with_slabs_and_bias_partials(amd):
    """With the permission an eligible layer's job is in the plain layout (mode word 0, bias partials [S][O]) whatever the
    fp32 plan says -- (f) exchanges roles there and (g) is a Winograd mode -- and the workspace is exactly the S slabs plus
    the S bias rows; the layer that is not eligible plans as without the flag."""
    from vqvae2_amd import ops
    for c in ALL:
        nbytes, job, d, _ = _plan(amd, c, ops.VQ2_ALLOW_BF16)
        nb0, job0, _, _ = _plan(amd, c, 0)
        if c[0] == "n":
            assert bytes(job) == bytes(job0) and nbytes == nb0
            continue
        taps, ci, co = c[3] * c[4], ops.ceil4(c[1]), ops.ceil4(c[2])
        assert (job.swapped, job.bias_splits, job.O, job.I, job.Or, job.Ir, job.taps) == (0, 0, co, ci, c[2], c[1], taps), c[0]
        assert job.n_units_w == (co * ci * taps + 31) // 32 and job.n_units_b == (c[2] + 31) // 32
        assert job.S >= 1 and nbytes == 4 * job.S * (co * ci * taps + co)
        assert job.S <= max(1, (W.rows(c) + 255) // 256)
    assert _plan(amd, W.BY_NAME["f"], 0)[1].swapped & 1 == 1               # the fp32 plans of (f) and (g): sw and wino
    assert (_plan(amd, W.BY_NAME["g"], 0)[1].swapped >> 1) & 3 == 1
    assert _plan(amd, W.BY_NAME["e"], ops.VQ2_ALLOW_BF16)[1].S > 1          # several splits, the last one short


def test_a_large_layer_is_split_to_fill_the_chip(amd):
    """The 5x5 256 -> 256 layer of the top prior at batch 32: hundreds of workgroups, every split a multiple of 32 rows."""
    from vqvae2_amd import ops
    c = ("big", 256, 256, 5, 5, 4, 2, 32, 32, 32)
    nbytes, job, _, _ = _plan(amd, c, ops.VQ2_ALLOW_BF16)
    assert 2 <= job.S <= 128 and nbytes == 4 * job.S * (256 * 6400 + 256)


# ----------------------------------------------------------------------------- spec, precision levels, scripts
def test_conv_spec_field_defaults_to_false(amd):
    from vqvae2_amd.ops import ConvSpec
    a = ConvSpec.geom(16, 32, 5, 5, 4, 2)
    assert a.bf16_wgrad is False and "bf16_wgrad" in [f.name for f in dataclasses.fields(ConvSpec)]
    b = dataclasses.replace(a, bf16_wgrad=True)
    assert b != a and b.bf16_wgrad and not b.bf16 and dataclasses.replace(b, bf16_wgrad=False) == a


def test_set_conv_precision_levels(amd):
    model = amd.PixelSNAIL([6, 8], 12, 64, 5, 2, 2, 32)
    convs = [m for m in model.modules() if isinstance(m, amd.WNConv2d) and m not in (model.horizontal.conv, model.vertical.conv)]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    counts = amd.set_conv_precision(model, "bf16")
    assert amd.set_conv_precision(model, "bf16_wgrad") == counts
    assert all(m.spec.bf16 and m.spec.bf16_wgrad for m in convs) and amd.conv_precision(model) == "bf16_wgrad"
    assert not model.horizontal.conv.spec.bf16_wgrad and not model.vertical.conv.spec.bf16_wgrad
    assert amd.set_conv_precision(model, "bf16") == counts and amd.conv_precision(model) == "bf16"
    assert all(m.spec.bf16 and not m.spec.bf16_wgrad for m in convs)
    amd.set_conv_precision(model, "bf16_wgrad")
    assert amd.set_conv_precision(model, "fp32") == counts and amd.conv_precision(model) == "fp32"
    assert not any(m.spec.bf16 or m.spec.bf16_wgrad for m in convs)
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    with pytest.raises(ValueError):
        amd.set_conv_precision(model, "bf16_dgrad")


@pytest.mark.parametrize("script", ["train_pixelsnail", "eval_pixelsnail"])
def test_precision_flag_accepts_the_new_level(script):
    ex = _example(script)
    base = ["codes.db"] if script == "train_pixelsnail" else ["--ckpt", "x.pt", "codes.db"]
    assert ex.parse_args(["--precision", "bf16_wgrad"] + base).precision == "bf16_wgrad"
    with pytest.raises(SystemExit):
        ex.parse_args(["--precision", "wgrad_bf16"] + base)


def test_header_documents_the_new_entry_points(amd):
    header = open(os.path.join(ROOT, "include", "vq2.h")).read()
    for name in ("vq2_conv_wgrad_bf16_eligible", "vq2_conv_wgrad_workspace_bytes_ex", "vq2_wgrad_job_init_ex"):
        assert name in header and hasattr(amd._lib.lib, name)
    assert amd._lib.API_VERSION >= 18
