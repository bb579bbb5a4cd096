"""Host side of the bf16-operand conv path (--precision bf16), and the CPU checks that the GPU tests' tolerance bites.  No GPU."""
import importlib.util
import inspect
import os

import pytest
import torch

import _conv_bf16_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _example(name):
    spec = importlib.util.spec_from_file_location(name + "_example", os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_api_version_and_constants(amd):
    from vqvae2_amd import ops
    assert amd._lib.API_VERSION >= 17 and amd._lib.lib.vq2_version() == amd._lib.API_VERSION
    assert (ops.VQ2_ALLOW_BF16, ops.PACK_FWD_BF16, ops.PACK_DGRAD_BF16) == (16, 2, 3)
    assert ops.VQ2_ALLOW_BF16 & (ops.VQ2_RELU_IN | ops.VQ2_RELU_OUT | ops.VQ2_MASK_AFTER_RESIDUAL) == 0
    header = open(os.path.join(ROOT, "include", "vq2.h")).read()
    for line in ("#define VQ2_ALLOW_BF16 16", "#define VQ2_PACK_FWD_BF16 2", "#define VQ2_PACK_DGRAD_BF16 3"):
        assert line in header


def test_conv_spec_bf16_defaults_to_false(amd):
    from vqvae2_amd.ops import ConvSpec
    a, b = ConvSpec.geom(16, 32, 5, 5, 4, 2), ConvSpec(False, 16, 32, 5, 1, 4, 5, 2, True)
    assert a.bf16 is False and a == b and hash(a) == hash(b)
    assert [f.name for f in __import__("dataclasses").fields(ConvSpec)][-1] == "bf16"
    c = __import__("dataclasses").replace(a, bf16=True)
    assert c != a and c.bf16 is True and (c.cin, c.cout, c.k, c.kw, c.pad, c.pad_left, c.same_size) == (16, 32, 5, 5, 4, 2, True)


def test_stage2_trainer_signature_is_unchanged_and_precision_is_a_method(amd):
    """The constructor's parameter list is pinned (tests/test_optim_extras_cpu.py: clip_grad_norm, ema_decay last), so the
    precision of a run is set by a method after construction."""
    names = list(inspect.signature(amd.Stage2Trainer.__init__).parameters)
    assert names == ["self", "model", "hier", "lr", "sched", "n_iter", "arena", "clip_grad_norm", "ema_decay"]
    assert list(inspect.signature(amd.Stage2Trainer.set_precision).parameters) == ["self", "precision"]
    assert not hasattr(amd.Stage1Trainer, "set_precision")


@pytest.mark.parametrize("script", ["train_pixelsnail", "eval_pixelsnail"])
def test_precision_flag_accepts_fp32_and_bf16_only(script, capsys):
    """--amp of train_pixelsnail.py stays O0-only (tests/test_pixelsnail_model_cpu.py pins that O1 is refused): the
    reduced precision has a flag of its own."""
    ex = _example(script)
    base = ["codes.db"] if script == "train_pixelsnail" else ["--ckpt", "x.pt", "codes.db"]
    assert ex.parse_args(base).precision == "fp32"
    assert ex.parse_args(["--precision", "bf16"] + base).precision == "bf16"
    for bad in ("O1", "fp16", "BF16", "bfloat16"):
        with pytest.raises(SystemExit):
            ex.parse_args(["--precision", bad] + base)
    if script == "train_pixelsnail":
        assert ex.parse_args(["--amp", "O0", "--precision", "bf16"] + base).amp == "O0"
    with pytest.raises(SystemExit):
        ex.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "bf16-rounded operands and accumulate in fp32" in text and "weight gradients" in text


def test_host_mirror_of_the_eligibility_rule(amd):
    """ops.conv_bf16_eligible against the library's vq2_conv_bf16_eligible over same_size x channel counts."""
    import ctypes as C
    from vqvae2_amd import ops
    lib = amd._lib.lib
    for cin in (4, 12, 16, 20, 32, 36, 48, 256, 514, 516):
        for cout in (4, 16, 36, 64, 512, 514):
            geom = ops.ConvSpec.geom(cin, cout, 3, 3, 2, 1)
            square = ops.ConvSpec(False, cin, cout, 3, 1, 1)
            for spec in (geom, square):
                d = ops._desc(spec, 2, 8, 8, spec.ci, spec.co)
                for dgrad in (False, True):
                    want = bool(spec.same_size) and (ops.ceil4(cout) if dgrad else ops.ceil4(cin)) % 16 == 0
                    assert ops.conv_bf16_eligible(spec, dgrad) == want
                    assert bool(lib.vq2_conv_bf16_eligible(C.byref(d), int(dgrad))) == want
    assert not ops.conv_bf16_eligible(ops.ConvSpec.geom(514, 256, 1, 1, 0, 0))       # the 514-channel 1x1 convs stay fp32
    assert ops.conv_bf16_eligible(ops.ConvSpec.geom(514, 256, 1, 1, 0, 0), dgrad=True)


def test_set_conv_precision_walks_the_tree_and_leaves_state_alone(amd):
    model = amd.PixelSNAIL([6, 8], 12, 64, 5, 2, 2, 32)   # (64 channels: the attention needs dim_head = 64 / 2 / 8 >= 4)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    convs = [m for m in model.modules() if isinstance(m, amd.WNConv2d)]
    eligible, total = amd.set_conv_precision(model, "bf16")
    assert total == len(convs) - 2 and 0 < eligible <= total              # the two one-hot input convs are left out
    assert not model.horizontal.conv.spec.bf16 and not model.vertical.conv.spec.bf16
    assert all(m.spec.bf16 for m in convs if m not in (model.horizontal.conv, model.vertical.conv))
    assert amd.conv_precision(model) == "bf16"
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert amd.set_conv_precision(model, "fp32") == (eligible, total) and amd.conv_precision(model) == "fp32"
    assert not any(m.spec.bf16 for m in convs)
    with pytest.raises(ValueError):
        amd.set_conv_precision(model, "fp16")


# ----------------------------------------------------------------------------- the GPU tests' tolerance, checked on the CPU
def _ops(c):
    return (("fwd", c), ("dgrad", B.swapped(c)))


@pytest.mark.parametrize("c", B.CASES, ids=lambda c: c[0])
def test_one_dropped_product_exceeds_the_tolerance(c):
    """Plain fp32 torch on the rounded operands passes the tolerance of every case; with one tap of one (co, ci) pair
    zeroed it fails: the tolerance is tight enough to see a single missing product."""
    for op, cc in _ops(c):
        d = B.make_inputs(cc)
        f = B.fwd_ref if op == "fwd" else B.dgrad_ref
        ref, good = f(cc, d), f(cc, d, torch.float32)
        bad = f(cc, d, torch.float32, w=B.drop_one(cc, d["w"]))
        tol = B.tolerance(cc, op, ref, good)
        assert float((good.double() - ref).abs().max()) <= tol, "%s %s: plain fp32 misses the tolerance" % (c[0], op)
        assert float((bad.double() - ref).abs().max()) > tol, "%s %s: a dropped product goes unnoticed" % (c[0], op)


@pytest.mark.parametrize("c", B.CASES, ids=lambda c: c[0])
def test_the_rounding_is_visible_at_these_seeds(c):
    """The fp64 conv of the rounded operands misses the tolerance against the fp64 conv of the unrounded ones (by far:
    the relative gap is about 1e-3), so a GPU result inside the tolerance of the first proves that the rounding happened."""
    for op, cc in _ops(c):
        d = B.make_inputs(cc)
        f = B.fwd_ref if op == "fwd" else B.dgrad_ref
        rounded, exact = f(cc, d), f(cc, d, rounded=False)
        tol = B.tolerance(cc, op, exact, f(cc, d, torch.float32, rounded=False))
        gap = float((rounded - exact).abs().max())
        print("%s %s: rounding gap %.3e = %.1f x tolerance (%.2e of max|ref|)" % (c[0], op, gap, gap / tol, gap / float(exact.abs().max())))
        assert gap > 20 * tol
