"""Host side of the bf16-operand attention (--precision bf16_attn), and the CPU checks of the reference and tolerance that
tests/test_gpu_attention_bf16.py uses.  No GPU."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

import _attention_bf16_ref as B
import _attention_ref as R

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


def _keep(b, nh, l, p, seed):
    return torch.rand(b, nh, l, l, generator=torch.Generator().manual_seed(seed)) >= p


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("l,nh,dh", [(1, 2, 16), (3, 1, 32), (17, 2, 16), (65, 1, 48)])
def test_unrounded_restatement_is_the_attention_reference(l, nh, dh, p):
    q, k, v, do = B.inputs(2, l, nh, dh, 5 + l)
    keep = _keep(2, nh, l, p, 3) if p else None
    have = B.attention(q, k, v, do, nh, torch.float64, keep, p, rounding="none")
    t = [x.double().requires_grad_(True) for x in (q, k, v)]
    o = R.attention_core(t[0], t[1], t[2], nh, keep=keep, p=p)
    o.backward(do.double())
    for name, want in zip(B.NAMES, (o.detach(), t[0].grad, t[1].grad, t[2].grad)):
        assert float((have[name] - want).abs().max()) <= 1e-12, name


@pytest.mark.parametrize("nh,dh", B.HEADS)
@pytest.mark.parametrize("l", B.LENGTHS)
@pytest.mark.parametrize("b", B.BATCHES)
def test_the_fully_rounded_fp32_restatement_is_within_the_derived_bound(b, l, nh, dh):
    """The reference alone (the contract in float32 torch, every rounding point applied) stays inside the tolerance the
    GPU test allows the kernels, on every shape used there."""
    q, k, v, do = B.inputs(b, l, nh, dh, B.case_seed(b, l, nh, dh))
    ref, bound, _ = B.bounds(q, k, v, do, nh)
    full = B.attention(q, k, v, do, nh, torch.float32, rounding="full")
    for name in B.NAMES:
        ratio = B.worst_ratio(full[name], ref[name], bound[name])
        assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("case", B.EXTRA_CASES, ids=["L1024", "x4", "drop0.1", "drop0.5"])
def test_the_reference_is_within_the_bound_on_the_other_gpu_cases(case):
    """The same check on the remaining GPU cases: the workload's length, the x4 inputs (where the kernels come closest to
    the bound) and the two dropout cases, with the keep mask the library draws (restated in _attention_bf16_ref.keep_mask;
    the GPU test asserts that the two masks are equal)."""
    b, l, nh, dh, seed, scale, p, dseed = case
    q, k, v, do = B.inputs(b, l, nh, dh, seed, scale)
    keep = B.keep_mask(b, nh, l, p, dseed) if p else None
    if keep is not None:
        rate = float(keep.double().mean())
        assert abs(rate - (1 - p)) <= 5 * (p * (1 - p) / keep.numel()) ** 0.5
    ref, bound, _ = B.bounds(q, k, v, do, nh, keep, p)
    full = B.attention(q, k, v, do, nh, torch.float32, keep, p, rounding="full")
    for name in B.NAMES:
        ratio = B.worst_ratio(full[name], ref[name], bound[name])
        print(f"fully rounded fp32 restatement {case} {name}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)


def test_the_bound_tells_the_precisions_apart_and_bites():
    """At a mid-size shape the bf16 result misses the fp32 allowance against the UNROUNDED reference (so a test can tell that
    the bf16 path ran), and one dropped product of the dV sum exceeds the bound."""
    q, k, v, do = B.inputs(1, 65, 2, 16, 77)
    ref, bound, allowance = B.bounds(q, k, v, do, 2)
    exact = B.attention(q, k, v, do, 2, torch.float64, rounding="none")
    full = B.attention(q, k, v, do, 2, torch.float32, rounding="full")
    for name in B.NAMES:
        assert float((full[name].double() - exact[name]).abs().max()) > allowance[name], name
    broken = ref["O"].clone()
    # drop key 0 from the output of the last query of head 0: O_id loses p_i0 r(v_0d)
    terms = B.attention(q, k, v, do, 2, torch.float64, rounding="operands", terms=True)["_terms"]
    pt, rv = terms[0], terms[4]
    broken[0, 64, :16] -= pt[0, 0, 64, 0] * rv[0, 0, 0]
    assert B.worst_ratio(broken, ref["O"], bound["O"]) > 1.0


def test_set_attention_precision_on_cpu_modules(amd):
    model = amd.PixelSNAIL([6, 8], 12, 256, 5, 2, 2, 32)     # attention: 128 channels, 8 heads of 16
    keys = list(model.state_dict())
    layers = [m for m in model.modules() if isinstance(m, amd.CausalAttention)]
    assert len(layers) == 2 and not any(m.bf16 for m in layers) and amd.attention_precision(model) == "fp32"
    assert amd.set_attention_precision(model, "bf16") == (2, 2)
    assert all(m.bf16 for m in layers) and amd.attention_precision(model) == "bf16"
    assert amd.conv_precision(model) == "fp32"                 # the conv permission is a separate one
    assert list(model.state_dict()) == keys
    assert amd.set_attention_precision(model, "fp32") == (2, 2) and amd.attention_precision(model) == "fp32"
    small = amd.PixelSNAIL([6, 8], 12, 64, 5, 2, 2, 32)       # 32 channels, 8 heads of 4: permitted, never eligible
    assert amd.set_attention_precision(small, "bf16") == (0, 2) and amd.attention_precision(small) == "bf16"
    one = amd.CausalAttention(8, 8, 24, n_head=2)              # heads of 12
    assert amd.set_attention_precision(one, "bf16") == (0, 1) and one.bf16
    assert amd.set_attention_precision(amd.CausalAttention(8, 8, 32, n_head=2), "bf16") == (1, 1)
    assert amd.set_attention_precision(torch.nn.Linear(2, 2), "bf16") == (0, 0)
    for bad in ("bf16_attn", "fp16", "BF16", None):
        with pytest.raises(ValueError):
            amd.set_attention_precision(model, bad)
    with pytest.raises(ValueError):
        amd.set_conv_precision(model, "bf16_attn")             # the conv setter keeps its three values
    assert "bf16" not in dict(one.named_buffers()) and "bf16" not in dict(one.named_parameters())


def test_eligibility_rule_and_entry_points(amd):
    from vqvae2_amd import ops
    lib = amd._lib.lib
    assert amd._lib.API_VERSION >= 21 and lib.vq2_version() == amd._lib.API_VERSION
    for dh in range(4, 68, 4):
        d = amd._lib.AttnDesc()
        d.B, d.L, d.n_head, d.dim_head = 1, 5, 2, dh
        assert bool(lib.vq2_causal_attn_bf16_eligible(C.byref(d))) == (dh % 16 == 0) == ops.attn_bf16_eligible(2 * dh, 2)
    assert not lib.vq2_causal_attn_bf16_eligible(None)
    with pytest.raises(NotImplementedError):
        ops.attn_bf16_eligible(12, 2)       # dim_head 6: not a geometry of the attention at all
    # an unknown flag bit is refused before any pointer is looked at
    d = amd._lib.AttnDesc()
    d.B, d.L, d.n_head, d.dim_head = 1, 5, 2, 16
    d.ldq = d.ldk = d.ldv = d.ldo = 32
    for flags in (1, 2, 32, ops.VQ2_ALLOW_BF16 | 4):
        assert lib.vq2_causal_attn_fwd_ex(C.byref(d), flags, None, None, None, None, None, None) == 1      # VQ2_ERR_INVALID
        assert b"VQ2_ALLOW_BF16" in lib.vq2_last_error()
        assert lib.vq2_causal_attn_bwd_ex(C.byref(d), flags, None, None, None, None, None, 32, None, 32, None, 32, None, 32,
                                          None, None) == 1
    # null pointers are refused on both paths (nothing is launched)
    for flags in (0, ops.VQ2_ALLOW_BF16):
        assert lib.vq2_causal_attn_fwd_ex(C.byref(d), flags, None, None, None, None, None, None) == 1
    header = open(os.path.join(ROOT, "include", "vq2.h")).read()
    for name in ("vq2_causal_attn_bf16_eligible", "vq2_causal_attn_fwd_ex", "vq2_causal_attn_bwd_ex"):
        assert "int " + name + "(" in header


def test_autograd_function_takes_the_permission_last_with_default_false(amd):
    import inspect
    names = list(inspect.signature(amd.ops.CausalAttnFn.forward).parameters)
    assert names == ["ctx", "q", "k", "v", "n_head", "p", "seed", "bf16"]
    assert inspect.signature(amd.ops.CausalAttnFn.forward).parameters["bf16"].default is False


class _FakeTrainer:
    """Stage2Trainer's precision bookkeeping without its constructor (which needs the GPU arena)."""

    def __init__(self, model):
        self.model, self.precision = model, None


def test_trainer_precision_levels_on_a_cpu_model(amd):
    model = amd.PixelSNAIL([6, 8], 12, 256, 5, 2, 2, 32)
    tr = _FakeTrainer(model)
    set_precision = amd.Stage2Trainer.set_precision
    counts = set_precision(tr, "bf16_wgrad")
    assert amd.attention_precision(model) == "fp32"
    assert set_precision(tr, "bf16_attn") == counts and tr.precision == "bf16_attn"
    assert amd.conv_precision(model) == "bf16_wgrad" and amd.attention_precision(model) == "bf16"
    for level in ("bf16", "bf16_wgrad", "fp32"):
        set_precision(tr, "bf16_attn")
        assert set_precision(tr, level) == counts and tr.precision == level
        assert amd.conv_precision(model) == level and amd.attention_precision(model) == "fp32"
    with pytest.raises(ValueError):
        set_precision(tr, "bf16_attention")
    assert tr.precision == "fp32" and amd.attention_precision(model) == "fp32"      # a refused level changes nothing


@pytest.mark.parametrize("script", ["train_pixelsnail", "eval_pixelsnail"])
def test_precision_flag_accepts_the_new_level(script):
    ex = _example(script)
    base = ["codes.db"] if script == "train_pixelsnail" else ["--ckpt", "x.pt", "codes.db"]
    assert ex.parse_args(["--precision", "bf16_attn"] + base).precision == "bf16_attn"
    with pytest.raises(SystemExit):
        ex.parse_args(["--precision", "attn_bf16"] + base)
