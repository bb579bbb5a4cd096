"""The stage-2 prior with bf16 conv operands (set_conv_precision / Stage2Trainer.set_precision('bf16') / --precision bf16).

GatedResBlock: forward and every gradient against an fp64 restatement of the block (the formula of
tests/_pixelsnail_ref.py) whose convs are a small autograd.Function with exactly the contract of include/vq2.h: operands
rounded to bf16 in the forward where the (padded) input channels are a multiple of 16 and in the data gradient where the
output channels are, the weight gradient from the unrounded x and dy.  Tolerance: 4 x the gap between that restatement in
fp32 and in fp64 (the convention of tests/test_gpu_pixelsnail_model.py).
The tiny model is PixelSNAIL([6, 8], 12, 64, 5, 2, 2, 32): 64 channels, the fewest the attention's 8 heads accept."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _pixelsnail_ref as R
from test_gpu_dispatch import launched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _is_bf16(label):
    """The bf16-operand kernel's label: a tile of the conv_gemm family whose last field says bf16."""
    return label.startswith("conv_gemm<") and label.endswith(",bf16")


def _ceil4(c):
    return (c + 3) // 4 * 4


class ContractConv(torch.autograd.Function):
    """y = conv_at(r(x), r(w)) + b;  dx = conv_at^T(r(dy), r(w));  dw = wgrad(x, dy) unrounded;  r = bf16 rounding where
    the direction is eligible, the identity elsewhere."""

    @staticmethod
    def forward(ctx, x, w, b, pt, pl):
        ctx.save_for_backward(x, w)
        ctx.geom = (pt, pl)
        rf = _bf16 if _ceil4(w.shape[1]) % 16 == 0 else (lambda t: t)
        return R.conv_at(rf(x), rf(w), b, pt, pl)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        pt, pl = ctx.geom
        rd = _bf16 if _ceil4(w.shape[0]) % 16 == 0 else (lambda t: t)
        with torch.enable_grad():
            xd = x.detach().requires_grad_(True)
            wd = w.detach().requires_grad_(True)
            dx = torch.autograd.grad(R.conv_at(xd, rd(w.detach()), None, pt, pl), xd, rd(dy))[0]
            dw = torch.autograd.grad(R.conv_at(x.detach(), wd, None, pt, pl), wd, dy)[0]
        return dx, dw, dy.sum((0, 2, 3)), None, None


def _wn_conv(x, sd, prefix, mode):
    v, g = sd[prefix + "weight_v"], sd[prefix + "weight_g"]
    kh, kw = v.shape[2:]
    if mode == "causal":
        with torch.no_grad():
            v[:, :, -1, kw // 2:].zero_()
    b = sd.get(prefix + "bias")
    y = ContractConv.apply(x, R.weight_norm(v, g), b if b is not None else torch.zeros(v.shape[0], dtype=v.dtype), *R.geometry(mode, kh, kw))
    return y


def _block(x, sd, aux=None, condition=None):
    """R.gated_resblock with conv='causal', no dropout, on ContractConv."""
    h = _wn_conv(F.elu(x), sd, "conv1.conv.conv.", "causal")
    if aux is not None:
        h = h + _wn_conv(F.elu(aux), sd, "aux_conv.conv.", "wnconv2d")
    t = _wn_conv(F.elu(h), sd, "conv2.conv.conv.", "causal")
    if condition is not None:
        t = t + _wn_conv(condition, sd, "condition.conv.", "wnconv2d")
    return F.glu(t, 1) + x


def _restated(sd32, ins32, gout32, dtype):
    sd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd32.items()}
    ins = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in ins32.items()}
    out = _block(ins["x"], sd, ins.get("aux"), ins.get("condition"))
    out.backward(gout32.to(dtype))
    res = {"out": out.detach()}
    res.update({"d" + k: v.grad for k, v in ins.items()})
    res.update({"d." + k: v.grad for k, v in sd.items() if v.grad is not None})
    return res


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "aux+condition"])
def test_gated_resblock_matches_the_fp64_restatement_of_the_contract(amd, extras):
    torch.manual_seed(5 + extras)
    # aux 20 channels: its forward is NOT eligible (fp32), its data gradient (32 output channels) is
    blk = amd.GatedResBlock(32, 32, 5, conv='causal', dropout=0.0, **(dict(auxiliary_channel=20, condition_dim=16) if extras else {}))
    for p in blk.parameters():
        if p.dim() == 4 and p.shape[-1] == 1 and p.shape[1] == 1:       # weight_g: away from the initial norm
            p.data.mul_(torch.rand_like(p) + 0.5)
    blk.eval()
    ins = {"x": torch.randn(2, 32, 6, 7)}
    if extras:
        ins["aux"], ins["condition"] = torch.randn(2, 20, 6, 7), torch.randn(2, 16, 6, 7)
    gout = torch.randn(2, 32, 6, 7)
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    r64, r32 = _restated(sd, ins, gout, torch.float64), _restated(sd, ins, gout, torch.float32)

    blk = blk.to(DEV)
    eligible, total = amd.set_conv_precision(blk, "bf16")
    assert (eligible, total) == ((4, 4) if extras else (2, 2))
    dins = {k: v.to(DEV).requires_grad_(True) for k, v in ins.items()}

    def run():
        out = blk(dins["x"], dins.get("aux"), dins.get("condition"))
        out.backward(gout.to(DEV))
        return out
    out, seen = launched(amd, run)
    # (one label per kernel and shape) every conv forward and data gradient is on the bf16 kernel, except the forward of the
    # 20-channel aux conv
    assert sum(_is_bf16(s) for s in seen) >= 2, seen
    fp32 = [s for s in seen if s.startswith("conv_gemm<") and not _is_bf16(s)]
    assert all(",K=20," in s for s in fp32) and len(fp32) == (1 if extras else 0), seen
    got = {"out": out.detach()}
    got.update({"d" + k: v.grad for k, v in dins.items()})
    got.update({"d." + k: p.grad for k, p in blk.named_parameters()})
    assert set(got) == set(r64)
    bad = []
    for k in sorted(r64):
        gap = float((r32[k].double() - r64[k]).abs().max())
        err = float((got[k].detach().cpu().double() - r64[k]).abs().max())
        print("%s %s: err %.3e, fp32-fp64 gap %.3e, ratio %.2f" % ("aux+cond" if extras else "plain", k, err, gap, err / gap))
        if not (gap > 0 and err <= 4 * gap):
            bad.append((k, err, gap))
    assert not bad, bad


def _tiny(amd, seed=3):
    torch.manual_seed(seed)
    return amd.PixelSNAIL([6, 8], 12, 64, 5, 2, 2, 32).to(DEV)


def _codes(seed=11):
    return torch.randint(0, 12, (2, 6, 8), generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_tiny_model_takes_the_bf16_kernels_and_goes_back_bit_for_bit(amd):
    model = _tiny(amd).eval()
    codes = _codes()
    with torch.no_grad():
        base = model(codes)[0].clone()
    eligible, total = amd.set_conv_precision(model, "bf16")
    assert 0 < eligible <= total
    model.train()

    def run():
        torch.manual_seed(1)
        out, _ = model(codes)
        loss, _ = amd.prior_loss(out, codes)
        loss.backward()
    _, seen = launched(amd, run)
    assert any(_is_bf16(s) for s in seen), seen
    assert any(s.startswith("wgrad") for s in seen) and not any("bf16" in s for s in seen if s.startswith("wgrad"))
    model.eval()
    with torch.no_grad():
        low = model(codes)[0].clone()
        assert not torch.equal(low, base)
        rel = float((low - base).abs().max() / base.abs().max())
        print("bf16 vs fp32 logits: max relative difference %.3e" % rel)
        assert rel < 0.1
        amd.set_conv_precision(model, "fp32")
        assert torch.equal(model(codes)[0], base)
    # the sampler copies specs without the permission: its convs stay fp32
    amd.set_conv_precision(model, "bf16")
    from vqvae2_amd import sample
    conv1 = model.blocks[0].resblocks[0].conv1
    assert conv1.conv.spec.bf16 and not sample._Conv(conv1).spec.bf16


def _steps(amd, state, n, rng_seed, precision="bf16", resume=None):
    model = _tiny(amd)
    model.load_state_dict(state)
    model.train()
    tr = amd.Stage2Trainer(model, "top", lr=1e-3)
    if precision is not None:
        assert tr.set_precision(precision)[0] > 0
    if resume is not None:
        tr.load_state_dict(resume)
    torch.manual_seed(rng_seed)
    losses = [tr.step(_codes(20 + i))["loss"].item() for i in range(n)]
    return tr, losses


def test_trainer_steps_are_reproducible_and_resume_exactly(amd):
    state = copy.deepcopy(_tiny(amd).state_dict())
    a, la = _steps(amd, state, 3, 7)
    b, lb = _steps(amd, state, 3, 7)
    assert la == lb and all(torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters()))
    assert amd.conv_precision(a.model) == "bf16" and a.state_dict()["precision"] == "bf16"
    fp, lf = _steps(amd, state, 3, 7, precision=None)
    assert lf != la and "precision" not in fp.state_dict()
    # save after 3 steps, continue 2 more; a fresh trainer resumed from the save takes the same 2 steps
    saved = copy.deepcopy(a.state_dict())
    torch.manual_seed(9)
    more = [a.step(_codes(40 + i))["loss"].item() for i in range(2)]
    c = _steps(amd, state, 0, 0, resume=saved)[0]
    torch.manual_seed(9)
    again = [c.step(_codes(40 + i))["loss"].item() for i in range(2)]
    assert more == again and all(torch.equal(p, q) for p, q in zip(a.model.parameters(), c.model.parameters()))
    # a precision mismatch is refused before anything changes
    d = _steps(amd, state, 0, 0, precision=None)[0]
    before = [p.detach().clone() for p in d.model.parameters()]
    with pytest.raises(RuntimeError, match="precision"):
        d.load_state_dict(saved)
    assert all(torch.equal(p, q) for p, q in zip(before, d.model.parameters()))
    with pytest.raises(RuntimeError, match="precision"):
        c.load_state_dict(copy.deepcopy(fp.state_dict()))
