"""The stage-2 prior with bf16 weight gradients (set_conv_precision / Stage2Trainer.set_precision('bf16_wgrad') /
--precision bf16_wgrad), on the helpers and conventions of tests/test_gpu_prior_bf16.py.

GatedResBlock: the fp64 restatement of that file with a ContractConv whose dw is the gradient of the bf16-ROUNDED x and dy
where both (padded) channel counts are multiples of 16, the bias gradient the sum of the unrounded dy; every output and
gradient within 4 x the fp32 - fp64 gap of that restatement."""
import copy

import pytest
import torch

import _pixelsnail_ref as R
import test_gpu_prior_bf16 as P
from test_gpu_dispatch import launched

pytestmark = pytest.mark.gpu
DEV = P.DEV


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _is_bf16_wgrad(label):
    return label.startswith("wgrad<") and label.endswith(",bf16")


class ContractConvWgrad(torch.autograd.Function):
    """ContractConv of tests/test_gpu_prior_bf16.py, with dw = wgrad(r(x), r(dy)) where both channel counts are multiples
    of 16 (r = bf16 rounding), unrounded elsewhere; db the sum of the unrounded dy."""

    @staticmethod
    def forward(ctx, x, w, b, pt, pl):
        ctx.save_for_backward(x, w)
        ctx.geom = (pt, pl)
        rf = P._bf16 if P._ceil4(w.shape[1]) % 16 == 0 else (lambda t: t)
        return R.conv_at(rf(x), rf(w), b, pt, pl)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        pt, pl = ctx.geom
        rd = P._bf16 if P._ceil4(w.shape[0]) % 16 == 0 else (lambda t: t)
        rw = P._bf16 if (P._ceil4(w.shape[0]) % 16 == 0 and P._ceil4(w.shape[1]) % 16 == 0) else (lambda t: t)
        with torch.enable_grad():
            xd = x.detach().requires_grad_(True)
            wd = w.detach().requires_grad_(True)
            dx = torch.autograd.grad(R.conv_at(xd, rd(w.detach()), None, pt, pl), xd, rd(dy))[0]
            dw = torch.autograd.grad(R.conv_at(rw(x.detach()), wd, None, pt, pl), wd, rw(dy))[0]
        return dx, dw, dy.sum((0, 2, 3)), None, None


@pytest.fixture
def wgrad_contract(monkeypatch):
    """The restatement of tests/test_gpu_prior_bf16.py on the contract of this precision level."""
    monkeypatch.setattr(P, "ContractConv", ContractConvWgrad)


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "aux+condition"])
def test_gated_resblock_matches_the_fp64_restatement_of_the_contract(amd, wgrad_contract, extras):
    torch.manual_seed(5 + extras)
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
    r64, r32 = P._restated(sd, ins, gout, torch.float64), P._restated(sd, ins, gout, torch.float32)

    blk = blk.to(DEV)
    assert amd.set_conv_precision(blk, "bf16_wgrad") == ((4, 4) if extras else (2, 2))
    assert amd.conv_precision(blk) == "bf16_wgrad"
    dins = {k: v.to(DEV).requires_grad_(True) for k, v in ins.items()}

    def run():
        out = blk(dins["x"], dins.get("aux"), dins.get("condition"))
        out.backward(gout.to(DEV))
        return out
    out, seen = launched(amd, run)
    wg = [s for s in seen if s.startswith("wgrad")]
    assert any(_is_bf16_wgrad(s) for s in wg), seen
    # the 20-channel aux conv (K = 20 columns) is not eligible: its weight gradient stays on the fp32 kernel
    fp32 = [s for s in wg if not _is_bf16_wgrad(s)]
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


def _grads(amd, model, codes):
    model.train()
    for p in model.parameters():
        p.grad = None

    def run():
        torch.manual_seed(1)
        out, _ = model(codes)
        loss, _ = amd.prior_loss(out, codes)
        loss.backward()
    _, seen = launched(amd, run)
    return [None if p.grad is None else p.grad.clone() for p in model.parameters()], seen


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def test_tiny_model_takes_the_bf16_weight_gradient_and_goes_back_bit_for_bit(amd):
    model, codes = P._tiny(amd), P._codes()
    g32, seen32 = _grads(amd, model, codes)
    counts = amd.set_conv_precision(model, "bf16")
    g16, seen16 = _grads(amd, model, codes)
    assert not any(_is_bf16_wgrad(s) for s in seen32 + seen16)
    assert amd.set_conv_precision(model, "bf16_wgrad") == counts and amd.conv_precision(model) == "bf16_wgrad"
    gw, seenw = _grads(amd, model, codes)
    assert any(_is_bf16_wgrad(s) for s in seenw), seenw
    assert not _same(gw, g16)
    amd.set_conv_precision(model, "bf16")
    assert amd.conv_precision(model) == "bf16" and _same(_grads(amd, model, codes)[0], g16)
    amd.set_conv_precision(model, "fp32")
    assert amd.conv_precision(model) == "fp32" and _same(_grads(amd, model, codes)[0], g32)
    # the sampler's copy of a spec drops the new permission as well
    amd.set_conv_precision(model, "bf16_wgrad")
    from vqvae2_amd import sample
    conv1 = model.blocks[0].resblocks[0].conv1
    spec = sample._Conv(conv1).spec
    assert conv1.conv.spec.bf16_wgrad and not spec.bf16_wgrad and not spec.bf16


def test_trainer_steps_are_reproducible_differ_from_bf16_and_resume_exactly(amd):
    state = copy.deepcopy(P._tiny(amd).state_dict())
    a, la = P._steps(amd, state, 3, 7, precision="bf16_wgrad")
    b, lb = P._steps(amd, state, 3, 7, precision="bf16_wgrad")
    assert la == lb and all(torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters()))
    assert amd.conv_precision(a.model) == "bf16_wgrad" and a.state_dict()["precision"] == "bf16_wgrad"
    h, lh = P._steps(amd, state, 3, 7, precision="bf16")
    assert lh != la and not all(torch.equal(p, q) for p, q in zip(a.model.parameters(), h.model.parameters()))
    # save after 3 steps, continue 2 more; a fresh trainer resumed from the save takes the same 2 steps
    saved = copy.deepcopy(a.state_dict())
    torch.manual_seed(9)
    more = [a.step(P._codes(40 + i))["loss"].item() for i in range(2)]
    c = P._steps(amd, state, 0, 0, precision="bf16_wgrad", resume=saved)[0]
    torch.manual_seed(9)
    again = [c.step(P._codes(40 + i))["loss"].item() for i in range(2)]
    assert more == again and all(torch.equal(p, q) for p, q in zip(a.model.parameters(), c.model.parameters()))
    # checkpoints of each of the three precisions are refused by trainers of the other two, before anything changes
    f = P._steps(amd, state, 1, 7, precision=None)[0]
    saves = {"fp32": copy.deepcopy(f.state_dict()), "bf16": copy.deepcopy(h.state_dict()), "bf16_wgrad": saved}
    for mine in saves:
        t = P._steps(amd, state, 0, 0, precision=None if mine == "fp32" else mine)[0]
        before = [p.detach().clone() for p in t.model.parameters()]
        for theirs, sd in saves.items():
            if theirs != mine:
                with pytest.raises(RuntimeError, match="precision"):
                    t.load_state_dict(copy.deepcopy(sd))
                assert all(torch.equal(p, q) for p, q in zip(before, t.model.parameters())), (mine, theirs)
