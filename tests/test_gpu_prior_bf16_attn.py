"""The stage-2 prior at precision 'bf16_attn' (Stage2Trainer.set_precision / set_attention_precision): bf16 conv operands,
bf16 weight gradients and bf16-operand attention cores.

The helpers are those of tests/test_gpu_prior_bf16.py.  Its tiny model has attention heads of 4 channels, which are never
eligible, so the model here is PixelSNAIL([6, 8], 12, 256, 5, 2, 2, 32): 128 attention channels, 8 heads of 16, the
narrowest model whose attention takes the bf16 kernels.

Module tolerance (test_module_against_the_fp64_restatement).  Reference: the whole CausalAttention in float64, projections
unrounded, core operands-only (tests/_attention_bf16_ref.py).  Bound, elementwise: 4 x the gap between that restatement in
fp32 and in fp64, plus the derived bf16 term of the core (2^-8 x the sums of magnitudes, _attention_bf16_ref.bounds) carried
through the projections' backward, which is linear in dQ, dK, dV: dx = dq W, dW = dq^T x, db = sum dq, and the weight-norm
backward dv = (g / n)(dW - v (dW . v) / n^2), dg = (dW . v) / n; every factor enters by its absolute value."""
import copy

import pytest
import torch

import _attention_bf16_ref as B
import _attention_ref as R
import test_gpu_prior_bf16 as P
from test_gpu_dispatch import launched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _model(amd, seed=3):
    torch.manual_seed(seed)
    return amd.PixelSNAIL([6, 8], 12, 256, 5, 2, 2, 32).to(DEV)


@pytest.fixture
def wide(monkeypatch):
    """the helpers of test_gpu_prior_bf16 (_steps) build their model through its _tiny: give them the 256-channel one"""
    monkeypatch.setattr(P, "_tiny", _model)


def _is_attn_bf16(label):
    return label.startswith("attn_") and label.endswith(",bf16")


class _Core(torch.autograd.Function):
    """the operands-only core of _attention_bf16_ref, forward and backward, for autograd through the projections"""

    @staticmethod
    def forward(ctx, q, k, v, n_head):
        ctx.save_for_backward(q, k, v)
        ctx.n_head = n_head
        zero = torch.zeros_like(q)
        return B.attention(q, k, v, zero, n_head, q.dtype, rounding="operands")["O"]

    @staticmethod
    def backward(ctx, do):
        q, k, v = ctx.saved_tensors
        r = B.attention(q, k, v, do, ctx.n_head, q.dtype, rounding="operands")
        return r["dQ"], r["dK"], r["dV"], None


def _module_ref(sd32, query32, key32, gout32, n_head, dtype):
    sd = {n: t.detach().clone().to(dtype).requires_grad_(True) for n, t in sd32.items()}
    query, key = (t.detach().clone().to(dtype).requires_grad_(True) for t in (query32, key32))
    b, _, h, w = query.shape
    xq = query.reshape(b, query.shape[1], h * w).transpose(1, 2)
    xk = key.reshape(b, key.shape[1], h * w).transpose(1, 2)
    lin = lambda x, n: torch.nn.functional.linear(x, R.weight_norm(sd[n + ".weight_v"], sd[n + ".weight_g"]), sd[n + ".bias"])
    q, k, v = lin(xq, "query"), lin(xk, "key"), lin(xk, "value")
    o = _Core.apply(q, k, v, n_head)
    out = o.reshape(b, h, w, -1).permute(0, 3, 1, 2)
    out.backward(gout32.to(dtype))
    res = {"out": out.detach(), "query": query.grad, "key": key.grad}
    res.update({n: t.grad for n, t in sd.items()})
    return res, (q.detach(), k.detach(), v.detach(), xq.detach(), xk.detach())


def _bf16_terms(sd, taps, gout, n_head):
    """the core's derived bf16 term, elementwise, carried to every result of the module (float64)"""
    q, k, v, xq, xk = taps
    b, l, c = q.shape
    do = gout.double().permute(0, 2, 3, 1).reshape(b, l, c)
    _, bound, allowance = B.bounds(q, k, v, do, n_head)
    e = {n: bound[n] - allowance[n] for n in B.NAMES}          # the 2^-8 term alone
    h, w = gout.shape[2:]
    out = {"out": e["O"].reshape(b, h, w, c).permute(0, 3, 1, 2)}
    eff = {m: R.weight_norm(sd[m + ".weight_v"].double(), sd[m + ".weight_g"].double()).abs() for m in ("query", "key", "value")}
    img = lambda t: t.transpose(1, 2).reshape(b, -1, h, w)
    out["query"] = img(e["dQ"] @ eff["query"])
    out["key"] = img(e["dK"] @ eff["key"] + e["dV"] @ eff["value"])
    for m, eg, x in (("query", e["dQ"], xq), ("key", e["dK"], xk), ("value", e["dV"], xk)):
        out[m + ".bias"] = eg.sum((0, 1))
        ew = torch.einsum("blo,bli->oi", eg, x.abs())
        vv, g = sd[m + ".weight_v"].double(), sd[m + ".weight_g"].double()
        n = vv.norm(dim=1, keepdim=True)
        dot = (ew * vv.abs()).sum(1, keepdim=True)
        out[m + ".weight_v"] = (g.abs() / n) * (ew + vv.abs() * dot / n ** 2)
        out[m + ".weight_g"] = dot / n
    return out


def test_module_against_the_fp64_restatement(amd):
    torch.manual_seed(17)
    m = amd.CausalAttention(20, 24, 32, n_head=2, dropout=0.0)
    for p in m.parameters():
        if p.dim() == 2 and p.shape[1] == 1:
            p.data.mul_(torch.rand_like(p) + 0.5)           # weight_g away from the initial norm
    m.eval()
    query, key, gout = torch.randn(1, 20, 2, 5), torch.randn(1, 24, 2, 5), torch.randn(1, 32, 2, 5)
    sd = {n: t.clone() for n, t in m.state_dict().items()}
    r64, taps = _module_ref(sd, query, key, gout, 2, torch.float64)
    r32, _ = _module_ref(sd, query, key, gout, 2, torch.float32)
    term = _bf16_terms(sd, taps, gout, 2)
    m = m.to(DEV)
    assert amd.set_attention_precision(m, "bf16") == (1, 1)
    dq, dk = query.to(DEV).requires_grad_(True), key.to(DEV).requires_grad_(True)

    def run():
        out = m(dq, dk)
        out.backward(gout.to(DEV))
        return out
    out, seen = launched(amd, run)
    assert sum(_is_attn_bf16(s) for s in seen) == 4, seen
    got = {"out": out.detach(), "query": dq.grad, "key": dk.grad, **{n: p.grad for n, p in m.named_parameters()}}
    assert set(got) == set(r64)
    bad = []
    for name in sorted(r64):
        gap = float((r32[name].double() - r64[name]).abs().max())
        bound = term[name].reshape(r64[name].shape) + 4 * gap
        ratio = B.worst_ratio(got[name].detach().cpu(), r64[name], bound)
        print(f"attention module bf16 {name}: worst error / bound {ratio:.3f} (fp32-fp64 gap {gap:.3e})")
        if not ratio <= 1.0:
            bad.append((name, ratio))
    assert not bad, bad


def _grads(amd, model, codes, precision=None):
    """gradients and labels of one forward + backward; precision=None: at whatever the model carries (a trainer set it)"""
    if precision is not None:
        amd.set_conv_precision(model, precision)
        amd.set_attention_precision(model, "fp32")
    model.zero_grad(set_to_none=True)

    def run():
        torch.manual_seed(1)
        out, _ = model(codes)
        loss, _ = amd.prior_loss(out, codes)
        loss.backward()
    _, seen = launched(amd, run)
    return [p.grad.clone() for p in model.parameters()], seen


def test_levels_take_their_kernels_and_go_back_bit_for_bit(amd):
    model = _model(amd).train()
    codes = P._codes()
    base = {lvl: _grads(amd, model, codes, lvl) for lvl in ("fp32", "bf16_wgrad")}
    tr = amd.Stage2Trainer(model, "top", lr=1e-3)
    counts = tr.set_precision("bf16_wgrad")
    assert tr.set_precision("bf16_attn") == counts
    assert amd.conv_precision(model) == "bf16_wgrad" and amd.attention_precision(model) == "bf16"
    grads, seen = _grads(amd, model, codes)
    attn = [s for s in seen if _is_attn_bf16(s)]
    assert {s.split("<")[0] for s in attn} == {"attn_fwd", "attn_delta", "attn_dkv", "attn_dq"}, seen
    assert any(s.startswith("wgrad") and "bf16" in s for s in seen) and any(P._is_bf16(s) for s in seen), seen
    assert not all(torch.equal(a, b) for a, b in zip(grads, base["bf16_wgrad"][0]))
    for lvl in ("bf16_wgrad", "fp32"):
        tr.set_precision(lvl)
        assert amd.attention_precision(model) == "fp32"
        again, seen = _grads(amd, model, codes)
        assert not any(_is_attn_bf16(s) for s in seen), seen
        assert all(torch.equal(a, b) for a, b in zip(again, base[lvl][0])), lvl


def test_trainer_steps_are_reproducible_resume_exactly_and_refuse_another_precision(amd, wide):
    state = copy.deepcopy(_model(amd).state_dict())
    a, la = P._steps(amd, state, 3, 7, precision="bf16_attn")
    b, lb = P._steps(amd, state, 3, 7, precision="bf16_attn")
    assert la == lb and all(torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters()))
    assert a.state_dict()["precision"] == "bf16_attn" and amd.attention_precision(a.model) == "bf16"
    w, lw = P._steps(amd, state, 3, 7, precision="bf16_wgrad")
    assert lw != la
    # 3 steps, save, fresh trainer, load, 3 steps == 6 steps
    saved = copy.deepcopy(a.state_dict())
    torch.manual_seed(9)
    more = [a.step(P._codes(40 + i))["loss"].item() for i in range(3)]
    c = P._steps(amd, state, 0, 0, precision="bf16_attn", resume=saved)[0]
    torch.manual_seed(9)
    again = [c.step(P._codes(40 + i))["loss"].item() for i in range(3)]
    assert more == again and all(torch.equal(p, q) for p, q in zip(a.model.parameters(), c.model.parameters()))
    # a bf16_wgrad checkpoint is refused by a bf16_attn trainer, and the reverse, before anything changes
    before = [p.detach().clone() for p in w.model.parameters()]
    with pytest.raises(RuntimeError, match="precision"):
        w.load_state_dict(saved)
    assert all(torch.equal(p, q) for p, q in zip(before, w.model.parameters()))
    with pytest.raises(RuntimeError, match="precision"):
        c.load_state_dict(copy.deepcopy(w.state_dict()))


def test_evaluator_takes_the_bf16_forward_and_the_sampler_stays_fp32(amd):
    model = _model(amd).eval()
    codes = P._codes()
    amd.set_conv_precision(model, "bf16_wgrad")

    def evaluate():
        ev = amd.PriorEvaluator(model, "top", top_k=3)
        ev.update(codes)
        return ev
    _, seen = launched(amd, evaluate)
    assert not any(_is_attn_bf16(s) for s in seen), seen

    def sample():
        sampler = amd.PriorSampler(model)
        out = sampler.sample(2, 1.0, None, seed=5)
        return out, [[call[2] for call in prog.calls] for prog in sampler._plan[1].row_programs]
    (codes_w, calls_w), _ = launched(amd, sample)
    assert amd.set_attention_precision(model, "bf16") == (2, 2)
    _, seen = launched(amd, evaluate)
    assert {s.split("<")[0] for s in seen if _is_attn_bf16(s)} == {"attn_fwd"}, seen
    (codes_a, calls_a), seen = launched(amd, sample)
    assert calls_a == calls_w and torch.equal(codes_a, codes_w)
    assert not any(_is_attn_bf16(s) for s in seen), seen
