"""GPU: vq2_grad_norm and vq2_adam_step_ex against float64 at their launch edges, and what FusedAdam / Stage2Trainer /
Stage1Trainer build on them: clipping that never bites (bit for bit the plain run), clipping that does, averaged weights,
the averaged_weights() exchange, exact resume, the skipped step, the untouched default path and two ranks.

Assertions are of three kinds: bitwise (torch.equal / np.array_equal) wherever the same kernels see the same numbers; one
float32 ulp against float64 for the norm and the coefficient (the accumulation is float64: only the summation order and
the final rounding remain); and for everything Adam writes the rule of _bound in tests/test_gpu_small_kernels.py, restated
in _optim_extras_ref.bound: no farther from float64 than 4 x the float32 formula's own distance."""
import ctypes as C
import functools
import os
import socket
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import _optim_extras_child as X
import _optim_extras_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 777.0
GUARD = 64
# the launchers' own grids (csrc/vq2_elem.hip: GN_BLOCKS, ADAM_EX_BLOCKS) x 256 threads x 4 floats
GN_SWEEP, ADAM_SWEEP = 1024 * 256 * 4, 2048 * 256 * 4
# one float4, a partial block, one exact sweep of either grid, that plus one float4, every thread at least twice
SIZES = [4, 252, GN_SWEEP, GN_SWEEP + 4, ADAM_SWEEP, ADAM_SWEEP + 4, 2 * ADAM_SWEEP]
HYPERS = [(3e-4, 0.9, 0.999, 1e-8), (1e-2, 0.5, 0.9, 1e-3)]          # those of test_gpu_small_kernels.py::test_adam_step


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run(amd, name, *args):
    lib = amd._lib.lib
    rc = getattr(lib, name)(*args, amd.ops._stream())
    assert rc == 0, (name, rc, lib.vq2_last_error())


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def guarded(t):
    """Device copy of the flat host tensor t followed by a guard band."""
    buf = torch.full((t.numel() + GUARD,), SENT, dtype=t.dtype, device="cuda")
    buf[:t.numel()] = t.cuda()
    return buf


def guard_untouched(buf, n):
    return bool((buf[n:] == SENT).all())


# ================================================================================================ vq2_grad_norm
@functools.lru_cache(maxsize=None)
def grad_data(n):
    g = torch.randn(n, generator=gen("gnorm", n))
    g[3::5] = 0.0
    return g


def norm_buffers(amd, n, total=0.0):
    ws_bytes = amd._lib.lib.vq2_grad_norm_workspace_bytes(n)
    ws = torch.full((ws_bytes // 8 + GUARD,), SENT, dtype=torch.float64, device="cuda")
    ctl = guarded(torch.tensor([SENT, SENT, SENT, total]))
    return ctl, ws, ws_bytes


@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_against_fp64(amd, n):
    g = grad_data(n)
    gd = guarded(g)
    ctl, ws, ws_bytes = norm_buffers(amd, n, total=3.0)
    grad_scale, max_norm = 0.125, 0.75
    run(amd, "vq2_grad_norm", P(gd), n, grad_scale, max_norm, P(ctl), P(ws), ws_bytes)
    torch.cuda.synchronize()
    first, ws_first = ctl.clone(), ws.clone()
    want = R.grad_norm(g.numpy(), grad_scale)
    want_coef = R.clip_coef(want, max_norm)
    print(f"n {n}: norm {float(ctl[0])!r} fp64 {want!r}; coef {float(ctl[1])!r} fp64 {want_coef!r}")
    assert R.one_ulp(ctl[0], want) and R.one_ulp(ctl[1], want_coef)
    assert (want_coef < 1.0) == (n > 4 * 4), "the larger sizes must clip"
    assert float(ctl[2]) == 0.0 and float(ctl[3]) == 3.0
    assert guard_untouched(ctl, 4) and guard_untouched(ws, ws_bytes // 8) and torch.equal(gd[:n].cpu(), g) and guard_untouched(gd, n)
    run(amd, "vq2_grad_norm", P(gd), n, grad_scale, max_norm, P(ctl), P(ws), ws_bytes)      # the same bits again
    torch.cuda.synchronize()
    assert torch.equal(ctl, first) and torch.equal(ws, ws_first)
    run(amd, "vq2_grad_norm", P(gd), n, grad_scale, float("inf"), P(ctl), P(ws), ws_bytes)  # measure only
    torch.cuda.synchronize()
    assert float(ctl[1]) == 1.0 and float(ctl[0]) == float(first[0]) and float(ctl[2]) == 0.0


@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_of_a_zero_gradient(amd, n):
    gd = guarded(torch.zeros(n))
    ctl, ws, ws_bytes = norm_buffers(amd, n)
    run(amd, "vq2_grad_norm", P(gd), n, 1.0, 1e-3, P(ctl), P(ws), ws_bytes)
    torch.cuda.synchronize()
    assert ctl[:4].tolist() == [0.0, 1.0, 0.0, 0.0] and guard_untouched(ctl, 4)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_of_a_non_finite_gradient_is_a_value(amd, n, bad):
    g = grad_data(n).clone()
    g[n - 2] = bad                                       # in the last float4: the far end of the last sweep
    gd, good = guarded(g), guarded(grad_data(n))
    ctl, ws, ws_bytes = norm_buffers(amd, n, total=5.0)
    run(amd, "vq2_grad_norm", P(gd), n, 1.0, 1.0, P(ctl), P(ws), ws_bytes)
    torch.cuda.synchronize()
    assert not np.isfinite(float(ctl[0])) and ctl[1:4].tolist() == [0.0, 1.0, 6.0]
    run(amd, "vq2_grad_norm", P(good), n, 1.0, 1.0, P(ctl), P(ws), ws_bytes)
    torch.cuda.synchronize()
    assert R.one_ulp(ctl[0], R.grad_norm(grad_data(n).numpy(), 1.0)) and float(ctl[1]) > 0.0
    assert ctl[2:4].tolist() == [0.0, 6.0] and guard_untouched(ctl, 4) and guard_untouched(ws, ws_bytes // 8)


# ================================================================================================ vq2_adam_step_ex
@functools.lru_cache(maxsize=None)
def adam_data(n):
    g = gen("adam_ex", n)
    p, grad, m = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    v = (torch.randn(n, generator=g) * 0.1) ** 2
    avg = p + 0.01 * torch.randn(n, generator=g)
    grad[3::5] = 0.0
    m[3::10] = 0.0
    v[3::10] = 0.0
    return p, grad, m, v, avg


@pytest.mark.parametrize("hyper", HYPERS, ids=["lr3e-4", "lr1e-2"])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_ex_without_extras_is_adam_step_bit_for_bit(amd, n, step, hyper):
    p, grad, m, v, _ = adam_data(n)
    gd = grad.cuda()
    old = [guarded(t) for t in (p, m, v)]
    run(amd, "vq2_adam_step", P(old[0]), P(gd), P(old[1]), P(old[2]), n, *hyper, step, 0.125)
    one = torch.tensor([123.0, 1.0, 0.0, 0.0], device="cuda")
    for ctl in (None, one):                              # no ctl, and a coefficient of exactly 1
        new = [guarded(t) for t in (p, m, v)]
        run(amd, "vq2_adam_step_ex", P(new[0]), P(gd), P(new[1]), P(new[2]), None, n, *hyper, step, 0.125, P(ctl), 0.0)
        torch.cuda.synchronize()
        for k, a, b in zip("pmv", new, old):
            assert torch.equal(a, b), (k, ctl is None)   # the guard band included
    assert not torch.equal(old[0][:n].cpu(), p)


@pytest.mark.parametrize("hyper", HYPERS, ids=["lr3e-4", "lr1e-2"])
@pytest.mark.parametrize("decay", [0.5, 0.999])
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_ex_clipped_and_averaged_against_fp64(amd, n, decay, hyper):
    host = adam_data(n)
    p, grad, m, v, avg = host
    gd = grad.cuda()
    dev = [guarded(t) for t in (p, m, v, avg)]
    ctl = torch.tensor([9.0, 0.5, 0.0, 0.0], device="cuda")
    step, grad_scale = 2, 0.125
    run(amd, "vq2_adam_step_ex", P(dev[0]), P(gd), P(dev[1]), P(dev[2]), P(dev[3]), n, *hyper, step, grad_scale, P(ctl), decay)
    torch.cuda.synchronize()
    assert all(guard_untouched(t, n) for t in dev) and torch.equal(gd.cpu(), grad)
    assert ctl.tolist() == [9.0, 0.5, 0.0, 0.0]

    def ref(dtype):
        a = [t.numpy().astype(dtype) for t in host]
        return R.adam_ex(a[0], a[1], a[2], a[3], a[4], *hyper, step, grad_scale, 0.5, decay)

    ref64, ref32 = ref(np.float64), ref(np.float32)
    name = f"adam_ex n{n} lr{hyper[0]} decay{decay}"
    errs = [R.bound(f"{name} {k}", t[:n].cpu().numpy(), r64, r32) for k, t, r64, r32 in zip(("p", "m", "v", "avg"), dev, ref64, ref32)]
    assert max(errs) > 0
    assert not torch.equal(dev[3][:n].cpu(), avg)


@pytest.mark.parametrize("n", SIZES)
def test_adam_step_ex_skips_the_whole_launch(amd, n):
    host = adam_data(n)
    gd = host[1].cuda()
    dev = [guarded(t) for t in (host[0], host[2], host[3], host[4])]
    before = [t.clone() for t in dev]
    ctl = torch.tensor([float("nan"), 0.0, 1.0, 7.0], device="cuda")
    run(amd, "vq2_adam_step_ex", P(dev[0]), P(gd), P(dev[1]), P(dev[2]), P(dev[3]), n, *HYPERS[0], 3, 1.0, P(ctl), 0.5)
    torch.cuda.synchronize()
    for k, a, b in zip(("p", "m", "v", "avg"), dev, before):
        assert torch.equal(a, b), k
    assert ctl[1:].tolist() == [0.0, 1.0, 7.0]


# ================================================================================================ trainers
KINDS = ["s2-attention", "s2-conditioned", "s1-tiny"]
S2_KINDS = KINDS[:2]
SEED = 5


def make(amd, kind, sched=None, **extras):
    """(trainer, step(i) -> result of the trainer's i-th step, batches for evaluate(), the key evaluate() scores by)."""
    if kind.startswith("s1"):
        tr, batches = X.stage1(amd, sched=sched, **extras)
        return tr, (lambda i: tr.step(batches[i])), [batches[5]], "mse"
    tr, args = X.stage2(amd, KINDS.index(kind), sched=sched, **extras)
    return tr, (lambda i: tr.step(*args)), [(args[0], args[-1])], "nll"


def take(step, lo, hi, seed=None):
    """Steps lo .. hi - 1; the torch generator (dropout seeds) is seeded first when a seed is given."""
    if seed is not None:
        torch.manual_seed(seed)
    return [step(i) for i in range(lo, hi)]


def losses(results):
    return [float(r["loss"]) for r in results]


def arena_norm(tr):
    """float64 norm of the parameter gradients as they lie in the arena after a step."""
    return R.grad_norm(tr.arena.gp.cpu().numpy(), tr.optimizer.grad_scale)


@pytest.mark.parametrize("kind", KINDS)
def test_clipping_that_never_bites_is_the_plain_run(amd, kind):
    plain, step_plain, _, _ = make(amd, kind, sched="cycle")
    l_plain = losses(take(step_plain, 0, 3, SEED))
    assert sorted(take(step_plain, 3, 4)[0]) == (["accuracy", "loss", "lr"] if kind.startswith("s2") else ["latent", "loss", "recon"])
    clip, step_clip, _, _ = make(amd, kind, sched="cycle", clip_grad_norm=float("inf"))
    results = take(step_clip, 0, 3, SEED)
    assert losses(results) == l_plain
    r = results[-1]
    assert r["grad_norm"].dim() == 0 and r["grad_norm"].is_cuda and r["grad_norm"].data_ptr() == clip.optimizer.ctl.data_ptr()
    want = arena_norm(clip)
    print(f"{kind}: grad_norm {float(r['grad_norm'])!r} fp64 {want!r}")
    assert want > 0 and R.one_ulp(r["grad_norm"], want) and float(r["clip_coef"]) == 1.0
    assert clip.skipped_steps() == 0 and plain.skipped_steps() == 0
    take(step_clip, 3, 4)
    X.same(X.snapshot(clip), X.snapshot(plain), kind)


@pytest.mark.parametrize("kind", S2_KINDS)
def test_clipping_that_bites(amd, kind):
    free, step_free, _, _ = make(amd, kind, clip_grad_norm=float("inf"))
    r = take(step_free, 0, 1, SEED)[0]
    norm = float(r["grad_norm"])
    tr, step, _, _ = make(amd, kind, clip_grad_norm=norm / 2)
    # the parameters as Adam will find them: the step's forward zeroes the masked taps of every 'causal' weight_v in place
    tr.plan.prepare()
    tr.plan.invalidate()
    p0 = tr.arena.flat_p.cpu().numpy().copy()
    r = take(step, 0, 1, SEED)[0]
    g = tr.arena.gp.cpu().numpy().copy()
    assert np.array_equal(g, free.arena.gp.cpu().numpy())                    # the same gradient: only the step differs
    coef, want = float(r["clip_coef"]), R.clip_coef(arena_norm(tr), norm / 2)
    print(f"{kind}: norm {norm!r}, coef {coef!r} fp64 {want!r}")
    assert float(r["grad_norm"]) == norm and R.one_ulp(coef, want)
    assert abs(want - 0.5) <= 2.0 ** -24 + 0.5e-6 / norm                     # 0.5 up to the rounding of norm and the 1e-6 term
    zeros = np.zeros_like(p0)

    def ref(dtype):
        return R.adam_ex(p0.astype(dtype), g.astype(dtype), zeros.astype(dtype), zeros.astype(dtype), None, 1e-3, 0.9, 0.999, 1e-8, 1,
                         1.0, coef)

    (p64, m64, v64, _), (p32, m32, v32, _) = ref(np.float64), ref(np.float32)
    opt = tr.optimizer
    errs = [R.bound(f"{kind} {k}", t.cpu().numpy(), r64, r32) for k, t, r64, r32 in
            (("p", tr.arena.flat_p, p64, p32), ("m", opt._m, m64, m32), ("v", opt._v, v64, v32))]
    assert max(errs) > 0
    assert not np.array_equal(tr.arena.flat_p.cpu().numpy(), free.arena.flat_p.cpu().numpy())
    assert not np.array_equal(opt._m.cpu().numpy(), free.optimizer._m.cpu().numpy())


@pytest.mark.parametrize("kind", S2_KINDS)
def test_averaged_weights_follow_the_fp64_recurrence(amd, kind):
    tr, step, _, _ = make(amd, kind, ema_decay=0.5)
    assert tr.optimizer.clip_grad_norm is None and not hasattr(tr.optimizer, "_norm_ws")
    start = tr.arena.flat_p.cpu().numpy().copy()
    assert np.array_equal(tr.optimizer._avg.cpu().numpy(), start)            # taken when construction was done
    torch.manual_seed(SEED)
    states = []
    for i in range(3):
        r = step(i)
        assert sorted(r) == ["accuracy", "loss", "lr"]
        states.append(tr.arena.flat_p.cpu().numpy().copy())
    avg = tr.optimizer._avg.cpu().numpy()
    ref64 = R.ema([s.astype(np.float64) for s in states], start.astype(np.float64), 0.5)
    ref32 = R.ema(states, start, 0.5)
    R.bound(f"{kind} avg", avg, ref64, ref32)
    assert not np.array_equal(avg, states[-1]) and not np.array_equal(avg, start)
    sd = tr.averaged_state_dict()
    model_sd = tr.model.state_dict()
    assert list(sd) == list(model_sd)
    inside = 0
    for name, prm in tr.model.named_parameters():
        off = tr.arena.offset[id(prm)]
        assert np.array_equal(sd[name].cpu().numpy().ravel(), avg[off:off + prm.numel()]), name
        inside += prm.numel()
    assert inside == sum(p.numel() for p in tr.arena.params)
    for name in set(model_sd) - {n for n, _ in tr.model.named_parameters()}:
        assert torch.equal(sd[name], model_sd[name]), name                  # buffers as they are
    fresh = X.S.build(amd, KINDS.index(kind))
    fresh.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)


@pytest.mark.parametrize("kind", KINDS)
def test_averaged_weights_context_exchanges_and_restores(amd, kind):
    never, step_never, _, _ = make(amd, kind, sched="cycle", ema_decay=0.5)
    take(step_never, 0, 4, SEED)
    tr, step, batches, key = make(amd, kind, sched="cycle", ema_decay=0.5)
    take(step, 0, 2, SEED)
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    outside = tr.evaluate(batches)[key]             # (a forward zeroes the masked taps of a 'causal' weight_v in place)
    p_before, avg_before = tr.arena.flat_p.clone(), tr.optimizer._avg.clone()
    assert not torch.equal(p_before, avg_before)
    with tr.averaged_weights() as same_trainer:
        assert same_trainer is tr
        assert torch.equal(tr.arena.flat_p, avg_before) and torch.equal(tr.optimizer._avg, p_before)
        for prm in tr.arena.params:                                          # the model's parameters ARE the arena
            off = tr.arena.offset[id(prm)]
            assert torch.equal(prm.detach().reshape(-1), avg_before[off:off + prm.numel()])
        inside = tr.evaluate(batches)[key]
    assert torch.equal(tr.arena.flat_p, p_before) and torch.equal(tr.optimizer._avg, avg_before)
    print(f"{kind}: {key} outside {outside!r}, with averaged weights {inside!r}")
    assert inside != outside and tr.evaluate(batches)[key] == outside
    with pytest.raises(KeyError):
        with tr.averaged_weights():
            assert torch.equal(tr.arena.flat_p, avg_before)
            raise KeyError("inside")
    assert torch.equal(tr.arena.flat_p, p_before) and torch.equal(tr.optimizer._avg, avg_before)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), gpu_state)
    take(step, 2, 4)
    X.same(X.snapshot(tr), X.snapshot(never), kind)


def _cpu(ck):
    out = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ck.items()}
    out["model"] = {k: v.cpu() for k, v in ck["model"].items()}
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_resume_with_both_features_continues_exactly(amd, kind):
    extras = dict(sched="cycle", clip_grad_norm=0.01, ema_decay=0.9)
    whole, step_whole, _, _ = make(amd, kind, **extras)
    whole.optimizer.ctl[3] = 3.0                                             # as if three steps had been skipped before
    r_whole = take(step_whole, 0, 3, 21) + take(step_whole, 3, 5, 22)
    assert all(float(r["clip_coef"]) < 1.0 for r in r_whole), "0.01 must clip these models"
    first, step_first, _, _ = make(amd, kind, **extras)
    first.optimizer.ctl[3] = 3.0
    l_first = losses(take(step_first, 0, 3, 21))
    ck = first.state_dict()
    assert sorted(ck) == ["adam_m", "adam_t", "adam_v", "avg", "betas", "clip_grad_norm", "ema_decay", "lr", "model", "scheduler",
                          "skipped"]
    assert (ck["ema_decay"], ck["clip_grad_norm"], ck["skipped"], ck["adam_t"]) == (0.9, 0.01, 3, 3)
    assert ck["avg"].numel() == ck["adam_m"].numel() == sum(p.numel() for p in first.arena.params)
    ck = _cpu(ck)
    second, step_second, _, _ = make(amd, kind, **extras)
    with torch.no_grad():
        for prm in second.arena.params:                                      # the checkpoint is what counts
            off = second.arena.offset[id(prm)]
            prm.add_(0.25)
            second.optimizer._avg[off:off + prm.numel()].sub_(0.25)
    second.load_state_dict(ck)
    assert second.skipped_steps() == 3
    l_second = losses(take(step_second, 3, 5, 22))
    assert l_first + l_second == losses(r_whole)
    X.same(X.snapshot(second), X.snapshot(whole), kind)
    assert second.skipped_steps() == whole.skipped_steps() == 3
    # a checkpoint without an average: the average starts from the loaded weights
    bare = {k: v for k, v in ck.items() if k not in ("avg", "ema_decay")}
    third, _, _, _ = make(amd, kind, **extras)
    third.load_state_dict(bare)
    assert torch.equal(third.optimizer._avg, third.arena.flat_p) and torch.equal(third.arena.flat_p, first.arena.flat_p)
    third.load_state_dict(ck["model"])                                       # the reference's file: the same rule
    assert torch.equal(third.optimizer._avg, third.arena.flat_p) and third.optimizer._t == 3
    # a checkpoint with an average and a trainer without one: refused before anything changes
    fourth, _, _, _ = make(amd, kind, sched="cycle", clip_grad_norm=0.01)
    before = X.snapshot(fourth)
    with pytest.raises(RuntimeError, match="ema_decay"):
        fourth.load_state_dict(ck)
    X.same(X.snapshot(fourth), before, "refused load")
    assert fourth.optimizer._t == 0 and sorted(fourth.state_dict()) == ["adam_m", "adam_t", "adam_v", "betas", "clip_grad_norm", "lr",
                                                                      "model", "scheduler", "skipped"]


def test_fused_adam_skips_a_non_finite_step_and_takes_the_next(amd):
    from vqvae2_amd.optim import FusedAdam, ParamArena
    g0 = gen("skip")
    params = [torch.nn.Parameter(torch.randn(5, 3, generator=g0).cuda()), torch.nn.Parameter(torch.randn(7, generator=g0).cuda())]
    arena = ParamArena(params)
    opt = FusedAdam(params, lr=1e-2, arena=arena, clip_grad_norm=1.0, ema_decay=0.5)
    assert arena.n == 24 and opt._avg is None

    def fill(grads):
        for prm, g in zip(params, grads):
            prm._vq2_grad.copy_(g)
            prm.grad = prm._vq2_grad                                         # the gradient lies in its slot

    grads = [torch.randn(5, 3, generator=g0).cuda(), torch.randn(7, generator=g0).cuda()]
    bad = [grads[0].clone(), grads[1].clone()]
    bad[1][3] = float("inf")
    p0 = arena.flat_p.clone()
    fill(bad)
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(arena.flat_p, p0) and torch.equal(opt._avg, p0)
    assert not opt._m.any() and not opt._v.any()
    assert opt.ctl.tolist() == [float("inf"), 0.0, 1.0, 1.0] and opt._t == 1
    fill(grads)
    opt.step()
    torch.cuda.synchronize()
    ctl = opt.ctl.tolist()
    g = arena.gp.cpu().numpy()
    assert R.one_ulp(ctl[0], R.grad_norm(g, 1.0)) and R.one_ulp(ctl[1], R.clip_coef(R.grad_norm(g, 1.0), 1.0)) and ctl[1] < 1.0
    assert ctl[2:] == [0.0, 1.0] and opt._t == 2
    zeros = np.zeros(arena.n, dtype=np.float32)

    def ref(dtype):                                                          # the skipped step counted: this is step 2
        start = p0.cpu().numpy().astype(dtype)
        return R.adam_ex(start, g.astype(dtype), zeros.astype(dtype), zeros.astype(dtype), start, 1e-2, 0.9, 0.999, 1e-8, 2, 1.0,
                         ctl[1], 0.5)

    errs = [R.bound(f"after the skip {k}", t.cpu().numpy(), r64, r32) for k, t, r64, r32 in
            zip(("p", "m", "v", "avg"), (arena.flat_p, opt._m, opt._v, opt._avg), ref(np.float64), ref(np.float32))]
    assert max(errs) > 0 and not torch.equal(arena.flat_p, p0)


@pytest.mark.parametrize("kind", KINDS)
def test_defaults_make_the_launches_they_made(amd, kind, monkeypatch):
    lib = amd._lib.lib
    calls = {"vq2_grad_norm": 0, "vq2_adam_step_ex": 0, "vq2_adam_step": 0}

    def counted(name):
        inner = getattr(lib, name)

        def call(*args):
            calls[name] += 1
            return inner(*args)
        return call

    for name in calls:
        monkeypatch.setattr(lib, name, counted(name))
    tr, step, _, _ = make(amd, kind)
    assert not hasattr(tr.optimizer, "ctl") and tr.optimizer._avg is None and not hasattr(tr.optimizer, "_norm_ws")
    take(step, 0, 1, SEED)
    assert calls == {"vq2_grad_norm": 0, "vq2_adam_step_ex": 0, "vq2_adam_step": 1}
    assert tr.skipped_steps() == 0
    with pytest.raises(RuntimeError, match="ema_decay"):
        tr.averaged_state_dict()
    ema, step_ema, _, _ = make(amd, kind, ema_decay=0.9)                     # alone: no norm launch
    take(step_ema, 0, 1, SEED)
    assert calls == {"vq2_grad_norm": 0, "vq2_adam_step_ex": 1, "vq2_adam_step": 1} and not hasattr(ema.optimizer, "_norm_ws")
    both, step_both, _, _ = make(amd, kind, ema_decay=0.9, clip_grad_norm=1.0)
    take(step_both, 0, 1, SEED)
    assert calls == {"vq2_grad_norm": 1, "vq2_adam_step_ex": 2, "vq2_adam_step": 1}


def test_features_need_the_arena_path(amd):
    model = X.S.build(amd, 0)
    with pytest.raises(ValueError, match="arena"):
        amd.Stage2Trainer(model, "top", arena=False, clip_grad_norm=1.0)
    with pytest.raises(ValueError, match="arena"):
        amd.Stage2Trainer(model, "top", arena=False, ema_decay=0.5)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("ci", X.S.CASES, ids=["attention", "conditioned"])
def test_two_ranks_hold_the_same_state_and_norm(amd, tmp_path, ci):
    """Two ranks over gloo on the one GPU, a split batch, both features on: after two steps both hold bitwise the same
    parameters, average and grad_norm, and that norm is the float64 norm of the reduced arena times 1 / world."""
    out, port = str(tmp_path / "two"), _free_port()
    child = os.path.join(ROOT, "tests", "_optim_extras_child.py")
    procs = [subprocess.Popen([sys.executable, child, str(rank), "2", str(port), out, str(ci)], cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in (0, 1)]
    logs = []
    try:
        for proc in procs:                                                   # each rank under its own time limit
            logs.append(proc.communicate(timeout=240)[0])
    finally:
        for proc in procs:
            if proc.poll() is None:
                proc.kill()
                proc.wait()
    for rank, proc in enumerate(procs):
        assert proc.returncode == 0, f"rank {rank}: " + logs[rank][-3000:]
    r0, r1 = (dict(np.load(f"{out}.rank{rank}.npz")) for rank in (0, 1))
    X.same(r0, r1, f"case {ci}: replicas")
    want = R.grad_norm(r0["gp"], 0.5)
    print(f"case {ci}: grad_norm {float(r0['grad_norm'])!r} fp64 of the reduced arena {want!r}")
    assert R.one_ulp(r0["grad_norm"], want) and float(r0["ctl"][0]) == float(r0["grad_norm"])
    assert R.one_ulp(r0["ctl"][1], R.clip_coef(want, X.TWO_RANK_CLIP)) and int(r0["skipped"]) == 0
    assert not np.array_equal(r0["avg"], r0["flat_p"])
