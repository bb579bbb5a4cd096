"""bf16-operand fused causal attention (csrc/vq2_attn_bf16.hip, ops.CausalAttnFn(..., bf16=True)) on the MI355X.

Reference: the operands-only restatement of the contract in float64 (tests/_attention_bf16_ref.py: q, k, v, dO rounded to
bf16, p~ and dS not).  Tolerance, elementwise and derived from the number format, not measured (see that file):
    2^-8 x (the product's sum of magnitudes) + A,   A = 4 x the error of the operands-only formula in fp32 torch.
tests/test_attention_bf16_cpu.py checks on the CPU that the contract stated in fp32 torch stays inside it on every shape
used here.  Every case prints its worst error / bound per tensor.

Measured on the MI355X (1 is the bound): worst 0.956 (dQ, x4 inputs), then 0.938 (dV, dropout 0.5) and 0.878 (dQ, B = 3,
L = 17, 1x48); DESIGN.md section 4, "bf16 attention"."""
import functools
import os
import re

import pytest
import torch

import _attention_bf16_ref as B
from test_gpu_dispatch import launched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


@functools.lru_cache(maxsize=None)
def _case(b, l, nh, dh, seed, scale=1.0):
    """inputs and (ref, bound, allowance), computed once per shape and shared, never modified"""
    ins = B.inputs(b, l, nh, dh, seed, scale)
    return ins, B.bounds(*ins, nh)


def _gpu(amd, q, k, v, do, nh, p=0.0, seed=0, bf16=True):
    """q, k, v, dO [B, L, C] -> {O, dQ, dK, dV} on the CPU"""
    t = [x.to(DEV).unsqueeze(1).requires_grad_(True) for x in (q, k, v)]       # [B, 1, L, C]: NHWC with H = 1
    o = amd.ops.CausalAttnFn.apply(t[0], t[1], t[2], nh, p, seed, bf16)
    o.backward(do.to(DEV).unsqueeze(1))
    return {n: x.detach().squeeze(1).cpu() for n, x in zip(B.NAMES, (o, t[0].grad, t[1].grad, t[2].grad))}


def _check(tag, have, ref, bound):
    bad = []
    for name in B.NAMES:
        ratio = B.worst_ratio(have[name], ref[name], bound[name])
        print(f"attention bf16 {tag} {name}: worst error / bound {ratio:.3f}")
        if not ratio <= 1.0:
            bad.append((name, ratio))
    assert not bad, (tag, bad)


@gpu
@pytest.mark.parametrize("nh,dh", B.HEADS)
@pytest.mark.parametrize("l", B.LENGTHS)
@pytest.mark.parametrize("b", B.BATCHES)
def test_core_against_the_operands_only_fp64_reference(amd, b, l, nh, dh):
    (q, k, v, do), (ref, bound, _) = _case(b, l, nh, dh, B.case_seed(b, l, nh, dh))
    have = _gpu(amd, q, k, v, do, nh)
    assert torch.count_nonzero(have["O"][:, 0]) == 0 and not torch.signbit(have["O"][:, 0]).any()    # row 0: bitwise +0
    if l == 1:
        assert all(torch.count_nonzero(x) == 0 for x in have.values())
    _check(f"B={b} L={l} {nh}x{dh}", have, ref, bound)


@gpu
def test_core_at_the_workload_length_and_the_path_is_told_apart(amd):
    """L = 1024, 8 heads of 16.  Also: against the UNROUNDED fp64 reference the result misses the fp32 allowance A, so the
    bf16 kernels ran and this test can tell the two paths apart; the fp32 path on the same inputs stays inside A."""
    (q, k, v, do), (ref, bound, _) = _case(*B.EXTRA_CASES[0][:5])
    have, seen = launched(amd, lambda: _gpu(amd, q, k, v, do, 8))
    _check("L=1024 8x16", have, ref, bound)
    want = {"attn_%s<1>|B=1,L=1024,nh=8,dh=16,bf16" % s for s in ("fwd", "delta", "dkv", "dq")}
    assert want <= set(seen), seen
    exact = B.attention(q, k, v, do, 8, torch.float64, rounding="none")
    fp32, seen32 = launched(amd, lambda: _gpu(amd, q, k, v, do, 8, bf16=False))
    assert not any("bf16" in s for s in seen32), seen32
    a_exact = {n: 4.0 * float((B.attention(q, k, v, do, 8, torch.float32, rounding="none")[n].double() - exact[n]).abs().max())
               for n in B.NAMES}
    for n in B.NAMES:
        e16 = float((have[n].double() - exact[n]).abs().max())
        e32 = float((fp32[n].double() - exact[n]).abs().max())
        print(f"attention bf16 vs unrounded fp64 {n}: bf16 path {e16 / a_exact[n]:.1f} x A, fp32 path {e32 / a_exact[n]:.2f} x A")
        assert e16 > a_exact[n] >= e32, n
        assert not torch.equal(have[n], fp32[n])


@gpu
def test_peaked_softmax(amd):
    (q, k, v, do), (ref, bound, _) = _case(*B.EXTRA_CASES[1][:6])
    _check("x4 inputs", _gpu(amd, q, k, v, do, 2), ref, bound)


@gpu
def test_views_with_a_larger_pixel_stride_and_nothing_written_outside(amd):
    """ld = channel + 4 through the C entry points: operands and results are views into wider buffers with one spare row
    after each image.  The result buffers are pre-filled with NaN: the pad channels and the row i = L stay NaN, and the
    views hold what the dense call gives, bit for bit."""
    b, l, nh, dh = 2, 65, 2, 16
    c = nh * dh
    (q, k, v, do), (ref, bound, _) = _case(b, l, nh, dh, 31)
    lib, ops = amd._lib.lib, amd.ops
    import ctypes as C

    def wide(t):
        buf = torch.full((b, l + 1, c + 4), float("nan"), device=DEV)      # one spare row after the last image
        buf[:, :l, :c] = t.to(DEV)
        return buf
    wq, wk, wv, wg = wide(q), wide(k), wide(v), wide(do)
    outs = [torch.full((b * (l + 1) * (c + 4),), float("nan"), device=DEV) for _ in range(4)]     # o, dq, dk, dv
    lse = torch.empty(b, nh, l, device=DEV)
    delta = torch.empty(b, nh, l, device=DEV)
    # one image at a time, so that the image stride (l + 1 rows) is free
    ld = c + 4
    for i in range(b):
        d = amd._lib.AttnDesc()
        d.B, d.L, d.n_head, d.dim_head = 1, l, nh, dh
        d.ldq = d.ldk = d.ldv = d.ldo = ld
        off = i * (l + 1) * ld * 4
        p = lambda t: C.c_void_p(t.data_ptr() + off)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.vq2_causal_attn_fwd_ex(C.byref(d), ops.VQ2_ALLOW_BF16, p(wq), p(wk), p(wv), p(outs[0]),
                                          C.c_void_p(lse[i].data_ptr()), s) == 0, lib.vq2_last_error()
        assert lib.vq2_causal_attn_bwd_ex(C.byref(d), ops.VQ2_ALLOW_BF16, p(wq), p(wk), p(wv), C.c_void_p(lse[i].data_ptr()),
                                          p(wg), ld, p(outs[1]), ld, p(outs[2]), ld, p(outs[3]), ld,
                                          C.c_void_p(delta[i].data_ptr()), s) == 0, lib.vq2_last_error()
    torch.cuda.synchronize()
    got = [t.view(b, l + 1, ld).cpu() for t in outs]
    for t in got:
        assert torch.isnan(t[:, l]).all() and torch.isnan(t[:, :, c:]).all()       # the spare row and the pad channels
        assert not torch.isnan(t[:, :l, :c]).any()
    have = {n: t[:, :l, :c].contiguous() for n, t in zip(B.NAMES, got)}
    _check("ld = channel + 4", have, ref, bound)
    dense = _gpu(amd, q, k, v, do, nh)
    assert all(torch.equal(have[n], dense[n]) for n in B.NAMES)


@gpu
@pytest.mark.parametrize("case", B.EXTRA_CASES[2:], ids=["p0.1", "p0.5"])
def test_dropout_against_the_keep_mask(amd, case):
    b, l, nh, dh, in_seed, _, p, seed = case
    q, k, v, do = B.inputs(b, l, nh, dh, in_seed)
    keep = amd.ops.causal_attn_keep_mask(b, nh, l, p, seed, DEV).cpu()
    assert torch.equal(keep, B.keep_mask(b, nh, l, p, seed))      # the mask the CPU check of the bound used
    ref, bound, _ = B.bounds(q, k, v, do, nh, keep, p)
    _check(f"dropout p={p}", _gpu(amd, q, k, v, do, nh, p=p, seed=seed), ref, bound)


@gpu
def test_two_calls_give_equal_bits_and_an_image_does_not_depend_on_its_batch(amd):
    q, k, v, do = B.inputs(3, 130, 2, 16, 21)
    for p in (0.0, 0.1):
        a = _gpu(amd, q, k, v, do, 2, p=p, seed=5)
        c = _gpu(amd, q, k, v, do, 2, p=p, seed=5)
        assert all(torch.equal(a[n], c[n]) for n in B.NAMES)
        one = _gpu(amd, q[:1], k[:1], v[:1], do[:1], 2, p=p, seed=5)
        assert all(torch.equal(a[n][:1], one[n]) for n in B.NAMES)


@gpu
def test_a_non_eligible_geometry_runs_the_fp32_kernels(amd):
    q, k, v, do = B.inputs(2, 65, 2, 12, 8)
    with_perm, seen = launched(amd, lambda: _gpu(amd, q, k, v, do, 2, bf16=True))
    without = _gpu(amd, q, k, v, do, 2, bf16=False)
    assert all(torch.equal(with_perm[n], without[n]) for n in B.NAMES)
    assert not any("bf16" in s for s in seen), seen


@gpu
def test_unknown_flag_bits_are_refused(amd):
    import ctypes as C
    lib = amd._lib.lib
    x = torch.zeros(1, 1, 5, 32, device=DEV)
    d = amd.ops._attn_desc(1, 5, 2, 16, x, x, x, x, 0.0, 0)
    assert lib.vq2_causal_attn_fwd_ex(C.byref(d), 4, *(C.c_void_p(x.data_ptr()),) * 5, None) == 1      # VQ2_ERR_INVALID
    with pytest.raises(RuntimeError):
        amd._lib.check(lib.vq2_causal_attn_fwd_ex(C.byref(d), amd.ops.VQ2_ALLOW_BF16 | 1, *(C.c_void_p(x.data_ptr()),) * 5, None), "fwd_ex")


def test_bf16_attention_kernels_do_not_spill():
    """The compiler's resource report of csrc/vq2_attn_bf16.hip (written by csrc/build.sh): no spilled register and no
    scratch in any of the 4 kernels x 4 head widths."""
    path = os.path.join(ROOT, "vq-vae-2-pytorch_amd", "csrc", "_obj", "vq2_attn_bf16.res")
    assert os.path.exists(path), "csrc/_obj/vq2_attn_bf16.res is missing: csrc/build.sh lists vq2_attn_bf16 and writes the report"
    hot = re.compile(r"attn_(fwd|delta|dq|dkv)_bf16_kernel")
    seen, name = 0, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen += bool(hot.search(name))
            continue
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name and hot.search(name):
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
    assert seen == 16, f"{seen} bf16 attention kernels found in the report, expected 4 kernels x 4 head widths"
