"""The bf16-operand attention core (include/vq2.h, vq2_causal_attn_fwd_ex / _bwd_ex with VQ2_ALLOW_BF16) restated in plain
torch at a given dtype, forward and backward written out (the backward has rounding points of its own, so it is not torch's
autograd of the forward).  r() is t.float().bfloat16().to(dtype): round to nearest even to bfloat16.

    S = r(q) r(k)^T / sqrt(dh);  P = softmax over j < i (row 0 all zero);  p~ = P * keep / (1 - p)
    O = r(p~) r(v)
    dP = r(dO) r(v)^T;  dPe = dP * keep / (1 - p);  D = sum_j P dPe;  dS = P (dPe - D)
    dV = r(p~)^T r(dO);  dQ = r(dS) r(k) / sqrt(dh);  dK = r(dS)^T r(q) / sqrt(dh)

rounding='full' rounds all of these, 'operands' only q, k, v, dO (p~ and dS stay unrounded: the reference the GPU tests
compare against), 'none' nothing (then it is tests/_attention_ref.py's formula with its hand-written backward).

bounds(): the elementwise tolerance of the fully rounded evaluation against the operands-only one, derived from the number
format alone: rounding p~ and dS to bf16 changes each by at most 2^-8 of its magnitude (2^-9 for round to nearest; 2^-8 is
the bound the project states), and each enters one product linearly, so
    |O - ref|  <= 2^-8 sum_j p~_ij |r(v_jd)|            |dV - ref| <= 2^-8 sum_i p~_ij |r(dO_id)|
    |dQ - ref| <= 2^-8 scale sum_j |dS_ij| |r(k_jd)|    |dK - ref| <= 2^-8 scale sum_i |dS_ij| |r(q_id)|
plus the fp32 allowance A of each tensor: 4 x the max error of the operands-only formula in float32 against float64 (the
yardstick of tests/test_gpu_attention.py)."""
import math

import torch

NAMES = ("O", "dQ", "dK", "dV")


def _r(t, on):
    return t.float().bfloat16().to(t.dtype) if on else t


def attention(q, k, v, do, n_head, dtype, keep=None, p=0.0, rounding="full", terms=False):
    """q, k, v, dO [B, L, C] -> {O, dQ, dK, dV} [B, L, C] at `dtype`; with terms=True also the tensors bounds() needs."""
    assert rounding in ("full", "operands", "none")
    ops_on, inner_on = rounding != "none", rounding == "full"
    b, l, c = q.shape
    dh = c // n_head
    scale = 1.0 / math.sqrt(dh)
    rq, rk, rv, rg = (_r(t.to(dtype).reshape(b, l, n_head, dh).transpose(1, 2), ops_on) for t in (q, k, v, do))
    s = rq @ rk.transpose(2, 3) * scale
    vis = torch.ones(l, l, dtype=torch.bool).tril(-1)          # [i, j]: j < i
    some = vis.any(-1, keepdim=True)
    s = torch.where(some, s.masked_fill(~vis, -math.inf), torch.zeros_like(s))
    pr = torch.softmax(s, -1) * vis.to(dtype)
    kscale = 1.0 if keep is None else keep.to(dtype) / (1.0 - p)
    pt = pr * kscale
    o = _r(pt, inner_on) @ rv
    dpe = (rg @ rv.transpose(2, 3)) * kscale
    ds = pr * (dpe - (pr * dpe).sum(-1, keepdim=True))
    dv = _r(pt, inner_on).transpose(2, 3) @ rg
    dq = (_r(ds, inner_on) @ rk) * scale
    dk = (_r(ds, inner_on).transpose(2, 3) @ rq) * scale
    out = {n: t.transpose(1, 2).reshape(b, l, c) for n, t in zip(NAMES, (o, dq, dk, dv))}
    if terms:
        out["_terms"] = (pt, ds, rq, rk, rv, rg, scale)
    return out


def bounds(q, k, v, do, n_head, keep=None, p=0.0):
    """-> (ref, bound, allowance): the operands-only float64 reference {name: [B, L, C]}, the elementwise tolerance
    {name: [B, L, C]} (bf16 term + allowance) and the fp32 allowance A {name: float} alone."""
    ref = attention(q, k, v, do, n_head, torch.float64, keep, p, "operands", terms=True)
    r32 = attention(q, k, v, do, n_head, torch.float32, keep, p, "operands")
    pt, ds, rq, rk, rv, rg, scale = ref.pop("_terms")
    b, l, c = q.shape
    e = 2.0 ** -8
    term = {"O": e * (pt.abs() @ rv.abs()), "dV": e * (pt.abs().transpose(2, 3) @ rg.abs()),
            "dQ": e * scale * (ds.abs() @ rk.abs()), "dK": e * scale * (ds.abs().transpose(2, 3) @ rq.abs())}
    allowance = {n: 4.0 * float((r32[n].double() - ref[n]).abs().max()) for n in NAMES}
    bound = {n: term[n].transpose(1, 2).reshape(b, l, c) + allowance[n] for n in NAMES}
    return ref, bound, allowance


def worst_ratio(have, ref, bound):
    """max over elements of |have - ref| / bound, with 0 / 0 = 0 and x / 0 = inf."""
    err = (have.double() - ref).abs()
    ratio = torch.zeros_like(err)
    pos = bound > 0
    ratio[pos] = err[pos] / bound[pos]
    ratio[~pos & (err > 0)] = math.inf
    return float(ratio.max()) if ratio.numel() else 0.0


def inputs(b, l, n_head, dh, seed, scale=1.0):
    """q, k, v, dO [B, L, C] float32, reproducible."""
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(b, l, n_head * dh, generator=gen) * s for s in (scale, scale, 1.0, 1.0)]


def keep_mask(b, n_head, l, p, seed):
    """The dropout decision of the library (include/vq2.h) restated: keep(seed, b, h, i, j) = word (j & 3) of Philox4x32
    with 7 rounds, counter (j >> 2, i, b, h), key = the 64-bit seed, compared >= floor(p * 2^32).  bool [B, n_head, L, L]."""
    import numpy as np
    m32 = np.uint64(0xFFFFFFFF)
    lq = (l + 3) // 4
    bb, hh, ii, jq = np.meshgrid(*(np.arange(n, dtype=np.uint64) for n in (b, n_head, l, lq)), indexing="ij")
    c0, c1, c2, c3 = jq, ii, bb, hh
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(7):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    words = np.stack([c0, c1, c2, c3], -1).reshape(b, n_head, l, 4 * lq)[..., :l]
    return torch.from_numpy(words >= np.uint64(int(p * 4294967296.0)))


# the shapes of tests/test_gpu_attention_bf16.py (the CPU test checks the reference's own error on the same ones)
LENGTHS = (1, 2, 3, 17, 64, 65, 130)
BATCHES = (1, 3)
HEADS = ((2, 16), (1, 32), (1, 48), (1, 64))


def case_seed(b, l, nh, dh):
    return 1000 * l + 100 * b + nh + dh


# the other cases of the GPU tests: (b, l, nh, dh, seed, input scale, dropout p, dropout seed)
EXTRA_CASES = ((1, 1024, 8, 16, 99, 1.0, 0.0, 0),            # the workload's length
               (2, 130, 2, 16, 5, 4.0, 0.0, 0),              # peaked softmax
               (2, 130, 2, 16, 11, 1.0, 0.1, 1234567),       # dropout, checked through the keep mask
               (2, 130, 2, 16, 11, 1.0, 0.5, 1234567))
