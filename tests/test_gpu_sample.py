"""GPU checks of the sampling path: the row convolution and the row attention against the formula in float64 (the project's
criterion: error at most 4 x the gap between the same formula in CPU float32 and float64, ratios printed), the categorical
draw against the float64 CDF, PriorSampler teacher-forced against the goldens, free runs, and the example."""
import argparse
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attention_ref as A
import _pixelsnail_model_ref as M
import _pixelsnail_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_CAUSAL_TAPS = 8


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


@pytest.fixture(scope="module")
def g():
    return M.load()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------- 1. row convolution
def _row_conv_case(amd, tag, n, h, w, cir, cor, kh, kw, mode, rows, relu=False):
    ops, lib = amd.ops, amd._lib.lib
    gen = _gen(sum(map(ord, tag)))
    ci, co = ops.ceil4(cir), ops.ceil4(cor)
    pad_top, pad_left = R.geometry(mode, kh, kw)
    x = torch.randn(n, cir, h, w, generator=gen)
    wt = torch.randn(cor, cir, kh, kw, generator=gen) / math.sqrt(cir * kh * kw)
    flags = 0
    if mode == "causal":
        wt[:, :, -1, kw // 2:] = 0
        flags = ROW_CAUSAL_TAPS
    bias = torch.randn(cor, generator=gen)
    res = torch.randn(n, cor, h, w, generator=gen)

    def formula(dtype, with_res):
        """[relu](conv([relu]x) + bias [+ residual]): relu = VQ2_RELU_IN | VQ2_RELU_OUT, as vq2_conv_fwd applies them"""
        xin = x.to(dtype).relu() if relu else x.to(dtype)
        y = R.conv_at(xin, wt.to(dtype), bias.to(dtype), pad_top, pad_left)
        if with_res:
            y = y + res.to(dtype)
        return y.relu() if relu else y

    want = {r: formula(torch.float64, r) for r in (False, True)}
    gaps = {r: float((formula(torch.float32, r).double() - want[r]).abs().max()) for r in (False, True)}
    gap_plain = gaps[False]
    assert gaps[False] > 0 and gaps[True] > 0
    if relu:
        flags |= ops.VQ2_RELU_IN | ops.VQ2_RELU_OUT
    spec = ops.ConvSpec.geom(cir, cor, kh, kw, pad_top, pad_left)
    wd = wt.cuda()
    wp = ops.packed_weight(spec, wd, ops.PACK_FWD)
    xn = torch.zeros(n, h, w, ci)
    xn[..., :cir] = x.permute(0, 2, 3, 1)
    rn = torch.zeros(n, h, w, co)
    rn[..., :cor] = res.permute(0, 2, 3, 1)
    layouts = {"batch-outer": (xn.cuda(), h * w * ci, w * ci),
               "row-outer": (xn.permute(1, 0, 2, 3).contiguous().cuda(), w * ci, n * w * ci)}
    full = ops.conv_forward(spec, xn.cuda(), wd, bias.cuda(), flags & 3).cpu().double()      # the existing kernel on the whole image
    d = amd._lib.ConvDesc()
    d.N, d.H, d.W, d.Ci, d.Co, d.KH, d.KW, d.pad_top, d.pad_left = n, h, w, ci, co, kh, kw, pad_top, pad_left
    d.stride, d.same_size = 1, 1
    d.ldx, d.ldy, d.Cir, d.Cor = ci, co, cir, cor
    nbytes = lib.vq2_conv_fwd_row_workspace_bytes(C.byref(d), flags)
    ws = torch.empty(nbytes // 4, device="cuda")
    bad = []
    for row in rows:
        ref = want[False][:, :, row].permute(0, 2, 1)                                            # [N, W, Cor]
        print("%s row %d: existing kernel ratio %.2f" % (tag, row, float((full[:, row, :, :cor] - ref).abs().max()) / gap_plain))
        for name, (xd, image_stride, row_stride) in layouts.items():
            for with_res in (False, True):
                rrow = rn[:, row].contiguous().cuda() if with_res else None
                outs = []
                for _ in range(2):
                    y = torch.full((n, w, co), float("nan"), device="cuda")
                    amd._lib.check(lib.vq2_conv_fwd_row(C.byref(d), row, image_stride, row_stride, flags, ops._p(xd), ops._p(wp),
                                                         ops._p(bias.cuda()), ops._p(rrow), co if with_res else 0, ops._p(y),
                                                         ops._p(ws), nbytes, ops._stream()), "conv_fwd_row")
                    outs.append(y.cpu())
                assert torch.equal(outs[0], outs[1]), (tag, row, name)                           # bit-reproducible
                assert torch.all(outs[0][..., cor:] == 0)                                        # pad lanes
                target = want[with_res][:, :, row].permute(0, 2, 1)
                err = float((outs[0][..., :cor].double() - target).abs().max())
                gap = gaps[with_res]
                print("%s row %d %s res=%d: err %.3e gap %.3e ratio %.2f" % (tag, row, name, with_res, err, gap, err / gap))
                if not err <= 4 * gap:
                    bad.append((tag, row, name, with_res, err, gap))
    assert not bad, bad


@pytest.mark.parametrize("tag,cir,cor,kh,kw,mode", [
    ("causal3x3", 6, 10, 3, 3, "causal"), ("down2x3", 6, 10, 2, 3, "down"), ("downright2x1", 6, 10, 2, 1, "downright"),
    ("causal5x5", 8, 8, 5, 5, "causal")])
def test_row_conv_against_float64(amd, tag, cir, cor, kh, kw, mode):
    _row_conv_case(amd, tag, 2, 4, 5, cir, cor, kh, kw, mode, [0, 1, 3])


def test_row_conv_relu_flags(amd):
    # VQ2_RELU_IN | VQ2_RELU_OUT, the prologue and epilogue of vq2_conv_fwd, with and without a residual
    _row_conv_case(amd, "relu3x3", 2, 4, 5, 6, 10, 3, 3, "causal", [0, 3], relu=True)


def test_row_conv_several_splits_and_ragged_tiles(amd):
    # K = 7 taps x 64 channels in 7 splits; M = 2 * 33 = 66 pixels and 68 stored output channels: no tile multiple
    _row_conv_case(amd, "wide", 2, 3, 33, 64, 66, 3, 3, "causal", [0, 2])


# ----------------------------------------------------------------------------- 2. row attention
# W = 33, third row: keys cross a 64-key block.  W = 70, second row: 70 queries at 70..139 -- two query tiles whose first
# position is no multiple of 64, and the queries themselves cross the key block boundary at 128
@pytest.mark.parametrize("dh,w,h,rows", [(4, 5, 3, [0, 1]), (8, 5, 3, [0, 1]), (8, 33, 3, [2]), (8, 70, 2, [0, 1])])
def test_row_attention(amd, dh, w, h, rows):
    ops, lib = amd.ops, amd._lib.lib
    b, nh = 2, 8
    c, l = nh * dh, h * w
    gen = _gen(11 + dh + w)
    q, k, v = (torch.randn(b, l, c, generator=gen) for _ in range(3))
    want = A.attention_core(q.double(), k.double(), v.double(), nh)
    gap = float((A.attention_core(q, k, v, nh).double() - want).abs().max())
    assert gap > 0
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    full = torch.empty(b, l, c, device="cuda")
    lse = torch.empty(b, nh, l, device="cuda")
    d = amd._lib.AttnDesc()
    d.B, d.L, d.n_head, d.dim_head = b, l, nh, dh
    d.ldq = d.ldk = d.ldv = d.ldo = c
    amd._lib.check(lib.vq2_causal_attn_fwd(C.byref(d), ops._p(qd), ops._p(kd), ops._p(vd), ops._p(full), ops._p(lse), ops._stream()), "attn")
    print("full kernel ratio %.2f" % (float((full.cpu().double() - want).abs().max()) / gap))
    # keys and values as the sampler keeps them: [H, B, W, C]
    kr = k.view(b, h, w, c).permute(1, 0, 2, 3).contiguous().cuda()
    vr = v.view(b, h, w, c).permute(1, 0, 2, 3).contiguous().cuda()
    for row in rows:
        q0 = row * w
        qrow = q[:, q0:q0 + w].contiguous().cuda()
        # rows past `row` must not be read: poison them
        kp, vp = kr.clone(), vr.clone()
        kp[row + 1:] = float("nan")
        vp[row + 1:] = float("nan")
        kp[row, :, w - 1] = float("nan")                    # nor the last query's own position: no query sees it
        vp[row, :, w - 1] = float("nan")
        o = torch.full((b, w, c), float("nan"), device="cuda")
        amd._lib.check(lib.vq2_causal_attn_fwd_rows(C.byref(d), q0, w, w, w * c, b * w * c, ops._p(qrow), ops._p(kp), ops._p(vp),
                                                    ops._p(o), ops._stream()), "attn_rows")
        err = float((o.cpu().double() - want[:, q0:q0 + w]).abs().max())
        print("dh %d W %d row %d: err %.3e gap %.3e ratio %.2f" % (dh, w, row, err, gap, err / gap))
        assert err <= 4 * gap
        assert torch.equal(o, full[:, q0:q0 + w])           # the bits of the full-sequence kernel
        if row == 0:
            assert torch.all(o[:, 0] == 0)                  # position 0 sees nothing: exactly 0
    d.p_drop = 0.5
    assert lib.vq2_causal_attn_fwd_rows(C.byref(d), 0, w, w, w * c, b * w * c, ops._p(qd), ops._p(kr), ops._p(vr), ops._p(full),
                                        ops._stream()) == 1


# ----------------------------------------------------------------------------- 3. the draw
def _uniforms(amd, m, seed, position):
    u = torch.empty(m, device="cuda")
    amd._lib.check(amd._lib.lib.vq2_sample_uniforms(amd.ops._p(u), m, seed, position, amd.ops._stream()), "uniforms")
    return u.cpu().double().numpy()


def _draw(amd, logits, n_class, temperature, seed, position):
    m = logits.shape[0]
    out = torch.full((m,), -1, device="cuda", dtype=torch.int64)
    amd._lib.check(amd._lib.lib.vq2_sample_categorical(amd.ops._p(logits), logits.shape[1], m, n_class, temperature, seed, position,
                                                       amd.ops._p(out), 1, amd.ops._stream()), "draw")
    return out.cpu().numpy()


def _check_interval(codes, u, logits64, temperature, tol):
    """Every code c has cdf[c - 1] - tol <= u <= cdf[c] + tol for the float64 softmax CDF of its row."""
    p = torch.softmax(torch.as_tensor(logits64, dtype=torch.float64) / temperature, -1).numpy()
    cdf = np.cumsum(p, -1)
    rows = np.arange(len(codes))
    lo = np.where(codes > 0, cdf[rows, np.maximum(codes - 1, 0)], 0.0)
    hi = cdf[rows, codes]
    bad = np.nonzero((lo - tol > u) | (u > hi + tol))[0]
    assert bad.size == 0, (bad[:5], codes[bad[:5]], u[bad[:5]], lo[bad[:5]], hi[bad[:5]])


@pytest.mark.parametrize("n_class", [5, 6, 512, 1000])
@pytest.mark.parametrize("temperature", [0.5, 1.0])
def test_draw_lies_in_the_float64_cdf_interval(amd, n_class, temperature):
    m, ld = 300, amd.ops.ceil4(n_class) + 4                  # padded rows; the pad lanes hold NaN and are never read
    logits = torch.full((m, ld), float("nan"))
    logits[:, :n_class] = torch.randn(m, n_class, generator=_gen(n_class)) * 3
    logits[7, 3] += 50.0                                     # one row with a dominant logit
    seed, position = 0x1234567890ABCDEF, (1 << 33) + 5
    codes = _draw(amd, logits.cuda(), n_class, temperature, seed, position)
    assert codes.min() >= 0 and codes.max() < n_class
    u = _uniforms(amd, m, seed, position)
    assert u.min() >= 0 and u.max() < 1
    _check_interval(codes, u, logits[:, :n_class].double(), temperature, n_class * 2.0 ** -23)
    assert np.array_equal(codes, _draw(amd, logits.cuda(), n_class, temperature, seed, position))       # same (seed, position)
    assert not np.array_equal(u, _uniforms(amd, m, seed, position + 1))
    assert not np.array_equal(u, _uniforms(amd, m, seed + 1, position))


def test_draw_frequencies(amd):
    n = 65536
    row = torch.tensor([0.3, -1.0, 2.0, 0.0, 1.1, -0.4, 9.0, 9.0])          # 6 classes, two pad lanes
    p = torch.softmax(row[:6].double(), 0).numpy()
    logits = row.cuda().view(1, 8)
    out = torch.empty(n, device="cuda", dtype=torch.int64)
    rc = 0
    for pos in range(n):        # one 6-class row at 65,536 positions
        rc |= amd._lib.lib.vq2_sample_categorical(amd.ops._p(logits), 8, 1, 6, 1.0, 99, pos, C.c_void_p(out.data_ptr() + 8 * pos), 1,
                                                  amd.ops._stream())
    assert rc == 0
    counts = np.bincount(out.cpu().numpy(), minlength=6).astype(np.float64)
    chi2 = float(((counts - n * p) ** 2 / (n * p)).sum())
    # critical value at p = 1e-6 for 5 degrees of freedom: the survival function of chi-square with 5 degrees of freedom is
    # erfc(sqrt(x / 2)) + sqrt(2 x / pi) exp(-x / 2) (1 + x / 3), solved by bisection
    def sf(x):
        return math.erfc(math.sqrt(x / 2)) + math.sqrt(2 * x / math.pi) * math.exp(-x / 2) * (1 + x / 3)
    lo, hi = 1.0, 200.0
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if sf(mid) > 1e-6 else (lo, mid)
    print("chi-square %.2f, critical %.2f, counts %s" % (chi2, hi, counts))
    assert 35 < hi < 40 and chi2 < hi


# ----------------------------------------------------------------------------- 4. the model, teacher-forced
def _golden_model(amd, g, ci):
    c = M.cases(g)[ci]
    m = amd.PixelSNAIL(c["shape"], c["n_class"], *c["args"], **c["kw"])
    m.load_state_dict(M.state_dict(g, ci), strict=True)
    t = f"c{ci}.in."
    ins = {k[len(t):]: torch.from_numpy(g[k]).cuda() for k in g.files if k.startswith(t)}
    return c, m.cuda().eval(), ins


@pytest.mark.parametrize("ci", [0, 1, 2, 4])
def test_teacher_forced_logits_against_the_goldens(amd, g, ci):
    c, m, ins = _golden_model(amd, g, ci)
    sampler = amd.PriorSampler(m)
    have = sampler.logits_given(ins["input"], ins.get("condition"))
    f64, f32 = M.golden_pair(g, f"c{ci}.logits")
    assert tuple(have.shape) == f64.shape
    gap = float(np.abs(f32 - f64).max())
    err = np.abs(have.double().cpu().numpy() - f64)
    print("case %d: err %.3e (row 0: %.3e), golden gap %.3e, ratio %.2f" % (ci, err.max(), err[:, :, 0].max(), gap, err.max() / gap))
    assert gap > 0 and err.max() <= 4 * gap
    # the weights are those of the moment of construction
    with torch.no_grad():
        next(m.parameters()).add_(0.0)
    with pytest.raises(RuntimeError, match="refresh"):
        sampler.logits_given(ins["input"], ins.get("condition"))
    sampler.refresh()
    assert torch.equal(sampler.logits_given(ins["input"], ins.get("condition")), have)


def test_teacher_forced_logits_kernel_size_5(amd):
    torch.manual_seed(21)
    m = amd.PixelSNAIL([5, 6], 7, 8, 5, 2, 2, 8, attention=False, n_out_res_block=1)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=_gen(p.numel())) * 0.3 + (1.0 if p.dim() == 4 and p.shape[1:] == (1, 1, 1) else 0.0))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    codes = torch.randint(0, 7, (2, 5, 6), generator=_gen(5))
    with torch.no_grad():
        want = M.pixelsnail(codes, {k: v.double() for k, v in sd.items()}, 7, False)
        gap = float((M.pixelsnail(codes, {k: v.clone() for k, v in sd.items()}, 7, False).double() - want).abs().max())
    have = amd.PriorSampler(m.cuda().eval()).logits_given(codes.cuda())
    err = float((have.double().cpu() - want).abs().max())
    print("kernel 5: err %.3e, gap %.3e, ratio %.2f" % (err, gap, err / gap))
    assert gap > 0 and err <= 4 * gap


# ----------------------------------------------------------------------------- 5. free run
@pytest.mark.parametrize("ci", [0, 1])
def test_free_run(amd, g, ci):
    c, m, ins = _golden_model(amd, g, ci)
    cond = ins.get("condition")
    b, (h, w), n_class = c["n"], c["shape"], c["n_class"]
    temperature = 0.8
    torch.manual_seed(5)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())      # what sample() takes from the default generator
    torch.manual_seed(5)
    codes = amd.sample_model(m, "cuda", b, [h, w], temperature, condition=cond)
    assert codes.shape == (b, h, w) and codes.dtype == torch.int64 and codes.is_cuda
    assert int(codes.min()) >= 0 and int(codes.max()) < n_class
    torch.manual_seed(5)
    assert torch.equal(codes, amd.sample_model(m, "cuda", b, [h, w], temperature, condition=cond))
    # sample_model's sampler lives beside the model, not on it: the model still copies and pickles, and the cache entry
    # goes with the model
    assert not any("sampler" in k for k in m.__dict__)
    import copy, gc, io, weakref
    clone = copy.deepcopy(m)
    torch.save(m, io.BytesIO())
    torch.manual_seed(5)
    assert torch.equal(codes, amd.sample_model(clone, "cuda", b, [h, w], temperature, condition=cond))
    held = weakref.ref(amd.sample._SAMPLERS[clone]["row"])
    del clone
    gc.collect()
    assert held() is None and "row" in amd.sample._SAMPLERS[m]
    sampler = amd.PriorSampler(m)
    first = sampler.sample(b, temperature, cond, seed=seed)
    assert torch.equal(first, codes)
    other = sampler.sample(b, temperature, cond, seed=seed + 1)
    assert not torch.equal(other, codes)
    assert torch.equal(sampler.sample(b, temperature, cond, seed=seed), codes)       # no history left dirty
    # every drawn code against the float64 softmax of the logits its step saw
    logits = sampler.logits_given(codes, cond)
    with torch.no_grad():
        full, _ = m(codes, condition=cond)
    delta = float((logits - full).abs().max())
    tol = 0.5 * delta / temperature + n_class * 2.0 ** -23
    print("case %d: max |logits_given - forward| %.3e, tol %.3e" % (ci, delta, tol))
    l64 = logits.double().cpu().permute(0, 2, 3, 1)
    cc = codes.cpu().numpy()
    for i in range(h):
        for j in range(w):
            u = _uniforms(amd, b, seed, i * w + j)
            _check_interval(cc[:, i, j], u, l64[:, i, j], temperature, tol)


# ----------------------------------------------------------------------------- 6. the example
def test_sample_example_runs(amd, tmp_path):
    ck = tmp_path / "checkpoint"
    ck.mkdir()
    torch.manual_seed(3)
    vq = dict(channel=16, n_res_block=1, n_res_channel=8, embed_dim=8, n_embed=6)
    torch.save(amd.VQVAE(**vq).state_dict(), str(ck / "vqvae.pt"))
    common = dict(lr=3e-4, n_res_block=1, n_res_channel=8, n_out_res_block=0, n_cond_res_block=1, dropout=0.1, size=[4, 4], n_class=6,
                  n_block=1, kernel_size=3)
    top = amd.PixelSNAIL([4, 4], 6, 64, 3, 1, 1, 8)
    torch.save({"model": top.state_dict(), "args": argparse.Namespace(hier="top", channel=64, **common)}, str(ck / "top.pt"))
    bottom = amd.PixelSNAIL([8, 8], 6, 8, 3, 1, 1, 8, attention=False, n_cond_res_block=1, cond_res_channel=8)
    torch.save({"model": bottom.state_dict(), "args": argparse.Namespace(hier="bottom", channel=8, **common)}, str(ck / "bottom.pt"))
    out = tmp_path / "sample.png"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "sample.py"), "--batch", "2", "--vqvae", "vqvae.pt", "--top", "top.pt",
           "--bottom", "bottom.pt", "--temp", "1.0", "--ckpt_dir", str(ck), "--seed", "1"] + \
          [a for k, v in vq.items() for a in ("--vqvae_arg", f"{k}={v}")] + [str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    hc, wc, _ = amd.grid_layout(2, 32, 32)                  # 8 x 8 bottom codes decode to 32 x 32 pixels
    if out.exists():
        from PIL import Image
        assert Image.open(str(out)).size == (wc, hc)
    else:
        assert np.load(str(tmp_path / "sample.npy")).shape == (hc, wc, 3)
