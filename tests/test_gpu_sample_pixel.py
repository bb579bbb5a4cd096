"""GPU checks of pixel stepping: vq2_conv_fwd_col against the formula in float64 (the project's criterion: error at most 4 x
the gap between the same formula in CPU float32 and float64, ratios printed) with every cell it must not read poisoned,
its refusals, PriorSampler(stepping='pixel') teacher-forced against the goldens, free runs, and what the programs hold."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _pixelsnail_model_ref as M
import _pixelsnail_ref as R

pytestmark = pytest.mark.gpu

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


# ----------------------------------------------------------------------------- 1. column convolution
def _desc(amd, n, h, w, ci, co, kh, kw, pad_top, pad_left, cir, cor):
    d = amd._lib.ConvDesc()
    d.N, d.H, d.W, d.Ci, d.Co, d.KH, d.KW, d.pad_top, d.pad_left = n, h, w, ci, co, kh, kw, pad_top, pad_left
    d.stride, d.same_size = 1, 1
    d.ldx, d.ldy, d.Cir, d.Cor = ci, co, cir, cor
    return d


def _col_conv_case(amd, tag, n, h, w, cir, cor, kh, kw, mode, rows, cols, relu=False, min_splits=1):
    """The yardstick of test_gpu_sample.py::_row_conv_case at single pixels.  In the 'causal' cases (VQ2_ROW_CAUSAL_TAPS)
    rows > row and row `row` from column col on hold NaN; without the flag only rows > row do."""
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
        xin = x.to(dtype).relu() if relu else x.to(dtype)
        y = R.conv_at(xin, wt.to(dtype), bias.to(dtype), pad_top, pad_left)
        if with_res:
            y = y + res.to(dtype)
        return y.relu() if relu else y

    want = {r: formula(torch.float64, r) for r in (False, True)}
    gaps = {r: float((formula(torch.float32, r).double() - want[r]).abs().max()) for r in (False, True)}
    assert gaps[False] > 0 and gaps[True] > 0
    if relu:
        flags |= ops.VQ2_RELU_IN | ops.VQ2_RELU_OUT
    spec = ops.ConvSpec.geom(cir, cor, kh, kw, pad_top, pad_left)
    wp = ops.packed_weight(spec, wt.cuda(), ops.PACK_FWD)
    xn = torch.zeros(n, h, w, ci)
    xn[..., :cir] = x.permute(0, 2, 3, 1)
    rn = torch.zeros(n, h, w, co)
    rn[..., :cor] = res.permute(0, 2, 3, 1)
    d = _desc(amd, n, h, w, ci, co, kh, kw, pad_top, pad_left, cir, cor)
    nbytes = lib.vq2_conv_fwd_col_workspace_bytes(C.byref(d), flags)
    assert nbytes >= min_splits * n * co * 4 and nbytes % (n * co * 4) == 0
    ws = torch.empty(nbytes // 4, device="cuda")
    bd = bias.cuda()
    bad, ratios = [], []
    for row in rows:
        for col in cols:
            xp = xn.clone()
            xp[:, row + 1:] = float("nan")
            if mode == "causal":
                xp[:, row, col:] = float("nan")
            layouts = {"batch-outer": (xp.cuda(), h * w * ci, w * ci),
                       "row-outer": (xp.permute(1, 0, 2, 3).contiguous().cuda(), w * ci, n * w * ci)}
            for name, (xd, image_stride, row_stride) in layouts.items():
                for with_res in (False, True):
                    rcol = rn[:, row, col].contiguous().cuda() if with_res else None
                    outs = []
                    for _ in range(2):
                        y = torch.full((n, co), float("nan"), device="cuda")
                        amd._lib.check(lib.vq2_conv_fwd_col(C.byref(d), row, col, image_stride, row_stride, flags, ops._p(xd),
                                                             ops._p(wp), ops._p(bd), ops._p(rcol), co if with_res else 0, ops._p(y),
                                                             ops._p(ws), nbytes, ops._stream()), "conv_fwd_col")
                        outs.append(y.cpu())
                    assert bool(torch.isfinite(outs[0]).all()), (tag, row, col, name)             # no poisoned cell was read
                    assert torch.equal(outs[0], outs[1]), (tag, row, col, name)                     # bit-reproducible
                    assert torch.all(outs[0][:, cor:] == 0)                                         # pad lanes
                    target = want[with_res][:, :, row, col]
                    err = float((outs[0][:, :cor].double() - target).abs().max())
                    gap = gaps[with_res]
                    ratios.append(err / gap)
                    if not err <= 4 * gap:
                        bad.append((tag, row, col, name, with_res, err, gap))
    print("%s: %d pixels x layouts x residual, err / gap in %.2f .. %.2f" % (tag, len(rows) * len(cols), min(ratios), max(ratios)))
    assert not bad, bad


@pytest.mark.parametrize("tag,cir,cor,kh,kw,mode", [
    ("causal3x3", 6, 10, 3, 3, "causal"), ("down2x3", 6, 10, 2, 3, "down"), ("downright2x1", 6, 10, 2, 1, "downright"),
    ("causal5x5", 8, 8, 5, 5, "causal")])
def test_col_conv_against_float64(amd, tag, cir, cor, kh, kw, mode):
    _col_conv_case(amd, tag, 2, 4, 5, cir, cor, kh, kw, mode, [0, 1, 3], [0, 1, 4])


# 17 crosses a 16-image tile (the four-tile kernel), 65 a 64-image workgroup
@pytest.mark.parametrize("n", [1, 3, 17, 65])
def test_col_conv_batch_sizes(amd, n):
    _col_conv_case(amd, "batch%d" % n, n, 4, 5, 6, 10, 3, 3, "causal", [0, 3], [0, 4])


def test_col_conv_width_one(amd):
    _col_conv_case(amd, "w1", 2, 4, 1, 6, 10, 3, 3, "causal", [0, 1, 3], [0])


def test_col_conv_relu_flags(amd):
    _col_conv_case(amd, "relu3x3", 2, 4, 5, 6, 10, 3, 3, "causal", [0, 3], [0, 1, 4], relu=True)


def test_col_conv_several_splits_and_ragged_tiles(amd):
    # 7 taps x 64 channels: 7 steps in several splits; 68 stored output channels are three 32-channel workgroups, the last
    # one ragged; 3 images in a 16-image tile
    _col_conv_case(amd, "wide", 3, 3, 5, 64, 66, 3, 3, "causal", [0, 2], [0, 2, 4], min_splits=2)


def test_col_conv_several_channel_blocks(amd):
    # 136 input channels: three 64-channel steps per tap, the last one 8 channels wide (waves 1 .. 3 idle in it)
    _col_conv_case(amd, "blocks", 2, 3, 4, 134, 12, 3, 3, "causal", [2], [0, 3], min_splits=2)


# ----------------------------------------------------------------------------- 2. refusals
def test_col_conv_refusals(amd):
    ops, lib = amd.ops, amd._lib.lib
    n, h, w, c = 2, 4, 5, 8
    d = _desc(amd, n, h, w, c, c, 3, 3, 2, 1, c, c)
    nbytes = lib.vq2_conv_fwd_col_workspace_bytes(C.byref(d), ROW_CAUSAL_TAPS)
    x = torch.randn(n, h, w, c, device="cuda")
    wp = torch.randn(c * c * 9, device="cuda")
    ws = torch.zeros(nbytes // 4 + 4, device="cuda")
    y = torch.full((n, c), 7.0, device="cuda")

    def call(desc, row, col, ws_bytes):
        return lib.vq2_conv_fwd_col(C.byref(desc), row, col, h * w * c, w * c, ROW_CAUSAL_TAPS, ops._p(x), ops._p(wp), None, None, 0,
                                    ops._p(y), ops._p(ws), ws_bytes, ops._stream())

    assert call(d, 0, w, nbytes) == 1
    assert call(d, 0, -1, nbytes) == 1
    assert call(d, h, 0, nbytes) == 1
    assert call(d, 0, 0, nbytes - 1) == 1
    bad = _desc(amd, n, h, w, c, c, 3, 3, 1, 1, c, c)                      # pad_top != KH - 1
    assert call(bad, 0, 0, nbytes) == 1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call(d, 0, 0, nbytes) == 0                                       # the same call, accepted
    torch.cuda.synchronize()
    assert not bool((y == 7.0).any())


# ----------------------------------------------------------------------------- 3. the model, teacher-forced
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
    have = amd.PriorSampler(m, stepping="pixel").logits_given(ins["input"], ins.get("condition"))
    f64, f32 = M.golden_pair(g, f"c{ci}.logits")
    assert tuple(have.shape) == f64.shape
    gap = float(np.abs(f32 - f64).max())
    err = np.abs(have.double().cpu().numpy() - f64)
    row = np.abs(amd.PriorSampler(m).logits_given(ins["input"], ins.get("condition")).double().cpu().numpy() - f64).max()
    print("case %d: pixel err %.3e (row 0: %.3e, column 0: %.3e), golden gap %.3e, ratio %.2f; row stepping ratio %.2f"
          % (ci, err.max(), err[:, :, 0].max(), err[:, :, :, 0].max(), gap, err.max() / gap, row / gap))
    assert gap > 0 and err.max() <= 4 * gap


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
    have = amd.PriorSampler(m.cuda().eval(), stepping="pixel").logits_given(codes.cuda())
    err = float((have.double().cpu() - want).abs().max())
    print("kernel 5: err %.3e, gap %.3e, ratio %.2f" % (err, gap, err / gap))
    assert gap > 0 and err <= 4 * gap


# ----------------------------------------------------------------------------- 4. free runs
def _uniforms(amd, m, seed, position):
    u = torch.empty(m, device="cuda")
    amd._lib.check(amd._lib.lib.vq2_sample_uniforms(amd.ops._p(u), m, seed, position, amd.ops._stream()), "uniforms")
    return u.cpu().double().numpy()


def _check_interval(codes, u, logits64, temperature, tol):
    """Every code c has cdf[c - 1] - tol <= u <= cdf[c] + tol for the float64 softmax CDF of its row."""
    p = torch.softmax(torch.as_tensor(logits64, dtype=torch.float64) / temperature, -1).numpy()
    cdf = np.cumsum(p, -1)
    rows = np.arange(len(codes))
    lo = np.where(codes > 0, cdf[rows, np.maximum(codes - 1, 0)], 0.0)
    hi = cdf[rows, codes]
    bad = np.nonzero((lo - tol > u) | (u > hi + tol))[0]
    assert bad.size == 0, (bad[:5], codes[bad[:5]], u[bad[:5]], lo[bad[:5]], hi[bad[:5]])


@pytest.mark.parametrize("ci", [0, 1])
def test_free_run(amd, g, ci):
    c, m, ins = _golden_model(amd, g, ci)
    cond = ins.get("condition")
    b, (h, w), n_class = c["n"], c["shape"], c["n_class"]
    temperature, seed = 0.8, 0x5EED0 + ci
    sampler = amd.PriorSampler(m, stepping="pixel")
    codes = sampler.sample(b, temperature, cond, seed=seed)
    assert codes.shape == (b, h, w) and codes.dtype == torch.int64 and codes.is_cuda
    assert int(codes.min()) >= 0 and int(codes.max()) < n_class
    assert torch.equal(codes, sampler.sample(b, temperature, cond, seed=seed))          # the same seed: the same bits
    assert not torch.equal(codes, sampler.sample(b, temperature, cond, seed=seed + 1))
    torch.manual_seed(5)
    drawn = int(torch.randint(0, 2 ** 62, (1,)).item())      # what sample() takes from the default generator
    torch.manual_seed(5)
    via = amd.sample_model(m, "cuda", b, [h, w], temperature, condition=cond, stepping="pixel")
    assert torch.equal(via, sampler.sample(b, temperature, cond, seed=drawn))
    assert amd.sample._SAMPLERS[m]["pixel"].stepping == "pixel" and "row" not in amd.sample._SAMPLERS[m]
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
            _check_interval(cc[:, i, j], _uniforms(amd, b, seed, i * w + j), l64[:, i, j], temperature, tol)
    # a prefix of 2 rows stays; the first free step (2, 0) saw the logits logits_given has there: its log-probability
    done, logp = sampler.sample(b, temperature, cond, seed=seed + 2, prefix=codes[:, :2].contiguous(), return_logp=True)
    assert torch.equal(done[:, :2], codes[:, :2]) and bool((logp[:, :2] == 0).all())
    given = sampler.logits_given(done, cond).double().cpu()[:, :, 2, 0]                 # [B, n_class]
    want = torch.log_softmax(given / temperature, -1).gather(1, done[:, 2, :1].cpu())[:, 0]
    step = float((logp[:, 2, 0].double().cpu() - want).abs().max())
    print("case %d: first free step |logp - log_softmax(logits_given)| %.3e" % (ci, step))
    assert step <= 1e-5
    # the filtered draw
    cut, lp = sampler.sample(b, temperature, cond, seed=seed, top_k=3, top_p=0.9, return_logp=True)
    assert cut.shape == (b, h, w) and lp.shape == (b, h, w) and lp.dtype == torch.float32
    assert bool(torch.isfinite(lp).all()) and float(lp.max()) <= 0


# ----------------------------------------------------------------------------- 5. programs
def _expected_calls(m, row, conditioned, multi_row):
    """The library calls of one step of row `row`, from the model's structure alone; multi_row names the call of a conv over
    several rows."""
    def gated(causal, aux=False, cond=False):
        conv = multi_row if causal else "conv_fwd"
        return (["elu_fwd", "conv_fwd"] if aux else []) + ["elu_fwd", conv, "elu_fwd"] + (["conv_fwd"] if cond else []) + \
               [conv, "glu_res_fwd"]

    calls = (["onehot_conv_fwd"] if row > 0 else []) + ["onehot_conv_fwd", "slice_copy"]
    for block in m.blocks:
        for _ in block.resblocks:
            calls += gated(True, cond=conditioned)
        if block.attention:
            calls += ["slice_copy"] * 3 + gated(False) + ["slice_copy"] * 2 + gated(False)
            calls += ["conv_fwd"] * 3 + ["causal_attn_fwd_rows"] + gated(False, aux=True)
        else:
            calls += ["slice_copy"] * 2 + ["conv_fwd"]
    for _ in range(len(m.out) - 2):
        calls += gated(False)
    return calls + ["elu_fwd", "conv_fwd"]


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_programs(amd, g, ci):
    c, m, ins = _golden_model(amd, g, ci)
    cond = ins.get("condition")
    b, (h, w) = c["n"], c["shape"]
    row = amd.PriorSampler(m)                               # the default
    assert row.stepping == "row"
    row.logits_given(ins["input"], cond)
    plan = row._plan[1]
    # a row-mode plan has no pixel programs: a step runs the row's program, and no column buffer exists
    assert type(plan).__name__ == "_Plan" and plan.step_programs is plan.row_programs and len(plan.row_programs) == h
    assert not any(name.startswith("px.") for name in plan.bufs)
    for i in range(h):
        calls = plan.row_programs[i].calls
        assert [call[2] for call in calls] == _expected_calls(m, i, cond is not None, "conv_fwd_row"), i
        _check_row_program(amd, calls, i, w)
    pix = amd.PriorSampler(m, stepping="pixel")
    pix.logits_given(ins["input"], cond)
    plan = pix._plan[1]
    assert type(plan).__name__ == "_Plan" and plan.step_programs is not plan.row_programs
    for i in range(h):
        names = [call[2] for call in plan.step_programs[i].calls]
        assert "conv_fwd_col" in names and "conv_fwd_row" not in names
        assert names == _expected_calls(m, i, cond is not None, "conv_fwd_col"), i
        calls = plan.row_programs[i].calls
        assert [call[2] for call in calls] == _expected_calls(m, i, cond is not None, "conv_fwd_row"), i
        _check_row_program(amd, calls, i, w)
        _check_pixel_program(amd, plan, plan.step_programs[i].calls, i, w)
    # recorded per row, not per pixel: h programs, each with as many calls as a step makes
    assert len(plan.step_programs) == h and len(plan.row_programs) == h


def _check_row_program(amd, calls, i, w):
    """No argument of a row program moves; the attention takes the row's W queries."""
    for fn, args, what, moving in calls:
        assert not moving and not any(isinstance(a, amd.sample._Moving) for a in args), what
        if what == "causal_attn_fwd_rows":                   # (desc, q0, nq, ...)
            assert (args[1], args[2]) == (i * w, w)


def _check_pixel_program(amd, plan, calls, i, w):
    """The arguments of step (i, j), resolved as run(j) resolves them but without a launch: the column conv is at (i, j), the
    attention takes the one query i * W + j, and every pointer that moves does so by the channels of the buffer it addresses."""
    Moving = amd.sample._Moving
    held = list(plan.bufs.values()) + [plan.bg_rows] + ([plan.cond_rows] if plan.cond_rows is not None else [])

    def channels_at(address):
        owners = [t for t in held if t.data_ptr() <= address < t.data_ptr() + t.numel() * t.element_size()]
        assert len(owners) == 1, address
        return owners[0].shape[3]

    # the integers that move, where the C signatures have them: (desc, row, col, ...) and (desc, q0, nq, ...)
    moving_ints = {"conv_fwd_col": [2], "causal_attn_fwd_rows": [1]}
    n_pointers = 0
    for j in sorted({0, w - 1}):
        for fn, args, what, moving in calls:
            assert all(k in dict(moving) for k, a in enumerate(args) if isinstance(a, Moving)), what      # none left unpatched
            at = list(args)
            for k, a in moving:
                assert isinstance(a, Moving)
                at[k] = a.at(j)
            assert [k for k, a in moving if not a.pointer] == moving_ints.get(what, []), what
            if what == "conv_fwd_col":
                assert (at[1], at[2]) == (i, j)
            if what == "causal_attn_fwd_rows":
                assert (at[1], at[2]) == (i * w + j, 1)
            for k, a in moving:
                if a.pointer:
                    n_pointers += 1
                    assert at[k].value == a.at(0).value + j * 4 * channels_at(a.at(0).value), (what, k)
    assert n_pointers > 0
