"""GPU checks of the stage-2 GatedResBlock work: the same_size form of vq2_conv_desc against float64 torch, the two
forms of the descriptor bit for bit where both can state a layer, causality, the ELU / ELU+dropout / GLU kernels against float64, the dropout
decisions, and the modules against the goldens captured from the reference."""
import ctypes
import glob
import json
import os
import re
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _pixelsnail_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def ceil4(c):
    return (c + 3) // 4 * 4


def to_dev_nhwc(t):
    """[N,C,H,W] float64 CPU -> float32 NHWC on the GPU with ceil4(C) stored channels, pad lanes 0."""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, ceil4(c), dtype=torch.float32)
    out[..., :c] = t.permute(0, 2,3, 1).float()
    return out.cuda()


def from_dev_nhwc(t, c):
    return t[..., :c].permute(0, 3, 1, 2).double().cpu()


# ----------------------------------------------------------------------------------------------- geometry against float64
# (KH, KW, pad_top, pad_left) of the issue, each on the three image sizes (smaller than the kernel, one pixel, and
# M = 2 * 9 * 8 = 144 rows: past the 128-row tile), with the channel counts dealt round over them: Ci 4, 6 -> 8, 36, 64
# (uniform chunks with the taps innermost: Ci > 32, Ci % 32 == 0), Co 4, 36, 132, and 5 -> 8 real channels on both sides
KERNELS = [(5, 5, 4, 2), (3, 3, 2, 1), (2, 5, 1, 2), (3, 2, 2, 1), (1, 3, 0, 1), (7, 4, 6, 3), (1, 1, 0, 0)]
IMAGES = [(2, 1, 1), (2, 3, 2), (2, 9, 8)]
CHANNELS = [(4, 4), (6, 36), (64, 132), (36, 5), (5, 5), (64, 4), (4, 132)]


def _geometry_cases():
    out = []
    i = 0
    for k in KERNELS:
        for img in IMAGES:
            cin, cout = CHANNELS[i % len(CHANNELS)]
            out.append((k, img, cin, cout, i % 2 == 1, i % 5 == 0))
            i += 1
    for k in ((5, 5, 4, 2), (2, 5, 1, 2), (3, 2, 2, 1), (7, 4, 6, 3)):   # every kernel with several taps on the tap-inner branch
        out.append((k, (2, 9, 8), 64, 36, False, False))
    out.append(((5, 5, 4, 2), (1, 4, 4), 256, 8, False, False))           # reduction depth 6,400
    return out


def _gid(c):
    (kh, kw, pt, pl), (n, h, w), cin, cout, relu, res = c
    return f"k{kh}x{kw}p{pt}_{pl}-{n}x{h}x{w}-{cin}to{cout}" + ("-relu" if relu else "") + ("-res" if res else "")


def _geometry_reference(c, d, dtype):
    (kh, kw, pt, pl), _, cin, cout, relu, res = c
    x = d["x"].detach().to(dtype).clone().requires_grad_(True)
    w = d["w"].detach().to(dtype).clone().requires_grad_(True)
    b = d["b"].detach().to(dtype).clone().requires_grad_(True)
    y = R.conv_at(F.relu(x) if relu else x, w, b, pt, pl)
    if res:
        y = y + d["res"].detach().to(dtype)
    y.backward(d["dy"].detach().to(dtype))
    return {"y": y.detach().double(), "dx": x.grad.double(), "dw": w.grad.double(), "db": b.grad.double()}


@pytest.mark.parametrize("case", _geometry_cases(), ids=_gid)
def test_geometry_against_fp64(amd, case):
    ops = amd.ops
    (kh, kw, pt, pl), (n, h, w), cin, cout, relu, res = case
    g = torch.Generator().manual_seed(zlib.crc32(_gid(case).encode()))
    d = {"x": torch.randn(n, cin, h, w, generator=g, dtype=torch.float64),
         "w": torch.randn(cout, cin, kh, kw, generator=g, dtype=torch.float64) / (cin * kh * kw) ** 0.5,
         "b": torch.randn(cout, generator=g, dtype=torch.float64),
         "dy": torch.randn(n, cout, h, w, generator=g, dtype=torch.float64),
         "res": torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)}
    d = {k: v.float().double() for k, v in d.items()}          # the values the GPU sees
    ref = _geometry_reference(case, d, torch.float64)
    spec = ops.ConvSpec.geom(cin, cout, kh, kw, pt, pl)
    x, dy = to_dev_nhwc(d["x"]), to_dev_nhwc(d["dy"])
    wt, bias = d["w"].float().cuda(), d["b"].float().cuda()
    resid = to_dev_nhwc(d["res"]) if res else None
    y = ops.conv_forward(spec, x, wt, bias, ops.VQ2_RELU_IN if relu else 0, resid)
    dx = ops.conv_dgrad(spec, x.shape, dy, wt, mask=x if relu else None)
    dw, db = ops.conv_wgrad(spec, x, dy, relu, wt, bias)
    torch.cuda.synchronize()
    assert y.shape == (n, h, w, ceil4(cout)) and dx.shape == (n, h, w, ceil4(cin))
    assert float(y[..., cout:].abs().sum()) == 0 and float(dx[..., cin:].abs().sum()) == 0      # pad lanes
    got = {"y": from_dev_nhwc(y, cout), "dx": from_dev_nhwc(dx, cin), "dw": dw.double().cpu(), "db": db.double().cpu()}
    depth = {"y": kh * kw * cin, "dx": kh * kw * cout, "dw": n * h * w, "db": n * h * w}
    ref32 = None
    for k in ("y", "dx", "dw", "db"):
        scale = float(ref[k].abs().max())
        tol = (5e-6 if k in ("y", "dx") else 1e-5) * scale
        if depth[k] > 4096:     # past the project's depth: max(project tolerance, 4 x the error of plain fp32 torch on the CPU)
            ref32 = ref32 or _geometry_reference(case, d, torch.float32)
            err32 = float((ref32[k] - ref[k]).abs().max())
            tol = max(tol, 4 * err32)
            print("deep %s %s: fp32-vs-fp64 max err %.3e, tolerance %.3e (%.3e of max|ref|)" % (_gid(case), k, err32, tol, tol / scale))
        err = float((got[k] - ref[k]).abs().max())
        print("%s %s: err %.3e = %.3f of the tolerance" % (_gid(case), k, err, err / tol if tol else 0.0))
        assert err <= tol, (k, err, tol)


@pytest.mark.parametrize("cin,cout,k,n,h,w", [(8, 12, 3, 2, 9, 8), (64, 64, 3, 1, 8, 32), (6, 36, 1, 2, 9, 8), (64, 128, 1, 1, 8, 32)])
def test_old_and_new_descriptor_agree_bitwise(amd, cin, cout, k, n, h, w):
    ops = amd.ops
    old, new = ops.ConvSpec(False, cin, cout, k, 1, k // 2), ops.ConvSpec.geom(cin, cout, k, k, k // 2, k // 2)
    g = torch.Generator().manual_seed(5)
    x = to_dev_nhwc(torch.randn(n, cin, h, w, generator=g, dtype=torch.float64))
    dy = to_dev_nhwc(torch.randn(n, cout, h, w, generator=g, dtype=torch.float64))
    wt, bias = torch.randn(cout, cin, k, k, generator=g).cuda(), torch.randn(cout, generator=g).cuda()
    outs = []
    for spec in (old, new):
        w2 = wt.clone()      # (the packed panels are cached on the weight tensor, per spec)
        y = ops.conv_forward(spec, x, w2, bias, ops.VQ2_RELU_IN)
        dx = ops.conv_dgrad(spec, x.shape, dy, w2, mask=x)
        dw, db = ops.conv_wgrad(spec, x, dy, True, w2, bias)
        outs.append((y, dx, dw, db))
    torch.cuda.synchronize()
    for a, b, name in zip(outs[0], outs[1], ("y", "dx", "dw", "db")):
        assert torch.equal(a, b), name


# ----------------------------------------------------------------------------------------------- causality
@pytest.mark.parametrize("k,padding,shift", [(5, "causal", False), ([3, 2], "downright", True)])
def test_causality(amd, k, padding, shift):
    torch.manual_seed(3)
    m = amd.CausalConv2d(4, 8, k, padding=padding).cuda()
    n, h, w = 1, 6, 7
    h0, w0 = 3, 4
    x = torch.randn(n, 4, h, w, device="cuda")

    def run(inp):
        return m(R.shift_right(inp) if shift else inp)

    y0 = run(x).clone()
    if padding == "causal":
        assert float(m.conv.conv.weight_v[:, :, -1, 2:].abs().max()) == 0          # the parameter itself, after a forward
        assert float(m.conv.conv.weight_v[:, :, -1, :2].abs().min()) > 0
    x1 = x.clone()
    x1[:, :, h0, w0] += 1.5
    y1 = run(x1)
    raster = torch.arange(h * w, device="cuda").view(h, w)
    upto = raster <= h0 * w + w0
    assert torch.equal(y0[:, :, upto], y1[:, :, upto])
    assert not torch.equal(y0, y1)
    xg = x.clone().requires_grad_(True)
    gout = torch.zeros(n, 8, h, w, device="cuda")
    gout[:, :, h0, w0] = torch.randn(n, 8, device="cuda")
    (run(xg) * gout).sum().backward()
    assert float(xg.grad[:, :, raster >= h0 * w + w0].abs().max()) == 0
    assert float(xg.grad.abs().max()) > 0


# ----------------------------------------------------------------------------------------------- elementwise kernels
def _probe_values(count, gen):
    special = torch.tensor([0.0, -0.0, 1e-5, -1e-5, 3e-5, -7e-5, 9.9e-5, -9.9e-5, 20.0, -20.0, 1.0, -1.0])
    v = torch.empty(count).uniform_(-20, 20, generator=gen)
    v[:special.numel()] = special
    v[special.numel():2 * special.numel()] = torch.empty(special.numel()).uniform_(-1e-4, 1e-4, generator=gen)
    return v[torch.randperm(count, generator=gen)]


def _strided(vals, pixels, c, extra):
    """[pixels, c] values inside a device buffer of pixel stride ceil4(c) + extra whose other lanes hold 7."""
    ld = ceil4(c) + extra
    buf = torch.full((pixels, ld), 7.0)
    buf[:, :c] = vals
    return buf.cuda(), ld


def _check_rows(buf, c, what):
    """pad lanes are exactly 0, lanes beyond ceil4(c) untouched (NaN)"""
    assert float(buf[:, c:ceil4(c)].abs().sum()) == 0, what
    assert bool(torch.isnan(buf[:, ceil4(c):]).all()), what


def _bound(name, got, ref64, ref32):
    err = float((got.double() - ref64).abs().max())
    err32 = float((ref32.double() - ref64).abs().max())
    print("%s: err %.3e, fp32 torch %.3e, ratio %.2f" % (name, err, err32, err / err32 if err32 else float("inf") if err else 0.0))
    assert err <= 4 * err32, name


@pytest.mark.parametrize("c", [4, 5, 6, 7, 514])
def test_elementwise_kernels_against_fp64(amd, c):
    L = amd._lib.lib
    check = amd._lib.check
    S = amd.ops._stream()          # torch's current stream: the fills before and the reads after each call are ordered on it
    gen = torch.Generator().manual_seed(100 + c)
    pixels = 37 if c < 100 else 5
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    nan = lambda ld: torch.full((pixels, ld), float("nan"), device="cuda")
    x32 = _probe_values(pixels * c, gen).view(pixels, c)
    dy32 = torch.randn(pixels, c, generator=gen)
    x64, dy64 = x32.double(), dy32.double()
    xb, ldx = _strided(x32, pixels, c, 8)
    dyb, lddy = _strided(dy32, pixels, c, 4)

    # ELU forward, backward from y
    yb = nan(ceil4(c) + 12)
    check(L.vq2_elu_fwd(P(xb), ldx, P(yb), yb.shape[1], pixels, c, S), "elu_fwd")
    _check_rows(yb, c, "elu_fwd")
    y64 = torch.where(x64 > 0, x64, torch.expm1(x64))
    _bound(f"elu_fwd C={c}", yb[:, :c].cpu(), y64, torch.where(x32 > 0, x32, torch.expm1(x32)))
    y32 = yb[:, :c].cpu()                          # the backward's operand is the forward's output
    dxb = nan(ceil4(c) + 4)
    check(L.vq2_elu_bwd(P(dyb), lddy, P(yb), yb.shape[1], P(dxb), dxb.shape[1], pixels, c, S), "elu_bwd")
    _check_rows(dxb, c, "elu_bwd")
    _bound(f"elu_bwd C={c}", dxb[:, :c].cpu(), dy64 * torch.where(y32 > 0, 1.0, y32.double() + 1.0),
           dy32 * torch.where(y32 > 0, torch.ones(()), y32 + 1.0))

    # ELU + dropout forward, backward from x
    for p in (0.1, 0.5):
        seed = 0x123456789ABCDEF + c
        keep = amd.ops.dropout_keep_mask(pixels, c, p, seed, "cuda").cpu()
        hb = nan(ceil4(c) + 8)
        check(L.vq2_elu_dropout_fwd(P(xb), ldx, P(hb), hb.shape[1], pixels, c, p, seed, S), "elu_dropout_fwd")
        _check_rows(hb, c, "elu_dropout_fwd")
        assert bool(((hb[:, :c].cpu() == 0) | keep).all())
        _bound(f"elu_dropout_fwd C={c} p={p}", hb[:, :c].cpu(), y64 * keep.double() / (1.0 - p),
               torch.where(x32 > 0, x32, torch.expm1(x32)) * keep.float() / (1.0 - p))
        gxb = nan(ceil4(c) + 4)
        check(L.vq2_elu_dropout_bwd(P(dyb), lddy, P(xb), ldx, P(gxb), gxb.shape[1], pixels, c, p, seed, S), "elu_dropout_bwd")
        _check_rows(gxb, c, "elu_dropout_bwd")
        _bound(f"elu_dropout_bwd C={c} p={p}", gxb[:, :c].cpu(),
               dy64 * keep.double() / (1.0 - p) * torch.where(x64 > 0, 1.0, torch.exp(x64)),
               dy32 * keep.float() / (1.0 - p) * torch.where(x32 > 0, torch.ones(()), torch.exp(x32)))

    # GLU + residual: Ch = c, t has 2 c real channels
    t32 = _probe_values(pixels * 2 * c, gen).view(pixels, 2 * c)
    r32 = torch.randn(pixels, c, generator=gen)
    tb, ldt = _strided(t32, pixels, 2 * c, 8)
    rb, ldr = _strided(r32, pixels, c, 4)
    ob = nan(ceil4(c) + 4)
    check(L.vq2_glu_res_fwd(P(tb), ldt, P(rb), ldr, P(ob), ob.shape[1], pixels, c, S), "glu_res_fwd")
    _check_rows(ob, c, "glu_res_fwd")
    a64, b64, a32, b32 = t32[:, :c].double(), t32[:, c:].double(), t32[:, :c], t32[:, c:]
    _bound(f"glu_res_fwd Ch={c}", ob[:, :c].cpu(), a64 * torch.sigmoid(b64) + r32.double(), a32 * torch.sigmoid(b32) + r32)
    dtb = nan(ceil4(2 * c) + 8)
    check(L.vq2_glu_res_bwd(P(dyb), lddy, P(tb), ldt, P(dtb), dtb.shape[1], pixels, c, S), "glu_res_bwd")
    _check_rows(dtb, 2 * c, "glu_res_bwd")
    s64, s32 = torch.sigmoid(b64), torch.sigmoid(b32)
    _bound(f"glu_res_bwd da Ch={c}", dtb[:, :c].cpu(), dy64 * s64, dy32 * s32)
    _bound(f"glu_res_bwd db Ch={c}", dtb[:, c:2 * c].cpu(), dy64 * a64 * s64 * (1 - s64), dy32 * a32 * s32 * (1 - s32))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- dropout
def _module_seed(torch_seed):
    """The integer the module draws from torch's CPU generator after torch.manual_seed(torch_seed)."""
    torch.manual_seed(torch_seed)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(torch_seed)
    return seed


def _run_module(m, ins, gout):
    xs = {k: v.detach().float().cuda().requires_grad_(True) for k, v in ins.items()}
    m.zero_grad()
    out = m(xs["input"], *([xs["aux"]] if "aux" in xs else []), **({"condition": xs["condition"]} if "condition" in xs else {}))
    (out * gout.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.double().cpu() for k, v in xs.items()}
    grads.update({k: p.grad.double().cpu() for k, p in m.named_parameters()})
    return out.detach().double().cpu(), grads


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_train_mode_matches_the_formula_with_the_written_mask(amd, p):
    n, cin, ch, h, w = 2, 5, 6, 5, 7                       # the dropped tensor is [2, 5, 7, 6] in NHWC
    torch.manual_seed(11)
    m = amd.GatedResBlock(cin, ch, 3, conv="causal", dropout=p).cuda().train()
    with torch.no_grad():
        for q in m.parameters():
            q.mul_(1.0 + 0.25 * torch.randn_like(q))
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ins = {"input": torch.randn(n, cin, h, w)}
    gout = torch.randn(n, cin, h, w)
    seed = _module_seed(77)
    keep = amd.ops.dropout_keep_mask(n * h * w, ch, p, seed, "cuda").view(n, h, w, ch).permute(0, 3, 1, 2).cpu()
    out, grads = _run_module(m, ins, gout)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        s2 = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        x = ins["input"].to(dtype).requires_grad_(True)
        o = R.gated_resblock(x, s2, "causal", keep=keep, p=p)
        (o * gout.to(dtype)).sum().backward()
        refs[dtype] = {"out": o.detach().double(), "input": x.grad.double(), **{k: v.grad.double() for k, v in s2.items()}}
    have = {"out": out, **grads}
    assert sorted(have) == sorted(refs[torch.float64])
    for k in have:
        _bound(f"train p={p} {k}", have[k], refs[torch.float64][k], refs[torch.float32][k])
    # the same seed gives the same bits
    torch.manual_seed(77)
    out2, grads2 = _run_module(m, ins, gout)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    out3, _ = _run_module(m, ins, gout)                    # the generator has moved on: another mask
    assert not torch.equal(out, out3)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_fraction(amd, p):
    keep = amd.ops.dropout_keep_mask(1 << 10, 1 << 6, p, 987654321, "cuda")
    frac = float(keep.float().mean())
    sigma = (p * (1 - p) / (1 << 16)) ** 0.5
    print("p=%.1f kept %.5f, expected %.5f, %.2f sigma" % (p, frac, 1 - p, (frac - (1 - p)) / sigma))
    assert abs(frac - (1 - p)) <= 5 * sigma


def test_no_draw_without_dropout(amd):
    x = torch.randn(1, 8, 4, 4, device="cuda")
    m0 = amd.GatedResBlock(8, 8, 3, dropout=0.0).cuda().train()
    m1 = amd.GatedResBlock(8, 8, 3, dropout=0.1).cuda().eval()
    for m in (m0, m1):
        state = torch.get_rng_state()
        m(x)
        assert torch.equal(state, torch.get_rng_state())
    state = torch.get_rng_state()
    m1.train()(x)
    assert not torch.equal(state, torch.get_rng_state())


# ----------------------------------------------------------------------------------------------- modules against the goldens
def _cases(g):
    return json.loads(str(g["cases"]))


def _build(amd, c):
    if c["kind"] == "conv":
        return amd.CausalConv2d(c["cin"], c["ch"], c["k"], padding=c["conv"])
    return amd.GatedResBlock(c["cin"], c["ch"], c["k"], conv=c["conv"], auxiliary_channel=c["aux"], condition_dim=c["cond"])


def _golden_module(amd, g, ci):
    c = _cases(g)[ci]
    t = f"c{ci}."
    m = _build(amd, c)
    names = [k[len(t) + 3:] for k in g.files if k.startswith(t + "sd.")]
    m.load_state_dict({k: torch.from_numpy(g[t + "sd." + k]) for k in names}, strict=True)
    assert sorted(m.state_dict().keys()) == sorted(names)
    ins = {k[len(t) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(t + "in.") and k != t + "in.gout"}
    return c, m.cuda().eval(), ins, torch.from_numpy(g[t + "in.gout"])


@pytest.mark.parametrize("ci", range(9))
def test_modules_against_the_goldens(amd, golden, ci):
    g = golden("pixelsnail_gated_resblock")
    assert len(_cases(g)) == 9
    c, m, ins, gout = _golden_module(amd, g, ci)
    t = f"c{ci}."
    out, grads = _run_module(m, ins, gout)
    have = {"out": out, **{"grad." + k: v for k, v in grads.items()}}
    want = ["out"] + ["grad." + k[len(t) + 9:] for k in g.files if k.startswith(t + "grad.f64.")]
    assert sorted(have) == sorted(want), (sorted(have), sorted(want))
    for k in have:
        f64 = g[t + ("out.f64" if k == "out" else k.replace("grad.", "grad.f64."))]
        f32 = g[t + ("out.f32" if k == "out" else k.replace("grad.", "grad.f32."))]
        gap = float(np.abs(f32.astype(np.float64) - f64).max())
        err = float((have[k] - torch.from_numpy(f64)).abs().max())
        print("case %d %s: err %.3e, golden gap %.3e, ratio %.2f" % (ci, k, err, gap, err / gap))
        assert gap > 0 and err <= 4 * gap, (ci, k, err, gap)
    for k in (k for k in g.files if k.startswith(t + "after.")):      # 'causal': the parameter itself was edited
        assert np.array_equal(m.state_dict()[k[len(t) + 6:]].cpu().numpy(), g[k]), k


def test_two_runs_are_bitwise_equal(amd, golden):
    g = golden("pixelsnail_gated_resblock")
    for ci in (0, 5, 7):
        c, m, ins, gout = _golden_module(amd, g, ci)
        m.train()
        runs = []
        for _ in range(2):
            torch.manual_seed(5)
            runs.append(_run_module(m, ins, gout))
        assert torch.equal(runs[0][0], runs[1][0])
        for k in runs[0][1]:
            assert torch.equal(runs[0][1][k], runs[1][1][k]), (ci, k)


def test_nhwc_path_chains_blocks(amd):
    """Two blocks chained through nhwc() give what they give through the NCHW interface."""
    torch.manual_seed(2)
    a = amd.GatedResBlock(6, 8, 3, conv="causal", dropout=0.0).cuda()
    b = amd.GatedResBlock(6, 4, 1, dropout=0.0).cuda()
    x = torch.randn(2, 6, 5, 4, device="cuda")
    y1 = b(a(x))
    y2 = amd.ops.from_nhwc(b.nhwc(a.nhwc(amd.ops.to_nhwc(x))), 6)
    assert y2.shape == y1.shape and torch.equal(y1, y2)


def test_gated_kernels_do_not_spill():
    """The compiler's resource report of csrc/vq2_gated.hip (written by csrc/build.sh): no spilled register and no scratch
    in any of the elementwise kernels."""
    files = glob.glob(os.path.join(ROOT, "vq-vae-2-pytorch_amd", "csrc", "_obj", "vq2_gated.res"))
    assert files, "csrc/_obj/vq2_gated.res is missing: csrc/build.sh lists vq2_gated and writes the report with the object"
    hot = re.compile(r"elu_fwd_kernel|elu_bwd_kernel|dropout_keep_mask_kernel|glu_res_fwd_kernel|glu_res_bwd_kernel")
    seen, name = 0, None
    for line in open(files[0]):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen += bool(hot.search(name))
            continue
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name and hot.search(name):
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
    assert seen == 8, f"{seen} kernels found in the report, expected 8 (ELU fwd, two backwards, the mask, GLU fwd / bwd x 2)"
