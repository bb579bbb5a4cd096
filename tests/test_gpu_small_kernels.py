"""GPU checks of the HBM-bound helper kernels that every training step runs (csrc/vq2_norm.hip, csrc/vq2_elem.hip, the small
kernels of csrc/vq2_vq.hip, vq2_colsum of csrc/vq2_wgrad.hip), called through the C entry points at the sizes where their
loops, tails, strides and grid caps change behaviour.  Three kinds of assertion:

  exact            torch.equal where the operation has no rounding freedom (copies, masks, one float32 add);
  integer-exact    reductions over small integers (sum of |terms| < 2^24): every summation order is exact, so the result has
                   to equal the float64 one, and a single non-zero element at the far end pins a dropped or doubled element;
  bounded          random inputs: max abs error against float64 <= 4 x the error of the float32 reference of
                   _small_kernel_ref.py (sequential sums) against float64, per output tensor, the ratio printed.

Operands with a pixel stride above C are channel slices of a wider tensor whose other lanes hold 777; outputs must leave
those lanes alone.  Indices handed to vq_bwd are built on the host and lie inside the codebook."""
import ctypes as C
import functools
import zlib

import pytest
import torch

import _small_kernel_ref as R

pytestmark = pytest.mark.gpu

SENT = 777.0
GUARD = 64
VQ2_OK, VQ2_ERR_INVALID = 0, 1
VQ2_RELU_OUT = 2
EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    import vqvae2_amd
    return vqvae2_amd.ops


def P(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * off)


def run(ops, name, *args):
    rc = getattr(ops.lib, name)(*args, ops._stream())
    assert rc == VQ2_OK, (name, rc, ops.lib.vq2_last_error())


def refused(ops, name, *args):
    rc = getattr(ops.lib, name)(*args, ops._stream())
    msg = ops.lib.vq2_last_error()
    assert rc == VQ2_ERR_INVALID and msg, (name, rc, msg)


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(g, shape, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def wide(t, ld, off=0):
    """Host [rows, C] -> device [rows, ld] full of the sentinel with t in lanes off .. off + C."""
    rows, c = t.shape
    buf = torch.full((rows, ld), SENT, dtype=torch.float32, device="cuda")
    buf[:, off:off + c] = t.cuda()
    return buf


def blank(rows, ld):
    return torch.full((rows, ld), SENT, dtype=torch.float32, device="cuda")


def others_untouched(buf, c, off=0):
    keep = torch.ones(buf.shape[1], dtype=torch.bool, device="cuda")
    keep[off:off + c] = False
    return bool((buf[:, keep] == SENT).all())


def flat(n):
    """n floats of sentinel followed by a guard band of sentinel."""
    return torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")


def guard_untouched(buf, n):
    return bool((buf[n:] == SENT).all())


def _bound(name, got, ref64, ref32):
    """err <= 4 x the float32 formula's error (the rule of test_gpu_prior_kernels.py); returns that error (0: the formula is
    exact there and so must the GPU be)."""
    err = float((got.double().cpu() - ref64).abs().max())
    err32 = float((ref32.double() - ref64).abs().max())
    print("%s: err %.3e, fp32 reference %.3e, ratio %.2f" % (name, err, err32, err / err32 if err32 else float("inf") if err else 0.0))
    assert err <= 4 * err32, name
    return err32


def ld_of(c, is_wide):
    return c + 8 if is_wide else c


STRIDES = pytest.mark.parametrize("is_wide", [False, True], ids=["dense", "wide"])
RELU = pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])

# ================================================================================================ AdaIN
HWS = [1, 15, 16, 17, 63, 64, 65, 113, 1031]       # around the 16-pixel step and the 64-pixel four-chain step of column_sum
CS = [4, 60, 64, 68, 132]                           # one partial block, a full one, full + partial, two full + partial
NS = [1, 3]
# every (HW, C) pair, N alternating so that every (HW, N) and (C, N) pair occurs too: pairwise covering, 45 triples
TRIPLES = [(hw, c, NS[(i + j) % 2]) for i, hw in enumerate(HWS) for j, c in enumerate(CS)]
# N * HW * C / 4 = 8192 * 256 + 257 float4 = 17 * 123377: one more than a full sweep of the capped grid of nrm_grid.  The
# second sweep owns float4 2097152 .. 2097408, i.e. pixel 123361 from channel 60 on and every later pixel (blocks 0 and 1).
WRAP_HW, WRAP_C = 123377, 68
assert WRAP_HW * (WRAP_C // 4) == 8192 * 256 + 257


def _tid(t):
    return "hw%d-c%d-n%d" % t


@functools.lru_cache(maxsize=None)
def adain_data(hw, c, n):
    """Host float32 inputs of one AdaIN case with its float32-rounded statistics; shared, never modified."""
    g = gen("adain", hw, c, n)
    x = torch.randn(n, hw, c, generator=g) * 1.5 + 0.5
    h = torch.randn(n, 2 * c, generator=g) * 0.5
    dy = torch.randn(n, hw, c, generator=g)
    mean, rstd = R.instnorm_stats(x.double(), EPS)
    return {"x": x, "h": h, "dy": dy, "mean": mean.float(), "rstd": rstd.float()}


def _stats(ops, x, ld):
    n, hw, c = x.shape
    xb = wide(x.reshape(n * hw, c), ld)
    mean, rstd = flat(n * c), flat(n * c)
    run(ops, "vq2_instnorm_stats", P(xb), ld, n, hw, c, EPS, P(mean), P(rstd))
    torch.cuda.synchronize()
    assert guard_untouched(mean, n * c) and guard_untouched(rstd, n * c)
    return mean[:n * c].view(n, c), rstd[:n * c].view(n, c)


@STRIDES
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("hw", HWS)
def test_instnorm_stats(ops, hw, c, n, is_wide):
    x = torch.randn(n, hw, c, generator=gen("stats", hw, c, n)) * 1.5 + 0.5
    mean, rstd = _stats(ops, x, ld_of(c, is_wide))
    m64, r64 = R.instnorm_stats(x.double(), EPS)
    m32, r32 = R.instnorm_stats(x, EPS)
    e1 = _bound(f"instnorm_stats mean hw{hw} c{c} n{n}", mean, m64, m32)
    e2 = _bound(f"instnorm_stats rstd hw{hw} c{c} n{n}", rstd, r64, r32)
    assert e2 > 0 and (hw == 1 or e1 > 0)
    if hw == 1:
        assert torch.equal(mean.cpu(), x[:, 0])


@STRIDES
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("hw", [1, 16, 64])
def test_instnorm_mean_integer_exact(ops, hw, c, is_wide):
    """HW a power of two: an integer sum times an exact reciprocal."""
    n = 3
    x = ints(gen("stats-int", hw, c), (n, hw, c))
    mean, _ = _stats(ops, x, ld_of(c, is_wide))
    assert torch.equal(mean.double().cpu(), x.double().mean(1))
    probe = torch.zeros(n, hw, c)
    probe[-1, -1, -1] = 8.0                                                      # last pixel of the last image, last channel
    mean, _ = _stats(ops, probe, ld_of(c, is_wide))
    assert torch.equal(mean.double().cpu(), probe.double().mean(1))


def test_instnorm_stats_mean_far_above_the_spread(ops):
    """x = 50 + 0.1 * normal: a one-pass variance (E[x^2] - mean^2) loses the spread here."""
    n, hw, c = 3, 1031, 68
    x = 50.0 + 0.1 * torch.randn(n, hw, c, generator=gen("offset"))
    mean, rstd = _stats(ops, x, c)
    m64, r64 = R.instnorm_stats(x.double(), EPS)
    m32, r32 = R.instnorm_stats(x, EPS)
    assert _bound("instnorm_stats mean offset50", mean, m64, m32) > 0
    assert _bound("instnorm_stats rstd offset50", rstd, r64, r32) > 0


def test_instnorm_stats_single_pixel(ops):
    n, c = 3, 68
    x = torch.randn(n, 1, c, generator=gen("hw1")) * 3.0
    mean, rstd = _stats(ops, x, c + 8)
    assert torch.equal(mean.cpu(), x[:, 0])
    want = torch.full((n, c), 1.0 / EPS ** 0.5, dtype=torch.float64)
    assert _bound("instnorm_stats rstd hw1", rstd, want, R.instnorm_stats(x, EPS)[1]) > 0


def _adain_fwd_gpu(ops, d, ldx, ldy, relu, x=None):
    x = d["x"] if x is None else x
    n, hw, c = x.shape
    xb, yb = wide(x.reshape(n * hw, c), ldx), blank(n * hw, ldy)
    mean, rstd, h = d["mean"].cuda(), d["rstd"].cuda(), d["h"].cuda()
    run(ops, "vq2_adain_fwd", P(xb), ldx, P(mean), P(rstd), P(h), n, hw, c, VQ2_RELU_OUT if relu else 0, P(yb), ldy)
    torch.cuda.synchronize()
    assert others_untouched(yb, c)
    return yb[:, :c].reshape(n, hw, c)


def _check_adain_fwd(ops, name, d, is_wide, relu):
    c = d["x"].shape[2]
    y = _adain_fwd_gpu(ops, d, ld_of(c, is_wide), ld_of(c, is_wide), relu)
    ref = [R.adain_fwd(d["x"].to(t), d["mean"].to(t), d["rstd"].to(t), d["h"].to(t), relu) for t in (torch.float64, torch.float32)]
    return _bound(name, y, *ref)


@RELU
@STRIDES
@pytest.mark.parametrize("triple", TRIPLES, ids=_tid)
def test_adain_fwd(ops, triple, is_wide, relu):
    hw = triple[0]
    e = _check_adain_fwd(ops, "adain_fwd y " + _tid(triple), adain_data(*triple), is_wide, relu)
    assert hw == 1 or e > 0                                                     # one pixel: x == mean, y = beta exactly


def test_adain_fwd_relu_at_zero(ops):
    """x == mean gives (1 + gamma) * (+-0) + beta: beta in {0, -0, tiny, -tiny} walks the mask through both zeros."""
    n, hw, c = 1, 4, 8
    x = torch.full((n, hw, c), 2.5)
    h = torch.zeros(n, 2 * c)
    h[0, :c] = torch.tensor([0.0, -2.0] * 4)                                    # (1 + gamma) = 1, -1: products +0 and -0
    h[0, c:] = torch.tensor([0.0, 0.0, -0.0, -0.0, 1e-30, 1e-30, -1e-30, -1e-30])
    d = {"x": x, "h": h, "mean": torch.full((n, c), 2.5), "rstd": torch.ones(n, c)}
    for relu in (False, True):
        y = _adain_fwd_gpu(ops, d, c, c, relu)
        assert torch.equal(y.cpu(), R.adain_fwd(x, d["mean"], d["rstd"], h, relu))
    assert bool((y >= 0).all()) and int((y > 0).sum()) == 2 * hw


def _adain_bwd_gpu(ops, d, lds, y, dy=None):
    """lds = (lddy, ldy, ldx, lddx); returns dh [N, 2C], dx [N, HW, C]."""
    x = d["x"]
    dy = d["dy"] if dy is None else dy
    n, hw, c = x.shape
    lddy, ldy, ldx, lddx = lds
    dyb, xb, dxb = wide(dy.reshape(n * hw, c), lddy), wide(x.reshape(n * hw, c), ldx), blank(n * hw, lddx)
    yb = None if y is None else wide(y.reshape(n * hw, c), ldy)
    dh = flat(n * 2 * c)
    mean, rstd, h = d["mean"].cuda(), d["rstd"].cuda(), d["h"].cuda()
    run(ops, "vq2_adain_bwd", P(dyb), lddy, P(yb), ldy, P(xb), ldx, P(mean), P(rstd), P(h), n, hw, c, P(dh), P(dxb), lddx)
    torch.cuda.synchronize()
    assert others_untouched(dxb, c) and guard_untouched(dh, n * 2 * c)
    return dh[:n * 2 * c].view(n, 2 * c), dxb[:, :c].reshape(n, hw, c)


def _relu_output(d):
    """The saved output of a forward with ReLU as the backward reads it, with some of its zeros written as -0.0."""
    y = R.adain_fwd(d["x"], d["mean"], d["rstd"], d["h"], True).clone()
    zeros = (y == 0).flatten().nonzero().flatten()
    y.view(-1)[zeros[::2]] = -0.0
    return y


def _check_adain_bwd(ops, name, d, is_wide, relu):
    c = d["x"].shape[2]
    y = _relu_output(d) if relu else None
    dh, dx = _adain_bwd_gpu(ops, d, (ld_of(c, is_wide),) * 4, y)
    ref = [R.adain_bwd(d["dy"].to(t), None if y is None else y.to(t), d["x"].to(t), d["mean"].to(t), d["rstd"].to(t), d["h"].to(t))
           for t in (torch.float64, torch.float32)]
    return (_bound(name + " dh", dh, ref[0][0], ref[1][0]), _bound(name + " dx", dx, ref[0][1], ref[1][1]))


@RELU
@STRIDES
@pytest.mark.parametrize("triple", TRIPLES, ids=_tid)
def test_adain_bwd(ops, triple, is_wide, relu):
    hw = triple[0]
    e = _check_adain_bwd(ops, "adain_bwd " + _tid(triple), adain_data(*triple), is_wide, relu)
    assert hw == 1 or min(e) > 0                                                # one pixel: xhat = 0, dh = (0 | dz), dx = 0


@STRIDES
@pytest.mark.parametrize("triple", TRIPLES, ids=_tid)
def test_adain_bwd_beta_gradient_integer_exact(ops, triple, is_wide):
    d = adain_data(*triple)
    n, hw, c = d["x"].shape
    lds = (ld_of(c, is_wide),) * 4
    dy = ints(gen("beta-int", triple), (n, hw, c))
    dh, _ = _adain_bwd_gpu(ops, d, lds, None, dy)
    assert torch.equal(dh[:, c:].double().cpu(), dy.double().sum(1))
    probe = torch.zeros(n, hw, c)
    probe[-1, -1, -1] = 5.0
    dh, _ = _adain_bwd_gpu(ops, d, lds, None, probe)
    assert torch.equal(dh[:, c:].double().cpu(), probe.double().sum(1))


@functools.lru_cache(maxsize=None)
def _wrap_adain():
    return adain_data(WRAP_HW, WRAP_C, 1)


def test_adain_fwd_grid_wrap(ops):
    assert _check_adain_fwd(ops, "adain_fwd y wrap", _wrap_adain(), False, True) > 0


def test_adain_bwd_grid_wrap(ops):
    assert min(_check_adain_bwd(ops, "adain_bwd wrap", _wrap_adain(), False, True)) > 0


def test_adain_refusals(ops):
    """Bad arguments are refused before any launch: VQ2_ERR_INVALID and a message.  (The buffers are large enough for every
    call below even if it were launched.)"""
    n, hw, c = 2, 5, 8
    big = lambda: torch.zeros(n * hw * (c + 8) + GUARD, device="cuda")
    x, y, dy, dx, mean, rstd, h, dh = (big() for _ in range(8))
    for cc, ld in ((6, 8), (8, 4)):                                             # C % 4 != 0; pixel stride below C
        refused(ops, "vq2_instnorm_stats", P(x), ld, n, hw, cc, EPS, P(mean), P(rstd))
        refused(ops, "vq2_adain_fwd", P(x), ld, P(mean), P(rstd), P(h), n, hw, cc, 0, P(y), 8)
        refused(ops, "vq2_adain_bwd", P(dy), 8, P(y), 8, P(x), ld, P(mean), P(rstd), P(h), n, hw, cc, P(dh), P(dx), 8)
    refused(ops, "vq2_adain_fwd", P(x), c, P(mean), P(rstd), P(h), n, hw, c, 0, P(y), 4)
    refused(ops, "vq2_adain_bwd", P(dy), c, P(y), c, P(x), c, P(mean), P(rstd), P(h), n, hw, c, P(dh), P(dx), 4)
    refused(ops, "vq2_adain_bwd", P(dy), 4, None, c, P(x), c, P(mean), P(rstd), P(h), n, hw, c, P(dh), P(dx), c)
    refused(ops, "vq2_adain_fwd", P(x, 1), c, P(mean), P(rstd), P(h), n, hw, c, 0, P(y), c)             # 4 bytes off
    refused(ops, "vq2_adain_fwd", P(x), c, P(mean), P(rstd), P(h), n, hw, c, 0, P(y, 1), c)
    refused(ops, "vq2_adain_fwd", P(x), c, P(mean, 1), P(rstd), P(h), n, hw, c, 0, P(y), c)
    refused(ops, "vq2_adain_bwd", P(dy, 1), c, P(y), c, P(x), c, P(mean), P(rstd), P(h), n, hw, c, P(dh), P(dx), c)
    refused(ops, "vq2_adain_bwd", P(dy), c, P(y), c, P(x), c, P(mean), P(rstd), P(h), n, hw, c, P(dh), P(dx, 1), c)
    refused(ops, "vq2_adain_bwd", P(dy), c, P(y, 1), c, P(x), c, P(mean), P(rstd), P(h), n, hw, c, P(dh), P(dx), c)
    for flags in (1, 4, VQ2_RELU_OUT | 1):                                      # anything but VQ2_RELU_OUT
        refused(ops, "vq2_adain_fwd", P(x), c, P(mean), P(rstd), P(h), n, hw, c, flags, P(y), c)
    torch.cuda.synchronize()
    assert float(y.abs().sum() + dx.abs().sum() + dh.abs().sum() + mean.abs().sum() + rstd.abs().sum()) == 0


# ================================================================================================ relu_bwd, slice_copy
PIXELS = [1, 255, 257]
SLICE_CS = [4, 12, 132]
# pixels * C / 4 = 4096 * 256 + 257 float4 = 3 * 349611: the second sweep of the capped grid of grid_for owns the last 257
WRAP_PIXELS, WRAP_SLICE_C = 349611, 12
assert WRAP_PIXELS * (WRAP_SLICE_C // 4) == 4096 * 256 + 257


def _masked_y(g, shape):
    y = torch.randn(shape, generator=g)
    y.view(-1)[0::5] = 0.0
    y.view(-1)[1::5] = -0.0
    return y


def _check_relu_bwd(ops, pixels, c, lds):
    g = gen("relu_bwd", pixels, c)
    dy, y = torch.randn(pixels, c, generator=g), _masked_y(g, (pixels, c))
    dyb, yb, gb = wide(dy, lds[0]), wide(y, lds[1]), blank(pixels, lds[2])
    run(ops, "vq2_relu_bwd", P(dyb), lds[0], P(yb), lds[1], P(gb), lds[2], pixels, c)
    torch.cuda.synchronize()
    assert others_untouched(gb, c)
    assert torch.equal(gb[:, :c].cpu(), torch.where(y > 0, dy, torch.zeros_like(dy)))


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("c", SLICE_CS)
@pytest.mark.parametrize("pixels", PIXELS)
def test_relu_bwd(ops, pixels, c, order):
    lds = [c, c + 4, c + 8]
    _check_relu_bwd(ops, pixels, c, lds[order:] + lds[:order])                  # three different strides per call


def test_relu_bwd_grid_wrap(ops):
    _check_relu_bwd(ops, WRAP_PIXELS, WRAP_SLICE_C, (WRAP_SLICE_C, WRAP_SLICE_C + 4, WRAP_SLICE_C))


def _check_slice_copy(ops, pixels, c, lds, ldd, off, accumulate):
    g = gen("slice_copy", pixels, c)
    src, old = torch.randn(pixels, c, generator=g), torch.randn(pixels, c, generator=g)
    sb, db = wide(src, lds), wide(old, ldd, off)
    run(ops, "vq2_slice_copy", P(sb), lds, P(db, off), ldd, pixels, c, int(accumulate))
    torch.cuda.synchronize()
    assert others_untouched(db, c, off)
    assert torch.equal(db[:, off:off + c].cpu(), src + old if accumulate else src)      # one float32 add, or none


@pytest.mark.parametrize("accumulate", [False, True], ids=["copy", "accumulate"])
@pytest.mark.parametrize("c", SLICE_CS)
@pytest.mark.parametrize("pixels", PIXELS)
def test_slice_copy(ops, pixels, c, accumulate):
    _check_slice_copy(ops, pixels, c, c + 4, c + 16, 8, accumulate)             # into channels 8 .. 8 + C of a wider tensor
    _check_slice_copy(ops, pixels, c, c + 8, c, 0, accumulate)


@pytest.mark.parametrize("accumulate", [False, True], ids=["copy", "accumulate"])
def test_slice_copy_grid_wrap(ops, accumulate):
    _check_slice_copy(ops, WRAP_PIXELS, WRAP_SLICE_C, WRAP_SLICE_C, WRAP_SLICE_C + 4, 4, accumulate)


# ================================================================================================ MSE, stage-1 loss
NUMELS = [1, 3, 4, 5, 1023, 1027, 1024 * 256 * 4 + 7]     # the last: 1024 blocks (the cap) of 256 float4 and a tail of 3
DENOMS = pytest.mark.parametrize("padded", [False, True], ids=["denom-numel", "denom-3of4"])


@functools.lru_cache(maxsize=None)
def mse_data(numel, padded):
    """a, b and denom.  padded: every fourth lane is a zero pad lane of both operands and is not counted."""
    g = gen("mse", numel, padded)
    a, b = torch.randn(numel, generator=g), torch.randn(numel, generator=g)
    if padded:
        a[3::4] = 0.0
        b[3::4] = 0.0
    return a, b, numel - numel // 4 if padded else numel


def _mse_gpu(ops, a, b, denom, gscale, with_grad):
    numel = a.numel()
    ws_bytes = ops.lib.vq2_mse_workspace_bytes(numel)
    ws = torch.empty(ws_bytes // 4 + GUARD, device="cuda")
    loss, grad = flat(1), flat(numel) if with_grad else None
    gs = None if gscale is None else torch.tensor([gscale], device="cuda")
    ad, bd = a.cuda(), b.cuda()
    run(ops, "vq2_mse_fwd_bwd", P(ad), P(bd), numel, denom, P(gs), P(loss), P(grad), P(ws), ws_bytes)
    torch.cuda.synchronize()
    assert guard_untouched(loss, 1) and (grad is None or guard_untouched(grad, numel))
    return loss[:1].clone(), None if grad is None else grad[:numel].clone()


@pytest.mark.parametrize("with_grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("gscale", [None, 0.37], ids=["gs-null", "gs-0.37"])
@DENOMS
@pytest.mark.parametrize("numel", NUMELS)
def test_mse_fwd_bwd(ops, numel, padded, gscale, with_grad):
    a, b, denom = mse_data(numel, padded)
    loss, grad = _mse_gpu(ops, a, b, denom, gscale, with_grad)
    gs32 = None if gscale is None else float(torch.tensor(gscale))              # the float32 value on the device
    l64, g64 = R.mse(a.double(), b.double(), denom, gs32)
    l32, g32 = R.mse(a, b, denom, gs32)
    name = f"mse numel{numel} denom{denom} gs{gscale}"
    assert _bound(name + " loss", loss, l64.reshape(1), l32.reshape(1)) > 0
    if with_grad:
        _bound(name + " grad", grad, g64, g32)


@pytest.mark.parametrize("numel", NUMELS)
def test_mse_integer_exact(ops, numel):
    """Differences in [-2, 2] and denom = 1024: loss and gradient have one exact value.  The big case sums 1024 partials in
    mse_final_kernel."""
    g = gen("mse-int", numel)
    a, b = ints(g, (numel,), -1, 1), ints(g, (numel,), -1, 1)
    loss, grad = _mse_gpu(ops, a, b, 1024, None, True)
    d = a.double() - b.double()
    assert float(loss) == float((d * d).sum() / 1024)
    assert torch.equal(grad.double().cpu(), d / 512)
    for at in sorted({numel - 1, numel // 4 * 4, max(numel // 4 * 4 - 1, 0)} & set(range(numel))):
        probe = torch.zeros(numel)
        probe[at] = 3.0                                                          # the last element, the ragged tail, the last float4
        loss, grad = _mse_gpu(ops, probe, torch.zeros(numel), 1024, None, True)
        assert float(loss) == 9.0 / 1024, at
        assert torch.equal(grad.cpu(), probe / 512), at


@DENOMS
@pytest.mark.parametrize("numel", NUMELS)
def test_stage1_loss(ops, numel, padded):
    a, b, denom = mse_data(numel, padded)
    weight, latent = 0.25, torch.tensor([0.8137], device="cuda")
    ws_bytes = ops.lib.vq2_mse_workspace_bytes(numel)
    ws = torch.empty(ws_bytes // 4 + GUARD, device="cuda")
    recon, total, grad = flat(1), flat(1), flat(numel)
    ad, bd = a.cuda(), b.cuda()
    run(ops, "vq2_stage1_loss", P(ad), P(bd), numel, denom, P(latent), weight, P(recon), P(total), P(grad), P(ws), ws_bytes)
    torch.cuda.synchronize()
    assert guard_untouched(recon, 1) and guard_untouched(total, 1) and guard_untouched(grad, numel)
    loss, g = _mse_gpu(ops, a, b, denom, None, True)
    assert torch.equal(recon[:1], loss) and torch.equal(grad[:numel], g)       # bit-identical to mse_fwd_bwd
    rc, lat = recon[:1].cpu(), latent.cpu()
    _bound(f"stage1_loss total numel{numel} denom{denom}", total[:1], R.stage1_total(rc.double(), lat.double(), weight),
           R.stage1_total(rc, lat, weight))
    l64, _ = R.mse(a.double(), b.double(), denom)
    want = l64 + float(torch.tensor(weight)) * lat.double()
    assert _bound(f"stage1_loss total-from-inputs numel{numel} denom{denom}", total[:1], want,
                  R.stage1_total(R.mse(a, b, denom)[0].reshape(1), lat, weight)) > 0


# ================================================================================================ Adam, axpby, scale
FLAT_WRAP = 4096 * 256 + 257                              # one element per thread: the second sweep owns the last 257
HYPERS = [(3e-4, 0.9, 0.999, 1e-8), (1e-2, 0.5, 0.9, 1e-3)]


@functools.lru_cache(maxsize=None)
def adam_data(n):
    g = gen("adam", n)
    p, grad, m = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    v = (torch.randn(n, generator=g) * 0.1) ** 2
    grad[3::5] = 0.0                                                             # gradients of exactly 0 ...
    m[3::10] = 0.0                                                               # ... some on parameters with no history
    v[3::10] = 0.0
    return p, grad, m, v


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("hyper", HYPERS, ids=["lr3e-4", "lr1e-2"])
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("n", [1, 255, 257, FLAT_WRAP])
def test_adam_step(ops, n, step, hyper, grad_scale):
    p, grad, m, v = adam_data(n)
    pd, md, vd = flat(n), flat(n), flat(n)
    pd[:n], md[:n], vd[:n] = p.cuda(), m.cuda(), v.cuda()
    gd = grad.cuda()
    run(ops, "vq2_adam_step", P(pd), P(gd), P(md), P(vd), n, *hyper, step, grad_scale)
    torch.cuda.synchronize()
    assert guard_untouched(pd, n) and guard_untouched(md, n) and guard_untouched(vd, n)
    ref64 = R.adam_step(p.double(), grad.double() * grad_scale, m.double(), v.double(), *hyper, step)
    ref32 = R.adam_step(p, grad * grad_scale, m, v, *hyper, step)
    name = f"adam n{n} step{step} lr{hyper[0]} gs{grad_scale}"
    errs = [_bound(f"{name} {k}", t[:n], r64, r32) for k, t, r64, r32 in zip("pmv", (pd, md, vd), ref64, ref32)]
    assert max(errs) > 0
    still = (v == 0) & (grad == 0)
    assert torch.equal(pd[:n].cpu()[still], p[still])                            # no history, no gradient: p stays, bit for bit
    assert n < 10 or int(still.sum()) > 0


@pytest.mark.parametrize("n", [1, 257, FLAT_WRAP])
def test_axpby(ops, n):
    g = gen("axpby", n)
    a, b, alpha = torch.randn(n, generator=g), torch.randn(n, generator=g), 0.3
    a32 = float(torch.tensor(alpha))
    ref64, ref32 = a.double() + a32 * b.double(), a + alpha * b
    out, ad = flat(n), flat(n)
    ad[:n] = a.cuda()
    a0, bd = a.cuda(), b.cuda()
    run(ops, "vq2_axpby", P(a0), P(bd), alpha, P(out), n)
    run(ops, "vq2_axpby", P(ad), P(bd), alpha, P(ad), n)                        # in place, dst == a
    torch.cuda.synchronize()
    assert guard_untouched(out, n) and guard_untouched(ad, n)
    assert _bound(f"axpby n{n}", out[:n], ref64, ref32) > 0
    assert torch.equal(out, ad)


@pytest.mark.parametrize("n", [1, 257, FLAT_WRAP])
def test_scale(ops, n):
    src = torch.randn(n, generator=gen("scale", n))
    scalar, alpha = torch.tensor([0.37]), 3.0
    ref64 = src.double() * (scalar.double() * alpha)
    ref32 = src * (scalar * alpha)
    out, sd = flat(n), flat(n)
    sd[:n] = src.cuda()
    s0, sc = src.cuda(), scalar.cuda()
    run(ops, "vq2_scale", P(s0), P(sc), alpha, P(out), n)
    run(ops, "vq2_scale", P(sd), P(sc), alpha, P(sd), n)                        # in place
    torch.cuda.synchronize()
    assert guard_untouched(out, n) and guard_untouched(sd, n)
    assert _bound(f"scale n{n}", out[:n], ref64, ref32) > 0
    assert torch.equal(out, sd)


# ================================================================================================ layout conversion
LAYOUT_HW = [(1, 1), (31, 1), (4, 8), (3, 11), (25, 41)]  # HW = 1, 31, 32, 33, 1025 around the 32-pixel tile


def _check_layout(ops, n, c, h, w, ld):
    hw = h * w
    src = torch.randn(n, c, h, w, generator=gen("layout", n, c, h, w))
    nhwc, srcd = flat(n * hw * ld), src.cuda()
    run(ops, "vq2_nchw_to_nhwc", P(srcd), P(nhwc), n, c, h, w, ld)
    torch.cuda.synchronize()
    assert guard_untouched(nhwc, n * hw * ld)
    got = nhwc[:n * hw * ld].view(n, hw, ld).cpu()
    assert torch.equal(got[..., :c], src.reshape(n, c, hw).permute(0, 2, 1))
    assert torch.equal(got[..., c:], torch.zeros(n, hw, ld - c))                # pad lanes C .. ld - 1
    back_src = torch.full((n, hw, ld), SENT)
    back_src[..., :c] = src.reshape(n, c, hw).permute(0, 2, 1)
    nchw, backd = flat(n * c * hw), back_src.cuda()
    run(ops, "vq2_nhwc_to_nchw", P(backd), P(nchw), n, c, h, w, ld)
    torch.cuda.synchronize()
    assert guard_untouched(nchw, n * c * hw)                                     # nothing outside [N, C, H, W]
    assert torch.equal(nchw[:n * c * hw].view(n, c, h, w).cpu(), src)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("extra", [0, 28], ids=["ld-ceil4", "ld-ceil4+28"])
@pytest.mark.parametrize("hw", LAYOUT_HW, ids=lambda p: "hw%d" % (p[0] * p[1]))
@pytest.mark.parametrize("c", [5, 31, 32, 33, 64, 65])
def test_layout_generic(ops, c, hw, extra, n):
    _check_layout(ops, n, c, hw[0], hw[1], (c + 3) // 4 * 4 + extra)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_layout_four_lane_pixels(ops, c, n):
    _check_layout(ops, n, c, 257, 1, 4)


# ================================================================================================ Quantize helpers
K = 37
VQ_DS = [4, 12, 64, 256]
VQ_MS = [1, 127, 129]
WRAP_M, WRAP_D = 349611, 12
assert WRAP_M * (WRAP_D // 4) == 4096 * 256 + 257


def _check_vq_bwd(ops, m, d, is_wide, mode):
    g = gen("vq_bwd", m, d)
    x, g_out, embed_t = torch.randn(m, d, generator=g), torch.randn(m, d, generator=g), torch.randn(K, d, generator=g)
    idx = torch.randint(0, K, (m,), generator=g)                                 # host-built, inside [0, K)
    idx[-1], idx[0] = K - 1, 0
    assert int(idx.min()) >= 0 and int(idx.max()) < K
    g_diff = torch.tensor([0.6]) if mode != "out" else None
    if mode == "diff":
        g_out = None
    ld = ld_of(d, is_wide)
    xb, dxb = wide(x, ld), blank(m, ld)
    gb = None if g_out is None else wide(g_out, ld)
    gd, idxd, ed = None if g_diff is None else g_diff.cuda(), idx.cuda(), embed_t.cuda()
    run(ops, "vq2_vq_bwd", P(gb), ld, P(gd), P(xb), ld, P(idxd), P(ed), m, d, K, P(dxb), ld)
    torch.cuda.synchronize()
    assert others_untouched(dxb, d)
    ref = [R.vq_bwd(None if g_out is None else g_out.to(t), None if g_diff is None else g_diff.to(t)[0], x.to(t), embed_t.to(t)[idx])
           for t in (torch.float64, torch.float32)]
    e = _bound(f"vq_bwd m{m} d{d} {mode}", dxb[:, :d], *ref)
    assert e > 0 or mode == "out"                                                # g_out alone: a copy, exact


@pytest.mark.parametrize("mode", ["out", "diff", "both"])
@STRIDES
@pytest.mark.parametrize("m", VQ_MS)
@pytest.mark.parametrize("d", VQ_DS)
def test_vq_bwd(ops, d, m, is_wide, mode):
    _check_vq_bwd(ops, m, d, is_wide, mode)


def test_vq_bwd_grid_wrap(ops):
    _check_vq_bwd(ops, WRAP_M, WRAP_D, False, "both")


def _check_vq_gather(ops, idx, d, is_wide):
    m = idx.numel()
    embed_t = torch.randn(K, d, generator=gen("vq_gather", d))
    ld = ld_of(d, is_wide)
    out, idxd, ed = blank(m, ld), idx.cuda(), embed_t.cuda()
    run(ops, "vq2_vq_gather", P(idxd), P(ed), m, d, K, P(out), ld)
    torch.cuda.synchronize()
    assert others_untouched(out, d)
    assert torch.equal(out[:, :d].cpu(), embed_t[idx.clamp(0, K - 1)])


@STRIDES
@pytest.mark.parametrize("m", VQ_MS)
@pytest.mark.parametrize("d", VQ_DS)
def test_vq_gather(ops, d, m, is_wide):
    idx = torch.randint(0, K, (m,), generator=gen("gather-idx", m, d))
    if m > 1:
        idx[0], idx[-1], idx[m // 2] = -3, K + 5, K - 1                          # clamped to rows 0 and K - 1
    _check_vq_gather(ops, idx, d, is_wide)


@STRIDES
def test_vq_gather_clamps(ops, is_wide):
    _check_vq_gather(ops, torch.tensor([-3, K + 5, 0, K - 1, -2 ** 40, 2 ** 40, K, -1]), 12, is_wide)


def test_vq_gather_grid_wrap(ops):
    idx = torch.randint(0, K, (WRAP_M,), generator=gen("gather-wrap"))
    idx[-1] = K + 5
    _check_vq_gather(ops, idx, WRAP_D, False)


def _vq_loss_gpu(ops, part, m, d):
    diff, partd = flat(1), part.cuda()
    run(ops, "vq2_vq_loss", P(partd), m, d, P(diff))
    torch.cuda.synchronize()
    assert guard_untouched(diff, 1)
    return diff[:1].cpu()


@pytest.mark.parametrize("nparts", [1, 255, 256, 257, 1000])
def test_vq_loss(ops, nparts):
    """Hand-made partials, one per 128 rows.  Integers: the sum is exact and the one division rounds once, so the result is
    the float64 quotient rounded to float32.  Random: the bounded rule."""
    m, d = 128 * nparts - 5, 12
    g = gen("vq_loss", nparts)
    part = ints(g, (nparts,), 0, 8)
    assert float(_vq_loss_gpu(ops, part, m, d)) == float((part.double().sum() / (m * d)).float())
    probe = torch.zeros(nparts)
    probe[-1] = 5.0
    assert float(_vq_loss_gpu(ops, probe, m, d)) == float(torch.tensor(5.0 / (m * d), dtype=torch.float64).float())
    part = torch.rand(nparts, generator=g) * 100.0
    e = _bound(f"vq_loss nparts{nparts}", _vq_loss_gpu(ops, part, m, d), R.vq_loss(part.double(), m, d).reshape(1),
               R.vq_loss(part, m, d).reshape(1))
    assert e > 0


# ================================================================================================ vq2_colsum
COLSUM_CS = [4, 12, 256, 1000, 1024, 1028, 4096]          # C/4 divides 256; does not; 250; the cbase loop without and with a rest
COLSUM_ROWS = [1, 255, 256, 257, 2049, 4097, 512 * 256 + 3]   # 1, 1, 1, 2, 9, 17 and 511 partial blocks
COLSUM_CASES = [(c, rows) for c in COLSUM_CS for rows in COLSUM_ROWS if rows < 512 * 256 or c <= 12]


def _colsum_gpu(ops, xb, rows, c, ld):
    ws_bytes = ops.lib.vq2_colsum_workspace_bytes(rows, c)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws, out = flat(ws_bytes // 4), flat(c)
    run(ops, "vq2_colsum", P(xb), rows, c, ld, P(out), P(ws), ws_bytes)
    torch.cuda.synchronize()
    assert guard_untouched(ws, ws_bytes // 4) and guard_untouched(out, c)
    return out[:c].clone()


@pytest.mark.parametrize("extra", [0, 4], ids=["ld-c", "ld-c+4"])
@pytest.mark.parametrize("c,rows", COLSUM_CASES)
def test_colsum(ops, c, rows, extra):
    ld = c + extra
    x = torch.randn(rows, c, generator=gen("colsum", c, rows))
    xb = wide(x, ld)
    out = _colsum_gpu(ops, xb, rows, c, ld)
    assert _bound(f"colsum c{c} rows{rows}", out, R.colsum(x.double()), R.colsum(x)) > 0 or rows == 1
    assert torch.equal(out, _colsum_gpu(ops, xb, rows, c, ld))                  # fixed order: bit for bit
    xi = (x * 3).round().clamp(-8, 8)                                            # integers: 8 * rows < 2^24
    xb[:, :c] = xi.cuda()
    assert torch.equal(_colsum_gpu(ops, xb, rows, c, ld).double().cpu(), xi.double().sum(0))
    xb[:, :c] = 0
    xb[-1, c - 1] = 7.0                                                          # last row, last channel
    want = torch.zeros(c, dtype=torch.float64)
    want[-1] = 7.0
    assert torch.equal(_colsum_gpu(ops, xb, rows, c, ld).double().cpu(), want)


def test_colsum_refusals(ops):
    rows, c = 257, 12
    x, out = torch.zeros(rows * 4104, device="cuda"), torch.zeros(4104, device="cuda")
    ws_bytes = ops.lib.vq2_colsum_workspace_bytes(rows, c)
    big = max(ws_bytes, ops.lib.vq2_colsum_workspace_bytes(rows, 4100))
    ws = torch.zeros(big // 4 + GUARD, device="cuda")
    refused(ops, "vq2_colsum", P(x), rows, c, c, P(out), P(ws), ws_bytes - 1)   # one byte short
    refused(ops, "vq2_colsum", P(x), rows, 4100, 4100, P(out), P(ws), big)      # C above 4096
    refused(ops, "vq2_colsum", P(x), rows, c, c - 4, P(out), P(ws), ws_bytes)
    refused(ops, "vq2_colsum", P(x, 1), rows, c, c, P(out), P(ws), ws_bytes)
    run(ops, "vq2_colsum", P(x), rows, c, c, P(out), P(ws), ws_bytes)           # the exact size is accepted
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0
