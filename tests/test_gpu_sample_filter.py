"""GPU checks of vq2_sample_filtered through the C ABI, against tests/_sample_filter_ref.py in float64: the filters off
(the codes of vq2_sample_categorical), top-k (exact), top-p (between the reference counts at top_p -/+ delta), the draw
(float64 CDF interval over the kept set), the log-probability, and the refusals.

Rows are padded and the pad lanes hold NaN.  Temperatures of the truncation tests are powers of two: l / T is then exact, and
the reference forms the very float32 z of the kernel.  Every shape's logits are built once and shared."""
import functools
import math

import numpy as np
import pytest
import torch

import _sample_filter_ref as F

pytestmark = pytest.mark.gpu

# n_class <= 512 stays in registers, longer rows go through LDS; M = 9 leaves the last workgroup ragged, and 16,384
# classes are the largest chunk (256 per lane, one wave per workgroup)
SHAPES = [(5, 300), (6, 300), (512, 300), (1000, 300), (16384, 9), (6, 9)]
SEED, POSITION = 0x1234567890ABCDEF, (1 << 33) + 5
TIE_ROWS, INF_ROW, WORKED_ROW, DOMINANT_ROW = (1, 2, 3), 4, 5, 7


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


@functools.lru_cache(maxsize=None)
def _case(n_class, m):
    """(padded float32 logits on the host with NaN pad lanes, the same on the device)."""
    ld = (n_class + 3) // 4 * 4 + 4
    gen = torch.Generator().manual_seed(n_class * 1000 + m)
    logits = torch.full((m, ld), float("nan"))
    body = torch.randn(m, n_class, generator=gen) * 3
    for r in TIE_ROWS:
        body[r] = torch.round(body[r])                      # integers: duplicates at the k-th value for most k
    body[INF_ROW, ::3] = -math.inf                          # legal, mass 0
    body[INF_ROW, 1] = 0.5
    body[WORKED_ROW] = -torch.arange(n_class, dtype=torch.float64).mul(math.log(2.0)).float()    # masses 1/2, 1/4, ...
    body[DOMINANT_ROW, 3] += 50.0
    logits[:, :n_class] = body
    return logits, logits.cuda()


def _z64(logits, n_class, temperature):
    return logits[:, :n_class].double().numpy() / temperature


def _filtered(amd, dev, n_class, temperature, top_k, top_p, seed=SEED, position=POSITION):
    m = dev.shape[0]
    out = torch.full((m,), -1, device="cuda", dtype=torch.int64)
    logp = torch.full((m,), float("nan"), device="cuda")
    kept = torch.full((m,), -1, device="cuda", dtype=torch.int32)
    p = amd.ops._p
    amd._lib.check(amd._lib.lib.vq2_sample_filtered(p(dev), dev.shape[1], m, n_class, temperature, top_k, top_p, seed, position,
                                                    p(out), 1, p(logp), p(kept), amd.ops._stream()), "sample_filtered")
    return out.cpu().numpy(), logp.cpu().double().numpy(), kept.cpu().numpy().astype(np.int64)


def _uniforms(amd, m, seed=SEED, position=POSITION):
    u = torch.empty(m, device="cuda")
    amd._lib.check(amd._lib.lib.vq2_sample_uniforms(amd.ops._p(u), m, seed, position, amd.ops._stream()), "uniforms")
    return u.cpu().double().numpy()


def _top_ks(n_class):
    return sorted({min(max(k, 1), n_class) for k in (1, 2, 63, 64, 65, n_class - 1, n_class)})


def _mask_of_count(z, count):
    """The `count` largest values of every row as a mask; a threshold set has exactly `count` members."""
    zs = -np.sort(-z, axis=1)
    mask = z >= zs[np.arange(len(z)), count - 1][:, None]
    assert np.array_equal(mask.sum(1), count), "the kept set is not closed over ties"
    return mask


# ----------------------------------------------------------------------------- 1. filters off
@pytest.mark.parametrize("n_class,m", SHAPES)
def test_filters_off_gives_the_codes_of_the_plain_draw(amd, n_class, m):
    _, dev = _case(n_class, m)
    for temperature in (0.5, 0.7, 1.0):
        plain = torch.full((m,), -1, device="cuda", dtype=torch.int64)
        amd._lib.check(amd._lib.lib.vq2_sample_categorical(amd.ops._p(dev), dev.shape[1], m, n_class, temperature, SEED, POSITION,
                                                           amd.ops._p(plain), 1, amd.ops._stream()), "draw")
        codes, _, kept = _filtered(amd, dev, n_class, temperature, 0, 1.0)
        assert np.array_equal(codes, plain.cpu().numpy()), temperature
        assert np.all(kept == n_class)
        codes, _, kept = _filtered(amd, dev, n_class, temperature, n_class, 1.0)        # top_k == n_class keeps every class too
        assert np.array_equal(codes, plain.cpu().numpy()) and np.all(kept == n_class)


# ----------------------------------------------------------------------------- 2. top-k
@pytest.mark.parametrize("n_class,m", SHAPES)
def test_top_k_is_exact(amd, n_class, m):
    logits, dev = _case(n_class, m)
    tied = 0
    for temperature in (0.5, 1.0, 2.0):
        z = _z64(logits, n_class, temperature)
        assert np.array_equal(z, z.astype(np.float32))                                  # l / T is exact: the kernel's z
        for k in _top_ks(n_class):
            codes, _, kept = _filtered(amd, dev, n_class, temperature, k, 1.0)
            want = F.kept_counts(z, k)
            for r in (0,) + TIE_ROWS + (INF_ROW,):                                      # the batched count against the row form
                mask = F.kept_mask(z[r], k)
                assert want[r] == mask.sum()
                assert mask[codes[r]]
            assert np.array_equal(kept, want), (temperature, k, np.nonzero(kept != want)[0][:5])
            assert np.all(_mask_of_count(z, want)[np.arange(m), codes]), (temperature, k)
            tied += int((want[list(TIE_ROWS)] > k).sum())
    assert tied > 0 or n_class <= 6                                                     # ties at the k-th value did occur


# ----------------------------------------------------------------------------- 3. top-p
@pytest.mark.parametrize("n_class,m", SHAPES)
def test_top_p_lies_between_the_reference_counts(amd, n_class, m):
    logits, dev = _case(n_class, m)
    delta = 4 * n_class * 2.0 ** -24
    for temperature in (0.5, 1.0):
        z = _z64(logits, n_class, temperature)
        for k in (0, min(64, n_class - 1)):
            size = F.kept_counts(z, k)
            for p in (0.05, 0.5, 0.9, 0.999, 1.0):
                _, _, kept = _filtered(amd, dev, n_class, temperature, k, p)
                lo = F.kept_counts(z, k, p - delta)
                hi = F.kept_counts(z, k, p + delta) if p + delta <= 1 else size
                bad = np.nonzero((kept < lo) | (kept > hi))[0]
                assert bad.size == 0, (temperature, k, p, bad[:5], kept[bad[:5]], lo[bad[:5]], hi[bad[:5]])
                _mask_of_count(z, kept)                                                 # tie-closed
    # the worked row (masses 1/2, 1/4, ... at temperature 1): where the float64 margin to every cut exceeds delta the count
    # is exact
    z = _z64(logits, n_class, 1.0)[WORKED_ROW:WORKED_ROW + 1]
    frac = np.cumsum(np.exp(z[0])) / np.exp(z[0]).sum()                                 # mass of the first q classes
    for p, obvious in ((0.7, 2), (0.5, 1), (0.76, 3)):
        margin = np.abs(frac - p).min()                                                 # on the reference alone
        # 0.7 and 0.76 lie well inside their intervals at every n; 0.5 is the first mass itself up to the total's 2^-n, so
        # it has a margin at the small shapes only and is held to the count interval above at the others
        assert margin > delta or (p == 0.5 and n_class > 12)
        want = int(F.kept_counts(z, 0, p)[0])
        assert want == F.kept_count(z[0], 0, p)
        if n_class >= 8:                                                                # the total 1 - 2^-n is close enough to 1
            assert want == obvious
        _, _, kept = _filtered(amd, dev, n_class, 1.0, 0, p)
        if margin > delta:
            assert kept[WORKED_ROW] == want, (p, kept[WORKED_ROW], want)
        else:
            assert F.kept_counts(z, 0, p - delta)[0] <= kept[WORKED_ROW] <= F.kept_counts(z, 0, p + delta)[0]


# ----------------------------------------------------------------------------- 4. the draw, 5. its log-probability
SETTINGS = [(0, 1.0), (8, 1.0), (0, 0.9), (64, 0.5), (1, 1.0)]


@pytest.mark.parametrize("n_class,m", SHAPES)
def test_draw_lies_in_the_float64_cdf_interval_of_the_kept_set(amd, n_class, m):
    logits, dev = _case(n_class, m)
    u = _uniforms(amd, m)
    tol = n_class * 2.0 ** -23
    rows = np.arange(m)
    for temperature in (0.5, 1.0):
        z = _z64(logits, n_class, temperature)
        for k, p in SETTINGS:
            k = min(k, n_class)
            codes, logp, kept = _filtered(amd, dev, n_class, temperature, k, p)
            mask = _mask_of_count(z, kept)
            assert np.all(mask[rows, codes])
            e = np.where(mask, np.exp(z - z.max(1, keepdims=True)), 0.0)
            cdf = np.cumsum(e / e.sum(1, keepdims=True), 1)
            lo = np.where(codes > 0, cdf[rows, np.maximum(codes - 1, 0)], 0.0)
            hi = cdf[rows, codes]
            bad = np.nonzero((lo - tol > u) | (u > hi + tol))[0]
            assert bad.size == 0, (temperature, k, p, bad[:5], codes[bad[:5]], u[bad[:5]], lo[bad[:5]], hi[bad[:5]])
            again = _filtered(amd, dev, n_class, temperature, k, p)                     # same (seed, position): same bits
            assert np.array_equal(codes, again[0]) and np.array_equal(logp, again[1]) and np.array_equal(kept, again[2])
            if k == 1:
                assert np.array_equal(codes, z.argmax(1)) or np.all(kept[codes != z.argmax(1)] > 1)
    other = _filtered(amd, dev, n_class, 1.0, 0, 1.0, position=POSITION + 1)[0]
    assert n_class <= 6 or not np.array_equal(other, _filtered(amd, dev, n_class, 1.0, 0, 1.0)[0])


@pytest.mark.parametrize("n_class,m", SHAPES)
def test_logp_against_float64_over_the_same_set(amd, n_class, m):
    logits, dev = _case(n_class, m)
    rows = np.arange(m)
    worst = 0.0
    for temperature in (0.5, 1.0):
        z = _z64(logits, n_class, temperature)
        for k, p in SETTINGS:
            codes, logp, kept = _filtered(amd, dev, n_class, temperature, min(k, n_class), p)
            mask = _mask_of_count(z, kept)
            rel = z - z.max(1, keepdims=True)
            want = rel[rows, codes] - np.log(np.where(mask, np.exp(rel), 0.0).sum(1))
            bound = (n_class + 8) * 2.0 ** -23 + 2.0 ** -22 * np.abs(rel[rows, codes])
            ratio = np.abs(logp - want) / bound
            worst = max(worst, float(ratio.max()))
            print("n_class %d T %.1f top_k %d top_p %.3f: max |logp - float64| / bound = %.3f" % (n_class, temperature, k, p, ratio.max()))
            assert np.all(np.isfinite(logp)) and np.all(logp <= 0)
            assert ratio.max() <= 1, (temperature, k, p, float(ratio.max()))
            if k == 1:
                assert np.all(logp[kept == 1] == 0)                                     # one class: probability 1
    print("n_class %d: worst ratio %.3f" % (n_class, worst))


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_output_untouched(amd):
    n_class, m = 6, 9
    _, dev = _case(n_class, m)
    out = torch.full((m,), -7, device="cuda", dtype=torch.int64)
    p = amd.ops._p
    for top_k, top_p in ((-1, 1.0), (n_class + 1, 1.0), (0, 0.0), (0, -0.1), (0, 1.5), (0, float("nan"))):
        rc = amd._lib.lib.vq2_sample_filtered(p(dev), dev.shape[1], m, n_class, 1.0, top_k, top_p, SEED, POSITION, p(out), 1, None, None,
                                              amd.ops._stream())
        assert rc != 0, (top_k, top_p)
    torch.cuda.synchronize()
    assert torch.all(out == -7)
    # null logp / kept are legal
    rc = amd._lib.lib.vq2_sample_filtered(p(dev), dev.shape[1], m, n_class, 1.0, 2, 0.9, SEED, POSITION, p(out), 1, None, None,
                                          amd.ops._stream())
    assert rc == 0 and int(out.min()) >= 0 and int(out.max()) < n_class
