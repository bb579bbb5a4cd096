"""GPU: the two dead-code restart entry points against tests/_code_restart_ref.py -- the draw and the gathered rows bit
for bit (one rank and two), the update's dead set, restarted codes and counters exactly, the codebook against the float64
statement, the prepared form against vq2_vq_prepare, and threshold = 0 against the plain update bit for bit."""
import functools

import numpy as np
import pytest
import torch

import _code_restart_ref as R

pytestmark = pytest.mark.gpu

# (D, K, M): K % 4 != 0 with the smallest D | M < K | the ragged width and the padded statistics buffer | both limits
SHAPES = [(4, 5, 37), (64, 512, 300), (48, 510, 1000), (256, 16384, 2048)]
IDS = ["D%d-K%d-M%d" % s for s in SHAPES]
SEED, STEP, SLOT = 0x1234567887654321, (3 << 32) + 11, 1       # 64-bit seed and step: both words reach the counter
DECAY, EPS, THRESHOLD = 0.99, 1e-5, 1.0
# tests/test_gpu_quantize_shapes.py::test_fixture_case compares the updated codebook with the oracle's at these
EMBED_RTOL, EMBED_ATOL = 1e-4, 1e-5


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def padded_rows(x, pad=4):
    """x [M, D] as a device tensor [M, 1, 1, D] whose rows are D + pad floats apart, the pad filled with NaN."""
    m, d = x.shape
    full = np.full((m, d + pad), np.nan, dtype=np.float32)
    full[:, :d] = x
    t = gpu(full)
    return t, t[:, :d]


def gather(amd, xfull, m, d, k, rank, world, want_picks=True):
    """vq2_vq_restart_candidates through the C ABI on rows of stride xfull.shape[1]."""
    lib, p = amd._lib.lib, amd.ops._p
    cand = torch.full((k, d), 7.0, device=dev())            # every element must be overwritten
    picks = torch.full((k,), -1, device=dev(), dtype=torch.int64) if want_picks else None
    amd._lib.check(lib.vq2_vq_restart_candidates(p(xfull), xfull.shape[1], m, d, k, SEED, STEP, SLOT, rank, world, p(cand),
                                                 p(picks), amd.ops._stream()), "vq_restart_candidates")
    torch.cuda.synchronize()
    return cand.cpu().numpy(), None if picks is None else picks.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(d, k, m):
    """Inputs and reference of one shape, computed once: 2M rows of x (no -0.0), the draws, and a codebook state in which
    about half the codes end below the threshold, none within 1e-3 relative of it."""
    g = np.random.default_rng(1000 * d + k)
    x2 = g.standard_normal((2 * m, d)).astype(np.float32)
    assert not np.signbit(x2[x2 == 0]).any()
    c = {"x2": x2, "picks1": R.picks(SEED, STEP, SLOT, k, m), "picks2": R.picks(SEED, STEP, SLOT, k, 2 * m)}
    target = g.random(k) < 0.5                                # codes meant to die
    if k >= 2:
        target[0], target[1] = True, False
    cs0 = np.where(target, g.uniform(0.0, 0.8, k), g.uniform(1.5, 4.0, k)).astype(np.float32)
    counts = np.where(target, g.integers(0, 3, k), g.integers(0, 40, k)).astype(np.float32)
    embed = g.standard_normal((d, k)).astype(np.float32)
    ea = (embed * np.maximum(cs0, 0.05)[None, :]).astype(np.float32)
    sums_t = (g.standard_normal((k, d)) * counts[:, None]).astype(np.float32)
    cand = R.candidates(x2[:m], c["picks1"])
    c.update(embed=embed, cs0=cs0, ea=ea, counts=counts, sums_t=sums_t, cand=cand, target=target)
    ref = R.ema_update_restart(embed, cs0, ea, counts, sums_t, cand, DECAY, EPS, THRESHOLD)
    new_cs = R.fma32(np.float32(1.0 - DECAY), counts, cs0 * np.float32(DECAY))
    # the test's own inputs keep the fp32 decision away from the threshold, so it cannot differ from the reference's
    assert (np.abs(new_cs - THRESHOLD) > 1e-3 * THRESHOLD).all()
    assert np.array_equal(ref["dead"], target) and 0 < target.sum() < k
    c["ref"] = ref
    return c


def run_update(amd, c, d, k, threshold, prepare=True, cand=None, counter0=(0, 0)):
    ops = amd.ops
    embed, cs, ea = gpu(c["embed"]), gpu(c["cs0"]), gpu(c["ea"])
    stats = ops.vq_stats_alloc(k, d, dev())
    counts, sums_t = ops.vq_stats_views(stats, k, d)
    counts.copy_(gpu(c["counts"]))
    sums_t.copy_(gpu(c["sums_t"]).reshape(-1))
    counter = torch.tensor(counter0, device=dev(), dtype=torch.int64)
    prep = (torch.full((k, d), 3.0, device=dev()), torch.full((k,), 3.0, device=dev())) if prepare else None
    candt = gpu(c["cand"] if cand is None else cand).reshape(-1)
    ops.vq_ema_update_restart(embed, cs, ea, stats, candt, DECAY, EPS, threshold, counter, prep)
    torch.cuda.synchronize()
    out = {"embed": embed, "cluster_size": cs, "embed_avg": ea, "counter": counter.cpu().tolist()}
    if prepare:
        out["embedT"], out["enorm"] = prep
    return out


def run_plain(amd, c, d, k, prepare):
    ops = amd.ops
    embed, cs, ea = gpu(c["embed"]), gpu(c["cs0"]), gpu(c["ea"])
    stats = ops.vq_stats_alloc(k, d, dev())
    counts, sums_t = ops.vq_stats_views(stats, k, d)
    counts.copy_(gpu(c["counts"]))
    sums_t.copy_(gpu(c["sums_t"]).reshape(-1))
    prep = (torch.empty((k, d), device=dev()), torch.empty((k,), device=dev())) if prepare else None
    ops.vq_ema_update(embed, cs, ea, stats, DECAY, EPS, prep)
    torch.cuda.synchronize()
    out = {"embed": embed, "cluster_size": cs, "embed_avg": ea}
    if prepare:
        out["embedT"], out["enorm"] = prep
    return out


def same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------- candidates
@pytest.mark.parametrize("d,k,m", SHAPES, ids=IDS)
def test_candidates_one_rank(amd, d, k, m):
    c = case(d, k, m)
    xfull, _ = padded_rows(c["x2"][:m])
    cand, picks = gather(amd, xfull, m, d, k, 0, 1)
    assert np.array_equal(picks, c["picks1"])
    assert same_bits(cand, c["x2"][:m][c["picks1"]])         # (a NaN from the pad would show here)
    again, _ = gather(amd, xfull, m, d, k, 0, 1, want_picks=False)      # picks = NULL; the same bits a second time
    assert same_bits(again, cand)


@pytest.mark.parametrize("d,k,m", SHAPES, ids=IDS)
def test_candidates_two_ranks_sum_to_the_gather_from_all_rows(amd, d, k, m):
    c = case(d, k, m)
    pk = c["picks2"]
    xfull, _ = padded_rows(c["x2"])
    whole, picks = gather(amd, xfull, 2 * m, d, k, 0, 1)
    assert np.array_equal(picks, pk) and same_bits(whole, c["x2"][pk])
    a, pa = gather(amd, xfull[:m], m, d, k, 0, 2)
    b, pb = gather(amd, xfull[m:], m, d, k, 1, 2)
    assert np.array_equal(pa, pk) and np.array_equal(pb, pk)
    own_a = pk // m == 0
    if k >= 64:
        assert own_a.any() and (~own_a).any()
    # a data row in exactly one of the two calls, zeros in the other
    assert same_bits(a[own_a], whole[own_a]) and not a[~own_a].any()
    assert same_bits(b[~own_a], whole[~own_a]) and not b[own_a].any()
    assert same_bits(a + b, whole)


# ----------------------------------------------------------------------------- update
@pytest.mark.parametrize("d,k,m", SHAPES, ids=IDS)
def test_update_restarts_exactly_the_dead_codes(amd, d, k, m):
    c = case(d, k, m)
    ref, dead = c["ref"], c["ref"]["dead"]
    out = run_update(amd, c, d, k, THRESHOLD, counter0=(123, 1000))
    cs, ea, embed = (out[n].cpu().numpy() for n in ("cluster_size", "embed_avg", "embed"))
    assert np.array_equal(cs == np.float32(THRESHOLD), dead)                 # the dead set
    n_dead = int(dead.sum())
    assert out["counter"] == [n_dead, 1000 + n_dead]
    assert same_bits(cs[dead], ref["cluster_size"][dead]) and same_bits(ea[:, dead], ref["embed_avg"][:, dead])
    np.testing.assert_allclose(cs[~dead], ref["cluster_size"][~dead], rtol=1e-6, atol=0)
    np.testing.assert_allclose(ea[:, ~dead], ref["embed_avg"][:, ~dead], rtol=1e-5, atol=1e-6)
    err = np.abs(embed - ref["embed64"])
    print("embed vs float64: max abs err %.3e, max rel err %.3e" % (err.max(), (err / (np.abs(ref["embed64"]) + 1e-30)).max()))
    np.testing.assert_allclose(embed, ref["embed64"], rtol=EMBED_RTOL, atol=EMBED_ATOL)
    embed_t, enorm = amd.ops.vq_prepare(out["embed"])
    torch.cuda.synchronize()
    assert same_bits(out["embedT"], embed_t) and same_bits(out["enorm"], enorm)
    # without embedT / enorm: the same codebook
    bare = run_update(amd, c, d, k, THRESHOLD, prepare=False)
    assert bare["counter"] == [n_dead, n_dead]
    for n in ("embed", "cluster_size", "embed_avg"):
        assert same_bits(bare[n], out[n]), n


@pytest.mark.parametrize("d,k,m", SHAPES, ids=IDS)
def test_threshold_zero_is_the_plain_update_bit_for_bit(amd, d, k, m):
    c = case(d, k, m)
    out, plain = run_update(amd, c, d, k, 0.0, counter0=(9, 40)), run_plain(amd, c, d, k, True)
    assert out["counter"] == [0, 40]
    for n in ("embed", "cluster_size", "embed_avg", "embedT", "enorm"):
        assert same_bits(out[n], plain[n]), n
    out, plain = run_update(amd, c, d, k, 0.0, prepare=False), run_plain(amd, c, d, k, False)
    for n in ("embed", "cluster_size", "embed_avg"):
        assert same_bits(out[n], plain[n]), n


@pytest.mark.parametrize("d,k,m", SHAPES, ids=IDS)
def test_non_finite_candidate_row_is_not_restarted(amd, d, k, m):
    c = case(d, k, m)
    dead = c["ref"]["dead"]
    victim = int(np.flatnonzero(dead)[-1])
    cand = c["cand"].copy()
    cand[victim, d - 1] = np.inf
    ref = R.ema_update_restart(c["embed"], c["cs0"], c["ea"], c["counts"], c["sums_t"], cand, DECAY, EPS, THRESHOLD)
    assert not ref["dead"][victim] and ref["dead"].sum() == dead.sum() - 1
    out, plain = run_update(amd, c, d, k, THRESHOLD, cand=cand), run_plain(amd, c, d, k, True)
    n_dead = int(dead.sum()) - 1
    assert out["counter"] == [n_dead, n_dead]
    cs, ea = out["cluster_size"].cpu().numpy(), out["embed_avg"].cpu().numpy()
    assert np.array_equal(cs == np.float32(THRESHOLD), ref["dead"])
    assert cs[victim] == plain["cluster_size"].cpu().numpy()[victim]         # the plain EMA path
    assert same_bits(ea[:, victim], plain["embed_avg"].cpu().numpy()[:, victim])
    assert np.isfinite(out["embed"].cpu().numpy()).all()
