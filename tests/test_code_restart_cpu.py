"""Dead-code restart without a GPU: the reference draw and rule (tests/_code_restart_ref.py) checked against their own
statement, the two entry points' bindings and every argument they refuse before a launch, and the host surface (trainer
methods, pinned constructor lists, the example's options)."""
import ctypes
import glob
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

import _code_restart_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VQ2_ERR_INVALID = 1


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


# ----------------------------------------------------------------------------- the reference draw
def test_philox_known_answer():
    """Random123's known-answer vectors are for 10 rounds; seven rounds of the same round function are pinned here by
    running ten with this file's loop and comparing with the published 10-round answer for the all-zero input."""
    c, k = [0, 0, 0, 0], [0, 0]
    for _ in range(10):
        p0, p1 = R.PHILOX_M0 * c[0], R.PHILOX_M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & R.M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & R.M32]
        k = [(k[0] + R.PHILOX_W0) & R.M32, (k[1] + R.PHILOX_W1) & R.M32]
    assert c == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # ... and the seven-round function is that loop stopped early
    c, k = [1, 2, 3, 4], [5, 6]
    for _ in range(7):
        p0, p1 = R.PHILOX_M0 * c[0], R.PHILOX_M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & R.M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & R.M32]
        k = [(k[0] + R.PHILOX_W0) & R.M32, (k[1] + R.PHILOX_W1) & R.M32]
    assert list(R.philox4x32_7((1, 2, 3, 4), (5, 6))) == c


def test_draw_is_in_range_and_a_pure_function():
    for m_total in (1, 37, 300, 1 << 20, (1 << 32) - 1):
        pk = R.picks(7, 3, 1, 257, m_total)
        assert pk.min() >= 0 and pk.max() < m_total
        assert np.array_equal(pk, R.picks(7, 3, 1, 257, m_total))
    assert [R.draw(7, 3, 1, k, 1000) for k in range(257)] == list(R.picks(7, 3, 1, 257, 1000))
    # the step is 64 bits wide: its high word is part of the counter
    assert not np.array_equal(R.picks(7, 3, 1, 64, 1 << 20), R.picks(7, 3 + (1 << 32), 1, 64, 1 << 20))
    assert not np.array_equal(R.picks(7, 3, 1, 64, 1 << 20), R.picks(7 + (1 << 32), 3, 1, 64, 1 << 20))


def test_steps_slots_and_seeds_give_different_picks():
    base = R.picks(11, 0, 0, 512, 32768)
    for other in (R.picks(11, 1, 0, 512, 32768), R.picks(11, 0, 1, 512, 32768), R.picks(12, 0, 0, 512, 32768)):
        assert (base != other).mean() > 0.9


def test_draw_is_uniform_chi_square():
    """65,536 draws into 64 bins (M_total = 64): expected 1024 per bin, 63 degrees of freedom; the 99.9 % point of chi^2_63
    is 103.44.  The seed is fixed, so the statistic is one number."""
    pk = R.picks(20240607, 5, 0, 65536, 64)
    hist = np.bincount(pk, minlength=64).astype(np.float64)
    chi2 = float(((hist - 1024.0) ** 2 / 1024.0).sum())
    print("chi-square over 64 bins:", chi2)
    assert chi2 < 103.44


# ----------------------------------------------------------------------------- the reference rule
def _state(d, k, m, seed):
    g = np.random.default_rng(seed)
    embed = g.standard_normal((d, k)).astype(np.float32)
    cs = g.uniform(0.0, 4.0, k).astype(np.float32)
    ea = (embed * cs[None, :]).astype(np.float32)
    counts = np.floor(g.uniform(0.0, 3.0, k)).astype(np.float32)
    sums_t = (g.standard_normal((k, d)) * counts[:, None]).astype(np.float32)
    x = g.standard_normal((m, d)).astype(np.float32)
    return embed, cs, ea, counts, sums_t, x


def test_threshold_zero_is_the_plain_update():
    embed, cs, ea, counts, sums_t, x = _state(8, 37, 50, 1)
    cand = R.candidates(x, R.picks(3, 0, 0, 37, 50))
    got = R.ema_update_restart(embed, cs, ea, counts, sums_t, cand, 0.99, 1e-5, 0.0)
    want = R.plain_ema_update(embed, cs, ea, counts, sums_t, 0.99, 1e-5)
    assert not got["dead"].any()
    for key in ("embed", "cluster_size", "embed_avg"):
        assert got[key].tobytes() == want[key].tobytes(), key


def test_dead_code_lands_on_its_candidate():
    d, k, thr, eps = 8, 37, 1.0, 1e-5
    embed, cs, ea, counts, sums_t, x = _state(d, k, 50, 2)
    cand = R.candidates(x, R.picks(3, 0, 0, k, 50))
    got = R.ema_update_restart(embed, cs, ea, counts, sums_t, cand, 0.99, eps, thr)
    dead = got["dead"]
    assert 0 < dead.sum() < k
    assert (got["cluster_size"][dead] == np.float32(thr)).all()
    assert got["embed_avg"][:, dead].tobytes() == (np.float32(thr) * cand[dead]).T.astype(np.float32).tobytes()
    n = float(got["cluster_size"].astype(np.float64).sum())
    want = cand[dead].T.astype(np.float64) * (n + k * eps) / n * thr / (thr + eps)
    rel = np.abs(got["embed"][:, dead] - want) / np.abs(want)
    assert rel.max() < 2.0 ** -20, rel.max()
    # live codes: exactly the plain update's embed_avg
    plain = R.plain_ema_update(embed, cs, ea, counts, sums_t, 0.99, eps)
    assert got["embed_avg"][:, ~dead].tobytes() == plain["embed_avg"][:, ~dead].tobytes()


def test_non_finite_candidate_restarts_nothing():
    d, k = 8, 37
    embed, cs, ea, counts, sums_t, x = _state(d, k, 50, 3)
    cs[:] = 0.5
    counts[:] = 0.0                                      # every code is below the threshold
    cand = R.candidates(x, R.picks(3, 0, 0, k, 50))
    cand[5, 3] = np.nan
    cand[9, 0] = np.inf
    got = R.ema_update_restart(embed, cs, ea, counts, sums_t, cand, 0.99, 1e-5, 1.0)
    assert not got["dead"][5] and not got["dead"][9] and got["dead"].sum() == k - 2
    plain = R.plain_ema_update(embed, cs, ea, counts, sums_t, 0.99, 1e-5)
    for j in (5, 9):
        assert got["cluster_size"][j] == plain["cluster_size"][j]
        assert got["embed_avg"][:, j].tobytes() == plain["embed_avg"][:, j].tobytes()
    cand[:] = np.nan                                     # a batch of NaNs: the whole update is the plain one
    got = R.ema_update_restart(embed, cs, ea, counts, sums_t, cand, 0.99, 1e-5, 1.0)
    assert not got["dead"].any() and got["embed_avg"].tobytes() == plain["embed_avg"].tobytes()


def test_two_rank_candidates_sum_to_the_one_rank_gather():
    _, _, _, _, _, x = _state(8, 64, 100, 4)
    pk = R.picks(9, 2, 1, 64, 100)
    whole = R.candidates(x, pk)
    a, b = R.candidates(x[:50], pk, 0, 2), R.candidates(x[50:], pk, 1, 2)
    assert (a + b).tobytes() == whole.tobytes()
    assert ((pk // 50 == 0) | (np.abs(a).sum(1) == 0)).all() and ((pk // 50 == 1) | (np.abs(b).sum(1) == 0)).all()


# ----------------------------------------------------------------------------- the library
CAND_ARGS = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
             ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
             ctypes.c_void_p]
UPDATE_ARGS = [ctypes.c_void_p] * 6 + [ctypes.c_int32] * 2 + [ctypes.c_double] * 3 + [ctypes.c_void_p] * 5


def test_entry_points_are_bound_with_the_documented_lists(amd):
    lib = amd._lib.lib
    assert amd._lib.API_VERSION >= 19 and lib.vq2_version() == amd._lib.API_VERSION
    for name, args in (("vq2_vq_restart_candidates", CAND_ARGS), ("vq2_vq_ema_update_restart", UPDATE_ARGS)):
        assert name in amd._lib.EXPORTS
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is ctypes.c_int, name
    hdr = open(os.path.join(ROOT, "include", "vq2.h")).read()
    decl = re.search(r"int vq2_vq_restart_candidates\((.*?)\);", hdr, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl).split(",")]
    assert names == ["x", "ldx", "M", "D", "K", "seed", "step", "slot", "rank", "world", "cand", "picks", "stream"]
    decl = re.search(r"int vq2_vq_ema_update_restart\((.*?)\);", hdr, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names == ["embed", "cluster_size", "embed_avg", "counts", "sumsT", "cand", "D", "K", "decay", "eps", "threshold",
                     "scratch", "embedT", "enorm", "counter", "stream"]
    assert callable(amd.vq_restart_candidates) and callable(amd.vq_ema_update_restart)


@pytest.fixture(scope="module")
def host_ptr():
    """A real, 16-byte aligned host allocation: a regression of a refusal cannot hand a kernel an address nobody owns."""
    backing = ctypes.create_string_buffer(4096 + 16)
    yield ctypes.c_void_p((ctypes.addressof(backing) + 15) & ~15)
    del backing


def _refused(lib, name, args):
    rc = getattr(lib, name)(*args)
    msg = lib.vq2_last_error()
    assert rc == VQ2_ERR_INVALID and msg, (name, rc, msg)
    return msg


def test_candidates_refuse_bad_arguments_before_any_launch(amd, host_ptr):
    """No device exists here: a call that reached a launch would fail differently (and not with VQ2_ERR_INVALID)."""
    lib, ok = amd._lib.lib, host_ptr
    good = dict(x=ok, ldx=64, M=300, D=64, K=512, seed=1, step=0, slot=0, rank=0, world=1, cand=ok, picks=None)

    def call(**kw):
        a = dict(good, **kw)
        return _refused(lib, "vq2_vq_restart_candidates", [a[k] for k in good] + [None])

    for k in ("x", "cand"):
        assert b"null" in call(**{k: None})
    for world in (0, -1):
        assert b"world" in call(world=world)
    for rank, world in ((-1, 1), (1, 1), (2, 2), (5, 4)):
        assert b"rank" in call(rank=rank, world=world)
    assert b"2^32" in call(M=1 << 32)
    assert b"2^32" in call(M=1 << 31, world=2, rank=1)
    assert b"2^32" in call(M=(1 << 32) // 3 + 1, world=3)
    assert b"2^32" in call(M=0)
    for d in (0, 2, 6, 260, -4):
        assert b"D %" in call(D=d, ldx=512)
    for k in (0, -1, 16385):
        assert b"K" in call(K=k)
    assert b"stride" in call(ldx=60) and b"stride" in call(ldx=66)
    assert b"aligned" in call(x=ctypes.c_void_p(ok.value + 4)) and b"aligned" in call(cand=ctypes.c_void_p(ok.value + 8))


def test_update_refuses_bad_arguments_before_any_launch(amd, host_ptr):
    lib, ok = amd._lib.lib, host_ptr
    order = ("embed", "cluster_size", "embed_avg", "counts", "sumsT", "cand", "D", "K", "decay", "eps", "threshold", "scratch",
             "embedT", "enorm", "counter")
    good = dict({k: ok for k in order}, D=64, K=512, decay=0.99, eps=1e-5, threshold=1.0)

    def call(**kw):
        a = dict(good, **kw)
        return _refused(lib, "vq2_vq_ema_update_restart", [a[k] for k in order] + [None])

    for k in ("embed", "cluster_size", "embed_avg", "counts", "sumsT", "cand", "scratch", "counter"):
        assert b"null" in call(**{k: None}), k
    assert b"together" in call(embedT=None) and b"together" in call(enorm=None)
    for thr in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf"), 1e39):
        assert b"threshold" in call(threshold=thr), thr
    for d in (0, 2, 6, 260, -4):
        assert b"D %" in call(D=d)
    for k in (0, -1, 16385):
        assert b"K" in call(K=k)


def test_new_kernels_use_no_scratch():
    """The compiler's resource report written by csrc/build.sh: the three restart kernels spill nothing."""
    files = glob.glob(os.path.join(ROOT, "vq-vae-2-pytorch_amd", "csrc", "_obj", "vq2_vq.res"))
    if not files:
        pytest.skip("no resource report: run __graft_entry__.build() first")
    new = re.compile(r"vq_restart_candidates_kernel|vq_ema_counts_restart_kernel|vq_ema_embed_kernelILb[01]ELb1E")
    seen, name = set(), None
    for line in open(files[0]):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1) if new.search(m.group(1)) else None
            if name:
                seen.add(name)
            continue
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
    assert len(seen) == 4, seen


# ----------------------------------------------------------------------------- host surface
def test_trainer_and_quantize_surface(amd):
    t = amd.Stage1Trainer
    assert list(inspect.signature(t.set_code_restart).parameters) == ["self", "threshold", "start", "seed"]
    p = inspect.signature(t.set_code_restart).parameters
    assert (p["threshold"].default, p["start"].default, p["seed"].default) == (1.0, 0, 0)
    assert callable(t.restarted_codes)
    # the pinned constructor lists (tests/test_optim_extras_cpu.py) are what they were
    params = list(inspect.signature(t.__init__).parameters)
    assert params[:8] == ["self", "model", "lr", "sched", "n_iter", "betas", "eps", "normalizer"]
    assert params[-2:] == ["clip_grad_norm", "ema_decay"] and len(params) == 10
    assert list(inspect.signature(amd.Quantize.__init__).parameters) == ["self", "dim", "n_embed", "decay", "eps"]
    q = amd.Quantize(8, 16)
    assert list(inspect.signature(q.enable_code_restart).parameters) == ["threshold", "start", "seed", "slot"]
    before = list(q.state_dict())
    q.enable_code_restart(0.5, start=3, seed=9, slot=1)
    assert q._restart == {"threshold": 0.5, "start": 3, "seed": 9, "slot": 1} and q.restart_step == 0
    q.restart_step = 17
    assert q.restart_step == 17
    assert list(q.state_dict()) == before == ["embed", "cluster_size", "embed_avg"]
    amd.Quantize(8, 16).load_state_dict(q.state_dict(), strict=True)        # both ways: nothing was registered
    q.load_state_dict(amd.Quantize(8, 16).state_dict(), strict=True)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            q.enable_code_restart(bad)
    q.disable_code_restart()
    assert q._restart is None


def test_example_parser_takes_the_two_options_and_defaults_to_off():
    spec = importlib.util.spec_from_file_location("train_stage1_example", os.path.join(ROOT, "examples", "train_stage1.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    d = ex.parse_args(["--size", "64"])
    assert d.code_restart is None and d.code_restart_start == 0
    a = ex.parse_args(["--code_restart", "1.0", "--code_restart_start", "500"])
    assert a.code_restart == 1.0 and a.code_restart_start == 500
    assert ex.restarted_text(None) == "" and ex.restarted_text([3, 40]) == "; restarted codes: 3/40"
