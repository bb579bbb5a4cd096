"""CPU checks of the sampling path: the row-incremental evaluation (tests/_sample_ref.py: per-conv row histories, key / value
histories, the row-0 input stage) gives the logits of the full model on the goldens, the draw rule behaves at its ends, and
the library declares the new entry points."""
import ctypes

import numpy as np
import pytest
import torch

import _pixelsnail_model_ref as M
import _sample_ref as S


@pytest.fixture(scope="module")
def g():
    return M.load()


@pytest.mark.parametrize("ci", [0, 1, 2, 4])
def test_row_stepping_reproduces_the_model_in_float64(g, ci):
    c = M.cases(g)[ci]
    t = f"c{ci}."
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in M.state_dict(g, ci).items()}
    codes = torch.from_numpy(g[t + "in.input"])
    cond = torch.from_numpy(g[t + "in.condition"]) if t + "in.condition" in g.files else None
    with torch.no_grad():
        want = M.pixelsnail(codes, {k: v.clone() for k, v in sd.items()}, c["n_class"], c["attention"], cond)
    have = S.logits_given(codes, sd, c["n_class"], c["attention"], cond)
    assert have.shape == want.shape
    err = (have - want).abs().amax(dim=(0, 1, 3))           # per row: row 0 has its own input-stage rule
    assert float(err.max()) <= 1e-12, err
    golden = g[t + "logits.f64"]
    assert np.abs(have.numpy() - golden).max() <= 1e-12 * max(1.0, np.abs(golden).max())


def test_draw_rule():
    p = np.array([0.0, 0.25, 0.0, 0.5, 0.25, 0.0])
    assert S.draw(p, 0.0) == 1                               # the first class with non-zero probability
    assert S.draw(p, np.nextafter(1.0, 0.0)) == 4            # the last one
    assert S.draw(p, 0.25) == 3                              # cumsum > u is strict
    us = np.linspace(0.0, 1.0, 1001, endpoint=False)
    cs = [S.draw(p, u) for u in us]
    assert cs == sorted(cs) and set(cs) == {1, 3, 4}         # monotone in u, zero-probability classes never drawn
    rng = np.random.default_rng(3)
    q = rng.random(37)
    q /= q.sum()
    cdf = np.cumsum(q)
    for u in rng.random(200):
        c = S.draw(q, u)
        assert (cdf[c - 1] if c else 0.0) <= u < cdf[c] or c == len(q) - 1
    assert S.draw(np.array([0.5, 0.25]), 0.9) == 1           # rounding leaves none: the last class


def test_library_declares_the_sampling_entry_points():
    import vqvae2_amd as amd
    L = amd._lib
    P, I32, I64, F, U64, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64, ctypes.c_size_t
    GP, AP = ctypes.POINTER(L.ConvDesc), ctypes.POINTER(L.AttnDesc)
    want = {
        "vq2_conv_fwd_row_workspace_bytes": (SZ, [GP, ctypes.c_int]),
        "vq2_conv_fwd_row": (ctypes.c_int, [GP, I32, I64, I64, ctypes.c_int, P, P, P, P, I32, P, P, SZ, P]),
        "vq2_causal_attn_fwd_rows": (ctypes.c_int, [AP, I32, I32, I32, I64, I64, P, P, P, P, P]),
        "vq2_sample_categorical": (ctypes.c_int, [P, I64, I32, I32, F, U64, U64, P, I64, P]),
        "vq2_sample_uniforms": (ctypes.c_int, [P, I32, U64, U64, P]),
    }
    for name, (res, args) in want.items():
        assert name in L.EXPORTS, name
        fn = getattr(L.lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert L.API_VERSION >= 13
    for name in ("PriorSampler", "sample_model", "load_model"):
        assert hasattr(amd, name)
    # argument checks that reach no kernel
    d = L.ConvDesc()
    d.N, d.H, d.W, d.Ci, d.Co, d.KH, d.KW, d.pad_top, d.pad_left, d.ldx, d.ldy = 1, 4, 4, 4, 4, 3, 3, 1, 1, 4, 4
    d.stride, d.same_size = 1, 1
    one = ctypes.c_void_p(16)
    assert L.lib.vq2_conv_fwd_row(ctypes.byref(d), 0, 16, 64, 0, one, one, None, None, 0, one, one, 1 << 20, None) == 1   # pad_top != KH - 1
    assert b"pad_top" in L.lib.vq2_last_error()
    assert L.lib.vq2_sample_categorical(one, 8, 1, 8, 0.0, 1, 0, one, 1, None) == 1
    assert L.lib.vq2_sample_categorical(one, 16385, 1, 16385, 1.0, 1, 0, one, 1, None) == 1
    d.pad_top = 2
    assert L.lib.vq2_conv_fwd_row_workspace_bytes(ctypes.byref(d), 0) == 9 * 4 * 4 * 4      # one slab per tap of [N * W, Co]
    assert L.lib.vq2_conv_fwd_row_workspace_bytes(ctypes.byref(d), 8) == 7 * 4 * 4 * 4      # the two 'causal' taps skipped
