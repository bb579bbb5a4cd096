"""CPU checks of pixel stepping: the column-incremental evaluation (tests/_sample_pixel_ref.py: column buffers, conv
histories that start as NaN, single-query attention) gives the logits of the full model on the goldens, the library and
the package declare the new entry point and keyword, and the sampler's recorder keeps its replay contract (a program's
moving arguments, the views the two step geometries give of a history row)."""
import ctypes

import numpy as np
import pytest
import torch

import _pixelsnail_model_ref as M
import _sample_pixel_ref as P


@pytest.fixture(scope="module")
def g():
    return M.load()


@pytest.mark.parametrize("ci", [0, 1, 2, 4])
def test_pixel_stepping_reproduces_the_model_in_float64(g, ci):
    c = M.cases(g)[ci]
    t = f"c{ci}."
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in M.state_dict(g, ci).items()}
    codes = torch.from_numpy(g[t + "in.input"])
    cond = torch.from_numpy(g[t + "in.condition"]) if t + "in.condition" in g.files else None
    with torch.no_grad():
        want = M.pixelsnail(codes, {k: v.clone() for k, v in sd.items()}, c["n_class"], c["attention"], cond)
    have = P.logits_given(codes, sd, c["n_class"], c["attention"], cond)
    assert have.shape == want.shape
    assert bool(torch.isfinite(have).all())                 # no step read a history cell nobody had written
    err = (have - want).abs()
    print("case %d: max err %.3e, row 0 %.3e, column 0 %.3e" % (ci, float(err.max()), float(err[:, :, 0].max()),
                                                                float(err[:, :, :, 0].max())))
    assert float(err.max()) <= 1e-12, err.amax(dim=(0, 1))
    golden = g[t + "logits.f64"]
    assert np.abs(have.numpy() - golden).max() <= 1e-12 * max(1.0, np.abs(golden).max())


def test_library_declares_the_column_conv():
    import vqvae2_amd as amd
    L = amd._lib
    P_, I32, I64, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    GP = ctypes.POINTER(L.ConvDesc)
    want = {
        "vq2_conv_fwd_col_workspace_bytes": (SZ, [GP, ctypes.c_int]),
        "vq2_conv_fwd_col": (ctypes.c_int, [GP, I32, I32, I64, I64, ctypes.c_int, P_, P_, P_, P_, I32, P_, P_, SZ, P_]),
    }
    for name, (res, args) in want.items():
        assert name in L.EXPORTS, name
        fn = getattr(L.lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert L.API_VERSION >= 20
    # argument checks that reach no kernel
    d = L.ConvDesc()
    d.N, d.H, d.W, d.Ci, d.Co, d.KH, d.KW, d.pad_top, d.pad_left, d.ldx, d.ldy = 1, 4, 4, 4, 4, 3, 3, 2, 1, 4, 4
    d.stride, d.same_size = 1, 1
    backing = ctypes.create_string_buffer(4096 + 16)         # a real, 16-byte aligned host allocation behind every pointer
    one = ctypes.c_void_p((ctypes.addressof(backing) + 15) & ~15)
    call =lambda row, col, nbytes: L.lib.vq2_conv_fwd_col(ctypes.byref(d), row, col, 16, 64, 8, one, one, None, None, 0, one, one,
                                                           nbytes, None)
    need = L.lib.vq2_conv_fwd_col_workspace_bytes(ctypes.byref(d), 8)
    assert need >= 1 * 4 * 4 and need % 16 == 0
    assert call(0, 4, need) == 1 and b"col" in L.lib.vq2_last_error()
    assert call(0, -1, need) == 1
    assert call(4, 0, need) == 1 and b"row" in L.lib.vq2_last_error()
    assert call(0, 0, need - 1) == 1 and b"workspace" in L.lib.vq2_last_error()
    d.pad_top = 1
    assert call(0, 0, need) == 1 and b"pad_top" in L.lib.vq2_last_error()


def test_program_replay_contract():
    """_Program.run(j): the moving arguments are taken at column j, a call without one gets the objects it was recorded with."""
    from vqvae2_amd import sample as S
    got = {"still": [], "moving": []}

    def still(*args):
        got["still"].append(args)
        return 0

    def moving(*args):
        got["moving"].append(args)
        return 0

    prog = S._Program()
    fixed = (ctypes.c_void_p(64), 7, None)
    prog.add("still", still, *fixed)
    prog.add("moving", moving, 3, S._Moving(1000, 24), S._Moving(5, 1, pointer=False), None)
    assert [len(call) for call in prog.calls] == [4, 4]                   # one shape of entry
    assert [(call[2], len(call[3])) for call in prog.calls] == [("still", 0), ("moving", 2)]
    prog.run()
    prog.run(0)
    prog.run(3)
    assert len(got["still"]) == 3
    for args in got["still"]:
        assert len(args) == 3 and all(a is f for a, f in zip(args, fixed))
    seen = []
    for three, p, n, none in got["moving"]:
        assert three == 3 and none is None and type(p) is ctypes.c_void_p and type(n) is int
        seen.append((p.value, n))
    assert seen == [(1000, 5), (1000, 5), (1072, 8)]
    failing = S._Program()
    failing.add("elu_fwd", lambda *args: 1, 0)
    with pytest.raises(RuntimeError, match="elu_fwd"):
        failing.run()


def test_step_geometries_view_a_history_row():
    from vqvae2_amd import sample as S
    row = torch.zeros(2, 5, 8)                                            # [B, W, C]
    v = S._ColumnStep(2, 5).row(row)
    assert isinstance(v, S._View) and v.t is row and (v.c, v.ld, v.step) == (8, 40, 8)
    p = v.ptr()
    assert isinstance(p, S._Moving) and p.pointer
    for j in (0, 4):
        at = p.at(j)
        assert type(at) is ctypes.c_void_p and at.value == row.data_ptr() + 32 * j
    assert v.ptr(3).at(4).value == row.data_ptr() + 4 * 3 + 32 * 4
    v = S._RowStep(2, 5).row(row)
    assert isinstance(v, S._View) and v.t is row and (v.c, v.ld, v.step) == (8, 8, 0)
    p = v.ptr()
    assert type(p) is ctypes.c_void_p and p.value == row.data_ptr()
    assert v.ptr(3).value == row.data_ptr() + 12
    assert (S._ColumnStep(2, 5).pixels, S._RowStep(2, 5).pixels) == (2, 10)


def test_stepping_keyword():
    import inspect
    import vqvae2_amd as amd
    m = amd.PixelSNAIL([4, 4], 6, 8, 3, 1, 1, 8, attention=False)
    with pytest.raises(ValueError, match="stepping"):
        amd.PriorSampler(m, stepping="diagonal")
    with pytest.raises(ValueError, match="stepping"):
        amd.sample_model(m, "cpu", 1, [4, 4], 1.0, stepping="diagonal")
    assert inspect.signature(amd.PriorSampler).parameters["stepping"].default == "row"
    assert inspect.signature(amd.sample_model).parameters["stepping"].default == "row"
