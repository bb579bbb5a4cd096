"""Host side of the evaluation / 8-bit export path, no GPU: grid geometry, the denormalisation constants and the exact
round trip of the arithmetic the byte kernel executes, perplexity, and the C entry points' signatures."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _norms():
    spec = importlib.util.spec_from_file_location("train_stage1_example", os.path.join(ROOT, "examples", "train_stage1.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.NORMS


def reference_bytes(x, mean, std):
    """The reference's way from a normalised float image to the bytes of its PNG, restated with torch on the CPU:
    invTrans (train_vqvae.py:22-25) = Normalize(0, 1 / std) then Normalize(-mean, 1), each `sub_(mean).div_(std)` with
    fp32 tensors made from the Python doubles, then save_image's `mul(255).add_(0.5).clamp_(0, 255).to(uint8)`.
    x: float32 [..., C] (channels last)."""
    c = len(mean)
    std1 = torch.as_tensor([1.0 / s for s in std], dtype=torch.float32)
    mean2 = torch.as_tensor([-m for m in mean], dtype=torch.float32)
    t = x.clone().float()
    t = t.sub_(torch.zeros(c)).div_(std1)
    t = t.sub_(mean2).div_(torch.ones(c))
    return t.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def test_grid_layout_is_make_grid(amd):
    g = amd.grid_layout
    # a single image comes back as it is (make_grid returns before it pads)
    assert g(1, 8, 6, nrow=4, padding=2) == (8, 6, [(0, 0)])
    assert g(1, 8, 6, nrow=1, padding=0) == (8, 6, [(0, 0)])
    # fewer images than nrow: one row of n cells
    assert g(3, 8, 6, nrow=8, padding=2) == (12, 26, [(2, 2), (2, 10), (2, 18)])
    assert g(3, 8, 6, nrow=8, padding=0) == (8, 18, [(0, 0), (0, 6), (0, 12)])
    # n not a multiple of nrow: the last row is short, the canvas is not
    assert g(5, 4, 4, nrow=2, padding=2) == (20, 14, [(2, 2), (2, 8), (8, 2), (8, 8), (14, 2)])
    assert g(5, 4, 4, nrow=2, padding=0) == (12, 8, [(0, 0), (0, 4), (4, 0), (4, 4), (8, 0)])
    # the reference's sample grid: 2 * n images, nrow = n -> inputs over reconstructions
    h, w, o = g(6, 32, 32, nrow=3, padding=2)
    assert (h, w) == (70, 104) and o[0] == (2, 2) and o[3] == (36, 2) and o[5] == (36, 70)
    assert g(9, 8, 8, nrow=4, padding=2)[:2] == (32, 42)
    with pytest.raises(ValueError):
        g(0, 8, 8, 4, 2)


def test_denormalizer_constants_and_round_trip(amd):
    for name, (mean, std) in _norms().items():
        d = amd.ImageDenormalizer(mean, std)
        assert d.inv_s == tuple(float(np.float32(1.0 / s)) for s in std), name
        assert d.m == tuple(float(np.float32(m)) for m in mean), name
        assert d.inv_s == tuple(float(v) for v in torch.as_tensor([1.0 / s for s in std], dtype=torch.float32)), name
        norm = amd.ImageNormalizer(mean, std)
        inv = norm.inverse()
        assert (inv.inv_s, inv.m, inv.layout, inv.channels) == (d.inv_s, d.m, norm.layout, 3)
        table = norm.table                                       # [C,256]: every value a byte can normalise to
        back = reference_bytes(table.t().contiguous(), mean, std)   # [256,C]
        want = torch.arange(256, dtype=torch.uint8)[:, None].expand(256, len(mean))
        assert torch.equal(back, want), f"{name}: {int((back != want).sum())} table values do not return to their byte"
        # the kernel's statement of the same arithmetic: u = x / inv_s + m, every operation in fp32
        inv_s, m = torch.tensor(d.inv_s), torch.tensor(d.m)
        u = table.t() / inv_s + m
        v = (u * 255 + 0.5).clamp(0, 255).to(torch.uint8)
        assert torch.equal(v, want), name
    with pytest.raises(ValueError):
        amd.ImageDenormalizer((0.5,), (0.0,))
    with pytest.raises(ValueError):
        amd.ImageDenormalizer(layout="cwh")
    with pytest.raises(RuntimeError, match="no CPU path"):
        amd.ImageDenormalizer()(torch.zeros(1, 3, 4, 4))


def test_perplexity_from_counts(amd):
    p = amd.perplexity_from_counts
    for k in (1, 7, 512):
        assert abs(p(torch.full((k,), 13, dtype=torch.int64)) - k) < 1e-9 * k
    onehot = torch.zeros(512, dtype=torch.int64)
    onehot[77] = 123456
    assert p(onehot) == 1.0
    rng = np.random.default_rng(5)
    c = rng.integers(0, 1000, size=512)
    c[rng.integers(0, 512, size=200)] = 0
    assert (c == 0).sum() > 100
    q = c[c > 0].astype(np.float64) / c.sum()
    want = float(np.exp(-(q * np.log(q)).sum()))
    assert abs(p(torch.from_numpy(c)) - want) <= 1e-12 * want
    assert abs(p(c.tolist()) - want) <= 1e-12 * want
    assert np.isnan(p(torch.zeros(4, dtype=torch.int64)))


def test_evaluation_entry_points_exist_with_documented_signatures(amd):
    lib = ctypes.CDLL(amd._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "vq2.h")).read()
    P, I32, I64, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    FP = ctypes.POINTER(ctypes.c_float)
    want = {"vq2_nhwc_to_u8": (ctypes.c_int, [P, I32, I32, I32, I32, I32, FP, FP, P, ctypes.c_int, I32, I32, I64, I32, I32, I64, P]),
            "vq2_sse_workspace_bytes": (SZ, [I32, I32, I32, I32]),
            "vq2_sse_per_image": (ctypes.c_int, [P, P, I32, I32, I32, I32, P, P, SZ, P]),
            "vq2_index_hist": (ctypes.c_int, [P, I64, I32, P, P, P]),
            "vq2_eval_accumulate": (ctypes.c_int, [P, I32, I64, P, P, P])}
    for name, (res, args) in want.items():
        assert hasattr(lib, name) and name in amd._lib.EXPORTS, name
        fn = getattr(amd._lib.lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
        decl = hdr[hdr.index(name + "("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert decl.count(",") + 1 == len(args), f"{name}: vq2.h declares {decl.count(',') + 1} arguments"
    L = amd._lib.lib
    # refusals come before any launch (no GPU here): null pointers, bad geometry, too small a canvas or workspace
    assert L.vq2_nhwc_to_u8(None, 4, 1, 3, 8, 8, None, None, None, 0, 8, 8, 24, 1, 0, 0, None) == 1
    assert b"null pointer" in L.vq2_last_error()
    backing = ctypes.create_string_buffer(4096 + 16)
    dummy = ctypes.c_void_p((ctypes.addressof(backing) + 15) & ~15)
    one = (ctypes.c_float * 4)(2.0, 2.0, 2.0, 2.0)
    assert L.vq2_nhwc_to_u8(dummy, 4, 9, 3, 8, 8, one, one, dummy, 0, 31, 42, 126, 4, 2, 0, None) == 1   # needs 32 rows
    assert b"do not fit" in L.vq2_last_error()
    assert L.vq2_nhwc_to_u8(dummy, 4, 9, 3, 8, 8, one, one, dummy, 0, 32, 42, 125, 4, 2, 0, None) == 1   # pitch < 42 * 3
    assert b"pitch" in L.vq2_last_error()
    assert L.vq2_nhwc_to_u8(dummy, 4, 1, 5, 8, 8, one, one, dummy, 0, 8, 8, 40, 1, 0, 0, None) == 1
    assert L.vq2_nhwc_to_u8(dummy, 4, 1, 3, 8, 8, one, one, dummy, 2, 8, 8, 24, 1, 0, 0, None) == 1
    assert L.vq2_sse_workspace_bytes(9, 256, 256, 4) == 9 * 32 * 4       # 65,536 float4s per image: 32 splits of 2,048
    assert L.vq2_sse_workspace_bytes(5, 256, 256, 4) == 5 * 32 * 4       # the splits do not depend on N
    assert L.vq2_sse_workspace_bytes(1, 8, 8, 4) == 4 and L.vq2_sse_workspace_bytes(1, 8, 8, 3) == 0
    assert L.vq2_sse_per_image(dummy, dummy, 2, 8, 8, 4, dummy, dummy, 4, None) == 3    # VQ2_ERR_WORKSPACE
    assert L.vq2_sse_per_image(dummy, dummy, 2, 8, 8, 6, dummy, dummy, 64, None) == 1
    assert L.vq2_index_hist(dummy, 10, 16385, dummy, dummy, None) == 1
    assert L.vq2_index_hist(None, 10, 512, dummy, dummy, None) == 1
    assert L.vq2_eval_accumulate(None, 1, 1, None, None, None) == 1
    assert amd._lib.API_VERSION >= 6


def test_python_surface(amd):
    assert "return_u8" in inspect.signature(amd.Evaluator.update).parameters
    assert list(inspect.signature(amd.Stage1Trainer.evaluate).parameters) == ["self", "batches", "sample"]
    assert list(inspect.signature(amd.ImageDenormalizer.grid).parameters)[:5] == ["self", "batches", "nrow", "padding", "pad_value"]
    assert "return_ids" in inspect.signature(amd.VQVAE.forward_nhwc).parameters
    with pytest.raises(TypeError, match="forward_nhwc"):
        amd.Evaluator(amd.VQVAE_Deep())
