"""Host side of the 8-bit input path (no GPU): the normalisation table against the reference loader's transform
restated with plain torch, the CenterCrop origin, argument errors of ImageNormalizer / HostBatchPrefetcher /
Stage1Trainer.step, and the refusals of vq2_u8_to_nhwc4 that come before any launch."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))                               # extract_code.py:52
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))               # train_vqvae.py:154


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def reference_transform(img_u8_chw, mean, std):
    """ToTensor + Normalize as torchvision executes them on a uint8 [C,H,W] image (torchvision is not importable here):
    `img.to(torch.float32).div(255)`, then `tensor.sub_(mean[:, None, None]).div_(std[:, None, None])` with mean / std as
    float32 tensors."""
    x = img_u8_chw.to(dtype=torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32)
    s = torch.as_tensor(std, dtype=torch.float32)
    return x.sub_(m[:, None, None]).div_(s[:, None, None])


@pytest.mark.parametrize("stats", [HALF, IMAGENET], ids=["half", "imagenet"])
def test_table_equals_the_reference_transform_bit_for_bit(amd, stats):
    mean, std = stats
    ramp = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16).repeat(3, 1, 1)      # every byte value, every channel
    want = reference_transform(ramp, mean, std).reshape(3, 256)
    norm = amd.ImageNormalizer(mean, std)
    assert norm.table.dtype == torch.float32 and tuple(norm.table.shape) == (3, 256) and norm.table.is_contiguous()
    assert torch.equal(norm.table, want)
    assert norm.table.view(torch.int32).equal(want.view(torch.int32))                   # (-0.0 / NaN would hide in ==)
    assert norm.channels == 3 and norm.layout == "hwc" and norm.crop is None


def test_default_statistics_and_channel_counts(amd):
    assert torch.equal(amd.ImageNormalizer().table, amd.ImageNormalizer(*HALF).table)
    one = amd.ImageNormalizer((0.25,), (2.0,), layout="chw")
    assert tuple(one.table.shape) == (1, 256) and one.channels == 1
    assert float(one.table[0, 255]) == (1.0 - 0.25) / 2.0 and float(one.table[0, 0]) == -0.125
    assert tuple(amd.ImageNormalizer((0,) * 4, (1,) * 4).table.shape) == (4, 256)


def test_crop_origin_is_torchvisions(amd):
    """CenterCrop: crop_top = int(round((image_height - crop_height) / 2.0)); Python's round sends halves to the even
    neighbour, so odd differences alternate between rounding down and up."""
    origin = amd.ImageNormalizer.crop_origin
    assert origin(256, 256) == 0
    assert origin(300, 256) == 22          # even difference
    assert origin(257, 256) == 0           # 0.5 -> 0
    assert origin(259, 256) == 2           # 1.5 -> 2
    assert origin(261, 256) == 2           # 2.5 -> 2
    assert origin(68, 33) == 18            # 17.5 -> 18 (tests/test_host_cpu.py's resize_crop_box case)
    norm = amd.ImageNormalizer(crop=(33, 64))
    assert norm.box(68, 64) == (18, 0, 33, 64)
    assert norm.box(36, 71) == (2, 4, 33, 64)          # 1.5 -> 2, 3.5 -> 4
    assert amd.ImageNormalizer().box(5, 7) == (0, 0, 5, 7)
    assert norm.out_shape(torch.zeros((2, 68, 70, 3), dtype=torch.uint8)) == (2, 3, 33, 64)
    chw = amd.ImageNormalizer(layout="chw", crop=(8, 8))
    assert chw.out_shape(torch.zeros((2, 3, 11, 12), dtype=torch.uint8)) == (2, 3, 8, 8)


def test_constructor_and_call_errors(amd):
    with pytest.raises(ValueError, match="layout"):
        amd.ImageNormalizer(layout="nhwc")
    with pytest.raises(ValueError):
        amd.ImageNormalizer((0.5, 0.5), (0.5, 0.5, 0.5))
    with pytest.raises(ValueError):
        amd.ImageNormalizer((0.5,) * 5, (0.5,) * 5)
    with pytest.raises(ValueError):
        amd.ImageNormalizer(std=(0.5, 0.0, 0.5))
    with pytest.raises(ValueError):
        amd.ImageNormalizer(crop=(0, 4))
    with pytest.raises(ValueError, match="larger"):
        amd.ImageNormalizer(crop=(65, 64)).box(64, 64)
    norm = amd.ImageNormalizer()
    with pytest.raises(RuntimeError, match="no CPU path"):          # a CPU tensor: no fallback
        norm(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="uint8"):                # a float tensor to the 8-bit call
        norm(torch.zeros((1, 8, 8, 3)))
    with pytest.raises(RuntimeError):
        norm.nchw(torch.zeros((1, 8, 8, 3)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        amd.ops.u8_to_nhwc4(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), norm.table, "hwc")
    with pytest.raises(RuntimeError, match="GPU"):
        amd.HostBatchPrefetcher([], "cpu")
    with pytest.raises(ValueError):
        amd.HostBatchPrefetcher([], "cuda:0", depth=0)


def test_trainer_step_refuses_uint8_without_a_normalizer(amd):
    import inspect
    assert "normalizer" in inspect.signature(amd.Stage1Trainer.__init__).parameters
    import types
    fake = types.SimpleNamespace(model=None, normalizer=None)
    with pytest.raises(TypeError, match="normalizer"):
        amd.Stage1Trainer.step(fake, torch.zeros((1, 8, 8, 3), dtype=torch.uint8))


def test_entry_point_is_declared_exported_and_bound(amd):
    hdr = open(os.path.join(ROOT, "include", "vq2.h")).read()
    assert re.search(r"\bint\s+vq2_u8_to_nhwc4\s*\(", hdr)
    assert re.search(r"#define\s+VQ2_U8_HWC\s+0\b", hdr) and re.search(r"#define\s+VQ2_U8_CHW\s+1\b", hdr)
    assert "train_vqvae.py:149-155" in hdr and "extract_code.py:47-53" in hdr
    assert "vq2_u8_to_nhwc4" in amd._lib.EXPORTS
    assert hasattr(ctypes.CDLL(amd._lib.LIB_PATH), "vq2_u8_to_nhwc4")
    assert amd._lib.API_VERSION >= 5
    assert amd.ops.U8_LAYOUTS == {"hwc": 0, "chw": 1}


def test_bad_arguments_are_refused_before_any_launch(amd):
    lib = amd._lib.lib
    # non-null, 16-byte aligned host memory stands in for the device pointers: a regression of a refusal must not hand a
    # kernel an address nobody owns (tests/test_host_cpu.py does the same)
    backing = ctypes.create_string_buffer(4096 + 16)
    dummy = ctypes.c_void_p((ctypes.addressof(backing) + 15) & ~15)

    def call(src=dummy, layout=0, n=1, c=3, hs=8, ws=8, y0=0, x0=0, h=8, w=8, lut=dummy, dst=dummy):
        rc = lib.vq2_u8_to_nhwc4(src, layout, n, c, hs, ws, y0, x0, h, w, lut, dst, None)
        return rc, lib.vq2_last_error().decode()

    for kw in (dict(src=None), dict(lut=None), dict(dst=None)):
        rc, msg = call(**kw)
        assert rc == 1 and "u8" in msg and "null" in msg, (kw, rc, msg)
    for kw in (dict(c=5), dict(c=0), dict(layout=2), dict(n=0), dict(h=0),
               dict(y0=1), dict(x0=1), dict(y0=-1, h=4), dict(x0=-2, w=4), dict(h=9), dict(w=9), dict(hs=4), dict(y0=5, h=4),
               dict(dst=ctypes.c_void_p(dummy.value + 4))):
        rc, msg = call(**kw)
        assert rc == 1 and "u8" in msg, (kw, rc, msg)
    rc, msg = call(c=5)
    assert "5 channels" in msg
    rc, msg = call(y0=5, h=4)
    assert "crop 4x8 at (5, 0)" in msg and "8x8 source" in msg
    with pytest.raises(RuntimeError, match="u8_to_nhwc4"):
        amd._lib.check(rc, "u8_to_nhwc4")
