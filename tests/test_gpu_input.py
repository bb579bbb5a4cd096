"""The 8-bit input path on the GPU: vq2_u8_to_nhwc4 against the reference loader's transform restated with plain torch
(exact), Stage1Trainer.step from uint8 batches against the same steps from host-normalised floats (bitwise),
VQVAE_Deep through ImageNormalizer.nchw, the stream ordering of HostBatchPrefetcher, and the example end to end."""
import ctypes
import glob
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from oracle import vqvae_deep_oracle as OD
from oracle import vqvae_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)     # train_vqvae.py:154 (+ a fourth channel)


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def reference_transform(u8_nchw, mean, std):
    """ToTensor + Normalize as torchvision executes them (see tests/test_input_cpu.py), on a uint8 NCHW batch."""
    x = u8_nchw.to(dtype=torch.float32).div(255)
    m, s = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
    return x.sub_(m[None, :, None, None]).div_(s[None, :, None, None])


def random_bytes(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def host_normalised(u8, layout, mean, std, box=None):
    """float32 NCHW batch the reference's loader would hand the model for these pixels (cropped to box)."""
    nchw = u8.permute(0, 3, 1, 2) if layout == "hwc" else u8
    x = reference_transform(nchw, mean, std)
    if box is not None:
        y0, x0, h, w = box
        x = x[:, :, y0:y0 + h, x0:x0 + w]
    return x.contiguous()


def launched(amd, fn):
    lib = amd._lib.lib
    lib.vq2_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.vq2_prof_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.vq2_prof_report(buf, len(buf))
    return out, [ln.split()[0] for ln in buf.value.decode().splitlines()]


# (Hs, Ws, y0, x0, H, W)
SHAPES = {
    "256x256": (256, 256, 0, 0, 256, 256),              # every row segment on dword boundaries
    "w5": (7, 5, 0, 0, 7, 5),                           # tails: W % 4 != 0 (and less than one tile)
    "w30": (9, 30, 0, 0, 9, 30),
    "w257": (6, 257, 0, 0, 6, 257),
    "crop_odd": (40, 48, 3, 5, 32, 40),                 # odd crop origin
    "crop_aligned": (40, 48, 1, 8, 36, 32),             # a crop whose segments stay on dword boundaries
    "wide_source": (20, 37, 1, 4, 16, 28),              # Ws * C not a multiple of 4
}
GUARD = 256     # floats in front of and behind dst


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_kernel_equals_the_reference_transform_exactly(amd, layout, c, n, shape):
    hs, ws, y0, x0, h, w = SHAPES[shape]
    mean, std = MEAN[:c], STD[:c]
    u8 = random_bytes((n, hs, ws, c) if layout == "hwc" else (n, c, hs, ws), hs * 1000 + ws * 10 + c + n)
    view = u8 if layout == "hwc" else u8.permute(0, 2, 3, 1)
    view[0, y0, x0, :] = 0                              # both ends of the byte range, inside the window
    view[-1, y0 + h - 1, x0 + w - 1, :] = 255
    want = torch.zeros((n, h, w, 4))
    want[..., :c] = host_normalised(u8, layout, mean, std, (y0, x0, h, w)).permute(0, 2, 3, 1)

    norm = amd.ImageNormalizer(mean, std, layout=layout)
    img, lut = u8.to(DEV), norm.table_on(torch.device(DEV))
    flat = torch.full((n * h * w * 4 + 2 * GUARD,), float("nan"), device=DEV)
    dst = flat[GUARD:GUARD + n * h * w * 4]
    lib = amd._lib.lib

    def run():
        rc = lib.vq2_u8_to_nhwc4(img.data_ptr(), amd.ops.U8_LAYOUTS[layout], n, c, hs, ws, y0, x0, h, w, lut.data_ptr(),
                                 dst.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.vq2_last_error()
    _, labels = launched(amd, run)
    unit = c if layout == "hwc" else 1
    path = "dword" if (w * unit) % 4 == 0 and (x0 * unit) % 4 == 0 and (ws * unit) % 4 == 0 else "byte"
    assert labels == ["u8_to_nhwc4|N=%d,H=%d,W=%d,C=%d,%s,%s" % (n, h, w, c, layout, path)], labels
    got = dst.view(n, h, w, 4).cpu()
    assert torch.equal(got, want)                       # NaN anywhere (an unwritten pixel or pad lane) fails this too
    assert got.view(torch.int32).equal(want.view(torch.int32))
    assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all()), "written outside dst"
    if shape in ("256x256", "crop_odd"):                # the same through the public objects
        y0c, x0c = amd.ImageNormalizer.crop_origin(hs, h), amd.ImageNormalizer.crop_origin(ws, w)
        pub = amd.ImageNormalizer(mean, std, layout=layout, crop=(h, w))
        want_c = host_normalised(u8, layout, mean, std, (y0c, x0c, h, w))
        x = pub(img)
        assert tuple(x.shape) == (n, h, w, 4) and x.is_contiguous()
        assert torch.equal(x[..., :c].cpu(), want_c.permute(0, 2, 3, 1)) and float(x[..., c:].abs().sum()) == 0.0
        y = pub.nchw(img)
        assert tuple(y.shape) == (n, c, h, w) and torch.equal(y.cpu(), want_c)


def test_every_path_is_among_the_cases():
    paths = set()
    for layout in ("hwc", "chw"):
        for c in (1, 3, 4):
            for hs, ws, y0, x0, h, w in SHAPES.values():
                unit = c if layout == "hwc" else 1
                paths.add((layout, (w * unit) % 4 == 0 and (x0 * unit) % 4 == 0 and (ws * unit) % 4 == 0, y0 + x0 > 0))
    assert len(paths) == 8      # {hwc, chw} x {dword, byte} x {whole image, crop}


def test_call_time_errors_on_the_gpu(amd):
    norm = amd.ImageNormalizer()
    with pytest.raises(RuntimeError, match="channels"):
        norm(torch.zeros((1, 3, 8, 8), dtype=torch.uint8, device=DEV))            # CHW batch to an HWC normaliser
    with pytest.raises(RuntimeError, match="contiguous"):
        norm(torch.zeros((1, 8, 8, 6), dtype=torch.uint8, device=DEV)[..., ::2])
    with pytest.raises(RuntimeError, match="uint8"):
        norm(torch.zeros((1, 8, 8, 3), device=DEV))
    with pytest.raises(ValueError, match="larger"):
        amd.ImageNormalizer(crop=(9, 8))(torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV))


def build(amd, cfg, seed, **kw):
    model = amd.VQVAE(channel=cfg.channel, n_res_block=cfg.n_res_block, n_res_channel=cfg.n_res_channel,
                      embed_dim=cfg.embed_dim, n_embed=cfg.n_embed)
    model.load_state_dict(O.make_state(cfg, seed))
    model.to(DEV)
    return model, amd.Stage1Trainer(model, lr=3e-4, **kw)


STEP_CASES = {
    # config, layout, source H x W, crop
    "tiny_hwc": (O.TINY, "hwc", (32, 32), None),
    "tiny_hwc_crop": (O.TINY, "hwc", (37, 41), (32, 32)),
    "tiny_chw": (O.TINY, "chw", (32, 32), None),
    "default_hwc": (O.DEFAULT, "hwc", (64, 64), None),
    "default_chw_crop": (O.DEFAULT, "chw", (70, 67), (64, 64)),
}


@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_the_step_from_uint8_is_the_step_from_normalised_floats(amd, case):
    """Same seeded state, three steps on three batches: trainer.step(uint8) and trainer.step(host-normalised float NCHW)
    leave bitwise equal parameters, codebooks, EMA buffers and loss terms -- identical x, the same kernels downstream."""
    cfg, layout, (hs, ws), crop = STEP_CASES[case]
    mean, std = MEAN[:3], STD[:3]
    norm = amd.ImageNormalizer(mean, std, layout=layout, crop=crop)
    box = norm.box(hs, ws)
    m8, t8 = build(amd, cfg, 77, normalizer=norm)
    mf, tf = build(amd, cfg, 77)
    for i in range(3):
        u8 = random_bytes((2, hs, ws, 3) if layout == "hwc" else (2, 3, hs, ws), 500 + i)
        xf = host_normalised(u8, layout, mean, std, box)
        assert tuple(xf.shape) == (2, 3, box[2], box[3])
        (o8, labels) = launched(amd, lambda: t8.step(u8.to(DEV), return_dec=True))
        of = tf.step(xf.to(DEV), return_dec=True)
        assert any(l.startswith("u8_to_nhwc4|") for l in labels) and not any(l.startswith("nchw_to_nhwc4|") for l in labels)
        torch.cuda.synchronize()
        for k in ("loss", "recon", "latent", "dec"):
            assert torch.equal(o8[k], of[k]), (case, i, k)
        assert tuple(o8["dec"].shape) == tuple(xf.shape)
        assert bool(torch.isfinite(o8["loss"]))
    s8, sf = m8.state_dict(), mf.state_dict()
    assert list(s8.keys()) == list(sf.keys())
    for k in s8:
        assert torch.equal(s8[k], sf[k]), (case, k)
    moved = sum(not torch.equal(s8[k].cpu(), v) for k, v in O.make_state(cfg, 77).items() if not k.startswith("dec_ir."))
    assert moved > 10                                   # (the steps did train)
    with pytest.raises(TypeError, match="normalizer"):
        tf.step(random_bytes((2, hs, ws, 3), 1).to(DEV))


def test_deep_model_through_normalizer_nchw(amd):
    cfg = OD.DEEP_TINY
    m = amd.VQVAE_Deep(channel=cfg.channel, n_res_block=cfg.n_res_block, n_res_channel=cfg.n_res_channel,
                       embed_dim=cfg.embed_dim, n_embed=cfg.n_embed, style_dim=cfg.style_dim)
    m.load_state_dict(OD.make_deep_state(cfg, 7, 0.3, 1.5))
    m.to(DEV).eval()
    style = OD.make_style(2, cfg, 7).to(DEV)
    u8 = random_bytes((2, 36, 35, 3), 9)
    norm = amd.ImageNormalizer(MEAN[:3], STD[:3], crop=(32, 32))
    xf = host_normalised(u8, "hwc", MEAN[:3], STD[:3], norm.box(36, 35))
    with torch.no_grad():
        x8 = norm.nchw(u8.to(DEV))
        assert torch.equal(x8.cpu(), xf)
        dec8, diff8, _ = m(x8, style=style)
        decf, difff, _ = m(xf.to(DEV), style=style)
    assert torch.equal(dec8, decf) and torch.equal(diff8, difff) and bool(torch.isfinite(dec8).all())


def host_batches(count, shape=(4, 16, 16, 3), as_tensor=False):
    out = [random_bytes(shape, 40 + i) for i in range(count)]
    return out if as_tensor else [b.numpy() for b in out]


@pytest.mark.parametrize("trainer_first", [True, False], ids=["trainer_before", "trainer_after"])
@pytest.mark.parametrize("depth", [2, 3])
def test_prefetcher_delivers_in_order_across_the_stream_swap(amd, depth, trainer_first):
    """Stage1Trainer's constructor installs a high-priority stream as the thread's current stream: the prefetcher looks the
    consumer's stream up at every __next__, so it is right whether it was built (and started) before or after."""
    start = threading.active_count()
    torch.cuda.set_stream(torch.cuda.default_stream())
    src = host_batches(7, as_tensor=depth == 3)
    norm = amd.ImageNormalizer()
    if trainer_first:
        _, trainer = build(amd, O.TINY, 5, normalizer=norm)
        assert torch.cuda.current_stream().priority < 0
    got = []
    with amd.HostBatchPrefetcher(iter(src), DEV, depth=depth) as feed:
        for i, batch in enumerate(feed):
            assert batch.is_cuda and batch.dtype == torch.uint8 and tuple(batch.shape) == (4, 16, 16, 3)
            if i == 1 and not trainer_first:
                assert torch.cuda.current_stream().priority == 0
                _, trainer = build(amd, O.TINY, 5, normalizer=norm)
                assert torch.cuda.current_stream().priority < 0
            if i >= 2:
                trainer.step(batch)
            got.append(batch.clone())
        with pytest.raises(StopIteration):
            next(feed)
    torch.cuda.synchronize()
    assert len(got) == 7
    for g, s in zip(got, src):
        assert torch.equal(g.cpu(), torch.as_tensor(s))
    assert threading.active_count() == start


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_prefetcher_slot_reuse_waits_for_the_consumer(amd, depth):
    """The consumer queues a long chain of kernels behind every batch and only then reads it (a clone at the END of the
    chain): a slot refilled before the consumer's stream got there would show the wrong bytes.  One synchronise, at the end."""
    src = host_batches(7, shape=(4, 32, 32, 3))
    _, trainer = build(amd, O.TINY, 5, normalizer=amd.ImageNormalizer())
    a = torch.randn(4096, 4096, device=DEV) * 0.01
    c = torch.empty_like(a)
    got = []
    feed = amd.HostBatchPrefetcher(src, DEV, depth=depth)
    for batch in feed:
        for _ in range(3):
            torch.mm(a, a, out=c)                       # a few milliseconds of queue in front of the reads
        for _ in range(3):
            trainer.step(batch)
        got.append(batch.clone())
    torch.cuda.synchronize()
    assert len(got) == 7
    for g, s in zip(got, src):
        assert torch.equal(g.cpu(), torch.from_numpy(s))


def test_prefetcher_surfaces_source_errors_and_leaves_no_thread(amd):
    start = threading.active_count()

    def failing():
        for b in host_batches(3):
            yield b
        raise ValueError("the fourth item")

    feed = amd.HostBatchPrefetcher(failing(), DEV, depth=2)
    want = host_batches(3)
    for i in range(3):
        assert torch.equal(next(feed).cpu(), torch.from_numpy(want[i]))
    with pytest.raises(ValueError, match="the fourth item"):
        next(feed)
    feed.close()
    feed.close()
    assert threading.active_count() == start
    with pytest.raises(StopIteration):
        next(feed)
    # wrong dtype / a batch of another shape: errors of the source, too
    with pytest.raises(TypeError, match="uint8"):
        next(amd.HostBatchPrefetcher([np.zeros((2, 4, 4, 3), np.float32)], DEV))
    feed = amd.HostBatchPrefetcher([np.zeros((2, 4, 4, 3), np.uint8), np.zeros((2, 4, 5, 3), np.uint8)], DEV)
    next(feed)
    with pytest.raises(ValueError, match="shape"):
        next(feed)
    # empty source; early close with the worker waiting for a slot
    with pytest.raises(StopIteration):
        next(amd.HostBatchPrefetcher([], DEV))
    feed = amd.HostBatchPrefetcher(host_batches(6), DEV, depth=2)
    first = next(feed)
    feed.close()
    torch.cuda.synchronize()
    assert torch.equal(first.cpu(), torch.from_numpy(host_batches(1)[0]))
    assert threading.active_count() == start


def test_example_trains_from_uint8_files(amd, tmp_path):
    """examples/train_stage1.py on two uint8 [N,H,W,3] files, in a fresh process as a user would run it."""
    data = tmp_path / "data"
    data.mkdir()
    rng = np.random.default_rng(0)
    for i in range(2):
        np.save(data / f"batch{i}.npy", rng.integers(0, 256, (8, 64, 64, 3), dtype=np.uint8))
    out = tmp_path / "ckpt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_stage1.py"), "--size", "64", "--batch_size", "4",
                        "--epoch", "1", "--norm", "imagenet", "--path", str(data), "--out", str(out)],
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"it 0; mse: ([0-9.eE+-]+|nan|inf);", r.stdout)
    assert m and np.isfinite(float(m.group(1))), r.stdout[-2000:]
    sd = torch.load(out / "vqvae_001.pt", map_location="cpu", weights_only=True)
    assert list(sd.keys()) == list(amd.VQVAE().state_dict().keys())
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())


def test_u8_kernels_do_not_spill():
    files = glob.glob(os.path.join(ROOT, "vq-vae-2-pytorch_amd", "csrc", "_obj", "*.res"))
    if not files:
        pytest.skip("no resource reports: run __graft_entry__.build() first")
    seen, name = 0, None
    for f in files:
        for line in open(f):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                seen += "u8_to_nhwc4" in name
                continue
            m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
            if m and name and "u8_to_nhwc4" in name:
                assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
    assert seen == 4, f"{seen} u8_to_nhwc4 kernels in the reports"
