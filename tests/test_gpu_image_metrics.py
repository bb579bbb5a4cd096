"""GPU: vq2_image_metrics (integer squared error and fp64 SSIM of the two 8-bit images) against the fp64 numpy reference
of _image_metrics_ref.py at the kernel's tile boundaries, its exact cases and its independence of the launch size; the
Evaluator's psnr / ssim / mse_u8 in one batch, in split batches, on two ranks and through the example script; and that
neither the default Evaluator nor training notices any of it.

Tolerance of ssim: 1e-10 absolute.  The moments are 22-term fp64 sums of magnitude <= 65,025, so a variance is off by
at most 22 * 2^-53 * 65,025 = 1.6e-10, i.e. 3e-12 on a map value (the denominator is at least C2 = 58.5); 1e-10 is
about 30 times that bound and was not taken from a measurement."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _image_metrics_ref as R
from oracle import vqvae_oracle as O
from test_eval_cpu import reference_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
STATS = {"half": {c: ((0.5,) * c, (0.5,) * c) for c in (1, 3, 4)},
         "imagenet": {1: ((0.485,), (0.229,)), 3: IMAGENET, 4: (IMAGENET[0] + (0.5,), IMAGENET[1] + (0.5,))}}
T = 32                                  # the kernel's tile edge, in window positions
SSIM_TOL = 1e-10


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _model(amd, cfg, seed):
    m = amd.VQVAE(channel=cfg.channel, n_res_block=cfg.n_res_block, n_res_channel=cfg.n_res_channel,
                  embed_dim=cfg.embed_dim, n_embed=cfg.n_embed)
    m.load_state_dict(O.make_state(cfg, seed))
    return m.to(dev())


def _nhwc4(x, fill=7.0):
    """float32 [n,h,w,c] -> [n,h,w,4] on the GPU, the lanes beyond c filled with a value that must not count."""
    n, h, w, c = x.shape
    buf = torch.full((n, h, w, 4), fill)
    buf[..., :c] = x
    return buf.to(dev())


def _check(got, a_bytes, b_bytes, what):
    sse, ssim = got
    assert sse.dtype == torch.int64 and ssim.dtype == torch.float64 and sse.shape == ssim.shape == (a_bytes.shape[0],)
    want_sse, want_ssim = R.sse_u8(a_bytes, b_bytes), R.ssim_u8(a_bytes, b_bytes)
    err = np.abs(ssim.cpu().numpy() - want_ssim).max()
    print(what, "ssim", want_ssim, "max abs error", err)
    assert np.array_equal(sse.cpu().numpy(), want_sse), what
    assert err <= SSIM_TOL, (what, err)


# ------------------------------------------------------------------ 1. the kernel at its boundaries
# one position; one partial tile; exactly one tile; one position past it; several tiles with a ragged edge -- in each
# direction on its own -- and a non-square multiple of 16
SIZES = [(11, 11), (12, T + 11), (T + 10, T + 10), (T + 11, 12), (2 * T + 13, 2 * T + 13), (11, 2 * T + 13),
         (2 * T + 13, T + 10), (48, 80)]


@pytest.mark.parametrize("c", [1, 3, 4])
def test_kernel_matches_the_reference_at_tile_boundaries(amd, c):
    for name in ("half", "imagenet"):
        mean, std = STATS[name][c]
        norm = amd.ImageNormalizer(mean, std)
        table = norm.table                                           # [c,256]: what each byte normalises to
        d = norm.inverse()
        for h, w in SIZES:
            g = torch.Generator().manual_seed(1000 * h + w + c)
            a = torch.randint(0, 256, (3, h, w, c), dtype=torch.uint8, generator=g)
            b = torch.randint(0, 256, (3, h, w, c), dtype=torch.uint8, generator=g)
            b[1] = (a[1].int() + torch.randint(-6, 7, a[1].shape, generator=g)).clamp(0, 255).to(torch.uint8)   # a noisy copy
            xa = torch.stack([table[k][a[..., k].long()] for k in range(c)], -1)
            xb = torch.stack([table[k][b[..., k].long()] for k in range(c)], -1)
            got = amd.ops.image_metrics(_nhwc4(xa), _nhwc4(xb, -3.0), c, d.inv_s, d.m)
            _check(got, a.numpy(), b.numpy(), (name, c, h, w))


# ------------------------------------------------------------------ 2. arbitrary floats; scalar loads
def test_arbitrary_floats_and_the_scalar_load_path(amd):
    mean, std = IMAGENET
    d = amd.ImageDenormalizer(mean, std)
    g = torch.Generator().manual_seed(77)
    for h, w in ((T + 11, 2 * T + 13), (24, 16)):
        xa = torch.randn(3, h, w, 3, generator=g) * 1.5             # beyond the clamp on both sides
        xb = torch.randn(3, h, w, 3, generator=g) * 1.5
        ba, bb = reference_bytes(xa, mean, std), reference_bytes(xb, mean, std)
        assert int((ba == 0).sum()) and int((ba == 255).sum())
        vec = amd.ops.image_metrics(_nhwc4(xa), _nhwc4(xb), 3, d.inv_s, d.m)
        _check(vec, ba.numpy(), bb.numpy(), ("floats", h, w))
        # pixel stride 8: the first three lanes of an 8-lane tensor, and a channel slice of another one
        a8 = torch.full((3, h, w, 8), 7.0)
        a8[..., :3] = xa
        b8 = torch.full((3, h, w, 8), 7.0)
        b8[..., 4:7] = xb
        a8, b8 = a8.to(dev()), b8.to(dev())
        for pair in ((a8, b8[..., 4:8]), (a8, _nhwc4(xb)), (_nhwc4(xa), b8[..., 4:8])):
            sse, ssim = amd.ops.image_metrics(pair[0], pair[1], 3, d.inv_s, d.m)
            assert torch.equal(sse, vec[0]) and torch.equal(ssim, vec[1]), (h, w)


# ------------------------------------------------------------------ 3. exact cases
def test_identical_images_and_symmetry(amd):
    mean, std = IMAGENET
    d = amd.ImageDenormalizer(mean, std)
    g = torch.Generator().manual_seed(5)
    for h, w in ((11, 11), (T + 11, 2 * T + 13)):
        a = _nhwc4(torch.randn(3, h, w, 3, generator=g) * 1.5)
        b = _nhwc4(torch.randn(3, h, w, 3, generator=g) * 1.5)
        sse, ssim = amd.ops.image_metrics(a, a, 3, d.inv_s, d.m)
        assert torch.equal(sse, torch.zeros_like(sse)) and torch.equal(ssim, torch.ones_like(ssim)), ssim
        ab, ba = amd.ops.image_metrics(a, b, 3, d.inv_s, d.m), amd.ops.image_metrics(b, a, 3, d.inv_s, d.m)
        assert torch.equal(ab[0], ba[0]) and float((ab[1] - ba[1]).abs().max()) <= 1e-12


# ------------------------------------------------------------------ 4. launch size
def test_image_metrics_do_not_depend_on_the_launch_size(amd):
    d = amd.ImageDenormalizer()
    for size in (24, 64, 256):
        g = torch.Generator().manual_seed(size)
        a = _nhwc4(torch.randn(9, size, size, 3, generator=g))
        b = _nhwc4(torch.randn(9, size, size, 3, generator=g))
        whole = amd.ops.image_metrics(a, b, 3, d.inv_s, d.m)
        parts = [amd.ops.image_metrics(a[lo:hi], b[lo:hi], 3, d.inv_s, d.m) for lo, hi in ((0, 5), (5, 8), (8, 9))]
        assert torch.equal(whole[0], torch.cat([p[0] for p in parts])), size
        assert torch.equal(whole[1], torch.cat([p[1] for p in parts])), size
        assert bool((whole[1] < 1).all()) and bool((whole[0] > 0).all())


# ------------------------------------------------------------------ 5. arguments
def test_too_small_images_and_too_many_channels_are_refused(amd):
    d = amd.ImageDenormalizer()
    x = torch.zeros(2, 10, 16, 4, device=dev())
    with pytest.raises(RuntimeError, match="10x16"):
        amd.ops.image_metrics(x, x, 3, d.inv_s, d.m)
    assert b"10x16" in amd._lib.lib.vq2_last_error()
    y = torch.zeros(2, 16, 16, 8, device=dev())
    with pytest.raises(RuntimeError):
        amd.ops.image_metrics(y, y, 5, (2.0,) * 5, (0.5,) * 5)
    with pytest.raises(RuntimeError):
        amd.ops.image_metrics(y, y[:, :12], 3, d.inv_s, d.m)


# ------------------------------------------------------------------ 6-8. the Evaluator
@pytest.fixture(scope="module")
def runs(amd):
    """The seed-7 default model on nine 64x64 uint8 images: metrics in one batch (with the bytes it exported), metrics in
    batches of 5 + 3 + 1, and no metrics.  Computed once; nobody modifies it."""
    m = _model(amd, O.DEFAULT, 7).eval()
    img = torch.randint(0, 256, (9, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))
    imgd = img.to(dev())
    norm = amd.ImageNormalizer(*IMAGENET, layout="hwc")
    one = amd.Evaluator(m, norm, image_metrics=True)
    rec = one.update(imgd, return_u8=True)
    split = amd.Evaluator(m, norm, image_metrics=True)
    for lo, hi in ((0, 5), (5, 8), (8, 9)):
        split.update(imgd[lo:hi].contiguous())
    plain = amd.Evaluator(m, norm)
    plain.update(imgd)
    return {"img": img.numpy(), "rec": rec.cpu().numpy(), "one": one.result(), "split": split.result(), "plain": plain.result()}


def test_evaluator_saw_the_exported_bytes(runs):
    img, rec, r = runs["img"], runs["rec"], runs["one"]
    assert rec.shape == img.shape and rec.dtype == np.uint8
    sse = int(R.sse_u8(img, rec).sum())
    want_mse, want_psnr, want_ssim = R.mse_u8(sse, img.size), R.psnr(sse, img.size), float(R.ssim_u8(img, rec).mean())
    print("mse_u8", r["mse_u8"], want_mse, "psnr", r["psnr"], want_psnr, "ssim", r["ssim"], want_ssim)
    assert sse > 0 and r["images"] == 9
    assert abs(r["mse_u8"] - want_mse) <= 1e-12 * want_mse
    assert abs(r["psnr"] - want_psnr) <= 1e-12 * want_psnr
    assert abs(r["ssim"] - want_ssim) <= SSIM_TOL


def test_evaluator_batches_of_5_3_1_equal_one_batch_of_9(runs):
    a, b = runs["one"], runs["split"]
    print({k: (a[k], b[k]) for k in ("psnr", "ssim", "mse_u8")})
    # equality, by derivation: every image's values are bitwise those of any other launch (the test above), the integer
    # total is exact, and the SSIM total is ONE double that the images are added to in image order, batch after batch
    assert a["psnr"] == b["psnr"] and a["ssim"] == b["ssim"] and a["mse_u8"] == b["mse_u8"]


TEN = ["mse", "latent", "images", "perplexity_t", "perplexity_b", "used_t", "used_b", "n_embed", "counts_t", "counts_b"]


def test_default_evaluator_is_unchanged(runs):
    plain, one = runs["plain"], runs["one"]
    assert list(plain.keys()) == TEN
    assert list(one.keys()) == TEN + ["mse_u8", "psnr", "ssim"]
    for k in TEN:
        if isinstance(plain[k], torch.Tensor):
            assert torch.equal(plain[k], one[k]), k
        else:
            assert plain[k] == one[k], k


# ------------------------------------------------------------------ 9. training is left alone
def _same(a, b, path=""):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), f"{path} differs"
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for k, (u, v) in enumerate(zip(a, b)):
            _same(u, v, f"{path}[{k}]")
    else:
        assert a == b, f"{path}: {a!r} != {b!r}"


def test_evaluation_with_image_metrics_leaves_training_alone(amd):
    imgs = [O.make_images(4, 32, 500 + s).to(dev()) for s in range(2)]
    val_u8 = torch.randint(0, 256, (3, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(dev())
    val_f = O.make_images(2, 32, 998).to(dev())

    def run(evaluate):
        m = _model(amd, O.TINY, 21)
        tr = amd.Stage1Trainer(m, lr=3e-4, normalizer=amd.ImageNormalizer(layout="hwc"))
        tr.step(imgs[0])
        if evaluate:
            r = tr.evaluate_image_metrics([val_u8, val_f], sample=val_u8)
            assert r["images"] == 5 and 0 < r["psnr"] < 100 and -1 <= r["ssim"] <= 1 and r["mse_u8"] > 0
            assert "sample" in r and m.training and all(mod.training for mod in m.modules())
            assert "psnr" not in tr.evaluate([val_f])
        tr.step(imgs[1])
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in m.state_dict().items()}, tr.state_dict()

    model_a, trainer_a = run(True)
    model_b, trainer_b = run(False)
    _same(model_a, model_b, "model")
    _same(trainer_a, trainer_b, "trainer")


# ------------------------------------------------------------------ 10. the example script
def test_eval_example_prints_psnr_and_ssim(amd, tmp_path):
    val_data = np.random.default_rng(12).integers(0, 256, (10, 64, 64, 3), dtype=np.uint8)
    (tmp_path / "val").mkdir()
    np.save(tmp_path / "val" / "v.npy", val_data)
    torch.manual_seed(12)
    m = amd.VQVAE()
    ckpt = tmp_path / "fresh.pt"
    torch.save(m.state_dict(), ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "examples", "eval_stage1.py"), "--ckpt", str(ckpt), "--path", str(tmp_path / "val"),
           "--size", "64", "--batch_size", "4"]
    on = subprocess.run(cmd + ["--image_metrics"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert on.returncode == 0, on.stdout[-2000:] + on.stderr[-3000:]
    off = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert off.returncode == 0, off.stdout[-2000:] + off.stderr[-3000:]
    assert "images: 10" in off.stdout and "psnr" not in off.stdout and "ssim" not in off.stdout
    m.to(dev()).eval()
    ev = amd.Evaluator(m, amd.ImageNormalizer(layout="hwc", crop=(64, 64)), image_metrics=True)
    for lo in range(0, 10, 4):
        ev.update(torch.from_numpy(val_data[lo:lo + 4]).to(dev()))
    r = ev.result()
    line = [l for l in on.stdout.splitlines() if "images: 10" in l][0]
    print(line)
    assert line.endswith(f"; psnr: {r['psnr']:.2f} dB; ssim: {r['ssim']:.4f}"), (line, r["psnr"], r["ssim"])
    assert line.startswith([l for l in off.stdout.splitlines() if "images: 10" in l][0])
    assert re.search(r"psnr: \d+\.\d\d dB; ssim: -?\d\.\d{4}$", line)


# ------------------------------------------------------------------ 11. two ranks over gloo sharing the card
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _metrics_run(imgs):
    import vqvae2_amd
    m = _model(vqvae2_amd, O.TINY, 1234).eval()
    ev = vqvae2_amd.Evaluator(m, vqvae2_amd.ImageNormalizer(layout="hwc"), image_metrics=True)
    for lo in range(0, imgs.shape[0], 2):
        ev.update(imgs[lo:lo + 2].contiguous().cuda())
    r = ev.result()
    return {k: np.float64(r[k]) for k in ("psnr", "ssim", "mse_u8", "mse", "images")}


def _images():
    return torch.randint(0, 256, (8, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321))


def _metrics_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    share = _images()[:6] if rank == 0 else _images()[6:]           # unequal shares: 3 batches and 1
    np.savez(out + f".rank{rank}.npz", **_metrics_run(share))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_image_metrics_equal_one_rank_on_the_whole_set(tmp_path):
    out = str(tmp_path / "metrics_dp")
    mp.spawn(_metrics_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    ref = _metrics_run(_images())
    for r in (r0, r1):
        print({k: (float(r[k]), float(ref[k])) for k in ref})
        assert int(r["images"]) == int(ref["images"]) == 8
        assert float(r["mse_u8"]) == float(ref["mse_u8"]) and float(r["psnr"]) == float(ref["psnr"])   # integer totals
        assert abs(float(r["ssim"]) - float(ref["ssim"])) <= 1e-12 * abs(float(ref["ssim"]))          # the collective's order
    assert float(r0["ssim"]) == float(r1["ssim"])
