"""GPU: the evaluation / 8-bit export path -- vq2_nhwc_to_u8 bit for bit against the reference's arithmetic restated on
the CPU, the Evaluator against the reference's golden indices and the oracle's loss terms, batch-size independence,
evaluation between train steps leaving the run bitwise alone, two ranks, the example scripts, the out-of-range flag."""
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

from oracle import vqvae_oracle as O
from oracle.make_golden_cases import SEED
from test_eval_cpu import reference_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
STATS = {1: ((0.5,), (0.5,)), 3: IMAGENET, 4: (IMAGENET[0] + (0.5,), IMAGENET[1] + (0.5,))}


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


# ------------------------------------------------------------------ 1. byte conversion, bit-exact
def _inputs(amd, n, h, w, c, seed):
    """float32 [n,h,w,c]: N(0, 1.5^2) noise with the special values written over its head -- every table value (must
    return to its byte), the neighbours of both clamp edges, +-inf, +-1e30 -- and NaNs (returned as a mask)."""
    mean, std = STATS[c]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g) * 1.5
    table = amd.ImageNormalizer(mean, std).table.t().contiguous()           # [256,c]
    lo, hi = table[0], table[255]
    step = (hi - lo) / 255
    edge = [lo, torch.nextafter(lo, lo - 1), lo - 0.4 * step, lo - 0.6 * step, lo - step, lo + 0.4 * step,
            hi, torch.nextafter(hi, hi + 1), hi + 0.4 * step, hi + 0.6 * step, hi + step, hi - 0.6 * step]
    special = torch.cat([table, torch.stack(edge), torch.full((2, c), float("inf")) * torch.tensor([[1.], [-1.]]),
                         torch.full((2, c), 1e30) * torch.tensor([[1.], [-1.]])], 0)
    flat = x.reshape(-1, c)
    k = min(special.shape[0], flat.shape[0])
    flat[:k] = special[:k]
    nan = torch.zeros(flat.shape, dtype=torch.bool)
    if flat.shape[0] > k + 7:
        nan[k + 3, 0] = nan[k + 7, c - 1] = True
        flat[nan] = float("nan")
    return flat.reshape(n, h, w, c), nan.reshape(n, h, w, c)


def _expected_canvas(ref, nan, layout, hc, wc, origins, fill):
    """ref uint8 [n,h,w,c] placed at `origins` of an [hc,wc,c] canvas of `fill`; NaN inputs give 0."""
    n, h, w, c = ref.shape
    ref = ref.clone()
    ref[nan] = 0
    canvas = torch.full((hc, wc, c), fill, dtype=torch.uint8)
    for k, (y, x) in enumerate(origins):
        canvas[y:y + h, x:x + w] = ref[k]
    return canvas if layout == "hwc" else canvas.permute(2, 0, 1).contiguous()


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_byte_conversion_is_bit_exact(amd, layout, c):
    ops = amd.ops
    mean, std = STATS[c]
    d = amd.ImageDenormalizer(mean, std, layout)
    h = 6
    for w in (5, 7, 33, 64, 256):
        for n in (1, 9):
            x, nan = _inputs(amd, n, h, w, c, 1000 * w + n)
            ref = reference_bytes(torch.where(nan, torch.zeros(()), x), mean, std)
            for sliced in (False, True):
                # the kernel's operand: NHWC with 4 lanes, or a channel slice of an 8-lane buffer (ld > C, scalar loads)
                buf = torch.full((n, h, w, 8 if sliced else 4), 7.0)
                buf[..., 4 if sliced else 0:(4 if sliced else 0) + c] = x
                xd = buf.to(dev())[..., 4:8] if sliced else buf.to(dev())
                # a plain batch
                got = ops.nhwc_to_u8(xd, c, d.inv_s, d.m, layout)
                want = torch.where(nan, torch.zeros((), dtype=torch.uint8), ref)
                want = want if layout == "hwc" else want.permute(0, 3, 1, 2)
                assert torch.equal(got.cpu(), want), (layout, c, w, n, sliced, "batch")
                if sliced and w not in (7, 64):
                    continue
                # grids of 4 columns: every canvas byte, the padding against the caller's fill
                for pad in (0, 2, 4):
                    cols = 4
                    rows = (n + cols - 1) // cols
                    hc, wc = rows * (h + pad) + pad + 1, cols * (w + pad) + pad     # one spare row, whole width
                    origins = [((k // cols) * (h + pad) + pad, (k % cols) * (w + pad) + pad) for k in range(n)]
                    shape = (hc, wc, c) if layout == "hwc" else (c, hc, wc)
                    canvas = torch.full(shape, 77, dtype=torch.uint8, device=dev())
                    out = ops.nhwc_to_u8(xd, c, d.inv_s, d.m, layout, canvas=canvas, cols=cols, pad=pad)
                    assert out.data_ptr() == canvas.data_ptr()
                    assert torch.equal(canvas.cpu(), _expected_canvas(ref, nan, layout, hc, wc, origins, 77)), \
                        (layout, c, w, n, sliced, pad)
            # the public object: batch from NHWC and from an NCHW-shaped tensor, and make_grid's canvas
            xd = torch.zeros(n, h, w, 4)
            xd[..., :c] = x
            xd = xd.to(dev())
            want = torch.where(nan, torch.zeros((), dtype=torch.uint8), ref)
            want_l = want if layout == "hwc" else want.permute(0, 3, 1, 2)
            assert torch.equal(d(xd, nhwc=True).cpu(), want_l)
            assert torch.equal(d(x.permute(0, 3, 1, 2).contiguous().to(dev())).cpu(), want_l)     # [n,c,6,w]: reads as NCHW only
            for pad in (0, 2):
                hc, wc, origins = amd.grid_layout(n, h, w, 4, pad)
                got = d.grid([xd], nrow=4, padding=pad, pad_value=9, nhwc=True)
                assert torch.equal(got.cpu(), _expected_canvas(ref, nan, layout, hc, wc, origins, 9)), (layout, c, w, n, pad)
    # two batches in one grid (the sample image: inputs over reconstructions)
    x, nan = _inputs(amd, 6, h, 64, c, 5)
    ref = reference_bytes(torch.where(nan, torch.zeros(()), x), mean, std)
    xd = torch.zeros(6, h, 64, 4)
    xd[..., :c] = x
    xd = xd.to(dev())
    hc, wc, origins = amd.grid_layout(6, h, 64, 3, 2)
    got = d.grid([xd[:3], xd[3:]], nrow=3, nhwc=True)
    assert torch.equal(got.cpu(), _expected_canvas(ref, nan, layout, hc, wc, origins, 0))


def test_denormalizer_asks_when_a_shape_reads_both_ways(amd):
    """[2,3,5,4] for 3 channels is NHWC (H=3, W=5, 4 lanes) and NCHW (H=5, W=4): an error unless the caller says which,
    and each reading gives its own bytes.  Shapes that read as neither, and host tensors, are errors."""
    mean, std = IMAGENET
    d = amd.ImageDenormalizer(mean, std, "hwc")
    x = torch.randn(2, 3, 5, 4, generator=torch.Generator().manual_seed(2))
    xd = x.to(dev())
    with pytest.raises(RuntimeError, match="reads as NHWC and as NCHW"):
        d(xd)
    with pytest.raises(RuntimeError, match="reads as NHWC and as NCHW"):
        d.grid([xd], nrow=2)
    assert torch.equal(d(xd, nhwc=True).cpu(), reference_bytes(x[..., :3], mean, std))                       # [2,3,5,3]
    assert torch.equal(d(xd, nhwc=False).cpu(), reference_bytes(x.permute(0, 2, 3, 1).contiguous(), mean, std))   # [2,5,4,3]
    with pytest.raises(RuntimeError, match="neither"):
        d(torch.zeros(2, 5, 6, 7, device=dev()))
    with pytest.raises(RuntimeError, match="NHWC input"):
        d(torch.zeros(2, 3, 6, 7, device=dev()), nhwc=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        d(x)


# ------------------------------------------------------------------ 2. Evaluator against the reference's goldens
def test_evaluator_matches_golden_indices_and_oracle_losses(amd, golden):
    g = golden("full256")
    cfg = O.DEFAULT
    st = O.make_state(cfg, SEED)
    m = amd.VQVAE()
    m.load_state_dict(st)
    m.to(dev()).train()
    img = O.make_images(2, 256, SEED)
    ev = amd.Evaluator(m)
    assert ev.update(img.to(dev())) is None and m.training
    r = ev.result()
    assert r["images"] == 2 and r["n_embed"] == 512
    for key in ("t", "b"):
        want = np.bincount(g[f"id_{key}"].astype(np.int64).reshape(-1), minlength=512)
        assert np.array_equal(r[f"counts_{key}"].numpy(), want), f"counts_{key}"
        assert r[f"used_{key}"] == int((want > 0).sum())
        p = want[want > 0] / want.sum()
        assert abs(r[f"perplexity_{key}"] - float(np.exp(-(p * np.log(p)).sum()))) < 1e-9
    dec, diff, _, _ = O.vqvae_forward(st, cfg, img, training=False)
    _, recon, latent = O.stage1_loss(dec, diff, img)
    print("mse", r["mse"], "oracle", float(recon), "latent", r["latent"], "oracle", float(latent))
    # tolerance of tests/test_gpu_parity.py for the same two loss terms of a step (recon, latent: rtol 1e-4)
    np.testing.assert_allclose(r["mse"], float(recon), rtol=1e-4)
    np.testing.assert_allclose(r["latent"], float(latent), rtol=1e-4)
    ev.reset()
    assert ev.result()["images"] == 0


# ------------------------------------------------------------------ 3. batching
def test_sse_per_image_does_not_depend_on_the_launch_size(amd):
    ops = amd.ops
    for size in (8, 64, 256):
        g = torch.Generator().manual_seed(size)
        a = torch.randn(9, size, size, 4, generator=g)
        b = torch.randn(9, size, size, 4, generator=g)
        a[..., 3] = 0
        b[..., 3] = 0
        a, b = a.to(dev()), b.to(dev())
        whole = ops.sse_per_image(a, b)
        parts = torch.cat([ops.sse_per_image(a[lo:hi], b[lo:hi]) for lo, hi in ((0, 5), (5, 8), (8, 9))])
        assert torch.equal(whole, parts), size
        want = (a.double() - b.double()).pow(2).sum((1, 2, 3))
        np.testing.assert_allclose(whole.cpu().numpy(), want.cpu().numpy(), rtol=1e-5)


def test_evaluator_batches_of_5_3_1_equal_one_batch_of_9(amd):
    m = _model(amd, O.DEFAULT, 7).eval()
    img = O.make_images(9, 64, 7).to(dev())
    one = amd.Evaluator(m)
    one.update(img)
    a = one.result()
    split = amd.Evaluator(m)
    for lo, hi in ((0, 5), (5, 8), (8, 9)):
        split.update(img[lo:hi].contiguous())
    b = split.result()
    assert a["images"] == b["images"] == 9
    assert torch.equal(a["counts_t"], b["counts_t"]) and torch.equal(a["counts_b"], b["counts_b"])
    assert int(a["counts_t"].sum()) == 9 * 8 * 8 and int(a["counts_b"].sum()) == 9 * 16 * 16
    print("mse one batch", repr(a["mse"]), "5+3+1", repr(b["mse"]))
    # tighter than 1e-6 relative, by derivation: each per-image fp32 sum is bitwise independent of the launch it was
    # part of (the test above), and vq2_eval_accumulate adds them to ONE double total image by image, batch after batch
    # -- the same additions of the same operands in the same order however the nine images are cut.  Hence equality.
    assert a["mse"] == b["mse"]
    np.testing.assert_allclose(a["latent"], b["latent"], rtol=1e-5)


# ------------------------------------------------------------------ 4. evaluation leaves training alone
def _same(a, b, path=""):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), f"{path} differs"
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    else:
        assert a == b, f"{path}: {a!r} != {b!r}"


@pytest.mark.parametrize("case", ["tiny", "default"])
def test_evaluation_leaves_training_alone(amd, case):
    cfg = O.TINY if case == "tiny" else O.DEFAULT
    imgs = [O.make_images(4, 64, 300 + s).to(dev()) for s in range(6)]
    val_f = O.make_images(4, 64, 999).to(dev())
    val_u8 = torch.randint(0, 256, (3, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(dev())

    def run(evaluate):
        m = _model(amd, cfg, 21)
        tr = amd.Stage1Trainer(m, lr=3e-4, normalizer=amd.ImageNormalizer(layout="hwc"))
        for s in range(3):
            tr.step(imgs[s])
        if evaluate:
            torch.cuda.synchronize()
            before = {k: v.clone() for k, v in m.state_dict().items()}
            slots, preps = tr.arena.extra.clone(), [q._prep for q in tr.quantizers]
            prep_vals = [(p[0].clone(), p[1].clone()) for p in preps]
            keys = [q._prep_key for q in tr.quantizers]
            assert m.training
            r = tr.evaluate([val_f, val_u8], sample=val_u8)
            torch.cuda.synchronize()
            assert m.training and all(mod.training for mod in m.modules())
            assert r["images"] == 7 and r["sample"].shape == (2 * 66 + 2, 3 * 66 + 2, 3) and np.isfinite(r["mse"])
            _same(before, dict(m.state_dict()), "model")
            assert torch.equal(slots, tr.arena.extra), "EMA statistics slots were written by evaluate()"
            for q, p, pv, key in zip(tr.quantizers, preps, prep_vals, keys):
                assert q._prep is p and q._prep_key == key and q._prepared() is p
                assert torch.equal(p[0], pv[0]) and torch.equal(p[1], pv[1])
            m.eval()                      # an eval-mode model stays in eval mode
            tr.evaluate([val_f])
            assert not m.training and not any(mod.training for mod in m.modules())
            m.train()
        for s in range(3, 6):
            tr.step(imgs[s])
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in m.state_dict().items()}, tr.state_dict()

    model_a, trainer_a = run(True)
    model_b, trainer_b = run(False)
    _same(model_a, model_b, "model")
    _same(trainer_a, trainer_b, "trainer")


def test_modules_in_a_mode_of_their_own_keep_it(amd):
    """A model in train mode with one quantizer frozen in eval mode (its EMA codebook stands still) comes back from
    Evaluator.update, Stage1Trainer.evaluate and sample_grid with every module's flag as it was."""
    m = _model(amd, O.TINY, 3).train()
    tr = amd.Stage1Trainer(m, lr=3e-4, normalizer=amd.ImageNormalizer(layout="hwc"))
    m.quantize_t.eval()
    flags = [mod.training for mod in m.modules()]
    assert any(flags) and not all(flags)
    img = O.make_images(2, 32, 3).to(dev())
    amd.Evaluator(m).update(img)
    assert [mod.training for mod in m.modules()] == flags
    tr.evaluate([img], sample=img)
    assert [mod.training for mod in m.modules()] == flags


# ------------------------------------------------------------------ 5. return_u8
def test_return_u8_is_the_denormalised_module_output(amd):
    m = _model(amd, O.DEFAULT, 11).eval()
    u8 = torch.randint(0, 256, (3, 3, 64, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(8)).to(dev())
    norm = amd.ImageNormalizer(*IMAGENET, layout="chw")
    twin = norm.nchw(u8).contiguous()                                   # the normalised float batch, NCHW
    ev = amd.Evaluator(m, norm)
    from_u8 = ev.update(u8, return_u8=True)
    res_u8 = ev.result()
    ev.reset()
    from_float = ev.update(twin, return_u8=True)
    res_float = ev.result()
    assert from_u8.dtype == torch.uint8 and tuple(from_u8.shape) == (3, 3, 64, 64)
    assert torch.equal(from_u8, from_float)
    _same({k: v for k, v in res_u8.items()}, {k: v for k, v in res_float.items()}, "result")
    with torch.no_grad():
        dec, _ = m(twin)
    assert torch.equal(amd.ImageDenormalizer(*IMAGENET, layout="chw")(dec), from_float)
    hwc = amd.Evaluator(m, amd.ImageNormalizer(*IMAGENET, layout="hwc"))
    assert torch.equal(hwc.update(u8.permute(0, 2, 3, 1).contiguous(), return_u8=True), from_u8.permute(0, 2, 3, 1))
    with pytest.raises(TypeError):
        amd.Evaluator(m).update(u8)
    with pytest.raises(TypeError, match="forward_nhwc"):
        amd.Evaluator(amd.VQVAE_Deep())


# ------------------------------------------------------------------ 6. two ranks over gloo sharing the card
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _eval_run(imgs):
    import vqvae2_amd
    m = _model(vqvae2_amd, O.TINY, 1234).eval()
    ev = vqvae2_amd.Evaluator(m)
    for lo in range(0, imgs.shape[0], 2):
        ev.update(imgs[lo:lo + 2].contiguous().cuda())
    r = ev.result()
    return {"mse": np.float64(r["mse"]), "latent": np.float64(r["latent"]), "images": np.int64(r["images"]),
            "counts_t": r["counts_t"].numpy(), "counts_b": r["counts_b"].numpy()}


def _eval_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    full = O.make_images(8, 32, 4321)
    np.savez(out + f".rank{rank}.npz", **_eval_run(full[rank * 4:(rank + 1) * 4]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_evaluation_equals_one_rank_on_the_whole_set(tmp_path):
    out = str(tmp_path / "eval_dp")
    mp.spawn(_eval_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    ref = _eval_run(O.make_images(8, 32, 4321))
    for r in (r0, r1):
        assert int(r["images"]) == int(ref["images"]) == 8
        assert np.array_equal(r["counts_t"], ref["counts_t"]) and np.array_equal(r["counts_b"], ref["counts_b"])
        print("mse two ranks", repr(float(r["mse"])), "one rank", repr(float(ref["mse"])))
        assert abs(float(r["mse"]) - float(ref["mse"])) <= 1e-12 * float(ref["mse"])
        np.testing.assert_allclose(float(r["latent"]), float(ref["latent"]), rtol=1e-6)
    assert float(r0["mse"]) == float(r1["mse"])


# ------------------------------------------------------------------ 7. example scripts
def test_example_scripts_train_sample_and_evaluate(amd, tmp_path):
    from PIL import Image
    g = np.random.default_rng(12)
    train, val = tmp_path / "train", tmp_path / "val"
    train.mkdir()
    val.mkdir()
    np.save(train / "a.npy", g.integers(0, 256, (16, 64, 64, 3), dtype=np.uint8))
    val_data = g.integers(0, 256, (10, 64, 64, 3), dtype=np.uint8)      # batches of 4, 4 and a ragged 2: both scripts keep it
    np.save(val / "v.npy", val_data)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_stage1.py"), "--size", "64", "--batch_size", "4",
                        "--epoch", "1", "--path", str(train), "--val_path", str(val), "--eval_every", "2", "--sample_every", "2",
                        "--out", "ckpt"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if "val images" in l]
    assert len(lines) == 2 and all(int(re.search(r"val images: (\d+)", l).group(1)) == 10 for l in lines), r.stdout
    assert "perplexity t/b" in lines[0] and "used codes t/b" in lines[0]
    assert sorted(os.listdir(tmp_path / "sample")) == ["00001_00000.png", "00001_00002.png"]
    sample = np.asarray(Image.open(tmp_path / "sample" / "00001_00000.png"))
    assert sample.shape == (2 * 66 + 2, 4 * 66 + 2, 3) and sample.dtype == np.uint8
    # top row of the first sample: the first training batch's own pixels (the round trip is exact), borders black
    first = np.load(train / "a.npy")[:4]
    for k in range(4):
        assert np.array_equal(sample[2:66, 2 + 66 * k:66 + 66 * k], first[k])
    assert not sample[:2].any() and not sample[:, :2].any() and not sample[66:68].any()
    ckpt = tmp_path / "ckpt" / "vqvae_001.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "eval_stage1.py"), "--ckpt", str(ckpt), "--path", str(val),
                        "--size", "64", "--batch_size", "4", "--dump", "recon", "--dump_images", "4"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert int(re.search(r"images: (\d+)", r.stdout).group(1)) == 10, r.stdout
    assert sorted(os.listdir(tmp_path / "recon")) == ["recon_00000.png", "recon_00001.png", "recon_00002.png"]
    # the PNG is exactly the device canvas: the same checkpoint and batch through the library in this process
    m = amd.VQVAE()
    m.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=True))
    m.to(dev()).eval()
    norm = amd.ImageNormalizer(layout="hwc", crop=(64, 64))
    ev = amd.Evaluator(m, norm)
    for b in range(3):
        batch = torch.from_numpy(val_data[4 * b:4 * b + 4]).to(dev())
        ev.update(batch)
        with torch.no_grad():
            x = norm(batch)
            dec, _ = m.forward_nhwc(x)
        canvas = norm.inverse().grid([x, dec], nrow=batch.shape[0], nhwc=True)
        png = np.asarray(Image.open(tmp_path / "recon" / f"recon_{b:05d}.png"))
        assert np.array_equal(png, canvas.cpu().numpy()), b
    mine = ev.result()
    assert abs(float(re.search(r"mse: ([0-9.]+)", r.stdout).group(1)) - mine["mse"]) < 1e-6


# ------------------------------------------------------------------ 8. out-of-range index
def test_out_of_range_index_is_reported_not_dereferenced(amd):
    # the kernel, on tensors of the test's own: K = 64, three of the seven indices are outside and are counted nowhere
    counts = torch.full((64,), 5, dtype=torch.int64, device=dev())
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    amd.ops.index_hist(torch.tensor([0, 3, 63, 3], dtype=torch.int64, device=dev()), counts, flag)
    assert int(flag) == 0
    amd.ops.index_hist(torch.tensor([0, 3, 63, 64, -1, 2 ** 40, 3], dtype=torch.int64, device=dev()), counts, flag)
    want = torch.full((64,), 5, dtype=torch.int64)
    want[0], want[3], want[63] = 5 + 2, 5 + 4, 5 + 2
    assert torch.equal(counts.cpu(), want) and int(flag) == 1
    # the Evaluator: a forward that hands out one index equal to K makes result() raise; reset() clears it
    m = _model(amd, O.TINY, 5).eval()
    img = O.make_images(2, 32, 5).to(dev())
    ev = amd.Evaluator(m)
    ev.update(img)
    good = ev.result()
    forward = m.forward_nhwc

    def one_bad_index(x, return_ids=False):
        dec, diff, id_t, id_b = forward(x, return_ids=True)
        id_t = id_t.clone()
        id_t.view(-1)[0] = ev.k_t
        return dec, diff, id_t, id_b

    m.forward_nhwc = one_bad_index
    ev.update(img)
    with pytest.raises(RuntimeError, match="outside"):
        ev.result()
    del m.forward_nhwc
    ev.reset()
    ev.update(img)
    assert torch.equal(ev.result()["counts_t"], good["counts_t"])
