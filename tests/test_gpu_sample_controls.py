"""GPU checks of the sampler's controls: PriorSampler.sample / sample_model with top_k, top_p, prefix and return_logp on the
smallest models the sampler tests use (one with attention, one conditioned bottom without; random weights), and
examples/sample.py with --top_k / --top_p / --from_images."""
import argparse
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CLASS, BATCH, SEED = 6, 2, 1234567


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


@pytest.fixture(scope="module")
def samplers(amd):
    """name -> (sampler, condition, rows, width): the top prior with attention, the conditioned bottom prior without."""
    torch.manual_seed(3)
    top = amd.PixelSNAIL([4, 4], N_CLASS, 64, 3, 1, 1, 8).cuda().eval()
    bottom = amd.PixelSNAIL([8, 8], N_CLASS, 8, 3, 1, 1, 8, attention=False, n_cond_res_block=1, cond_res_channel=8).cuda().eval()
    cond = torch.randint(0, N_CLASS, (BATCH, 4, 4), generator=torch.Generator().manual_seed(4)).cuda()
    return {"top": (amd.PriorSampler(top), None, 4, 4), "bottom": (amd.PriorSampler(bottom), cond, 8, 8)}


def _step_logits(sampler, codes, cond):
    """[B, H, W, n_class]: what every step saw, from the same row programs."""
    return sampler.logits_given(codes, cond).permute(0, 2, 3, 1)


def _logp_bound(rel):
    return (N_CLASS + 8) * 2.0 ** -23 + 2.0 ** -22 * rel.abs()


# ----------------------------------------------------------------------------- 7. defaults
@pytest.mark.parametrize("name", ["top", "bottom"])
def test_defaults_are_the_plain_sampler(samplers, name):
    s, cond, _, _ = samplers[name]
    a = s.sample(BATCH, 0.9, cond, seed=SEED)
    assert torch.equal(a, s.sample(BATCH, 0.9, cond, seed=SEED, top_k=0, top_p=1.0))
    assert torch.equal(a, s.sample(BATCH, 0.9, cond, seed=SEED, top_k=N_CLASS + 5))          # clamped to n_class: every class
    assert torch.equal(a, s.sample(BATCH, 0.9, cond, seed=SEED, return_logp=True)[0])        # the filtered kernel, filters off


# ----------------------------------------------------------------------------- 8. prefix
@pytest.mark.parametrize("name", ["top", "bottom"])
def test_prefix_of_a_free_run_is_completed_to_that_run(amd, samplers, name):
    s, cond, rows, w = samplers[name]
    a = s.sample(BATCH, 1.0, cond, seed=SEED)
    for r0 in (1, rows - 1):
        assert torch.equal(s.sample(BATCH, 1.0, cond, seed=SEED, prefix=a[:, :r0]), a), r0
    other = s.sample(BATCH, 1.0, cond, seed=SEED + 1)
    assert torch.equal(s.sample(BATCH, 1.0, cond, seed=SEED, prefix=other), other)           # r0 = rows: the prefix itself
    assert torch.equal(s.sample(BATCH, 1.0, cond, seed=SEED, prefix=a[:, :0]), a)            # r0 = 0: the free run
    # a prefix that is not the free run's is kept and changes what follows
    mixed = s.sample(BATCH, 1.0, cond, seed=SEED, prefix=other[:, :1])
    assert torch.equal(mixed[:, :1], other[:, :1]) and mixed.shape == a.shape
    assert int(mixed.min()) >= 0 and int(mixed.max()) < N_CLASS
    # through sample_model, with fewer rows than the model has
    m = s.model
    got = amd.sample_model(m, "cuda", BATCH, [rows - 1, w], 1.0, condition=cond, prefix=other[:, :1], top_k=2)
    assert got.shape == (BATCH, rows - 1, w) and torch.equal(got[:, :1], other[:, :1])


# ----------------------------------------------------------------------------- 9. greedy, 10. top-k membership
@pytest.mark.parametrize("name", ["top", "bottom"])
def test_top_k_1_takes_the_row_maximum(samplers, name):
    s, cond, _, _ = samplers[name]
    codes = s.sample(BATCH, 0.7, cond, seed=SEED, top_k=1)
    logits = _step_logits(s, codes, cond)
    assert torch.equal(logits.gather(3, codes.unsqueeze(3)).squeeze(3), logits[..., :N_CLASS].amax(3))


@pytest.mark.parametrize("name", ["top", "bottom"])
def test_top_k_3_draws_among_the_three_largest(samplers, name):
    s, cond, _, _ = samplers[name]
    codes = s.sample(BATCH, 1.0, cond, seed=SEED, top_k=3)
    logits = _step_logits(s, codes, cond)[..., :N_CLASS]
    third = logits.sort(3, descending=True).values[..., 2]
    assert torch.all(logits.gather(3, codes.unsqueeze(3)).squeeze(3) >= third)               # ties at the third value closed
    # a nucleus so small that one class holds it is the greedy run
    assert torch.equal(s.sample(BATCH, 1.0, cond, seed=SEED, top_p=1e-6), s.sample(BATCH, 1.0, cond, seed=SEED, top_k=1))


# ----------------------------------------------------------------------------- 11. return_logp
@pytest.mark.parametrize("name", ["top", "bottom"])
def test_return_logp(samplers, name):
    s, cond, rows, w = samplers[name]
    temperature = 0.5                                        # a power of two: l / T is exact
    codes, logp = s.sample(BATCH, temperature, cond, seed=SEED, return_logp=True)
    assert logp.shape == (BATCH, rows, w) and logp.dtype == torch.float32 and logp.is_cuda
    z = _step_logits(s, codes, cond)[..., :N_CLASS].double() / temperature
    want = torch.log_softmax(z, 3).gather(3, codes.unsqueeze(3)).squeeze(3)
    rel = (z.gather(3, codes.unsqueeze(3)).squeeze(3) - z.amax(3))
    ratio = ((logp.double() - want).abs() / _logp_bound(rel)).max()
    print("%s: max |logp - float64| / bound = %.3f" % (name, float(ratio)))
    assert float(ratio) <= 1
    # prefix positions hold 0, drawn ones what the free run gave them
    c2, l2 = s.sample(BATCH, temperature, cond, seed=SEED, prefix=codes[:, :1], return_logp=True)
    assert torch.equal(c2, codes) and torch.all(l2[:, :1] == 0) and torch.equal(l2[:, 1:], logp[:, 1:])
    _, l3 = s.sample(BATCH, temperature, cond, seed=SEED, top_k=3, return_logp=True)
    assert torch.all(torch.isfinite(l3)) and torch.all(l3 <= 0)


# ----------------------------------------------------------------------------- 12. bad arguments
def test_bad_arguments(amd, samplers):
    s, _, rows, w = samplers["top"]
    for kw in (dict(top_k=-1), dict(top_k=1.5), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=float("nan"))):
        with pytest.raises(ValueError):
            s.sample(BATCH, 1.0, seed=SEED, **kw)
    good = torch.zeros((BATCH, 2, w), dtype=torch.int64, device="cuda")
    for bad in (good.cpu(), good.int(), good.float(), good[:1], good[:, :, :w - 1], good.view(BATCH, 2 * w),
                torch.zeros((BATCH, rows + 1, w), dtype=torch.int64, device="cuda")):
        with pytest.raises(RuntimeError):
            s.sample(BATCH, 1.0, seed=SEED, prefix=bad)
    with pytest.raises(ValueError):
        amd.sample_model(s.model, "cuda", BATCH, [rows, w], 1.0, top_p=2.0)
    assert s.sample(BATCH, 1.0, seed=SEED, prefix=good).shape == (BATCH, rows, w)


# ----------------------------------------------------------------------------- 13. the example
def _checkpoints(amd, tmp_path):
    ck = tmp_path / "checkpoint"
    ck.mkdir()
    torch.manual_seed(3)
    vq = dict(channel=16, n_res_block=1, n_res_channel=8, embed_dim=8, n_embed=6)
    torch.save(amd.VQVAE(**vq).state_dict(), str(ck / "vqvae.pt"))
    common = dict(lr=3e-4, n_res_block=1, n_res_channel=8, n_out_res_block=0, n_cond_res_block=1, dropout=0.1, size=[4, 4], n_class=6,
                  n_block=1, kernel_size=3)
    top = amd.PixelSNAIL([4, 4], 6, 64, 3, 1, 1, 8)
    torch.save({"model": top.state_dict(), "args": argparse.Namespace(hier="top", channel=64, **common)}, str(ck / "top.pt"))
    bottom = amd.PixelSNAIL([8, 8], 6, 8, 3, 1, 1, 8, attention=False, n_cond_res_block=1, cond_res_channel=8)
    torch.save({"model": bottom.state_dict(), "args": argparse.Namespace(hier="bottom", channel=8, **common)}, str(ck / "bottom.pt"))
    argv = ["--vqvae", "vqvae.pt", "--top", "top.pt", "--bottom", "bottom.pt", "--temp", "1.0", "--ckpt_dir", str(ck), "--seed", "1"] + \
           [a for k, v in vq.items() for a in ("--vqvae_arg", f"{k}={v}")]
    return ck, vq, argv


def test_example_with_truncation_writes_its_output(amd, tmp_path):
    _, _, argv = _checkpoints(amd, tmp_path)
    out = tmp_path / "sample.png"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "sample.py"), "--batch", "2", "--top_k", "4", "--top_p", "0.9"] + argv + [str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    hc, wc, _ = amd.grid_layout(2, 32, 32)
    if out.exists():
        from PIL import Image
        assert Image.open(str(out)).size == (wc, hc)
    else:
        assert np.load(str(tmp_path / "sample.npy")).shape == (hc, wc, 3)


def test_example_completes_encoded_images(amd, tmp_path):
    ck, vq, argv = _checkpoints(amd, tmp_path)
    spec = importlib.util.spec_from_file_location("example_sample", os.path.join(ROOT, "examples", "sample.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    images = torch.randint(0, 256, (3, 32, 32, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    path = tmp_path / "images.npy"
    np.save(str(path), images.numpy())
    args = ex.parse_args(["--from_images", str(path), "--keep_rows", "1", "--top_k", "4"] + argv + [str(tmp_path / "out.png")])
    vqvae = amd.load_model("vqvae", "vqvae.pt", "cuda", ckpt_dir=str(ck), **vq)
    top = amd.load_model("pixelsnail_top", "top.pt", "cuda", ckpt_dir=str(ck))
    bottom = amd.load_model("pixelsnail_bottom", "bottom.pt", "cuda", ckpt_dir=str(ck))
    torch.manual_seed(1)
    top_codes, bottom_codes = ex.draw_codes(args, vqvae, top, bottom, "cuda")
    assert top_codes.shape == (3, 4, 4) and bottom_codes.shape == (3, 8, 8)                  # the batch follows the file
    with torch.no_grad():
        _, _, _, id_t, id_b = vqvae.encode(amd.ImageNormalizer([0.5] * 3, [0.5] * 3).nchw(images.cuda()))
    assert torch.equal(top_codes[:, :1], id_t[:, :1]) and torch.equal(bottom_codes[:, :2], id_b[:, :2])
    for codes in (top_codes, bottom_codes):
        assert int(codes.min()) >= 0 and int(codes.max()) < 6
