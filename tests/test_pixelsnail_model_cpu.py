"""CPU checks of the assembled stage-2 prior: the plain-torch yardstick (tests/_pixelsnail_model_ref.py) reproduces the goldens
captured from the reference, the modules refuse what they do not build, their state_dict is the reference's, and the example
keeps the reference's command line."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _pixelsnail_model_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


@pytest.fixture(scope="module")
def g():
    return M.load()


def _keys(g, ci):
    c = M.cases(g)[ci]
    return (["logits", "loss"] if c["kind"] == "model" else ["out", "loss"]) + ["grad." + n for n in M.grad_names(g, ci)]


def _scale(g, ci, k, want):
    if k.endswith("causal_attention.key.bias"):
        # a constant added to every key moves each row of scores as a whole, which the softmax ignores: this gradient is
        # exactly 0 and the golden holds the rounding of its summands; the key weights' gradient sums the same terms
        return float(np.abs(g[f"c{ci}.{k[:-4]}weight_v.f64"]).max())
    return float(np.abs(want).max())


@pytest.mark.parametrize("ci", range(5))
def test_yardstick_reproduces_the_goldens(g, ci):
    assert len(M.cases(g)) == 5
    c = M.cases(g)[ci]
    r64 = M.run_case(g, ci, torch.float64)
    r32 = M.run_case(g, ci, torch.float32)
    keys = _keys(g, ci)
    assert sorted(k for k in r64 if k != "accuracy") == sorted(keys)       # every parameter's gradient is stored
    for k in keys:
        want, ref32 = M.golden_pair(g, f"c{ci}.{k}")
        have = r64[k].detach().numpy()
        assert np.abs(have - want).max() <= 1e-12 * _scale(g, ci, k, want), (ci, k)
        # float32: within the gap the golden itself records (no allowance, as in test_attention_cpu.py).  The float16
        # storage of a gradient's float32 run moves the recorded gap by at most 2^-11 of itself
        gap = np.abs(ref32 - want).max()
        assert gap > 0
        err32 = np.abs(r32[k].detach().numpy().astype(np.float64) - want).max()
        assert err32 <= gap * (1 + 2.0 ** -10), (ci, k, err32, gap)
    if c["kind"] == "model":
        assert float(r64["accuracy"]) == float(r32["accuracy"]) == float(g[f"c{ci}.accuracy"])


def _build(amd, c):
    if c["kind"] == "block":
        return amd.PixelBlock(c["cin"], c["ch"], c["k"], c["n_res_block"], attention=c["attention"], condition_dim=c["cond"])
    return amd.PixelSNAIL(c["shape"], c["n_class"], *c["args"], **c["kw"])


@pytest.mark.parametrize("ci", range(5))
def test_state_dict_keys_and_shapes(amd, g, ci):
    m = _build(amd, M.cases(g)[ci])
    want = M.state_dict(g, ci)
    have = m.state_dict()
    assert sorted(have) == sorted(want)
    assert all(tuple(have[k].shape) == tuple(want[k].shape) for k in want)
    m.load_state_dict(want, strict=True)
    if "background" in want:
        assert torch.equal(m.background, want["background"])


def test_constructor_refusals(amd):
    ok = dict(shape=[4, 4], n_class=8, channel=64, kernel_size=3, n_block=1, n_res_block=1, res_channel=8)
    amd.PixelSNAIL(**ok)
    for bad in (dict(channel=6, attention=False), dict(channel=66), dict(channel=24), dict(kernel_size=4),
                dict(cond_res_kernel=2, n_cond_res_block=1, cond_res_channel=8), dict(n_class=0), dict(n_class=16385)):
        with pytest.raises(NotImplementedError):
            amd.PixelSNAIL(**{**ok, **bad})
    amd.PixelSNAIL(**{**ok, "channel": 24, "attention": False})          # without attention 24 channels are fine
    with pytest.raises(NotImplementedError):
        amd.PixelBlock(6, 8, 3, 1, attention=False)
    with pytest.raises(NotImplementedError):
        amd.PixelBlock(8, 8, 4, 1, attention=False)
    with pytest.raises(NotImplementedError):
        amd.CondResNet(8, 8, 2, 1)


def test_new_entry_points_are_bound(amd):
    for name in ("vq2_onehot_pack_weight", "vq2_onehot_conv_fwd", "vq2_onehot_conv_wgrad", "vq2_onehot_conv_wgrad_workspace_bytes",
                 "vq2_xent_fwd", "vq2_xent_bwd", "vq2_upsample2_fwd", "vq2_upsample2_bwd"):
        assert name in amd._lib.EXPORTS, name
    assert amd._lib.API_VERSION >= 10
    assert callable(amd.prior_loss) and amd.Stage2Trainer is not None


def _example():
    spec = importlib.util.spec_from_file_location("train_pixelsnail_example", os.path.join(ROOT, "examples", "train_pixelsnail.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_accepts_the_reference_command_lines():
    ex = _example()
    a = ex.parse_args(["--hier", "top", "--batch", "16", "--epoch", "3", "--lr", "1e-4", "--channel", "128", "--n_res_block", "2",
                       "--n_res_channel", "64", "--n_out_res_block", "1", "--n_cond_res_block", "2", "--dropout", "0.2",
                       "--amp", "O0", "--sched", "cycle", "--ckpt", "x.pt", "codes.db"])
    assert (a.hier, a.batch, a.epoch, a.lr, a.channel, a.n_res_block, a.n_res_channel) == ("top", 16, 3, 1e-4, 128, 2, 64)
    assert (a.n_out_res_block, a.n_cond_res_block, a.dropout, a.amp, a.sched, a.ckpt, a.path) == (1, 2, 0.2, "O0", "cycle", "x.pt", "codes.db")
    d = ex.parse_args(["codes.db"])        # the reference's defaults
    assert (d.batch, d.epoch, d.hier, d.lr, d.channel, d.n_res_block, d.n_res_channel) == (32, 420, "top", 3e-4, 256, 4, 256)
    assert (d.n_out_res_block, d.n_cond_res_block, d.dropout, d.amp, d.sched, d.ckpt) == (0, 3, 0.1, "O0", None, None)
    assert ex.parse_args(["--hier", "bottom", "codes.db"]).hier == "bottom"
    with pytest.raises(SystemExit):
        ex.parse_args(["--amp", "O1", "codes.db"])
