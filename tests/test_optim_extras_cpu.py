"""Host side of global-norm clipping, skipped steps and averaged weights: the exports, the defaults of the new arguments,
the pinned signatures, the example parsers, and every argument the two entry points refuse before a launch (no GPU)."""
import ctypes
import importlib.util
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VQ2_ERR_INVALID = 1


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def test_entry_points_are_bound(amd):
    for name in ("vq2_grad_norm_workspace_bytes", "vq2_grad_norm", "vq2_adam_step_ex"):
        assert hasattr(amd._lib.lib, name) and name in amd._lib.EXPORTS, name
    assert amd._lib.API_VERSION >= 16
    lib = amd._lib.lib
    assert lib.vq2_grad_norm_workspace_bytes(0) == 0 and lib.vq2_grad_norm_workspace_bytes(-4) == 0
    # a block count that depends on n alone, capped: one size serves every n
    assert lib.vq2_grad_norm_workspace_bytes(4) == lib.vq2_grad_norm_workspace_bytes(1 << 30) > 0
    assert lib.vq2_grad_norm_workspace_bytes(4) % 16 == 0


def test_new_arguments_default_to_none_and_come_last(amd):
    from vqvae2_amd.optim import FusedAdam
    for cls in (amd.Stage2Trainer, amd.Stage1Trainer, FusedAdam):
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[-2:] == ["clip_grad_norm", "ema_decay"], cls
        assert params["clip_grad_norm"].default is None and params["ema_decay"].default is None
    assert list(inspect.signature(amd.Stage2Trainer.__init__).parameters)[:7] == ["self", "model", "hier", "lr", "sched", "n_iter", "arena"]
    assert list(inspect.signature(amd.Stage1Trainer.__init__).parameters)[:8] == ["self", "model", "lr", "sched", "n_iter", "betas", "eps",
                                                                                  "normalizer"]
    for cls in (amd.Stage2Trainer, amd.Stage1Trainer):
        for name in ("skipped_steps", "averaged_state_dict", "averaged_weights"):
            assert callable(getattr(cls, name)), (cls, name)


def test_pinned_evaluate_signatures_are_unchanged(amd):
    assert list(inspect.signature(amd.Stage2Trainer.evaluate).parameters) == ["self", "batches", "top_k"]
    assert inspect.signature(amd.Stage2Trainer.evaluate).parameters["top_k"].default == 5
    assert list(inspect.signature(amd.Stage1Trainer.evaluate).parameters) == ["self", "batches", "sample"]
    assert list(inspect.signature(amd.Stage1Trainer.evaluate_image_metrics).parameters) == ["self", "batches", "sample"]


def _example(name):
    spec = importlib.util.spec_from_file_location(name + "_example", os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_parsers_accept_the_new_flags():
    ex = _example("train_pixelsnail")
    a = ex.parse_args(["--hier", "top", "--clip_grad_norm", "1.5", "--ema_decay", "0.9999", "codes.db"])
    assert (a.clip_grad_norm, a.ema_decay, a.path) == (1.5, 0.9999, "codes.db")
    d = ex.parse_args(["--hier", "top", "--batch", "16", "--epoch", "3", "--lr", "1e-4", "--channel", "128", "--n_res_block", "2",
                       "--n_res_channel", "64", "--n_out_res_block", "1", "--n_cond_res_block", "2", "--dropout", "0.2",
                       "--amp", "O0", "--sched", "cycle", "--ckpt", "x.pt", "codes.db"])       # the reference's command line
    assert (d.clip_grad_norm, d.ema_decay) == (None, None) and (d.batch, d.sched, d.path) == (16, "cycle", "codes.db")
    s1 = _example("train_stage1")
    a = s1.parse_args(["--clip_grad_norm", "2", "--ema_decay", "0.999", "--size", "64"])
    assert (a.clip_grad_norm, a.ema_decay, a.size) == (2.0, 0.999, 64)
    d = s1.parse_args(["--n_gpu", "1", "--dist_url", "env://", "--size", "256", "--epoch", "560", "--lr", "3e-4", "--sched", "cycle",
                       "--batch_size", "4", "--path", "data"])
    assert (d.clip_grad_norm, d.ema_decay) == (None, None) and (d.size, d.epoch, d.sched, d.path) == (256, 560, "cycle", "data")


def _refused(lib, name, *args):
    rc = getattr(lib, name)(*args, None)
    msg = lib.vq2_last_error()
    assert rc == VQ2_ERR_INVALID and msg, (name, args, rc, msg)
    return msg


def test_grad_norm_refuses_bad_arguments_before_any_launch(amd):
    """No device exists here: a call that reached a launch would fail differently (and not with VQ2_ERR_INVALID)."""
    lib = amd._lib.lib
    ok, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    ws = lib.vq2_grad_norm_workspace_bytes(64)
    good = dict(g=ok, n=64, gs=1.0, mx=1.0, ctl=ok, ws=ok, wsb=ws)

    def call(**kw):
        a = dict(good, **kw)
        return _refused(lib, "vq2_grad_norm", a["g"], a["n"], a["gs"], a["mx"], a["ctl"], a["ws"], a["wsb"])

    for n in (0, -4, 6, 63):
        assert b"multiple of 4" in call(n=n)
    for k in ("g", "ctl", "ws"):
        assert b"null" in call(**{k: None})
        assert b"aligned" in call(**{k: odd})
    for mx in (0.0, -1.0, float("nan"), float("-inf")):
        assert b"max_norm" in call(mx=mx)
    assert b"workspace" in call(wsb=ws - 1)


def test_adam_step_ex_refuses_bad_arguments_before_any_launch(amd):
    lib = amd._lib.lib
    ok, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    good = dict(p=ok, g=ok, m=ok, v=ok, avg=ok, n=64, step=1, ctl=ok, decay=0.5)

    def call(**kw):
        a = dict(good, **kw)
        return _refused(lib, "vq2_adam_step_ex", a["p"], a["g"], a["m"], a["v"], a["avg"], a["n"], 3e-4, 0.9, 0.999, 1e-8,
                        a["step"], 1.0, a["ctl"], a["decay"])

    for k in "pgmv":
        assert call(**{k: None})
        assert b"aligned" in call(**{k: odd})
    assert b"aligned" in call(avg=odd)
    assert call(step=0)
    for n in (0, -4, 6, 63):
        assert b"multiple of 4" in call(n=n)
    for decay in (-0.1, 1.0, 1.5, float("nan")):
        assert b"avg_decay" in call(decay=decay)


def test_fused_adam_needs_an_arena_for_either_feature():
    from vqvae2_amd.optim import FusedAdam
    w = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="arena"):
        FusedAdam([w], clip_grad_norm=1.0)
    with pytest.raises(ValueError, match="arena"):
        FusedAdam([w], ema_decay=0.999)
    opt = FusedAdam([w])
    assert not hasattr(opt, "ctl") and opt.clip_grad_norm is None and opt.ema_decay is None
