"""GPU checks of the assembled stage-2 prior (PixelBlock, CondResNet, PixelSNAIL, prior_loss, the train example) against the
goldens captured from the reference: 4 x the golden's own float32-vs-float64 gap per tensor, ratios printed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _pixelsnail_model_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


@pytest.fixture(scope="module")
def g():
    return M.load()


def _build(amd, c):
    if c["kind"] == "block":
        return amd.PixelBlock(c["cin"], c["ch"], c["k"], c["n_res_block"], attention=c["attention"], condition_dim=c["cond"])
    return amd.PixelSNAIL(c["shape"], c["n_class"], *c["args"], **c["kw"])


def _model(amd, g, ci):
    c = M.cases(g)[ci]
    m = _build(amd, c)
    want = M.state_dict(g, ci)
    m.load_state_dict(want, strict=True)                              # the reference's state_dict loads into ours ...
    assert sorted(m.state_dict()) == sorted(want)                     # ... and ours has exactly its keys
    return c, m.cuda().eval()


def _inputs(g, ci):
    t = f"c{ci}.in."
    return {k[len(t):]: torch.from_numpy(g[k]).cuda() for k in g.files if k.startswith(t)}


@pytest.mark.parametrize("ci", range(5))
def test_models_against_the_goldens(amd, g, ci):
    c, m = _model(amd, g, ci)
    ins = _inputs(g, ci)
    have = {}
    if c["kind"] == "model":
        out, cache = m(ins["input"], condition=ins.get("condition"))
        assert out.shape == (c["n"], c["n_class"], *ins["input"].shape[1:])
        loss, acc = amd.prior_loss(out, ins["input"])
        assert loss.dim() == 0 and acc.dim() == 0
        assert float(acc) == float(g[f"c{ci}.accuracy"])
        have["logits"] = out
    else:
        out = m(ins["input"], ins["background"], condition=ins.get("condition"))
        loss = (out * ins["gout"]).sum()          # (this sum is torch's, formed here to seed the backward: not a library result)
        have["out"] = out
    loss.backward()
    torch.cuda.synchronize()
    if c["kind"] == "model":
        have["loss"] = loss
    have.update({"grad." + k: p.grad for k, p in m.named_parameters()})
    assert sorted(k for k in have if k.startswith("grad.")) == ["grad." + n for n in M.grad_names(g, ci)]
    bad = []
    for k, v in have.items():
        f64, f32 = M.golden_pair(g, f"c{ci}.{k}")
        gap = float(np.abs(f32 - f64).max())
        err = float(np.abs(v.detach().double().cpu().numpy() - f64).max())
        print("case %d %s: err %.3e, golden gap %.3e, ratio %.2f" % (ci, k, err, gap, err / gap))
        if not (gap > 0 and err <= 4 * gap):
            bad.append((k, err, gap))
    assert not bad, bad


def _logits(m, codes, cond=None, cache=None):
    with torch.no_grad():
        out, cache = m(codes, condition=cond, cache=cache)
    return out.clone(), cache


@pytest.mark.parametrize("ci", [0, 1], ids=["attention", "conditioned"])
def test_causality(amd, g, ci):
    c, m = _model(amd, g, ci)
    ins = _inputs(g, ci)
    codes, cond = ins["input"], ins.get("condition")
    _, h, w = codes.shape
    y0, _ = _logits(m, codes, cond)
    raster = torch.arange(h * w, device="cuda").view(h, w)
    for p in ((h // 2) * w + w // 2, 1 * w + 0, h * w - 2):           # a middle, a first-column and the last position with a successor
        changed = codes.clone()
        changed[:, p // w, p % w] = (changed[:, p // w, p % w] + 1) % c["n_class"]
        y1, _ = _logits(m, changed, cond)
        upto = raster <= p
        assert torch.equal(y0[:, :, upto], y1[:, :, upto]), p
        assert not torch.equal(y0[:, :, ~upto], y1[:, :, ~upto]), p
    last = codes.clone()
    last[:, -1, -1] = (last[:, -1, -1] + 1) % c["n_class"]            # the last position is seen by nothing
    assert torch.equal(y0, _logits(m, last, cond)[0])


def test_cache_skips_the_condition_network(amd, g):
    c, m = _model(amd, g, 1)
    ins = _inputs(g, 1)
    calls = []
    m.cond_resnet.register_forward_hook(lambda *a: calls.append(1))
    y0, cache = _logits(m, ins["input"], ins["condition"])
    assert len(calls) == 1 and not cache["condition"].requires_grad
    assert cache["condition"].shape == (c["n"], 12, 4, 6)
    y1, cache2 = _logits(m, ins["input"], ins["condition"], cache)
    assert len(calls) == 1 and cache2 is cache
    assert torch.equal(y0, y1)
    y2, _ = _logits(m, ins["input"][:, :3], ins["condition"], cache)   # fewer rows: the first rows of the cached condition
    assert len(calls) == 1 and torch.equal(y2, y0[:, :, :3])


def _train_step(amd, g, ci, seed):
    c, m = _model(amd, g, ci)
    m.train()
    ins = _inputs(g, ci)
    torch.manual_seed(seed)
    tr = amd.Stage2Trainer(m, "bottom" if "condition" in ins else "top", lr=1e-3)
    r = tr.step(ins["condition"], ins["input"]) if "condition" in ins else tr.step(ins["input"])
    torch.cuda.synchronize()
    return r["loss"].clone(), {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("ci", [0, 1])
def test_train_step_is_repeatable(amd, g, ci):
    l1, s1 = _train_step(amd, g, ci, 5)
    l2, s2 = _train_step(amd, g, ci, 5)
    l3, s3 = _train_step(amd, g, ci, 6)
    assert torch.equal(l1, l2) and all(torch.equal(s1[k], s2[k]) for k in s1)
    assert not torch.equal(l1, l3)
    before = M.state_dict(g, ci)
    assert any(not torch.equal(s1[k].cpu(), before[k]) for k in s1 if k != "background")


@pytest.mark.parametrize("hier", ["top", "bottom"])
def test_train_example_runs(amd, tmp_path, hier):
    from vqvae2_amd import codes
    path = str(tmp_path / "codes.db")
    gen = torch.Generator().manual_seed(1)
    with codes.CodeStore(path, "w", backend="sqlite") as store:
        n = codes.write_code_rows(store, torch.randint(0, 6, (4, 4, 4), generator=gen),
                                  torch.randint(0, 6, (4, 8, 8), generator=gen), [f"{i}.png" for i in range(4)])
        store.put(b"length", str(n).encode())
    channel = "64" if hier == "top" else "8"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_pixelsnail.py"), "--hier", hier, "--batch", "2", "--epoch", "10",
           "--channel", channel, "--n_res_block", "1", "--n_res_channel", "8", "--n_cond_res_block", "1", "--sched", "cycle",
           "--size", "4", "4", "--n_class", "6", "--n_block", "1", "--kernel_size", "3", "--max_steps", "2", "--workers", "0",
           "--ckpt_dir", str(tmp_path / "checkpoint"), path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("epoch:")]
    assert len(lines) == 2
    for ln in lines:
        loss = float(ln.split("loss:")[1].split(";")[0])
        assert np.isfinite(loss) and loss > 0
    ck = torch.load(str(tmp_path / "checkpoint" / f"pixelsnail_{hier}_001.pt"), weights_only=False)
    assert ck["args"].hier == hier
    shape = [4, 4] if hier == "top" else [8, 8]
    kw = {} if hier == "top" else dict(attention=False, n_cond_res_block=1, cond_res_channel=8)
    fresh = amd.PixelSNAIL(shape, 6, int(channel), 3, 1, 1, 8, **kw)
    fresh.load_state_dict(ck["model"], strict=True)
