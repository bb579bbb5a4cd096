"""CPU checks of the stage-2 trainer's host side: the weight-norm table builder on a model that never saw a device, the new
entry points, and the example's command line."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _table(amd, model):
    from vqvae2_amd.optim import ParamArena
    live = list(model.parameters())
    early = [p for m in amd.Stage2Trainer._early_modules(model) for p in m.parameters()]
    order, offset, total = ParamArena.layout(live, early)
    entries, skipped = amd.ops.WeightNormPlan.entries(model, offset)
    return order, offset, total, entries, skipped


@pytest.mark.parametrize("kernel,kw", [(3, dict(attention=False, n_cond_res_block=1, cond_res_channel=8)), (5, dict())])
def test_table_builder_on_a_cpu_model(amd, kernel, kw):
    channel = 8 if "n_cond_res_block" in kw else 64
    model = amd.PixelSNAIL([4, 6], 6, channel, kernel, 2, 1, 8, **kw)
    order, offset, total, entries, skipped = _table(amd, model)
    names = dict(model.named_parameters())
    assert not skipped and len(entries) == sum(1 for k in names if k.endswith("weight_g"))     # one entry per weight_g
    assert sorted(e["name"] + ".weight_g" for e in entries) == sorted(k for k in names if k.endswith("weight_g"))
    # the arena: the early modules (later half of the blocks, the head) at the end, every slot on a 16-byte boundary
    assert len(order) == len(names) and total % 4 == 0
    first_early = min(offset[id(p)] for p in list(model.blocks[1].parameters()) + list(model.out.parameters()))
    assert all((offset[id(p)] >= first_early) == (k.startswith("blocks.1.") or k.startswith("out.")) for k, p in names.items())
    spans = sorted((offset[id(p)], offset[id(p)] + p.numel()) for p in names.values())
    assert all(lo % 4 == 0 for lo, _ in spans) and spans[-1][1] <= total
    assert all(a[1] <= b[0] for a, b in zip(spans[:-1], spans[1:]))
    # the entries: in arena order, offsets those of the parameters, weight slots aligned and disjoint, rows prefix-summed
    assert [e["v_off"] for e in entries] == sorted(e["v_off"] for e in entries)
    rows = 0
    w_spans = []
    for e in entries:
        v, g = names[e["name"] + ".weight_v"], names[e["name"] + ".weight_g"]
        assert (e["v_off"], e["g_off"]) == (offset[id(v)], offset[id(g)])
        assert e["rows"] == v.shape[0] == g.numel() and e["rows"] * e["cols"] == v.numel()
        assert (e["kh"], e["kw"]) == (tuple(v.shape[2:]) if v.dim() == 4 else (1, 1))
        assert e["row_start"] == rows and e["w_off"] % 4 == 0 and e["v_off"] % 4 == 0 and e["g_off"] % 4 == 0
        rows += e["rows"]
        w_spans.append((e["w_off"], e["w_off"] + v.numel()))
    w_spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(w_spans[:-1], w_spans[1:]))
    # mask_from: kernel // 2 for the 'causal' convs of the gated blocks, no mask (== kw) anywhere else
    by_name = {e["name"]: e for e in entries}
    for name, e in by_name.items():
        causal = ".resblocks." in name and (name.endswith("conv1.conv.conv") or name.endswith("conv2.conv.conv"))
        assert e["mask_from"] == (kernel // 2 if causal else e["kw"]), name
    down, downright = by_name["horizontal.conv.conv"], by_name["vertical.conv.conv"]
    assert (down["kh"], down["kw"], down["mask_from"]) == (kernel // 2, kernel, kernel)                      # 'down'
    assert (downright["kh"], downright["kw"], downright["mask_from"]) == ((kernel + 1) // 2, kernel // 2, kernel // 2)   # 'downright'
    one = by_name["out.1.conv"]
    assert (one["kh"], one["kw"], one["mask_from"]) == (1, 1, 1)                                              # 1x1
    assert sum(1 for e in entries if e["mask_from"] < e["kw"]) == 4            # two blocks x one gated block x two convs
    if "n_cond_res_block" not in kw:
        lin = by_name["blocks.0.causal_attention.query"]                          # weight_norm(nn.Linear): a 1x1 entry
        assert (lin["kh"], lin["kw"], lin["mask_from"], lin["cols"]) == (1, 1, 1, channel + 2)


def test_a_layer_outside_the_arena_stays_per_layer(amd):
    model = amd.PixelSNAIL([4, 6], 6, 8, 3, 1, 1, 8, attention=False)
    frozen = model.out[1].conv
    frozen.weight_v.requires_grad_(False)
    frozen.weight_g.requires_grad_(False)
    from vqvae2_amd.optim import ParamArena
    _, offset, _ = ParamArena.layout([p for p in model.parameters() if p.requires_grad])
    entries, skipped = amd.ops.WeightNormPlan.entries(model, offset)
    assert skipped == ["out.1.conv"] and "out.1.conv" not in [e["name"] for e in entries]


def test_new_entry_points_are_bound(amd):
    import ctypes
    assert amd._lib.API_VERSION >= 12
    for name in ("vq2_wn_table_fwd", "vq2_wn_table_bwd"):
        assert name in amd._lib.EXPORTS, name
    assert ctypes.sizeof(amd._lib.WnEntry) == 48          # three int64 offsets, six int32: include/vq2.h vq2_wn_entry
    assert callable(amd.ops.WeightNormPlan) and callable(amd.ops.planned_weight)
    import inspect
    sig = inspect.signature(amd.Stage2Trainer.__init__)
    assert sig.parameters["arena"].default is True
    assert all(hasattr(amd.Stage2Trainer, n) for n in ("state_dict", "load_state_dict"))
    # host-side argument checks of the new entry points (no launch: they fail before it)
    lib = amd._lib.lib
    dummy = ctypes.c_void_p(16)
    assert lib.vq2_wn_table_fwd(dummy, 0, dummy, dummy, None) != 0 and b"at least one entry" in lib.vq2_last_error()
    assert lib.vq2_wn_table_bwd(dummy, 3, 2, dummy, dummy, dummy, None) != 0 and b"not a range" in lib.vq2_last_error()
    assert lib.vq2_wn_table_bwd(None, 0, 0, dummy, dummy, dummy, None) != 0


def _example():
    spec = importlib.util.spec_from_file_location("train_pixelsnail_example", os.path.join(ROOT, "examples", "train_pixelsnail.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_parses_resume_and_seed_and_the_reference_command_line():
    ex = _example()
    a = ex.parse_args(["--hier", "bottom", "--resume", "checkpoint/trainer_bottom_011.pt", "--seed", "7", "codes.db"])
    assert (a.hier, a.resume, a.seed, a.path) == ("bottom", "checkpoint/trainer_bottom_011.pt", 7, "codes.db")
    d = ex.parse_args(["--hier", "top", "--batch", "16", "--epoch", "3", "--lr", "1e-4", "--channel", "128", "--n_res_block", "2",
                       "--n_res_channel", "64", "--n_out_res_block", "1", "--n_cond_res_block", "2", "--dropout", "0.2",
                       "--amp", "O0", "--sched", "cycle", "--ckpt", "x.pt", "codes.db"])
    assert (d.resume, d.seed) == (None, None)
    assert (d.hier, d.batch, d.epoch, d.lr, d.channel, d.n_res_block, d.n_res_channel) == ("top", 16, 3, 1e-4, 128, 2, 64)
    assert (d.n_out_res_block, d.n_cond_res_block, d.dropout, d.amp, d.sched, d.ckpt, d.path) == (1, 2, 0.2, "O0", "cycle", "x.pt", "codes.db")
    with pytest.raises(SystemExit):
        ex.parse_args(["--seed", "x", "codes.db"])
