"""CPU checks of the GatedResBlock yardstick (tests/_pixelsnail_ref.py) against the goldens captured from the
reference's GatedResBlock and CausalConv2d (scripts/make_golden_gated_resblock.py), and of the modules' host side."""
import json

import numpy as np
import pytest
import torch
from torch import nn

import _pixelsnail_ref as R


def cases(g):
    return json.loads(str(g["cases"]))


def load(g, ci, dtype):
    """(inputs, gout, sd) of case ci as leaf tensors of `dtype`."""
    t = f"c{ci}."
    ins = {k[len(t) + 3:]: torch.from_numpy(g[k]).to(dtype).requires_grad_(True)
           for k in g.files if k.startswith(t + "in.") and k != t + "in.gout"}
    sd = {k[len(t) + 3:]: torch.from_numpy(g[k]).to(dtype).requires_grad_(True) for k in g.files if k.startswith(t + "sd.")}
    return ins, torch.from_numpy(g[t + "in.gout"]).to(dtype), sd


def run_ref(g, ci, dtype):
    c = cases(g)[ci]
    ins, gout, sd = load(g, ci, dtype)
    if c["kind"] == "conv":
        out = R.wn_conv(ins["input"], sd, "conv.conv.", c["conv"])
    else:
        out = R.gated_resblock(ins["input"], sd, c["conv"], ins.get("aux"), ins.get("condition"))
    (out * gout).sum().backward()
    grads = {k: v.grad for k, v in ins.items()}
    grads.update({k: v.grad for k, v in sd.items()})
    return out.detach(), grads, sd


def wanted(g, ci, tag):
    t = f"c{ci}."
    want = {"out": g[t + f"out.{tag}"]}
    want.update({k[len(t) + 9:]: g[k] for k in g.files if k.startswith(t + f"grad.{tag}.")})
    return want


def test_reference_formula_reproduces_the_goldens(golden):
    g = golden("pixelsnail_gated_resblock")
    assert len(cases(g)) == 9
    for ci, c in enumerate(cases(g)):
        out64, g64, sd64 = run_ref(g, ci, torch.float64)
        want = wanted(g, ci, "f64")
        have = {"out": out64.numpy(), **{k: v.numpy() for k, v in g64.items()}}
        assert sorted(have) == sorted(want), ci
        for k in want:
            assert np.abs(have[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), (ci, k)
        # float32: the yardstick states the formula with torch's own operations in the order the layers are written, so its
        # float32 run stays within the float32-vs-float64 gap the golden itself records
        out32, g32, sd32 = run_ref(g, ci, torch.float32)
        have = {"out": out32.numpy(), **{k: v.numpy() for k, v in g32.items()}}
        want32 = wanted(g, ci, "f32")
        for k in want:
            gap = np.abs(want32[k].astype(np.float64) - want[k]).max()
            assert gap > 0, (ci, k)
            assert np.abs(have[k].astype(np.float64) - want[k]).max() <= gap, (ci, k, gap)
        if c["conv"] == "causal":        # the yardstick edits weight_v as the layer does
            after = [k for k in g.files if k.startswith(f"c{ci}.after.")]
            assert len(after) == (1 if c["kind"] == "conv" else 2)
            for k in after:
                assert np.array_equal(sd32[k[len(f"c{ci}.after."):]].detach().numpy(), g[k]), k


def build(amd, c):
    if c["kind"] == "conv":
        return amd.CausalConv2d(c["cin"], c["ch"], c["k"], padding=c["conv"])
    return amd.GatedResBlock(c["cin"], c["ch"], c["k"], conv=c["conv"], auxiliary_channel=c["aux"], condition_dim=c["cond"])


def test_state_dict_table_matches_the_golden(golden):
    import vqvae2_amd
    g = golden("pixelsnail_gated_resblock")
    for ci, c in enumerate(cases(g)):
        m = build(vqvae2_amd, c)
        sd = m.state_dict()
        names = [k[len(f"c{ci}.sd."):] for k in g.files if k.startswith(f"c{ci}.sd.")]
        assert sorted(sd.keys()) == sorted(names), ci
        for n in names:
            assert tuple(sd[n].shape) == g[f"c{ci}.sd.{n}"].shape, n
        m.load_state_dict({n: torch.from_numpy(g[f"c{ci}.sd.{n}"]) for n in names}, strict=True)
        back = m.state_dict()
        assert sorted(back.keys()) == sorted(names)
        for n in names:
            assert np.array_equal(back[n].numpy(), g[f"c{ci}.sd.{n}"])
    # weight_norm initialisation: g is the norm of v per output channel over in * kh * kw, so the weight starts as v
    f = vqvae2_amd.WNConv2d(6, 10, [3, 5], padding=[1, 2])
    assert sorted(f.state_dict()) == ["conv.bias", "conv.weight_g", "conv.weight_v"]
    assert f.conv.weight_g.shape == (10, 1, 1, 1) and f.conv.weight_v.shape == (10, 6, 3, 5)
    assert torch.allclose(f.conv.weight_g.flatten(), f.conv.weight_v.flatten(1).norm(2, dim=1))
    assert float(f.conv.bias.detach().abs().max()) <= 1 / (6 * 15) ** 0.5
    assert "conv.bias" not in vqvae2_amd.WNConv2d(6, 10, 1, bias=False).state_dict()


def test_refusals_without_gpu():
    import vqvae2_amd as A
    for bad in (lambda: A.CausalConv2d(8, 8, [3, 4], padding='causal'),          # even KW
                lambda: A.CausalConv2d(8, 8, 2, padding='down'),
                lambda: A.CausalConv2d(8, 8, 3, stride=2),
                lambda: A.WNConv2d(8, 8, 3, stride=2, padding=1),
                lambda: A.WNConv2d(8, 8, [5, 7], padding=[2, 3]),                # 35 taps
                lambda: A.CausalConv2d(8, 8, [5, 7], padding='downright'),
                lambda: A.WNConv2d(8, 8, 3, padding=0),                          # would shrink the image
                lambda: A.WNConv2d(8, 8, 4, padding=2),                          # would grow it
                lambda: A.WNConv2d(8, 8, 9, padding=4),
                lambda: A.WNConv2d(8, 8, 1, activation=nn.ReLU()),
                lambda: A.WNConv2d(8, 8, 1, activation=nn.ELU(alpha=0.5)),
                lambda: A.CausalConv2d(8, 8, 3, activation=nn.Tanh()),
                lambda: A.CausalConv2d(8, 8, 3, padding='up'),
                lambda: A.GatedResBlock(8, 8, 3, activation=nn.ReLU),
                lambda: A.GatedResBlock(8, 8, 4),                                # 'wnconv2d' with an even kernel
                lambda: A.GatedResBlock(8, 8, 3, conv='causal_upleft'),
                lambda: A.GatedResBlock(8, 8, 3, dropout=1.0)):
        with pytest.raises(NotImplementedError):
            bad()
    for ok in (None, nn.ELU, nn.ELU(), nn.ELU(inplace=True)):
        A.WNConv2d(8, 8, 3, padding=1, activation=ok)
    m = A.GatedResBlock(8, 12, 5, conv='causal')
    assert (m.conv1.conv.spec.pad_top, m.conv1.conv.spec.pad_left, m.conv1.causal) == (4, 2, 2)
    assert (A.CausalConv2d(4, 4, [3, 2]).conv.spec.pad_top, A.CausalConv2d(4, 4, [3, 2]).conv.spec.pad_left) == (2, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 8, 3, 3))


def test_new_descriptor_refusals_reach_no_kernel():
    """Everything outside the contract of the same_size form of vq2_conv_desc is refused by every entry point before any
    device work."""
    import ctypes
    import vqvae2_amd as A
    L = A._lib
    def geom(**kw):
        d = L.ConvDesc()
        d.N, d.H, d.W, d.Ci, d.Co, d.KH, d.KW, d.pad_top, d.pad_left, d.ldx, d.ldy = 1, 4, 4, 8, 8, 3, 3, 1, 1, 8, 8
        d.stride, d.same_size = 1, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def every(d):
        """(every pointer is null: a call that got past the descriptor checks would still stop at its null check)"""
        job, pj = L.WgradJob(), L.PackJob()
        return [L.lib.vq2_conv_fwd(ctypes.byref(d), 0, None, None, None, None, 0, None, None),
                L.lib.vq2_conv_dgrad(ctypes.byref(d), 0, None, None, None, 0, None, 0, None, 8, None),
                L.lib.vq2_conv_wgrad(ctypes.byref(d), 0, None, None, None, None, None, 1 << 30, None),
                L.lib.vq2_conv_wgrad_partial(ctypes.byref(d), 0, None, None, None, None, 1 << 30, None),
                L.lib.vq2_wgrad_job_init(ctypes.byref(d), None, None, None, ctypes.byref(job)),
                L.lib.vq2_pack_weight(ctypes.byref(d), 0, None, None, None),
                L.lib.vq2_pack_job_init(ctypes.byref(d), 0, None, None, ctypes.byref(pj))]

    # (same_size is 0 or 1; a stride or a transposition cannot go with it)
    for bad, code, word in ((geom(KH=5, KW=7, pad_top=4, pad_left=3), 2, b"32 taps"), (geom(KH=8, pad_top=1), 1, b"1..7"),
                            (geom(KW=0), 1, b"1..7"), (geom(pad_top=3), 1, b"pad_top"), (geom(pad_left=-1), 1, b"pad_top"),
                            (geom(same_size=2), 1, b"same_size"), (geom(stride=2), 1, b"same_size"),
                            (geom(transposed=1), 1, b"same_size")):
        for rc in every(bad):
            assert rc == code, (rc, code, L.lib.vq2_last_error())
            assert word in L.lib.vq2_last_error()
        assert L.lib.vq2_conv_wgrad_workspace_bytes(ctypes.byref(bad)) == 0
    assert L.lib.vq2_conv_fwd(ctypes.byref(geom(Ci=6)), 0, None, None, None, None, 0, None, None) == 1
    assert b"multiples of 4" in L.lib.vq2_last_error()
    assert L.lib.vq2_conv_fwd(None, 0, None, None, None, None, 0, None, None) == 1
    ok = geom(KH=2, KW=5, pad_top=1, pad_left=2)
    assert L.lib.vq2_conv_fwd(ctypes.byref(ok), 0, None, None, None, None, 0, None, None) == 1
    assert b"null pointer" in L.lib.vq2_last_error()           # the descriptor itself is accepted
    assert L.lib.vq2_conv_wgrad_workspace_bytes(ctypes.byref(ok)) > 0
    job = L.WgradJob()
    host = (ctypes.c_float * 4)()                              # job_init only records the addresses
    assert L.lib.vq2_wgrad_job_init(ctypes.byref(ok), host, host, None, ctypes.byref(job)) == 0
    assert job.taps == 10 and (job.swapped & 1) == 0
    assert L.lib.vq2_conv_fwd(ctypes.byref(geom(N=1 << 20, H=64, W=64)), 0, None, None, None, None, 0, None, None) == 1
    assert b"exceeds 2^31 elements" in L.lib.vq2_last_error()
    # the elementwise entry points refuse bad strides and probabilities
    assert L.lib.vq2_elu_fwd(None, 4, None, 8, 4, 5, None) == 1 and b"pixel stride" in L.lib.vq2_last_error()
    assert L.lib.vq2_glu_res_fwd(None, 8, None, 8, None, 8, 4, 5, None) == 1 and b"pixel stride" in L.lib.vq2_last_error()
    assert L.lib.vq2_elu_dropout_fwd(None, 8, None, 8, 4, 5, 1.0, 0, None) == 1 and b"[0, 1)" in L.lib.vq2_last_error()
    assert L.lib.vq2_elu_bwd(None, 8, None, 8, None, 8, 4, 5, None) == 1 and b"null pointer" in L.lib.vq2_last_error()
