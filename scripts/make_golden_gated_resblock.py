"""Capture tests/golden/pixelsnail_gated_resblock.npz from the reference's GatedResBlock and CausalConv2d
(pixelsnail.py:71-179).

Needs the reference checkout (VQ2_REFERENCE, read-only) at capture time only: per case the file holds the inputs, the
state_dict, the eval-mode output and the gradients of sum(out * gout) with respect to every input and parameter, each
from a float32 and from a float64 run of the reference, and for 'causal' layers weight_v as the forward leaves it.
Nothing of the reference itself is stored."""
import json
import os
import sys
import warnings

import numpy as np
import torch

REF = os.environ.get("VQ2_REFERENCE")
if not REF:
    raise SystemExit("set VQ2_REFERENCE to a checkout of the reference (read at capture time only)")
sys.path.insert(0, REF)
warnings.simplefilter("ignore", FutureWarning)
import pixelsnail as ref  # noqa: E402  (the reference module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kind "block": GatedResBlock(in, ch, k, conv, auxiliary_channel=aux, condition_dim=cond) on [n, in, h, w];
# kind "conv":  CausalConv2d(in, ch, k, padding=conv) on [n, in, h, w].
# A 5x5 causal block; an image smaller than the receptive field; the plain weight-normed block; the two rectangular
# causal kernels; half widths with C % 4 = 2 (with an auxiliary input) and 1; a conditioned block; and the key block's
# real width (514) with a narrow middle so that the weights stay small.
CASES = [
    dict(kind="block", cin=8, ch=12, k=5, conv="causal", aux=0, cond=0, n=2, h=6, w=7),
    dict(kind="block", cin=6, ch=10, k=3, conv="causal", aux=0, cond=0, n=2, h=3, w=2),
    dict(kind="block", cin=8, ch=8, k=3, conv="wnconv2d", aux=0, cond=0, n=1, h=4, w=3),
    dict(kind="conv", cin=8, ch=12, k=[2, 5], conv="down", aux=0, cond=0, n=1, h=4, w=6),
    dict(kind="conv", cin=8, ch=12, k=[3, 2], conv="downright", aux=0, cond=0, n=1, h=4, w=5),
    dict(kind="block", cin=6, ch=4, k=1, conv="wnconv2d", aux=4, cond=0, n=1, h=3, w=3),
    dict(kind="block", cin=5, ch=8, k=1, conv="wnconv2d", aux=0, cond=0, n=1, h=3, w=3),
    dict(kind="block", cin=8, ch=8, k=3, conv="causal", aux=0, cond=12, n=1, h=4, w=4),
    dict(kind="block", cin=514, ch=8, k=1, conv="wnconv2d", aux=0, cond=0, n=1, h=2, w=3),
]


def build(c):
    if c["kind"] == "conv":
        return ref.CausalConv2d(c["cin"], c["ch"], c["k"], padding=c["conv"]).eval()
    return ref.GatedResBlock(c["cin"], c["ch"], c["k"], conv=c["conv"], auxiliary_channel=c["aux"],
                             condition_dim=c["cond"]).eval()


def run(mod, ins, gout, dtype):
    mod = mod.to(dtype)
    xs = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in ins.items()}
    out = mod(xs["input"], *([xs["aux"]] if "aux" in xs else []), **({"condition": xs["condition"]} if "condition" in xs else {}))
    (out * gout.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in xs.items()}
    grads.update({n: p.grad for n, p in mod.named_parameters()})
    return out.detach(), grads, {n: p.detach().clone() for n, p in mod.named_parameters() if n.endswith("weight_v")}


def main():
    store = {"cases": np.asarray(json.dumps(CASES))}
    for ci, c in enumerate(CASES):
        torch.manual_seed(2000 + ci)
        mod = build(c)
        with torch.no_grad():
            for p in mod.parameters():      # move g and the biases off their init so that every gradient is generic
                p.mul_(1.0 + 0.25 * torch.randn_like(p))
        sd = {k_: v.detach().clone() for k_, v in mod.state_dict().items()}
        n, h, w = c["n"], c["h"], c["w"]
        ins = {"input": torch.randn(n, c["cin"], h, w)}
        if c["aux"]:
            ins["aux"] = torch.randn(n, c["aux"], h, w)
        if c["cond"]:
            ins["condition"] = torch.randn(n, c["cond"], h, w)
        gout = torch.randn(n, c["ch"] if c["kind"] == "conv" else c["cin"], h, w)
        t = f"c{ci}."
        for k_, v in ins.items():
            store[t + "in." + k_] = v.numpy()
        store[t + "in.gout"] = gout.numpy()
        for k_, v in sd.items():
            store[t + "sd." + k_] = v.numpy()
        res = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            m2 = build(c)
            m2.load_state_dict(sd)
            out, grads, after = run(m2, ins, gout, dtype)
            res[tag] = {"out": out, **{"grad." + k_: v for k_, v in grads.items()}}
            store[t + f"out.{tag}"] = out.contiguous().numpy()
            for k_, v in grads.items():
                store[t + f"grad.{tag}.{k_}"] = v.contiguous().numpy()
            if tag == "f32" and c["conv"] == "causal":
                for k_, v in after.items():
                    if "conv.conv." not in k_:       # aux_conv / condition are plain 1x1 layers
                        continue
                    kw = v.shape[3]
                    assert float(v[:, :, -1, kw // 2:].abs().max()) == 0.0
                    store[t + "after." + k_] = v.numpy()
        # the GPU tests bound their error by a multiple of this gap: it must not be 0 for any tensor
        for k_ in res["f32"]:
            gap = float((res["f32"][k_].double() - res["f64"][k_]).abs().max())
            assert gap > 0.0, (ci, k_)
    path = os.path.join(ROOT, "tests", "golden", "pixelsnail_gated_resblock.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
