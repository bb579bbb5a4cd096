"""Capture tests/golden/pixelsnail_model.npz from the reference's PixelSNAIL and PixelBlock (pixelsnail.py:237-431) with the
loss and accuracy of train_pixelsnail.py:39,46-48.

Needs the reference checkout (VQ2_REFERENCE, read-only) at capture time only: per case the file holds the inputs, the
state_dict, and from a float32 and a float64 eval-mode run of the reference the logits, the loss, the accuracy and the
gradient of the loss for every parameter.  Nothing of the reference itself is stored.

Size.  The smallest model the 8-head attention admits (channel 64) has 80,812 parameters; its state_dict and two gradient sets
in full are 1.3 MB, over the 1 MiB limit for a committed file.  So:
  - parameters are moved off their init as in make_golden_gated_resblock.py and then rounded to bfloat16 values (they are
    inputs: any values do, and these compress);
  - a gradient is stored as the float64 run in full and the float32 run's difference from it as float16 in units of its
    largest magnitude (tests/_pixelsnail_model_ref.py:golden_pair puts the pair back together);
  - the gradients of a case marked `own_file` go to pixelsnail_model_grads<case>.npz next to pixelsnail_model.npz, which
    holds everything else (tests/_pixelsnail_model_ref.py:load reads them as one)."""
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
warnings.simplefilter("ignore", UserWarning)
import pixelsnail as ref  # noqa: E402  (the reference module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kind "model": PixelSNAIL(shape, n_class, channel, kernel, n_block, n_res_block, res_channel, **kw) on codes [n, h, w]
#               (h defaults to shape[0]; `cond`: a condition of that size);
# kind "block": PixelBlock(cin, ch, k, n_res_block, attention=, condition_dim=cond) on [n, cin, h, w] with sum(out * gout).
CASES = [
    dict(kind="model", shape=[4, 5], n_class=6, args=[64, 3, 1, 1, 8], kw={}, attention=True, n=2, own_file=True),     # top-like
    dict(kind="model", shape=[4, 6], n_class=6, args=[8, 3, 1, 1, 12], attention=False, n=2, cond=[2, 3],               # bottom-like
         kw=dict(attention=False, n_cond_res_block=1, cond_res_channel=12)),
    dict(kind="model", shape=[3, 4], n_class=5, args=[8, 3, 2, 1, 4], attention=False, n=1,                             # out blocks
         kw=dict(attention=False, n_out_res_block=1)),
    dict(kind="block", cin=4, ch=8, k=5, n_res_block=2, attention=False, cond=4, n=2, h=5, w=6),                      # PixelBlock
    dict(kind="model", shape=[4, 5], n_class=6, args=[64, 3, 1, 1, 8], kw={}, attention=True, n=2, h=3, sd_of=0, own_file=True),   # partial height
]


def build(c):
    if c["kind"] == "block":
        return ref.PixelBlock(c["cin"], c["ch"], c["k"], c["n_res_block"], attention=c["attention"],
                              condition_dim=c["cond"]).eval()
    return ref.PixelSNAIL(c["shape"], c["n_class"], *c["args"], **c["kw"]).eval()


def run(c, mod, ins, dtype):
    mod = mod.to(dtype)
    if c["kind"] == "model":
        out, _ = mod(ins["input"], condition=ins.get("condition"))
        loss = torch.nn.CrossEntropyLoss()(out, ins["input"])
        _, pred = out.max(1)
        acc = (pred == ins["input"]).float().sum() / ins["input"].numel()
        res = {"logits": out.detach(), "loss": loss.detach(), "accuracy": acc}
    else:
        out = mod(ins["input"].to(dtype), ins["background"].to(dtype),
                  condition=ins["condition"].to(dtype) if "condition" in ins else None)
        loss = (out * ins["gout"].to(dtype)).sum()
        res = {"out": out.detach(), "loss": loss.detach()}
    loss.backward()
    res.update({"grad." + n: p.grad for n, p in mod.named_parameters()})
    return res


def main():
    store = {"cases": np.asarray(json.dumps(CASES))}
    own = {}
    sds = {}
    for ci, c in enumerate(CASES):
        torch.manual_seed(3000 + ci)
        t = f"c{ci}."
        if "sd_of" in c:
            sd = sds[c["sd_of"]]
        else:
            mod = build(c)
            with torch.no_grad():
                for p in mod.parameters():      # off the init so that every gradient is generic, then few mantissa bits
                    p.mul_(1.0 + 0.25 * torch.randn_like(p))
                    p.copy_(p.bfloat16().float())
            sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
            for k, v in sd.items():
                store[t + "sd." + k] = v.numpy()
        sds[ci] = sd
        n = c["n"]
        if c["kind"] == "model":
            h, w = c.get("h", c["shape"][0]), c["shape"][1]
            ins = {"input": torch.randint(0, c["n_class"], (n, h, w))}
            if "cond" in c:
                ins["condition"] = torch.randint(0, c["n_class"], (n, *c["cond"]))
        else:
            h, w = c["h"], c["w"]
            ins = {"input": torch.randn(n, c["cin"], h, w), "background": torch.randn(n, 2, h, w),
                   "gout": torch.randn(n, c["cin"], h, w)}
            if c["cond"]:
                ins["condition"] = torch.randn(n, c["cond"], h, w)
        for k, v in ins.items():
            store[t + "in." + k] = v.numpy()
        res = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            m2 = build(c)
            m2.load_state_dict(sd)
            res[tag] = run(c, m2, ins, dtype)
        assert float(res["f32"].get("accuracy", 0)) == float(res["f64"].get("accuracy", 0))
        for k in res["f64"]:
            a32, a64 = res["f32"][k].detach().double().contiguous(), res["f64"][k].detach().contiguous()
            if k == "accuracy":
                store[t + k] = a64.numpy()
                continue
            # the tests bound their error by a multiple of this gap: it must not be 0 for any stored tensor
            gap = float((a32 - a64).abs().max())
            assert gap > 0.0, (ci, k)
            if k.startswith("grad."):
                dst = own.setdefault(ci, {}) if c.get("own_file") else store
                dst[t + k + ".f64"] = a64.numpy()
                dst[t + k + ".d16"] = ((a32 - a64) / gap).numpy().astype(np.float16)
                dst[t + k + ".s"] = np.asarray(gap)
            else:
                store[t + k + ".f64"] = a64.numpy()
                store[t + k + ".f32"] = res["f32"][k].detach().contiguous().numpy()
    files = {"pixelsnail_model": store, **{f"pixelsnail_model_grads{ci}": d for ci, d in own.items()}}
    for name, d in files.items():
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print(path, size, "bytes")
        assert size < 1000000, size


if __name__ == "__main__":
    main()
