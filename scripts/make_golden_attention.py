"""Capture tests/golden/pixelsnail_attention.npz from the reference's CausalAttention (pixelsnail.py:195-234).

Needs the reference checkout (VQ2_REFERENCE, read-only) at capture time only: the file holds inputs, the state_dict,
the eval-mode output and the gradients of sum(out * gout) with respect to query, key and all nine parameters, each
from a float32 and from a float64 run of the reference.  Nothing of the reference itself is stored."""
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

# (B, H, W, Cq, Ck, channel, n_head): padded channel counts (10 -> 12, 18 -> 20, 14 -> 16, 7 -> 8, 9 -> 12), the
# workload's 8 heads of 16, a 3 x 3 map, a head width that is no multiple of 16, and the top prior's own input channel
# counts (258 -> 260, 514 -> 516) with a narrow output so that the weights stay small
CASES = [(2, 5, 13, 10, 18, 32, 2), (1, 5, 7, 10, 14, 128, 8), (2, 3, 3, 6, 6, 8, 2), (2, 4, 5, 7, 9, 60, 3),
         (1, 2, 3, 258, 514, 8, 2)]


def run(mod, query, key, gout, dtype):
    mod = mod.to(dtype)
    q = query.detach().to(dtype).clone().requires_grad_(True)
    k = key.detach().to(dtype).clone().requires_grad_(True)
    out = mod(q, k)
    (out * gout.to(dtype)).sum().backward()
    grads = {"query": q.grad, "key": k.grad}
    grads.update({n: p.grad for n, p in mod.named_parameters()})
    return out.detach(), grads


def main():
    store = {"cases": np.asarray(CASES, dtype=np.int64)}
    for ci, (b, h, w, cq, ck, ch, nh) in enumerate(CASES):
        torch.manual_seed(1000 + ci)
        mod = ref.CausalAttention(cq, ck, ch, n_head=nh).eval()
        with torch.no_grad():
            for p in mod.parameters():      # move g and the biases off their init so that every gradient is generic
                p.mul_(1.0 + 0.25 * torch.randn_like(p))
        sd = {k_: v.detach().clone() for k_, v in mod.state_dict().items()}
        query, key, gout = torch.randn(b, cq, h, w), torch.randn(b, ck, h, w), torch.randn(b, ch, h, w)
        t = f"c{ci}."
        store[t + "in.query"], store[t + "in.key"], store[t + "in.gout"] = query.numpy(), key.numpy(), gout.numpy()
        for k_, v in sd.items():
            store[t + "sd." + k_] = v.numpy()
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            m2 = ref.CausalAttention(cq, ck, ch, n_head=nh).eval()
            m2.load_state_dict(sd)
            out, grads = run(m2, query, key, gout, dtype)
            assert float(out[:, :, 0, 0].abs().max()) == 0.0
            store[t + f"out.{tag}"] = out.contiguous().numpy()
            for k_, v in grads.items():
                store[t + f"grad.{tag}.{k_}"] = v.contiguous().numpy()
    path = os.path.join(ROOT, "tests", "golden", "pixelsnail_attention.npz")
    np.savez(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
