"""Capture tests/golden/quantize_shapes.npz: the reference's own Quantize (and the state_dict layouts of its two models)
at latent widths and codebook sizes outside the power-of-two / multiple-of-4 set of tests/golden/quantize.npz.

Runs only where a checkout of the reference exists; the reference never travels.  Inputs are pure functions of
(seed, stream name) through oracle/rng.py, so the fixture holds the reference's numeric OUTPUTS and the seeds only:

    PYTHONDONTWRITEBYTECODE=1 python scripts/capture_quantize_shapes.py <path to the reference checkout>

The case table and the input builder below are also what the tests import (tests/test_quantize_shapes_cpu.py,
tests/test_gpu_quantize_shapes.py): importing this module touches neither the reference nor the GPU.

Bit-exact indices are a fair demand on these inputs: for every row that is not a crafted tie, the fp64 gap between the
two best codes, relative to ||x||^2 + 1, is at least MARGIN = 1e-5 -- five times the 2e-6 near-tie scale at which fp32
summation orders are known to disagree.  The script moves to the next seed until that holds and
stores the seed it used; the CPU test recomputes the margins from the stored seeds.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import rng  # noqa: E402
from oracle import vqvae_oracle as O  # noqa: E402

FIRST_SEED = 1234
MARGIN = 1e-5
EMBED_COL_STEP = 16     # embed / embed_avg after the update are stored as every 16th codebook column
OUT_ROW_STEP = 4        # the straight-through output as every 4th row

# tag, D, K, x shape, crafted ties
CASES = [
    ("s48_510", 48, 510, (2, 8, 8, 48), False),      # both dimensions ragged
    ("s64_510", 64, 510, (2, 8, 8, 64), False),      # K ragged only
    ("s48_512", 48, 512, (2, 8, 8, 48), False),      # D ragged only
    ("s96_1000", 96, 1000, (2, 8, 8, 96), False),    # D above 64: the 8-wave shape
    ("s192_512", 192, 512, (2, 8, 8, 192), False),
    ("s12_5", 12, 5, (2, 8, 8, 12), False),          # smaller than one float4 of codes
    ("s20_2050", 20, 2050, (2, 8, 8, 20), False),    # ragged K through the K-split
    ("s48_510_tie", 48, 510, (2, 8, 8, 48), True),   # duplicate code columns: the first index wins
]
TIE_ROWS = (0, 1, 2)    # rows of a tie case that sit exactly on duplicated codes

# (tag, class name, constructor kwargs) of the models whose state_dict layout is stored
MODEL_CASES = [
    ("vqvae_48_510", "VQVAE", dict(embed_dim=48, n_embed=510)),
    ("deep_192", "VQVAE_Deep", dict(embed_dim=192)),
]


def shape_inputs(tag, D, K, xshape, tie, seed):
    """(x, embed, cluster_size before, weights of the output in the test loss) -- like oracle.make_golden_cases.
    quantize_inputs, with the seed as an argument."""
    embed = rng.normal(seed, f"{tag}.embed", (D, K))
    if tie:
        embed[:, 300] = embed[:, 5]
        embed[:, 7] = embed[:, 5]
        embed[:, 100] = embed[:, 64]
    x = rng.normal(seed, f"{tag}.x", xshape)
    if tie:
        flat = x.reshape(-1, D)
        flat[0] = embed[:, 5]
        flat[1] = embed[:, 64]
        flat[2] = embed[:, 300]
        x = flat.reshape(xshape)
    gw = rng.normal(seed, f"{tag}.gw", xshape)
    cs0 = (np.abs(rng.normal(seed, f"{tag}.cs", (K,))) * 3.0).astype(np.float32)
    return x, embed, cs0, gw


def relative_margins(x, embed, tie):
    """fp64 gap between the two best codes over (||x||^2 + 1) for every row that is not a crafted tie."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).reshape(-1, embed.shape[0])
    gap, _ = O.quantize_margin(xt, torch.from_numpy(np.ascontiguousarray(embed)))
    rel = gap / (xt.double().pow(2).sum(1) + 1.0)
    if tie:
        keep = torch.ones(rel.numel(), dtype=torch.bool)
        keep[list(TIE_ROWS)] = False
        rel = rel[keep]
    return rel.numpy()


def pick_seed(tag, D, K, xshape, tie):
    seed = FIRST_SEED
    while True:
        x, embed, _, _ = shape_inputs(tag, D, K, xshape, tie, seed)
        if float(relative_margins(x, embed, tie).min()) >= MARGIN:
            return seed
        seed += 1


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _n(v):
    return v.detach().cpu().numpy().copy()


def capture_case(ref, tag, D, K, xshape, tie):
    seed = pick_seed(tag, D, K, xshape, tie)
    x, embed, cs0, gw = shape_inputs(tag, D, K, xshape, tie, seed)
    d = {f"{tag}.seed": np.int64(seed)}
    for training in (True, False):
        q = ref.Quantize(D, K)
        q.embed.copy_(_t(embed))
        q.embed_avg.copy_(_t(embed) * _t(cs0)[None, :])
        q.cluster_size.copy_(_t(cs0))
        q.train(training)
        xt = _t(x).clone().requires_grad_(True)
        out, diff, idx = q(xt)
        ((out * _t(gw)).sum() + 0.25 * diff).backward()
        if training:
            d.update({f"{tag}.idx": _n(idx).astype(np.int32), f"{tag}.diff": _n(diff),
                      f"{tag}.out_rows": _n(out).reshape(-1, D)[::OUT_ROW_STEP], f"{tag}.xgrad": _n(xt.grad),
                      f"{tag}.cluster_size_after": _n(q.cluster_size),
                      f"{tag}.embed_avg_after_cols": _n(q.embed_avg)[:, ::EMBED_COL_STEP],
                      f"{tag}.embed_after_cols": _n(q.embed)[:, ::EMBED_COL_STEP]})
        else:
            assert np.array_equal(_n(q.embed), embed) and np.array_equal(_n(q.cluster_size), cs0)
            d.update({f"{tag}.eval_idx": _n(idx).astype(np.int32), f"{tag}.eval_diff": _n(diff)})
    return d


def capture_layout(mod, tag, cls, kwargs):
    sd = getattr(mod, cls)(**kwargs).state_dict()
    return {f"{tag}.keys": np.array(list(sd.keys())),
            f"{tag}.shapes": np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], np.int64)}


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.abspath(argv[1]))
    import vqvae as ref             # the reference's modules
    import vqvae_deep as refd
    torch.manual_seed(0)
    d = {}
    for tag, D, K, xshape, tie in CASES:
        d.update(capture_case(ref, tag, D, K, xshape, tie))
        print(tag, "seed", int(d[f"{tag}.seed"]))
    for tag, cls, kwargs in MODEL_CASES:
        d.update(capture_layout(ref if cls == "VQVAE" else refd, tag, cls, kwargs))
    out = os.path.join(ROOT, "tests", "golden", "quantize_shapes.npz")
    np.savez_compressed(out, **d)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv)
