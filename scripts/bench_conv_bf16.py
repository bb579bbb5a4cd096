"""Conv forward / data gradient of the stage-2 priors' layers, one launch each: the fp32 kernel against the bf16-operand
kernel (ConvSpec.bf16), on one MI355X, timed with device events.  The four launches of a layer alternate inside every
repeat; WARMUP launches of each first, then REPEATS windows of INNER launches; [min, max] ms per launch of the windows,
TFLOP/s from the minimum.  The weight panels are packed once (the weight does not change), so the pack kernels are not
in these numbers: scripts/bench_pixelsnail.py --amp O1 times the step that contains them.

    python scripts/bench_conv_bf16.py [--out FILE]      (default profiles/conv_bf16.json)

--wgrad times the weight gradient of the same layers by the same method instead: the fp32 launch (its own plan: exchanged
roles or a Winograd mode where the layer has one) against the bf16-operand launch (ConvSpec.bf16_wgrad), each with its
reduction and the fused bias gradient, alternated inside every repeat.

    python scripts/bench_conv_bf16.py --wgrad [--out FILE]      (default profiles/wgrad_bf16.json)
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPEATS, INNER = 3, 5, 10
PEAK_BF16_TFLOPS, PEAK_FP32_TFLOPS = 2500, 157

# (name, cin, cout, kh, kw, pad_top, pad_left, n, h, w)
SHAPES = [
    ("top 5x5 256->256", 256, 256, 5, 5, 4, 2, 32, 32, 32),
    ("top 5x5 256->512", 256, 512, 5, 5, 4, 2, 32, 32, 32),
    ("bottom 5x5 256->256", 256, 256, 5, 5, 4, 2, 8, 64, 64),
    ("bottom 5x5 256->512", 256, 512, 5, 5, 4, 2, 8, 64, 64),
    ("1x1 256->256", 256, 256, 1, 1, 0, 0, 32, 32, 32),
    ("1x1 256->512", 256, 512, 1, 1, 0, 0, 32, 32, 32),
    ("1x1 128->256 aux", 128, 256, 1, 1, 0, 0, 32, 32, 32),
    ("3x3 256->256 cond", 256, 256, 3, 3, 1, 1, 32, 32, 32),
    ("1x1 256->512 n2", 256, 512, 1, 1, 0, 0, 2, 32, 32),
    ("5x5 256->256 n1", 256, 256, 5, 5, 4, 2, 1, 32, 32),
    ("5x5 32->32 tiny", 32, 32, 5, 5, 4, 2, 2, 6, 8),
    ("5x5 64->128 tiny", 64, 128, 5, 5, 4, 2, 2, 6, 8),
]


def time_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def measure(ops, shape, wgrad=False):
    name, ci, co, kh, kw, pt, pl, n, h, w = shape
    dev = torch.device("cuda:0")
    s32 = ops.ConvSpec.geom(ci, co, kh, kw, pt, pl)
    s16 = dataclasses.replace(s32, bf16=True)
    x = torch.randn(n, h, w, ci, device=dev)
    dy = torch.randn(n, h, w, co, device=dev)
    wt = torch.randn(co, ci, kh, kw, device=dev) / (ci * kh * kw) ** 0.5
    b = torch.randn(co, device=dev)
    y = torch.empty(n, h, w, co, device=dev)
    dx = torch.empty(n, h, w, ci, device=dev)
    w16 = dataclasses.replace(s32, bf16_wgrad=True)
    fns = {"wg32": lambda: ops.conv_wgrad(s32, x, dy, False, wt, b),
           "wg16": lambda: ops.conv_wgrad(w16, x, dy, False, wt, b)} if wgrad else \
          {"fwd32": lambda: ops.conv_forward(s32, x, wt, b, out=y),
           "fwd16": lambda: ops.conv_forward(s16, x, wt, b, out=y),
           "dg32": lambda: ops.conv_dgrad(s32, x.shape, dy, wt, out=dx),
           "dg16": lambda: ops.conv_dgrad(s16, x.shape, dy, wt, out=dx)}
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            t[k].append(time_ms(fn, INNER))
    flops = 2.0 * n * h * w * ci * co * kh * kw
    row = {"shape": name, "gflop": flops / 1e9}
    for k, v in t.items():
        row[k + "_ms"] = [round(min(v), 4), round(max(v), 4)]
        row[k + "_tflops"] = round(flops / min(v) / 1e9, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wgrad", action="store_true", help="time the weight gradient (fp32 against bf16 operands) instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "wgrad_bf16.json" if args.wgrad else "conv_bf16.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_bf16.py needs the MI355X")
    from vqvae2_amd import ops
    rows = []
    for shape in SHAPES:
        rows.append(measure(ops, shape, args.wgrad))
        print(json.dumps(rows[-1]), flush=True)
    what = "conv weight gradient with its reduction and bias gradient, fp32 launch (wg32) vs bf16-operand launch (wg16, " \
           "VQ2_ALLOW_BF16); the two launches" if args.wgrad else \
           "conv forward / data gradient, fp32 kernel vs bf16-operand kernel (VQ2_ALLOW_BF16); the four launches"
    out = {"what": what + " of a "
                   f"layer alternated in one process, {WARMUP} warm-up launches, {REPEATS} windows of {INNER} launches between "
                   "two events, [min, max] ms per launch; TFLOP/s from the minimum; the shape name ends in the batch where "
                   "it is not 32 x 32x32 (top, unnamed) or 8 x 64x64 (bottom)",
           "device": torch.cuda.get_device_name(0), "bf16_dense_peak_tflops": PEAK_BF16_TFLOPS,
           "fp32_matrix_peak_tflops": PEAK_FP32_TFLOPS, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
