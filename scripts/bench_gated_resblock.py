"""GatedResBlock of the stage-2 prior against the same formula in eager torch (tests/_pixelsnail_ref.py), on one MI355X,
timed with device events.

Shapes: the top prior's causal 5x5 block (256 channels, B = 32, 32 x 32), the 1x1 block with an auxiliary input of 128
channels at the same size, and the 5x5 block with a 256-channel condition at B = 8, 64 x 64; forward and forward +
backward, eval mode (no dropout) and training mode (p = 0.1).  The two paths alternate inside every repeat, the first
repeat of a series is discarded (warm-up), and the spread of the others is reported with the medians.  Writes one JSON
document (default profiles/gated_resblock.json).  No GPU: fails.

Counted from the shapes (not measured): conv FLOP = 2 * pixels * KH * KW * (in * channel + channel * 2 in) per forward,
every tap (also the ones a 'causal' layer zeroes), three times that for forward + backward; the rate is taken over the
time of the WHOLE block call, so it is a lower bound for the conv kernels, against the 157.3 TFLOP/s fp32 matrix peak.

--precision bf16: the second path is not eager torch but the SAME block with bf16 conv operands
(vqvae2_amd.set_conv_precision), built from the same weights; "fused" is then the fp32 block and "eager" reads "bf16" in
every key, the rate of the bf16 block is taken against the 2,500 TFLOP/s bf16 dense peak, and the agreement bound is 2e-2
of the largest output (two operand roundings of 2^-9 each, through two convs).  Default output
profiles/gated_resblock_bf16.json.

--precision bf16_wgrad: the two paths are the block with bf16 conv operands ("fused" in every key) and the same block with
bf16 weight gradients as well ("bf16_wgrad" in every key), built from the same weights.  Both rates are then taken against
the bf16 dense peak ("peak_tflops" in the output says so), and the two forwards are the same launches.  Default output
profiles/gated_resblock_bf16_wgrad.json."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TFLOPS = 157.3
PEAK_BF16_TFLOPS = 2500.0

CASES = [dict(cin=256, ch=256, k=5, conv="causal", aux=0, cond=0, b=32, hw=32),
         dict(cin=256, ch=256, k=1, conv="wnconv2d", aux=128, cond=0, b=32, hw=32),
         dict(cin=256, ch=256, k=5, conv="causal", aux=0, cond=256, b=8, hw=64)]


def time_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/gated_resblock.json, gated_resblock_bf16.json with --precision bf16")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "bf16_wgrad"],
                    help="bf16: time the block with bf16 conv operands against the fp32 block instead of eager torch; "
                         "bf16_wgrad: the block with bf16 weight gradients too against the bf16 block (then 'fused' in every key)")
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats per path (one more is run first and discarded)")
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    low = args.precision != "fp32"
    other = args.precision if low else "eager"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "gated_resblock_%s.json" % args.precision if low else "gated_resblock.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_gated_resblock.py needs the MI355X")
    import vqvae2_amd
    import _pixelsnail_ref as R
    dev = torch.device("cuda:0")
    fused_peak = PEAK_BF16_TFLOPS if args.precision == "bf16_wgrad" else PEAK_TFLOPS     # "fused" is the bf16 block there
    results = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "inner": args.inner,
               "peak_tflops": fused_peak, "cases": []}
    if low:
        results.update(precision=args.precision, peak_bf16_tflops=PEAK_BF16_TFLOPS)
    for c in CASES:
        b, hw, cin, ch = c["b"], c["hw"], c["cin"], c["ch"]
        torch.manual_seed(0)
        mod = vqvae2_amd.GatedResBlock(cin, ch, c["k"], conv=c["conv"], dropout=0.1, auxiliary_channel=c["aux"],
                                       condition_dim=c["cond"]).to(dev)
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
        mod16 = None
        if low:
            mod16 = copy.deepcopy(mod)
            vqvae2_amd.set_conv_precision(mod16, args.precision)
            if args.precision == "bf16_wgrad":      # bf16 against bf16_wgrad: the same forward and data gradient on both sides
                vqvae2_amd.set_conv_precision(mod, "bf16")

        def act(channels):
            return torch.randn(b, channels, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)

        x = act(cin)
        aux = act(c["aux"]) if c["aux"] else None
        cond = act(c["cond"]) if c["cond"] else None
        gout = act(cin).detach()

        def eager(training):
            if low:
                return mod16(x, aux, cond)
            keep = (torch.rand(b, ch, hw, hw, device=dev) >= 0.1) if training else None
            return R.gated_resblock(x, sd, c["conv"], aux, cond, keep=keep, p=0.1)

        # faster and different is not faster: the two paths must agree in eval mode at the timed size
        mod.eval()
        if low:
            mod16.eval()
        with torch.no_grad():
            want = eager(False)
            diff = float((mod(x, aux, cond) - want).abs().max())
            # fp32 sums of up to 6,400 products in two orders: ~1e-5 relative; bf16 operands: see the module docstring
            bound = (2e-2 if low else 1e-4) * float(want.abs().max())
        if not diff <= bound:
            raise SystemExit(f"case {c}: the fused block differs from the {other} one by {diff:.3e} (bound {bound:.3e}); not timed")
        conv_flop = 2.0 * b * hw * hw * c["k"] ** 2 * (cin * ch + ch * 2 * cin)
        for training in (False, True):
            mod.train(training)
            if low:
                mod16.train(training)

            def fused_f():
                with torch.no_grad():
                    mod(x, aux, cond)

            def eager_f():
                with torch.no_grad():
                    eager(training)

            def fused_fb():
                mod(x, aux, cond).backward(gout)

            def eager_fb():
                eager(training).backward(gout)

            row = {**c, "training": training, "eval_max_abs_diff": diff, "eval_diff_bound": bound}
            for tag, ff, ef, flop in (("fwd", fused_f, eager_f, conv_flop), ("fwd_bwd", fused_fb, eager_fb, 3 * conv_flop)):
                for fn in (ff, ef):      # warm every shape the timed window uses
                    fn()
                    fn()
                torch.cuda.synchronize()
                tf, te = [], []
                for _ in range(args.repeats + 1):   # alternate the two paths
                    tf.append(time_ms(ff, args.inner))
                    te.append(time_ms(ef, args.inner))
                tf, te = tf[1:], te[1:]              # the first window of a series still carries warm-up
                mf, me = statistics.median(tf), statistics.median(te)
                row[tag] = {"fused_ms": tf, other + "_ms": te, "fused_median_ms": mf, other + "_median_ms": me,
                            "fused_spread": (max(tf) - min(tf)) / mf, other + "_spread": (max(te) - min(te)) / me,
                            other + "_over_fused": me / mf, "counted_conv_flop": flop,
                            "fused_conv_tflops": flop / (mf * 1e-3) / 1e12,
                            "fused_fraction_of_peak": flop / (mf * 1e-3) / 1e12 / fused_peak}
                if low:
                    row[tag].update(bf16_conv_tflops=flop / (me * 1e-3) / 1e12,
                                    bf16_fraction_of_peak=flop / (me * 1e-3) / 1e12 / PEAK_BF16_TFLOPS)
                print(json.dumps({"case": f"{c['conv']} k{c['k']} B{b} {hw}x{hw}", "training": training, "pass": tag,
                                  "fused_ms": round(mf, 4), other + "_ms": round(me, 4),
                                  "tflops": round(row[tag]["fused_conv_tflops"], 2),
                                  "spread": [round(row[tag]["fused_spread"], 3), round(row[tag][other + "_spread"], 3)]}), flush=True)
            results["cases"].append(row)
            for t in (x, aux, cond, *sd.values(), *mod.parameters(), *(mod16.parameters() if low else ())):
                if t is not None:
                    t.grad = None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
