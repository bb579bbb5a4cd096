"""Fused CausalAttention against the same formula in eager torch, on one MI355X, timed with device events.

Shapes: the top prior's layer (B = 32, L = 32 * 32, 8 heads of 16; query 258 / key 514 channels as PixelSNAIL builds
them) and the same layer at L = 64 * 64 with B = 2, forward and forward + backward, eval mode (no dropout) and
training mode (p = 0.1).  The two paths alternate inside every repeat, the first repeat of a series is discarded
(warm-up), and the spread of the others is reported with the medians.  Writes one JSON document (default profiles/attention.json).  No GPU: fails.

Counted from the shapes (not measured): exponentials = B * n_head * L * (L - 1) / 2 per forward evaluation of P (the
backward pass evaluates P three times more: row terms, dK/dV, dQ); bytes = what the fused attention core must move (q, k, v in, o and the
log-sum-exp out; backward: q, k, v, dO and the log-sum-exp in, dq, dk, dv out) -- reported over the time of the WHOLE module call
(projections included), so both rates are lower bounds for the core kernels.

--precision both: the second path is not eager torch but the SAME module with bf16-operand attention
(vqvae2_amd.set_attention_precision), built from the same weights; "fused" is then the fp32 module and "eager" reads "bf16" in
every key, so "bf16_over_fused" below 1 means the bf16 core is faster.  eval_max_abs_diff is then the difference between the two
precisions.  Default output profiles/attention_bf16.json."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def eager_forward(query, key, sd, n_head, p, training):
    """The layer as a user writes it today: weight-normed linears, a materialised [B, n_head, L, L] score tensor filled
    with -1e4 above the strict diagonal, softmax, start mask, dropout, matmul."""
    b, _, h, w = query.shape
    l = h * w
    xq = query.reshape(b, query.shape[1], l).transpose(1, 2)
    xk = key.reshape(b, key.shape[1], l).transpose(1, 2)

    def lin(x, name):
        v, g = sd[name + ".weight_v"], sd[name + ".weight_g"]
        return torch.nn.functional.linear(x, v * (g / v.norm(2, dim=1, keepdim=True)), sd[name + ".bias"])

    c = sd["query.bias"].numel()
    dh = c // n_head
    q, k, v = (t.view(b, l, n_head, dh).transpose(1, 2) for t in (lin(xq, "query"), lin(xk, "key"), lin(xk, "value")))
    s = torch.matmul(q, k.transpose(2, 3)) / math.sqrt(dh)
    vis = torch.ones(l, l, dtype=torch.bool, device=query.device).tril(-1)
    start = torch.ones(l, 1, device=query.device)
    start[0] = 0
    pr = torch.softmax(s.masked_fill(~vis, -1e4), 3) * start
    pr = torch.nn.functional.dropout(pr, p, training)
    return (pr @ v).transpose(1, 2).reshape(b, h, w, c).permute(0, 3, 1, 2)


def time_ms(fn, repeats, inner):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/attention.json, attention_bf16.json with --precision both")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "both"],
                    help="both: time the fp32 fused module against the same module with bf16-operand attention")
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats per path (one more is run first and discarded)")
    ap.add_argument("--inner", type=int, default=50)
    args = ap.parse_args()
    low = args.precision != "fp32"
    other = "bf16" if low else "eager"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "attention_bf16.json" if low else "attention.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention.py needs the MI355X")
    import vqvae2_amd
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "inner": args.inner, "cases": []}
    if low:
        results["precision"] = args.precision
    for b, hw in ((32, 32), (2, 64)):
        l, nh, dh, cq, ck = hw * hw, 8, 16, 258, 514
        torch.manual_seed(0)
        mod = vqvae2_amd.CausalAttention(cq, ck, nh * dh, n_head=nh, dropout=0.1).to(dev)
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
        mod16 = None
        if low:
            mod16 = vqvae2_amd.CausalAttention(cq, ck, nh * dh, n_head=nh, dropout=0.1).to(dev)
            mod16.load_state_dict(mod.state_dict())
            assert vqvae2_amd.set_attention_precision(mod16, "bf16") == (1, 1)
        query = torch.randn(b, cq, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        key = torch.randn(b, ck, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        gout = torch.randn(b, nh * dh, hw, hw, device=dev).contiguous(memory_format=torch.channels_last)
        # faster and different is not faster: the two paths must agree in eval mode at the timed size
        mod.eval()
        with torch.no_grad():
            ref = mod16.eval()(query, key) if low else eager_forward(query, key, sd, nh, 0.0, False)
            diff = float((mod(query, key) - ref).abs().max())
        unit = b * l * nh * dh * 4
        exps = b * nh * l * (l - 1) // 2
        for training in (False, True):
            mod.train(training)
            if low:
                mod16.train(training)

            def fused_f():
                with torch.no_grad():
                    mod(query, key)

            def eager_f():
                with torch.no_grad():
                    mod16(query, key) if low else eager_forward(query, key, sd, nh, 0.1, training)

            def fused_fb():
                mod(query, key).backward(gout)

            def eager_fb():
                (mod16(query, key) if low else eager_forward(query, key, sd, nh, 0.1, training)).backward(gout)

            row = {"B": b, "L": l, "n_head": nh, "dim_head": dh, "training": training, "eval_max_abs_diff": diff}
            for tag, ff, ef, n_exp, byts in (("fwd", fused_f, eager_f, exps, 4 * unit + unit // dh),
                                             ("fwd_bwd", fused_fb, eager_fb, 4 * exps, 11 * unit + 2 * unit // dh)):
                for fn in (ff, ef):      # warm every shape the timed window uses
                    fn()
                    fn()
                torch.cuda.synchronize()
                tf, te = [], []
                for _ in range(args.repeats + 1):   # alternate the two paths
                    tf += time_ms(ff, 1, args.inner)
                    te += time_ms(ef, 1, args.inner)
                tf, te = tf[1:], te[1:]              # the first window of a series still carries warm-up
                mf, me = statistics.median(tf), statistics.median(te)
                row[tag] = {"fused_ms": tf, other + "_ms": te, "fused_median_ms": mf, other + "_median_ms": me,
                            "fused_spread": (max(tf) - min(tf)) / mf, other + "_spread": (max(te) - min(te)) / me,
                            other + "_over_fused": me / mf, "counted_exponentials": n_exp,
                            "fused_exponentials_per_s": n_exp / (mf * 1e-3), "counted_core_bytes": byts,
                            "fused_core_bytes_per_s": byts / (mf * 1e-3)}
                print(json.dumps({"B": b, "L": l, "training": training, "pass": tag, "fused_ms": round(mf, 4),
                                  other + "_ms": round(me, 4), "spread": [round(row[tag]["fused_spread"], 3),
                                                                          round(row[tag][other + "_spread"], 3)]}), flush=True)
            results["cases"].append(row)
            for t in (query, key, *sd.values(), *mod.parameters(), *(mod16.parameters() if low else ())):
                t.grad = None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
