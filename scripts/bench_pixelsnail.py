"""One Stage2Trainer step of the two priors at the reference's sizes, on one MI355X: the arena path (arena=True: one
weight-norm launch forward, one backward, one Adam launch) against the per-layer path (arena=False), timed with device
events.

Models: the top prior PixelSNAIL([32, 32], 512, 256, 5, 4, 4, 256) at batch 32 and the conditioned bottom prior
PixelSNAIL([64, 64], 512, 256, 5, 4, 4, 256, attention=False, n_cond_res_block=3, cond_res_channel=256) at batch 8 (the
same number of pixels per step), dropout 0.1, random codes from a seed.  Per model:

  * both trainers are built from the same weights in one process and alternate inside every repeat; the first repeat is
    discarded (warm-up) and the spread of the others is reported with the median;
  * the first step of both runs from the same generator seed and must give the same loss bit for bit -- a path that is
    faster and different is not faster;
  * library calls per step: every libvq2 entry point is wrapped for ONE step per path and the calls are counted on the
    host (a call is one or a few launches; torch's own launches -- zero_(), copies -- are not in this number);
  * peak device memory: torch.cuda.max_memory_allocated over steps of ONE path with only that trainer alive.

Writes one JSON document (default profiles/pixelsnail.json).  No GPU: fails.  Not measured here: kernel times (no
profiler run), anything on more than one GPU.

--amp O1: instead, per model, the arena trainers with bf16 conv operands (Stage2Trainer.set_precision('bf16'),
'bf16_wgrad' with bf16 weight gradients as well, and 'bf16_attn' with bf16-operand attention cores on top) against the
arena trainer in fp32, from the same weights, alternating in the same way; the first losses must agree to 1e-2 relative
(they cannot be bit-equal).  Default output profiles/pixelsnail_bf16.json.

--n_label N: instead, per model, the arena trainer of the class-conditional prior (PixelSNAIL(..., n_label=N), random labels
from the seed, the other weights shared) against the arena trainer of the unlabelled one, alternating in the same way; min,
max and median of the repeats.  Both first losses are recorded (the tables start at normal(0, 0.05): a small change of the
model, not none).  Default output profiles/label_cond.json."""
import argparse
import collections
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = [
    dict(name="top", hier="top", shape=[32, 32], batch=32, args=[512, 256, 5, 4, 4, 256], kw={}),
    dict(name="bottom", hier="bottom", shape=[64, 64], batch=8, args=[512, 256, 5, 4, 4, 256],
         kw=dict(attention=False, n_cond_res_block=3, cond_res_channel=256)),
]
TINY = [
    dict(name="tiny_top", hier="top", shape=[4, 4], batch=2, args=[6, 64, 3, 2, 1, 8], kw={}),
    dict(name="tiny_bottom", hier="bottom", shape=[8, 8], batch=2, args=[6, 8, 3, 2, 1, 8],
         kw=dict(attention=False, n_cond_res_block=1, cond_res_channel=8)),
]


class CallCounter:
    """Counts calls of libvq2 entry points on the host while active (the binding looks its functions up on `lib` at call
    time)."""

    def __init__(self, amd):
        self.lib, self.names = amd._lib.lib, [n for n in amd._lib.EXPORTS if n != "vq2_last_error"]
        self.counts = collections.Counter()

    def _wrap(self, name, fn):
        def counted(*a):
            self.counts[name] += 1
            return fn(*a)
        return counted

    def __enter__(self):
        self.saved = {n: getattr(self.lib, n) for n in self.names}
        for n, f in self.saved.items():
            setattr(self.lib, n, self._wrap(n, f))
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(self.lib, n, f)


def time_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def bench_model(amd, spec, repeats, inner):
    dev = torch.device("cuda:0")
    h, w = spec["shape"]
    gen = torch.Generator().manual_seed(1)
    n_class = spec["args"][0]
    codes = torch.randint(0, n_class, (spec["batch"], h, w), generator=gen).to(dev)
    top = torch.randint(0, n_class, (spec["batch"], h // 2, w // 2), generator=gen).to(dev)
    step_args = (codes,) if spec["hier"] == "top" else (top, codes)
    torch.manual_seed(0)
    state = amd.PixelSNAIL(spec["shape"], *spec["args"], dropout=0.1, **spec["kw"]).state_dict()

    def make(arena):
        m = amd.PixelSNAIL(spec["shape"], *spec["args"], dropout=0.1, **spec["kw"])
        m.load_state_dict(state)
        m = m.to(dev).train()
        return amd.Stage2Trainer(m, spec["hier"], lr=3e-4, sched="cycle", n_iter=1000, arena=arena)

    row = {"name": spec["name"], "shape": spec["shape"], "batch": spec["batch"], "args": spec["args"], "kw": spec["kw"],
           "parameters": sum(v.numel() for k, v in state.items() if k != "background")}
    # peak memory and call counts: one trainer alive at a time
    first_loss = {}
    for arena in (True, False):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        tr = make(arena)
        torch.manual_seed(7)
        first_loss[arena] = tr.step(*step_args)["loss"].clone()
        tr.step(*step_args)
        torch.cuda.synchronize()
        with CallCounter(amd) as cc:
            tr.step(*step_args)
        torch.cuda.synchronize()
        tag = "arena" if arena else "per_layer"
        row[tag + "_peak_memory_bytes"] = torch.cuda.max_memory_allocated()
        row[tag + "_library_calls_per_step"] = sum(cc.counts.values())
        row[tag + "_library_calls"] = dict(sorted(cc.counts.items()))
        if arena:
            row["plan_info"] = {k: v for k, v in tr.plan_info.items() if k != "per_layer_names"}
            row["bucket_bytes"] = tr.bucket_bytes
        del tr
    row["first_loss"] = float(first_loss[True])
    row["first_loss_bit_equal"] = bool(torch.equal(first_loss[True], first_loss[False]))
    if not row["first_loss_bit_equal"]:
        raise SystemExit(f"{spec['name']}: the two paths differ in their first loss "
                         f"({float(first_loss[True])!r} vs {float(first_loss[False])!r}); not timed")
    # timing: both alive, alternating
    gc.collect()
    torch.cuda.empty_cache()
    ta, tp = make(True), make(False)
    fa, fp = (lambda: ta.step(*step_args)), (lambda: tp.step(*step_args))
    for fn in (fa, fp):
        fn()
        fn()
    torch.cuda.synchronize()
    ms_a, ms_p = [], []
    for _ in range(repeats + 1):
        ms_a.append(time_ms(fa, inner))
        ms_p.append(time_ms(fp, inner))
    ms_a, ms_p = ms_a[1:], ms_p[1:]
    ma, mp_ = statistics.median(ms_a), statistics.median(ms_p)
    row.update(arena_ms=ms_a, per_layer_ms=ms_p, arena_median_ms=ma, per_layer_median_ms=mp_,
               arena_spread=(max(ms_a) - min(ms_a)) / ma, per_layer_spread=(max(ms_p) - min(ms_p)) / mp_,
               per_layer_over_arena=mp_ / ma)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()
                      if k in ("name", "batch", "arena_median_ms", "per_layer_median_ms", "arena_spread", "per_layer_spread",
                               "arena_library_calls_per_step", "per_layer_library_calls_per_step",
                               "arena_peak_memory_bytes", "per_layer_peak_memory_bytes", "first_loss_bit_equal")}), flush=True)
    del ta, tp
    return row


def bench_amp(amd, spec, repeats, inner):
    """One model: the fp32 arena trainer, the bf16 one, the bf16_wgrad one (bf16 weight gradients too) and the bf16_attn
    one (bf16 attention cores too; the bottom prior has no attention, so there it repeats bf16_wgrad), from the same
    weights, alternated."""
    dev = torch.device("cuda:0")
    h, w = spec["shape"]
    gen = torch.Generator().manual_seed(1)
    n_class = spec["args"][0]
    codes = torch.randint(0, n_class, (spec["batch"], h, w), generator=gen).to(dev)
    top = torch.randint(0, n_class, (spec["batch"], h // 2, w // 2), generator=gen).to(dev)
    step_args = (codes,) if spec["hier"] == "top" else (top, codes)
    torch.manual_seed(0)
    state = amd.PixelSNAIL(spec["shape"], *spec["args"], dropout=0.1, **spec["kw"]).state_dict()
    row = {"name": spec["name"], "shape": spec["shape"], "batch": spec["batch"], "args": spec["args"], "kw": spec["kw"]}
    trainers, first = {}, {}
    for prec in ("fp32", "bf16", "bf16_wgrad", "bf16_attn"):
        m = amd.PixelSNAIL(spec["shape"], *spec["args"], dropout=0.1, **spec["kw"])
        m.load_state_dict(state)
        tr = amd.Stage2Trainer(m.to(dev).train(), spec["hier"], lr=3e-4, sched="cycle", n_iter=1000)
        if prec != "fp32":
            row["eligible_layers"], row["conv_layers"] = tr.set_precision(prec)
        if prec == "bf16_attn":
            row["eligible_attention_layers"], row["attention_layers"] = amd.set_attention_precision(tr.model, "bf16")
        torch.manual_seed(7)
        first[prec] = float(tr.step(*step_args)["loss"])
        tr.step(*step_args)
        trainers[prec] = tr
    row["first_loss"] = first
    if not max(abs(first[p] - first["fp32"]) for p in first) <= 1e-2 * abs(first["fp32"]):
        raise SystemExit(f"{spec['name']}: first losses {first} are further apart than 1e-2 relative; not timed")
    fns = {p: (lambda t=t: t.step(*step_args)) for p, t in trainers.items()}
    torch.cuda.synchronize()
    ms = {p: [] for p in fns}
    for _ in range(repeats + 1):
        for p, fn in fns.items():
            ms[p].append(time_ms(fn, inner))
    for p in ms:
        v = ms[p][1:]
        med = statistics.median(v)
        row[p + "_ms"], row[p + "_median_ms"], row[p + "_spread"] = v, med, (max(v) - min(v)) / med
    row["fp32_over_bf16"] = row["fp32_median_ms"] / row["bf16_median_ms"]
    row["bf16_over_bf16_wgrad"] = row["bf16_median_ms"] / row["bf16_wgrad_median_ms"]
    row["fp32_over_bf16_wgrad"] = row["fp32_median_ms"] / row["bf16_wgrad_median_ms"]
    row["bf16_wgrad_over_bf16_attn"] = row["bf16_wgrad_median_ms"] / row["bf16_attn_median_ms"]
    row["fp32_over_bf16_attn"] = row["fp32_median_ms"] / row["bf16_attn_median_ms"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()
                      if k in ("name", "batch", "fp32_median_ms", "bf16_median_ms", "fp32_spread", "bf16_spread", "fp32_over_bf16",
                               "bf16_wgrad_median_ms", "bf16_wgrad_spread", "bf16_over_bf16_wgrad", "bf16_attn_median_ms", "bf16_attn_spread", "bf16_wgrad_over_bf16_attn",
                               "eligible_layers", "conv_layers", "eligible_attention_layers", "attention_layers", "first_loss")}), flush=True)
    return row


def bench_label(amd, spec, n_label, repeats, inner):
    """One model: the unlabelled arena trainer and the class-conditional one with n_label classes, alternated."""
    dev = torch.device("cuda:0")
    h, w = spec["shape"]
    gen = torch.Generator().manual_seed(1)
    n_class = spec["args"][0]
    codes = torch.randint(0, n_class, (spec["batch"], h, w), generator=gen).to(dev)
    top = torch.randint(0, n_class, (spec["batch"], h // 2, w // 2), generator=gen).to(dev)
    label = torch.randint(0, n_label, (spec["batch"],), generator=gen).to(dev)
    step_args = (codes,) if spec["hier"] == "top" else (top, codes)
    torch.manual_seed(0)
    state = amd.PixelSNAIL(spec["shape"], *spec["args"], dropout=0.1, **spec["kw"]).state_dict()
    row = {"name": spec["name"], "shape": spec["shape"], "batch": spec["batch"], "args": spec["args"], "kw": spec["kw"],
           "n_label": n_label}
    fns, first = {}, {}
    for tag, n in (("unlabelled", 0), ("labelled", n_label)):
        torch.manual_seed(3)
        m = amd.PixelSNAIL(spec["shape"], *spec["args"], dropout=0.1, n_label=n, **spec["kw"])
        missing = m.load_state_dict(state, strict=False)
        assert not missing.unexpected_keys and all(k.endswith("label_embed") for k in missing.missing_keys)
        row[tag + "_parameters"] = sum(p.numel() for p in m.parameters())
        tr = amd.Stage2Trainer(m.to(dev).train(), spec["hier"], lr=3e-4, sched="cycle", n_iter=1000)
        kw = {"label": label} if n else {}
        torch.manual_seed(7)
        first[tag] = float(tr.step(*step_args, **kw)["loss"])
        tr.step(*step_args, **kw)
        torch.cuda.synchronize()
        with CallCounter(amd) as cc:
            tr.step(*step_args, **kw)
        torch.cuda.synchronize()
        row[tag + "_library_calls_per_step"] = sum(cc.counts.values())
        row[tag + "_label_calls"] = {k: v for k, v in sorted(cc.counts.items()) if "label" in k or "glu_res" in k}
        fns[tag] = (lambda t=tr, kw=kw: t.step(*step_args, **kw))
    row["first_loss"] = first
    ms = {p: [] for p in fns}
    for _ in range(repeats + 1):
        for p, fn in fns.items():
            ms[p].append(time_ms(fn, inner))
    for p in ms:
        v = ms[p][1:]
        row[p + "_ms"], row[p + "_min_ms"], row[p + "_max_ms"], row[p + "_median_ms"] = v, min(v), max(v), statistics.median(v)
    row["labelled_over_unlabelled"] = row["labelled_median_ms"] / row["unlabelled_median_ms"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()
                      if k in ("name", "batch", "n_label", "unlabelled_min_ms", "unlabelled_max_ms", "labelled_min_ms",
                               "labelled_max_ms", "labelled_over_unlabelled", "labelled_label_calls", "first_loss")}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/pixelsnail.json, pixelsnail_bf16.json with --amp O1")
    ap.add_argument("--amp", default="O0", choices=["O0", "O1"],
                    help="O1: time the arena trainer with bf16 conv operands against the fp32 one (not arena against per-layer)")
    ap.add_argument("--repeats", type=int, default=4, help="timed repeats per path (one more is run first and discarded)")
    ap.add_argument("--inner", type=int, default=3, help="steps per timed window")
    ap.add_argument("--n_label", type=int, default=0,
                    help="N > 0: time the class-conditional arena trainer (n_label=N) against the unlabelled one")
    ap.add_argument("--tiny", action="store_true", help="toy models: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if args.n_label > 0 and args.amp == "O1":
        raise SystemExit("--n_label and --amp O1 are separate measurements")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "label_cond.json" if args.n_label > 0 else
                                "pixelsnail_bf16.json" if args.amp == "O1" else "pixelsnail.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_pixelsnail.py needs the MI355X")
    import vqvae2_amd

    def bench(amd, spec, repeats, inner):
        if args.n_label > 0:
            return bench_label(amd, spec, args.n_label, repeats, inner)
        return (bench_amp if args.amp == "O1" else bench_model)(amd, spec, repeats, inner)

    results = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "inner": args.inner, "tiny": args.tiny,
               "not_measured": ["kernel times (no profiler run)", "more than one GPU"],
               "models": [bench(vqvae2_amd, spec, args.repeats, args.inner) for spec in (TINY if args.tiny else MODELS)]}
    if args.amp == "O1":
        results["amp"] = "O1"
    if args.n_label > 0:
        results["n_label"] = args.n_label
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
