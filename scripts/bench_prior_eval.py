"""Rate of the held-out evaluation of the PixelSNAIL prior, the reference's two configurations (train_pixelsnail.py:99-126,
512 classes): the top prior on 32x32 codes at batch 32 and the bottom prior on 64x64 codes (conditioned on 32x32) at batch
8, freshly initialised weights, codes resident in HBM.  HIP events around `steps` calls after `warmup` calls, REPEATS times
in one session; every figure is reported as the mean of the repeats with their minimum and maximum.

  update          PriorEvaluator.update: eval forward + vq2_prior_eval_rows + vq2_prior_eval_accumulate + vq2_index_hist
  forward         the eval-mode forward under no_grad alone
  added launches  the three launches on logits that are already there
  rows kernel     vq2_prior_eval_rows alone, against the bytes it must read, M * ld * 4

    python scripts/bench_prior_eval.py            (REPEATS=3 STEPS=20 WARMUP=5 by default; writes profiles/prior_eval.json)
    python scripts/bench_prior_eval.py --amp O1   (also `update` of the same model with bf16 conv operands
                                                   (set_conv_precision), and with bf16 attention cores on top
                                                   (set_attention_precision, the evaluator's --precision bf16_attn),
                                                   alternated with the fp32 one inside every repeat;
                                                   writes profiles/prior_eval_bf16.json)
    --out PATH                                    write there instead
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import vqvae2_amd  # noqa: E402
from vqvae2_amd import ops  # noqa: E402
from vqvae2_amd.evaluate import eval_mode  # noqa: E402

REPEATS = int(os.environ.get("REPEATS", "3"))
STEPS = int(os.environ.get("STEPS", "20"))
WARMUP = int(os.environ.get("WARMUP", "5"))
N_CLASS = 512
AMP = "O0"
dev = torch.device("cuda:0")


def by_events(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e-3


def spread(values, scale=1.0, digits=3):
    return {"mean": round(sum(values) / len(values) * scale, digits), "min": round(min(values) * scale, digits),
            "max": round(max(values) * scale, digits)}


def measure(hier, batch):
    torch.manual_seed(0)
    if hier == "top":
        model = vqvae2_amd.PixelSNAIL([32, 32], N_CLASS, 256, 5, 4, 4, 256, dropout=0.1, n_out_res_block=0)
        size = (32, 32)
    else:
        model = vqvae2_amd.PixelSNAIL([64, 64], N_CLASS, 256, 5, 4, 4, 256, attention=False, dropout=0.1, n_cond_res_block=3,
                                      cond_res_channel=256)
        size = (64, 64)
    model = model.to(dev).train()
    g = torch.Generator().manual_seed(1)
    top = torch.randint(0, N_CLASS, (batch, 32, 32), generator=g).to(dev)
    bottom = torch.randint(0, N_CLASS, (batch, 64, 64), generator=g).to(dev)
    target = top if hier == "top" else bottom
    ev = vqvae2_amd.PriorEvaluator(model, hier)
    ev16 = ev16a = None
    if AMP == "O1":
        model16 = copy.deepcopy(model)
        layers = vqvae2_amd.set_conv_precision(model16, "bf16")
        ev16 = vqvae2_amd.PriorEvaluator(model16, hier)
        model16a = copy.deepcopy(model16)
        attn_layers = vqvae2_amd.set_attention_precision(model16a, "bf16")
        ev16a = vqvae2_amd.PriorEvaluator(model16a, hier)

    def forward():
        with eval_mode(model), torch.no_grad():
            return model(top)[0] if hier == "top" else model(bottom, condition=top)[0]

    x = ops.to_nhwc(forward())
    rows = target.numel()
    ld = ops.ld_of(x)
    pos_nll, pos_entropy, hit1, hitk, counters, counts, flag = ev._buffers(dev, size)

    def added():
        nll, entropy, rank = ops.prior_eval_rows(x, target, N_CLASS)
        ops.prior_eval_accumulate(nll, entropy, rank, batch, ev.top_k, pos_nll, pos_entropy, hit1, hitk, counters)
        ops.index_hist(target, counts, flag)

    t = {"update": [], "update_bf16": [], "update_bf16_attn": [], "forward": [], "added": [], "rows": []}
    for _ in range(REPEATS):
        t["update"].append(by_events(lambda: ev.update(top, bottom if hier == "bottom" else None), STEPS, WARMUP))
        if ev16 is not None:
            t["update_bf16"].append(by_events(lambda: ev16.update(top, bottom if hier == "bottom" else None), STEPS, WARMUP))
            t["update_bf16_attn"].append(by_events(lambda: ev16a.update(top, bottom if hier == "bottom" else None), STEPS, WARMUP))
        t["forward"].append(by_events(forward, STEPS, WARMUP))
        t["added"].append(by_events(added, 10 * STEPS, 10 * WARMUP))
        t["rows"].append(by_events(lambda: ops.prior_eval_rows(x, target, N_CLASS), 10 * STEPS, 10 * WARMUP))
    ev.reset()
    ev.update(top, bottom if hier == "bottom" else None)
    r = ev.result()
    nbytes = rows * ld * 4
    extra = {}
    if ev16 is not None:
        ev16.reset()
        ev16.update(top, bottom if hier == "bottom" else None)
        ev16a.reset()
        ev16a.update(top, bottom if hier == "bottom" else None)
        extra = {"update_bf16_ms": spread(t["update_bf16"], 1e3), "eligible_layers": layers[0], "conv_layers": layers[1],
                 "update_fp32_over_bf16": round(sum(t["update"]) / sum(t["update_bf16"]), 3),
                 "nll_of_the_untrained_model_bf16": round(ev16.result()["nll"], 4),
                 "update_bf16_attn_ms": spread(t["update_bf16_attn"], 1e3),
                 "eligible_attention_layers": attn_layers[0], "attention_layers": attn_layers[1],
                 "update_bf16_over_bf16_attn": round(sum(t["update_bf16"]) / sum(t["update_bf16_attn"]), 3),
                 "nll_of_the_untrained_model_bf16_attn": round(ev16a.result()["nll"], 4)}
    return {**extra, "hier": hier, "batch": batch, "codes_per_batch": rows, "n_class": N_CLASS, "row_stride": ld,
            "update_ms": spread(t["update"], 1e3), "update_codes_per_s": spread([rows / v for v in t["update"]], 1.0, 0),
            "forward_ms": spread(t["forward"], 1e3), "added_launches_us": spread(t["added"], 1e6, 2),
            "rows_kernel_us": spread(t["rows"], 1e6, 2), "rows_kernel_bytes": nbytes,
            "rows_kernel_TB_per_s": spread([nbytes / v / 1e12 for v in t["rows"]]),
            "nll_of_the_untrained_model": round(r["nll"], 4), "ln_n_class": round(float(torch.tensor(float(N_CLASS)).log()), 4)}


def main():
    global AMP
    ap = argparse.ArgumentParser()
    ap.add_argument("--amp", default="O0", choices=["O0", "O1"],
                    help="O1: also time update() with bf16 conv operands, and with bf16 attention cores on top")
    ap.add_argument("--out", default=None, help="default profiles/prior_eval.json, prior_eval_bf16.json with --amp O1")
    args = ap.parse_args()
    AMP = args.amp
    out = {"method": f"HIP events around {STEPS} calls after {WARMUP} warm-up calls (10x both for the launches alone), "
                     f"{REPEATS} repeats in one session; mean with min and max of the repeats",
           "device": torch.cuda.get_device_name(0), "results": [measure("top", 32), measure("bottom", 8)]}
    for r in out["results"]:
        print(json.dumps(r), flush=True)
    path = args.out or os.path.join(ROOT, "profiles", "prior_eval_bf16.json" if AMP == "O1" else "prior_eval.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
