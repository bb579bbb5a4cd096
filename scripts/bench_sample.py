"""Sampling from the PixelSNAIL prior on one MI355X: PriorSampler (row-incremental) against the reference's loop on this
package's modules, at the top prior's real size and at the bottom prior's with a reduced row count.

    python scripts/bench_sample.py [--batch 8] [--bottom_rows 8] [--top_k K] [--top_p P] [--out profiles/sample.json]

--top_k / --top_p time the sampler with the truncated draw (vq2_sample_filtered in place of vq2_sample_categorical, one launch per
step either way); the baseline loop is the reference's and has no such filter.

Priors (random weights; the time does not depend on them):
    top     PixelSNAIL([32, 32], 512, 256, 5, 4, 4, 256), no condition
    bottom  PixelSNAIL([64, 64], 512, 256, 5, 4, 4, 256, attention=False, n_cond_res_block=3, cond_res_channel=256),
            conditioned on a [32, 32] map of top codes; the first --bottom_rows rows only (a full map is 4,096 steps)

Measured, with a host clock around work that ends in a device synchronise (no GPU: fails):
    sampler   one warm-up map (or row set), then the median and spread of --repeats maps: seconds per sampled map
    baseline  the reference's loop body -- model(row[:, :i + 1], condition, cache), torch.softmax, torch.multinomial, the
              write -- timed per step at the first, a middle and the last row (two warm-up steps, then --baseline_steps steps
              each), and integrated over the map by the trapezoid rule over rows: an ESTIMATE of the loop's time, which
              avoids running its 1,024 full-model passes
    launches  per sampler step, counted from the recorded program of a middle row plus the draw: library calls, and kernel
              launches (a vq2_conv_fwd_row call is two kernels, every other call of the step one)
Not measured: kernel times (no profiler run), the share of launch overhead, the full 64 x 64 bottom map."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def baseline_step_seconds(model, batch, rows, width, row_index, condition, steps, temperature=1.0):
    """Seconds per step of the reference's loop at row `row_index` (the model sees rows 0..row_index)."""
    row = torch.zeros(batch, rows, width, dtype=torch.int64, device="cuda")
    cache = {}

    def step(j):
        out, _ = model(row[:, :row_index + 1, :], condition=condition, cache=cache)
        prob = torch.softmax(out[:, :, row_index, j] / temperature, 1)
        row[:, row_index, j] = torch.multinomial(prob, 1).squeeze(-1)

    with torch.no_grad():
        sync_time(lambda: [step(0), step(1)])
        return sync_time(lambda: [step(j % width) for j in range(steps)]) / steps


def bench(name, model, batch, rows, condition, repeats, baseline_steps, top_k=0, top_p=1.0):
    import vqvae2_amd
    width = model.background.shape[3]
    sampler = vqvae2_amd.PriorSampler(model)
    run = lambda: sampler.sample(batch, 1.0, condition, seed=1, rows=rows, top_k=top_k, top_p=top_p)
    sync_time(run)
    times = [sync_time(run) for _ in range(repeats)]
    plan = sampler._plan[1]
    picks = sorted({0, rows // 2, rows - 1})
    per_step = {i: baseline_step_seconds(model, batch, rows, width, i, condition, baseline_steps) for i in picks}
    # The map's time is the SUM over its rows of (per-step time at the row) * W.  For a per-step time that is linear between
    # two timed rows a < b, sum_{r = a}^{b} f(r) = (b - a) (f(a) + f(b)) / 2 + (f(a) + f(b)) / 2: the trapezoid over the b - a
    # intervals counts each end row half.  Over all segments the inner ends are made whole by their neighbours, and the half
    # rows missing at the first and the last timed row are the final term, so that the total covers `rows` rows.
    total = 0.0
    for a, b in zip(picks[:-1], picks[1:]):
        total += 0.5 * (per_step[a] + per_step[b]) * (b - a) * width
    total += 0.5 * (per_step[picks[0]] + per_step[picks[-1]]) * width if len(picks) > 1 else per_step[picks[0]] * width
    med = statistics.median(times)
    calls = plan.programs[rows // 2].calls
    two_kernels = sum(1 for _, _, what in calls if what == "conv_fwd_row")
    res = {
        "batch": batch, "rows": rows, "width": width, "steps": rows * width, "top_k": top_k, "top_p": top_p,
        "sampler_seconds_per_map": {"median": med, "min": min(times), "max": max(times), "repeats": repeats},
        "sampler_ms_per_step": 1e3 * med / (rows * width),
        "sampler_library_calls_per_step": len(calls) + 1,
        "sampler_kernel_launches_per_step": len(calls) + two_kernels + 1,
        "sampler_row_conv_calls_per_step": two_kernels,
        "baseline_steps_per_timed_row": baseline_steps,
        "baseline_ms_per_step_at_row": {str(i): 1e3 * t for i, t in per_step.items()},
        "baseline_seconds_per_map_estimate": total,
        "speedup_estimate": total / med,
    }
    print(name, json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--bottom_rows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline_steps", type=int, default=40)
    ap.add_argument("--skip_bottom", action="store_true")
    ap.add_argument("--top_k", type=int, default=0)
    ap.add_argument("--top_p", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample.py needs the MI355X")
    import vqvae2_amd
    torch.manual_seed(0)
    doc = {"device": torch.cuda.get_device_name(0), "method": "host clock around device-synchronised work; baseline integrated "
           "from per-step times at the first, middle and last row (an estimate)"}
    top = vqvae2_amd.PixelSNAIL([32, 32], 512, 256, 5, 4, 4, 256).cuda().eval()
    doc["top"] = bench("top", top, args.batch, 32, None, args.repeats, args.baseline_steps, args.top_k, args.top_p)
    del top
    if not args.skip_bottom:
        bottom = vqvae2_amd.PixelSNAIL([64, 64], 512, 256, 5, 4, 4, 256, attention=False, n_cond_res_block=3,
                                       cond_res_channel=256).cuda().eval()
        cond = torch.randint(0, 512, (args.batch, 32, 32), device="cuda")
        doc["bottom_first_rows"] = bench("bottom", bottom, args.batch, args.bottom_rows, cond, args.repeats, args.baseline_steps,
                                         args.top_k, args.top_p)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
