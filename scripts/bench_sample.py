"""Sampling from the PixelSNAIL prior on one MI355X: PriorSampler (row- or pixel-incremental) against the reference's loop on
this package's modules, at the top prior's real size and at the bottom prior's with a reduced row count.

    python scripts/bench_sample.py [--batch 8] [--bottom_rows 8] [--top_k K] [--top_p P] [--stepping row|pixel|both]
                                   [--skip_baseline] [--skip_top] [--skip_bottom] [--out FILE.json]

--top_k / --top_p time the sampler with the truncated draw (vq2_sample_filtered in place of vq2_sample_categorical, one launch per
step either way); the baseline loop is the reference's and has no such filter.
--stepping both builds one sampler per mode on the same model and alternates them map by map in one process, so that both see
the same card in the same state; the result then holds one entry per mode and their ratio, and goes to
profiles/sample_pixel.json unless --out says otherwise (row alone keeps profiles/sample.json).

Priors (random weights; the time does not depend on them):
    top     PixelSNAIL([32, 32], 512, 256, 5, 4, 4, 256), no condition
    bottom  PixelSNAIL([64, 64], 512, 256, 5, 4, 4, 256, attention=False, n_cond_res_block=3, cond_res_channel=256),
            conditioned on a [32, 32] map of top codes; the first --bottom_rows rows only (a full map is 4,096 steps)

Measured, with a host clock around work that ends in a device synchronise (no GPU: fails):
    sampler   one warm-up map (or row set), then the median and spread of --repeats maps: seconds per sampled map
    plan      seconds to build the sampler's plan for (batch, rows): buffers, histories and the recorded programs, timed on
              its own with a device synchronise, before the warm-up map
    baseline  the reference's loop body -- model(row[:, :i + 1], condition, cache), torch.softmax, torch.multinomial, the
              write -- timed per step at the first, a middle and the last row (two warm-up steps, then --baseline_steps steps
              each), and integrated over the map by the trapezoid rule over rows: an ESTIMATE of the loop's time, which
              avoids running its 1,024 full-model passes
    launches  per sampler step, counted from the recorded program of a middle row plus the draw: library calls, and kernel
              launches (a vq2_conv_fwd_row or vq2_conv_fwd_col call is two kernels, every other call of the step one)
    column conv  (pixel or both) vq2_conv_fwd_col alone, HIP events around --kernel_launches back-to-back launches, for the
              'causal' 5 x 5 layers 256 -> 256 and 256 -> 512 at 8 and 64 images, pixel (16, 16) of a 32 x 32 map; the
              floor is the bytes of the panel's computed taps at 6.3 TB/s
Not measured: kernel times inside a step (scripts/trace_step.sh style profiler runs are separate), the full 64 x 64 bottom
map, peak memory, more than one GPU."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_SECOND = 6.3e12


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


def baseline_estimate(model, batch, rows, width, condition, baseline_steps):
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
    return per_step, total


def bench(name, model, batch, rows, condition, repeats, baseline_steps, top_k=0, top_p=1.0, steppings=("row",)):
    import vqvae2_amd
    width = model.background.shape[3]
    samplers = {s: vqvae2_amd.PriorSampler(model, stepping=s) for s in steppings}
    runs = {s: (lambda sampler=sampler: sampler.sample(batch, 1.0, condition, seed=1, rows=rows, top_k=top_k, top_p=top_p))
            for s, sampler in samplers.items()}
    with torch.no_grad():
        build = {s: sync_time(lambda s=s: samplers[s]._plan_for(batch, rows, condition)) for s in steppings}
    for s in steppings:
        sync_time(runs[s])                                  # the warm-up map
    times = {s: [] for s in steppings}
    for _ in range(repeats):                                # alternating: both modes see the card in the same state
        for s in steppings:
            times[s].append(sync_time(runs[s]))
    res = {"batch": batch, "rows": rows, "width": width, "steps": rows * width, "top_k": top_k, "top_p": top_p}
    for s in steppings:
        plan = samplers[s]._plan[1]
        calls = plan.step_programs[rows // 2].calls
        two_kernels = sum(1 for call in calls if call[2] in ("conv_fwd_row", "conv_fwd_col"))
        med = statistics.median(times[s])
        entry = {
            "sampler_seconds_per_map": {"median": med, "min": min(times[s]), "max": max(times[s]), "repeats": repeats},
            "sampler_ms_per_step": 1e3 * med / (rows * width),
            "sampler_library_calls_per_step": len(calls) + 1,
            "sampler_kernel_launches_per_step": len(calls) + two_kernels + 1,
            "sampler_multi_row_conv_calls_per_step": two_kernels,
            "plan_build_seconds": build[s],
        }
        if len(steppings) == 1:
            entry["sampler_row_conv_calls_per_step"] = entry.pop("sampler_multi_row_conv_calls_per_step")
            res.update(entry)
        else:
            res[s] = entry
    if len(steppings) == 2:
        res["row_over_pixel_ms_per_step"] = res["row"]["sampler_ms_per_step"] / res["pixel"]["sampler_ms_per_step"]
    if baseline_steps > 0:
        per_step, total = baseline_estimate(model, batch, rows, width, condition, baseline_steps)
        res.update({"baseline_steps_per_timed_row": baseline_steps,
                    "baseline_ms_per_step_at_row": {str(i): 1e3 * t for i, t in per_step.items()},
                    "baseline_seconds_per_map_estimate": total})
        if len(steppings) == 1:
            res["speedup_estimate"] = total / res["sampler_seconds_per_map"]["median"]
        else:
            for s in steppings:
                res[s]["speedup_estimate"] = total / res[s]["sampler_seconds_per_map"]["median"]
    print(name, json.dumps(res))
    return res


def column_conv_times(launches):
    """vq2_conv_fwd_col on its own: milliseconds per launch from two HIP events around `launches` launches."""
    import vqvae2_amd
    from vqvae2_amd import ops
    from vqvae2_amd._lib import lib, check
    out = []
    h = w = 32
    for cin, cout in ((256, 256), (256, 512)):
        spec = ops.ConvSpec.geom(cin, cout, 5, 5, 4, 2)
        weight = torch.randn(cout, cin, 5, 5, device="cuda") / (25 * cin) ** 0.5
        weight[:, :, -1, 2:] = 0
        wp = ops.packed_weight(spec, weight, ops.PACK_FWD)
        bias = torch.randn(cout, device="cuda")
        taps = 5 * 5 - 3
        floor = taps * cin * cout * 4 / HBM_BYTES_PER_SECOND
        for n in (8, 64):
            d = ops._desc(spec, n, h, w, cin, cout)
            nbytes = lib.vq2_conv_fwd_col_workspace_bytes(ctypes.byref(d), 8)
            ws = torch.empty(nbytes // 4, device="cuda")
            hist = torch.randn(h, n, w, cin, device="cuda")
            y = torch.empty(n, cout, device="cuda")

            def launch():
                check(lib.vq2_conv_fwd_col(ctypes.byref(d), 16, 16, w * cin, n * w * cin, 8, ops._p(hist), ops._p(wp), ops._p(bias),
                                           None, 0, ops._p(y), ops._p(ws), nbytes, ops._stream()), "conv_fwd_col")

            for _ in range(10):
                launch()
            reps = []
            for _ in range(3):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(launches):
                    launch()
                b.record()
                torch.cuda.synchronize()
                reps.append(a.elapsed_time(b) * 1e-3 / launches)
            sec = statistics.median(reps)
            out.append({"layer": "causal 5x5 %d -> %d" % (cin, cout), "images": n, "launches": launches,
                        "splits": nbytes // (n * cout * 4), "panel_bytes_of_computed_taps": taps * cin * cout * 4,
                        "seconds_per_launch": {"median": sec, "min": min(reps), "max": max(reps)},
                        "floor_seconds_at_6.3_TB_per_s": floor, "fraction_of_floor": floor / sec})
            print("conv_fwd_col", json.dumps(out[-1]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--bottom_rows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline_steps", type=int, default=40)
    ap.add_argument("--skip_baseline", action="store_true")
    ap.add_argument("--skip_top", action="store_true")
    ap.add_argument("--skip_bottom", action="store_true")
    ap.add_argument("--top_k", type=int, default=0)
    ap.add_argument("--top_p", type=float, default=1.0)
    ap.add_argument("--stepping", choices=["row", "pixel", "both"], default="row")
    ap.add_argument("--kernel_launches", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample.py needs the MI355X")
    import vqvae2_amd
    torch.manual_seed(0)
    steppings = ("row", "pixel") if args.stepping == "both" else (args.stepping,)
    out = args.out or os.path.join(ROOT, "profiles", "sample.json" if args.stepping == "row" else "sample_pixel.json")
    baseline_steps = 0 if args.skip_baseline else args.baseline_steps
    doc = {"device": torch.cuda.get_device_name(0), "method": "host clock around device-synchronised work; baseline integrated "
           "from per-step times at the first, middle and last row (an estimate)"}
    if not args.skip_top:
        top = vqvae2_amd.PixelSNAIL([32, 32], 512, 256, 5, 4, 4, 256).cuda().eval()
        doc["top"] = bench("top", top, args.batch, 32, None, args.repeats, baseline_steps, args.top_k, args.top_p, steppings)
        del top
    if not args.skip_bottom:
        bottom = vqvae2_amd.PixelSNAIL([64, 64], 512, 256, 5, 4, 4, 256, attention=False, n_cond_res_block=3,
                                       cond_res_channel=256).cuda().eval()
        cond = torch.randint(0, 512, (args.batch, 32, 32), device="cuda")
        doc["bottom_first_rows"] = bench("bottom", bottom, args.batch, args.bottom_rows, cond, args.repeats, baseline_steps,
                                         args.top_k, args.top_p, steppings)
        del bottom
    if "pixel" in steppings:
        doc["conv_fwd_col"] = column_conv_times(args.kernel_launches)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
