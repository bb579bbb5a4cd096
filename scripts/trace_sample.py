"""A few sampling steps of the top prior for a kernel trace: kernel time summed over a step against the step's wall time.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python scripts/trace_sample.py --stepping pixel
    python scripts/trace_sample.py --summarise DIR/NAME_kernel_stats.csv --steps 256

The run draws the first --rows rows of a batch of top-prior maps twice (one warm-up, one timed with a host clock around a
device synchronise) and prints the steps it made and the timed wall time per step; under the profiler that wall time includes
the tracer's cost on the host, so the untraced figure of scripts/bench_sample.py is the one to quote.  --summarise folds the
profiler's per-kernel statistics into per-step figures: calls and microseconds per step for every kernel, and their sum."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarise(path, steps):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])))
    rows.sort(key=lambda r: -r[2])
    total = sum(r[2] for r in rows)
    doc = {"steps": steps, "kernel_us_per_step": total / steps / 1e3, "launches_per_step": sum(r[1] for r in rows) / steps,
           "kernels": [{"name": n[:100], "calls_per_step": c / steps, "us_per_step": t / steps / 1e3, "us_per_call": t / c / 1e3}
                       for n, c, t in rows[:12]]}
    print(json.dumps(doc, indent=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stepping", choices=["row", "pixel"], default="row")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--summarise", metavar="KERNEL_STATS.csv")
    ap.add_argument("--steps", type=int, default=256, help="with --summarise: the steps the traced run made")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.steps)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trace_sample.py needs the MI355X")
    import vqvae2_amd
    torch.manual_seed(0)
    top = vqvae2_amd.PixelSNAIL([32, 32], 512, 256, 5, 4, 4, 256).cuda().eval()
    sampler = vqvae2_amd.PriorSampler(top, stepping=args.stepping)
    run = lambda: sampler.sample(args.batch, 1.0, None, seed=1, rows=args.rows)
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    steps = args.rows * 32
    print(json.dumps({"stepping": args.stepping, "batch": args.batch, "steps_traced": 2 * steps, "steps_timed": steps,
                      "wall_ms_per_step_while_traced_or_not": 1e3 * wall / steps}))


if __name__ == "__main__":
    main()
