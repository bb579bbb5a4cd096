"""bench_input.py -- images/sec of the stage-1 train step INCLUDING the way the batch reaches HBM (bench.py times the
step with the batch already resident).  configs[1]: default VQ-VAE-2, 256x256, batch 32, one GPU, one process.

    python scripts/bench_input.py [--steps 100] [--warmup 20] [--rounds 3] > profiles/input_path.json

modes, alternated inside the process, the whole sequence repeated --rounds times (the spread between the repeats of
`resident` is the noise floor the other differences are read against):
  resident          fp32 NCHW batch already in HBM (what bench.py times)
  host_f32_sync     host fp32 batch, torch.from_numpy(..).to(device) every step: pageable, synchronous, 25 MB
  host_u8_prefetch  host uint8 HWC batches -> HostBatchPrefetcher (pinned, copy stream, 6.3 MB) -> step(uint8), which
                    normalises on the GPU (depth 2; host_u8_prefetch_d3: depth 3)
A pool of --pool distinct seeded host batches is cycled, so no mode lives on one cached page.  The first two modes use
only what the package offered before the 8-bit path existed: the same script on an older checkout gives their baseline
(the uint8 modes are then reported as null).  After the timed windows a separate pass with the library's profiler on
records the time of the conversion launches (u8_to_nhwc4 and the nchw_to_nhwc4 launch it replaces).  One JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, BATCH = 256, 32
MEAN = STD = (0.5, 0.5, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pool", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input.py needs an MI355X; there is no CPU fallback for the product path")
    import vqvae2_amd
    from oracle import vqvae_oracle as O
    dev = torch.device("cuda", 0)
    lib = vqvae2_amd._lib.lib
    has_u8 = hasattr(vqvae2_amd, "HostBatchPrefetcher")

    gen = np.random.default_rng(1234)
    host_u8 = [gen.integers(0, 256, (BATCH, SIZE, SIZE, 3), dtype=np.uint8) for _ in range(args.pool)]
    # the reference loader's arithmetic on the host (ToTensor + Normalize), NCHW: what the float modes are handed
    m, s = torch.tensor(MEAN)[None, :, None, None], torch.tensor(STD)[None, :, None, None]
    host_f32 = [torch.from_numpy(b).permute(0, 3, 1, 2).float().div(255).sub_(m).div_(s).contiguous().numpy() for b in host_u8]
    resident = [torch.from_numpy(b).to(dev) for b in host_f32]

    model = vqvae2_amd.VQVAE()
    model.load_state_dict(O.make_state(O.DEFAULT, 1234))
    model.to(dev)
    kw = {"normalizer": vqvae2_amd.ImageNormalizer(MEAN, STD, layout="hwc")} if has_u8 else {}
    trainer = vqvae2_amd.Stage1Trainer(model, lr=3e-4, **kw)

    def run_resident(n):
        for i in range(n):
            trainer.step(resident[i % args.pool])

    def run_host_f32(n):
        for i in range(n):
            trainer.step(torch.from_numpy(host_f32[i % args.pool]).to(dev))

    def run_u8(n, depth):
        with vqvae2_amd.HostBatchPrefetcher((host_u8[i % args.pool] for i in range(n)), dev, depth=depth) as feed:
            for batch in feed:
                trainer.step(batch)

    modes = {"resident": run_resident, "host_f32_sync": run_host_f32}
    if has_u8:
        modes["host_u8_prefetch"] = lambda n: run_u8(n, 2)
        modes["host_u8_prefetch_d3"] = lambda n: run_u8(n, 3)

    for fn in modes.values():
        fn(args.warmup)
    torch.cuda.synchronize()
    rates = {k: [] for k in modes}
    for _ in range(args.rounds):
        for name, fn in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.steps)
            torch.cuda.synchronize()
            rates[name].append(BATCH * args.steps / (time.perf_counter() - t0))

    # conversion launches, from the library's own labels (events around every instrumented launch: not a step timing)
    lib.vq2_prof_enable(1)
    run_resident(8)
    if has_u8:
        run_u8(8, 2)
    torch.cuda.synchronize()
    lib.vq2_prof_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    assert lib.vq2_prof_report(buf, len(buf)) == 0
    kernels = {}
    for line in buf.value.decode().splitlines():
        name, n, ms, _, nbytes = line.split()
        if name.startswith(("u8_to_nhwc4|", "nchw_to_nhwc4|")):
            us = float(ms) * 1e3 / int(n)
            kernels[name] = {"launches": int(n), "us_per_launch": round(us, 2),
                             "algorithmic_gbps": round(float(nbytes) / int(n) / us / 1e3, 1)}

    def summary(v):
        return {"images_per_s": [round(x, 1) for x in v], "median": round(statistics.median(v), 1),
                "spread_pct": round(100.0 * (max(v) - min(v)) / statistics.median(v), 2)}

    line = {"metric": "images/sec VQ-VAE-2 256px train step by input path", "unit": "images/s",
            "config": {"image": SIZE, "batch": BATCH, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "pool": args.pool, "has_uint8_path": has_u8},
            "modes": {k: summary(v) for k, v in rates.items()},
            "noise_floor_pct": summary(rates["resident"])["spread_pct"],
            "conversion_kernels": kernels or None}
    for k in ("host_u8_prefetch", "host_u8_prefetch_d3"):
        line["modes"].setdefault(k, None)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
