"""What clip_grad_norm and ema_decay cost per training step, and the two kernels behind them alone.

    python scripts/bench_step_extras.py [--out profiles/step_extras.json] [--repeats 3] [--steps 20] [--tiny]

Steps: the Stage2 top prior PixelSNAIL([32, 32], 512, 256, 5, 4, 4, 256) at batch 32 and the stage-1 default VQVAE at
256x256, batch 32 (bench.py's configs[1]), each with the settings off / clip / ema / both.  The four trainers of a model
are built once and ALTERNATED inside one session -- repeat r times setting s, then the next setting, `repeats` rounds -- so
that clock and temperature drift lands on every setting alike; a window is `steps` steps between two HIP events after a
warm-up, and the file keeps the minimum and the maximum window per setting (ms per step), never a single figure.  "off"
runs exactly the launches of the parent path and has to sit inside bench.py's own spread.

Kernels: vq2_grad_norm (4n bytes read) and vq2_adam_step_ex with averaging ((5 + 4) * 4n bytes: five arrays read, four
written) over an arena of the top prior's size, min .. max of `repeats` windows of 50 launches, and the fraction of the
6.3 TB/s HBM floor each reaches."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12
SETTINGS = {"off": {}, "clip": {"clip_grad_norm": 1.0}, "ema": {"ema_decay": 0.9999},
            "both": {"clip_grad_norm": 1.0, "ema_decay": 0.9999}}


def window(fn, n):
    """ms per call of n calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(steppers, repeats, steps, warmup):
    for fn in steppers.values():
        window(fn, warmup)
    seen = {k: [] for k in steppers}
    for _ in range(repeats):
        for k, fn in steppers.items():
            seen[k].append(window(fn, steps))
    return {k: {"ms_per_step_min": min(v), "ms_per_step_max": max(v), "windows": v} for k, v in seen.items()}


def stage2_steppers(amd, tiny):
    shape, args, batch = ([32, 32], (512, 256, 5, 4, 4, 256), 32) if not tiny else ([8, 8], (32, 16, 5, 1, 1, 16), 2)
    state = amd.PixelSNAIL(shape, *args, dropout=0.1).state_dict()
    codes = torch.randint(0, args[0], (batch, *shape), generator=torch.Generator().manual_seed(1)).cuda()
    out, n = {}, 0
    for name, kw in SETTINGS.items():
        m = amd.PixelSNAIL(shape, *args, dropout=0.1)
        m.load_state_dict(state)
        tr = amd.Stage2Trainer(m.cuda().train(), "top", lr=3e-4, **kw)
        out[name], n = (lambda tr=tr: tr.step(codes)), tr.arena.n
    return out, n


def stage1_steppers(amd, tiny):
    from oracle import vqvae_oracle as O
    size, batch = (256, 32) if not tiny else (64, 4)
    state = amd.VQVAE().state_dict()
    img = O.make_images(batch, size, 1234).cuda()
    out = {}
    for name, kw in SETTINGS.items():
        m = amd.VQVAE()
        m.load_state_dict(state)
        tr = amd.Stage1Trainer(m.cuda(), lr=3e-4, **kw)
        out[name] = lambda tr=tr: tr.step(img)
    return out


def kernels(amd, n, repeats):
    lib, check, stream = amd._lib.lib, amd._lib.check, amd.ops._stream
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.randn(n, device="cuda")
    prm, m, v, avg = (torch.randn(n, device="cuda") for _ in range(4))
    v.abs_()
    ctl = torch.zeros(4, device="cuda")
    ws_bytes = lib.vq2_grad_norm_workspace_bytes(n)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device="cuda")
    norm = lambda: check(lib.vq2_grad_norm(p(g), n, 1.0, 1.0, p(ctl), p(ws), ws_bytes, stream()), "grad_norm")
    adam = lambda: check(lib.vq2_adam_step_ex(p(prm), p(g), p(m), p(v), p(avg), n, 3e-4, 0.9, 0.999, 1e-8, 1, 1.0, p(ctl),
                                              0.9999, stream()), "adam_step_ex")
    out = {}
    for name, fn, nbytes in (("vq2_grad_norm", norm, 4 * n), ("vq2_adam_step_ex+avg", adam, (5 + 4) * 4 * n)):
        window(fn, 10)
        ms = [window(fn, 50) for _ in range(repeats)]
        out[name] = {"n": n, "bytes": nbytes, "ms_min": min(ms), "ms_max": max(ms),
                     "fraction_of_hbm_floor_best": nbytes / HBM_BYTES_PER_S / (min(ms) * 1e-3),
                     "fraction_of_hbm_floor_worst": nbytes / HBM_BYTES_PER_S / (max(ms) * 1e-3)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_extras.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="toy models: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    import vqvae2_amd as amd
    torch.manual_seed(0)
    s2, n = stage2_steppers(amd, args.tiny)
    result = {"tiny": args.tiny, "repeats": args.repeats, "steps_per_window": args.steps,
              "hbm_floor_bytes_per_s": HBM_BYTES_PER_S,
              "stage2_top_batch32": alternate(s2, args.repeats, args.steps, args.warmup)}
    del s2
    torch.cuda.empty_cache()
    result["stage1_configs1"] = alternate(stage1_steppers(amd, args.tiny), args.repeats, args.steps, args.warmup)
    result["kernels"] = kernels(amd, n, args.repeats)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: ({s: [round(v["ms_per_step_min"], 4), round(v["ms_per_step_max"], 4)] for s, v in r.items()}
                          if k.startswith("stage") else r) for k, r in result.items() if isinstance(r, dict)}))


if __name__ == "__main__":
    main()
