"""What the dead-code restart costs per stage-1 training step, and its two launches alone.

    python scripts/bench_code_restart.py [--out profiles/code_restart.json] [--repeats 3] [--steps 20] [--tiny]

Steps: the default VQVAE at 256x256, batch 32, with n_embed 512 (bench.py's configs[1]) and 8192 (configs[3]), each with
the feature off and on (threshold 1.0, start 0).  One process, the batch resident on the device; the two trainers of a
model are built once and ALTERNATED -- a window of `steps` steps of "off" between two HIP events, then one of "on",
`repeats` rounds after a warm-up -- so that clock and temperature drift lands on both alike.  The file keeps every window
and the minimum and maximum (ms per step), and the codes restarted per quantizer over the run: on random images and a
random codebook many codes are dead, so the "on" figure is that of a run in which the restart is busy.

Kernels: vq2_vq_restart_candidates and vq2_vq_ema_update_restart alone at (D, K, M) = (64, 512, 32768) and
(64, 8192, 32768), half the codes dead, min .. max of `repeats` windows of 50 launches, beside vq2_vq_ema_update_prepare
on the same state.

--bench A B: the parent-commit comparison -- `python bench.py --gpus 1` run as a child process in directory A (this
tree) and B (a build of the parent commit), alternated `repeats` times; the six step times go into the file."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, n):
    """ms per call of n calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def summary(v):
    return {"ms_min": min(v), "ms_max": max(v), "windows": v}


def steps(amd, n_embed, tiny, repeats, n_steps, warmup):
    from oracle import vqvae_oracle as O
    size, batch = (256, 32) if not tiny else (64, 4)
    state = amd.VQVAE(n_embed=n_embed).state_dict()
    img = O.make_images(batch, size, 1234).cuda()
    trainers = {}
    for name in ("off", "on"):
        m = amd.VQVAE(n_embed=n_embed)
        m.load_state_dict(state)
        trainers[name] = amd.Stage1Trainer(m.cuda(), lr=3e-4)
    trainers["on"].set_code_restart(1.0, start=0)
    seen = {k: [] for k in trainers}
    for tr in trainers.values():
        window(lambda: tr.step(img), warmup)
    for _ in range(repeats):
        for k, tr in trainers.items():
            seen[k].append(window(lambda: tr.step(img), n_steps))
    out = {k: summary(v) for k, v in seen.items()}
    out["on"]["restarted_total_per_quantizer"] = trainers["on"].restarted_codes()
    out["on"]["steps_run"] = warmup + repeats * n_steps
    return out


def kernels(amd, d, k, m, repeats):
    ops = amd.ops
    g = torch.Generator().manual_seed(k)
    x = torch.randn(m, 1, 1, d, generator=g).cuda()
    embed = torch.randn(d, k, generator=g).cuda()
    cs0 = torch.where(torch.arange(k) % 2 == 0, torch.tensor(0.5), torch.tensor(3.0)).cuda()      # half the codes dead
    ea0 = embed * cs0[None, :]
    stats = ops.vq_stats_alloc(k, d, x.device)
    counts, sums_t = ops.vq_stats_views(stats, k, d)
    counts.fill_(0.0)
    sums_t.fill_(0.0)
    cand = torch.empty(k * d, device=x.device)
    counter = torch.zeros(2, device=x.device, dtype=torch.int64)
    prep = (torch.empty((k, d), device=x.device), torch.empty(k, device=x.device))
    cs, ea = cs0.clone(), ea0.clone()

    def reset():
        cs.copy_(cs0)
        ea.copy_(ea0)

    def update_restart():
        reset()
        ops.vq_ema_update_restart(embed, cs, ea, stats, cand, 0.99, 1e-5, 1.0, counter, prep)

    def update_plain():
        reset()
        ops.vq_ema_update(embed, cs, ea, stats, 0.99, 1e-5, prep)

    out = {"D": d, "K": k, "M": m}
    for name, fn in (("state_reset_alone", reset), ("vq2_vq_restart_candidates", lambda: ops.vq_restart_candidates(x, k, cand, 1, 2, 0)),
                     ("reset+vq2_vq_ema_update_restart", update_restart), ("reset+vq2_vq_ema_update_prepare", update_plain)):
        window(fn, 10)
        out[name] = summary([window(fn, 50) for _ in range(repeats)])
    torch.cuda.synchronize()
    out["restarted_by_the_last_call"] = int(counter[0])
    return out


def bench_ab(here, parent, repeats):
    """bench.py's one JSON line from each tree in turn; a fresh child process per run."""
    runs = {"this_tree": [], "parent": []}
    for _ in range(repeats):
        for name, cwd in (("this_tree", here), ("parent", parent)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"], cwd=cwd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"bench.py failed in {cwd}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs[name].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    return runs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "code_restart.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--bench", nargs=2, metavar=("THIS", "PARENT"), default=None,
                    help="also alternate bench.py --gpus 1 between these two checkouts")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_code_restart.py measures on the GPU; none is visible")
    import vqvae2_amd as amd
    torch.manual_seed(0)
    result = {"tiny": args.tiny, "repeats": args.repeats, "steps_per_window": args.steps}
    for key, n_embed in (("configs1_n_embed_512", 512), ("configs3_n_embed_8192", 8192)):
        result[key] = steps(amd, n_embed if not args.tiny else n_embed // 8, args.tiny, args.repeats, args.steps, args.warmup)
        torch.cuda.empty_cache()
    m = 32768 if not args.tiny else 512
    result["kernels"] = [kernels(amd, 64, k, m, args.repeats) for k in (512, 8192)]
    if args.bench:
        result["bench_py"] = bench_ab(args.bench[0], args.bench[1], args.repeats)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "bench_py"}))
    if args.bench:
        print(json.dumps({k: [r["ms_per_step"] for r in v] for k, v in result["bench_py"].items()}))


if __name__ == "__main__":
    main()
