"""Rate of the held-out evaluation path and of the 8-bit export kernel, BASELINE configs[1] (default VQVAE, 256x256),
batch 32, input resident in HBM.  One JSON line per measurement:

  forward (reconstruction, eval)    the same eval forward scripts/bench_infer.py times (the yardstick: it exists in the
                                    parent commit), here through model(img)
  Evaluator.update float            forward_nhwc + per-image SSE + two histograms + accumulate, float32 NCHW input
  Evaluator.update uint8            the same from a device uint8 batch (plus vq2_u8_to_nhwc4)
  Evaluator.update uint8 + metrics  the same with image_metrics=True (vq2_image_metrics and its accumulate on top)
  nhwc_to_u8 hwc / chw              vq2_nhwc_to_u8 alone by HIP events, against its byte floor N*H*W*(16 + C) and
                                    against the nhwc_to_nchw launch it stands in for (N*H*W*(16 + 4C) bytes)
  image_metrics                     vq2_image_metrics alone (both of its kernels) by HIP events, C = 3, against its byte
                                    floor 2*N*H*W*16

    python scripts/bench_eval.py            (B=32 REPEATS=3 by default)
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import vqvae2_amd
from vqvae2_amd import ops
from oracle import vqvae_oracle as O

dev = torch.device("cuda:0")
B = int(os.environ.get("B", "32"))
REPEATS = int(os.environ.get("REPEATS", "3"))
m = vqvae2_amd.VQVAE()
m.load_state_dict(O.make_state(O.DEFAULT, 1234))
m.to(dev).eval()
img = O.make_images(B, 256, 1234).to(dev)
u8 = torch.randint(0, 256, (B, 256, 256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
norm = vqvae2_amd.ImageNormalizer(layout="hwc")
ev = vqvae2_amd.Evaluator(m, norm)
ev_metrics = vqvae2_amd.Evaluator(m, norm, image_metrics=True)


def timed(fn, steps=30, warmup=10):
    with torch.no_grad():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def by_events(fn, steps=200, warmup=20):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e-3


for rep in range(REPEATS):
    for name, fn in (("forward (reconstruction, eval)", lambda: m(img)),
                     ("Evaluator.update float", lambda: ev.update(img)),
                     ("Evaluator.update uint8", lambda: ev.update(u8)),
                     ("Evaluator.update uint8 + metrics", lambda: ev_metrics.update(u8))):
        dt = timed(fn)
        print(json.dumps({"path": name, "repeat": rep, "batch": B, "ms": round(dt * 1e3, 3),
                          "images_per_s": round(B / dt, 1)}), flush=True)
assert ev.result()["images"] == B * 40 * 2 * REPEATS
r = ev_metrics.result()
assert r["images"] == B * 40 * REPEATS
print(json.dumps({"metrics of the timed batches": {k: r[k] for k in ("psnr", "ssim", "mse_u8")}}), flush=True)

x = ops.to_nhwc(img)
xb = norm(u8)
d = norm.inverse()
pix = B * 256 * 256
nchw = torch.empty((B, 3, 256, 256), device=dev)
for rep in range(REPEATS):
    for name, fn, nbytes in (("nhwc_to_u8 hwc", lambda: ops.nhwc_to_u8(x, 3, d.inv_s, d.m, "hwc"), pix * 19),
                             ("nhwc_to_u8 chw", lambda: ops.nhwc_to_u8(x, 3, d.inv_s, d.m, "chw"), pix * 19),
                             ("nhwc_to_nchw (float, for comparison)", lambda: ops.from_nhwc(x, 3), pix * 28),
                             ("image_metrics", lambda: ops.image_metrics(x, xb, 3, d.inv_s, d.m), pix * 32)):
        dt = by_events(fn)
        print(json.dumps({"kernel": name, "repeat": rep, "batch": B, "us": round(dt * 1e6, 2), "bytes": nbytes,
                          "TB/s": round(nbytes / dt / 1e12, 3), "floor_us_at_6.3TB/s": round(nbytes / 6.3e12 * 1e6, 2)}),
              flush=True)
