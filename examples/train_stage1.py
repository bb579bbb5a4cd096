"""Stage-1 trainer on the MI355X path with the reference's command line.

Mirrors /root/reference/train_vqvae.py:209-237 (flags), :144-206 (main: model, optimizer, optional
CycleScheduler, --resume, checkpoint every 10 epochs as checkpoint/vqvae_{epoch:03d}.pt in the
reference's state_dict format) and :27-141 (per-step: recon MSE + 0.25 * latent, running mse
aggregated over ranks).  The re-ID parts of the fork are out of scope.  Data: a directory of .npy
image batches -- uint8 [N,H,W,3] pixels as an image decoder leaves them (pinned-memory prefetch on a copy
stream, ToTensor + Normalize + CenterCrop(--size) on the GPU inside the step; --norm picks the statistics:
half = 0.5 / 0.5 as extract_code.py:52, imagenet = those of train_vqvae.py:154), or [N,3,H,W] float32,
already normalised -- or, without --path, synthetic images: N(0,1) floats, with --dtype uint8 random pixels
through the 8-bit path (there is no torchvision / dataset access in this environment).

Every rank runs the SAME number of steps: the batches found under --path are dealt round-robin and the
remainder that would give some ranks one step more is dropped (what DistributedSampler's equal shards do for
the reference), and the CycleScheduler's n_iter is that per-rank count x epochs (train_vqvae.py:189-195).

    python examples/train_stage1.py --size 256 --batch_size 32 --epoch 1 --iters 50
    python examples/train_stage1.py --size 256 --batch_size 32 --epoch 1 --path /data/ffhq_u8 --norm half
    python examples/train_stage1.py ... --val_path /data/ffhq_val_u8 --eval_every 500 --sample_every 100

--val_path DIR (same file format as --path) with --eval_every N: every N steps the held-out set goes through
Stage1Trainer.evaluate -- its batches dealt over the ranks, totals summed -- and rank 0 prints mse, latent, perplexity
and used codes of both levels.  --sample_every N: rank 0 writes the reference's sample grid (train_vqvae.py:120-139:
the first min(batch, 25) inputs over their reconstructions, nrow = len(sample)) to sample/{epoch+1:05d}_{i:05d}.png.
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_stage1.py ...

--clip_grad_norm X clips the global gradient norm to X on the device (the printed line gains gnorm:, the norm before
clipping; a step whose norm is not finite is skipped and counted, the count is printed at the end).  --ema_decay D keeps
Polyak-averaged weights: every save also writes vqvae_<NNN>_ema.pt, the reference's file with the averaged weights (and the
codebooks as they are), and the held-out line is printed for both sets of weights.

--code_restart THRESHOLD restarts dead codes (Stage1Trainer.set_code_restart): from step --code_restart_start on, a code
whose EMA cluster size is below THRESHOLD is replaced by an encoder output of the current batch, on the device; the
periodic line and the held-out line then show the codes restarted so far at both levels.
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vqvae2_amd  # noqa: E402
from vqvae2_amd import distributed as dist  # noqa: E402


def plan_batches(args, rank, world):
    """-> list of (file, first row) this rank trains on per epoch (None = synthetic), equal length on every rank."""
    if not args.path:
        return [None] * args.iters
    every = []
    for f in sorted(glob.glob(os.path.join(args.path, "*.npy"))):
        rows = np.load(f, mmap_mode="r").shape[0]
        every += [(f, i) for i in range(0, rows - args.batch_size + 1, args.batch_size)]
    common = len(every) // world
    if common == 0:
        raise SystemExit(f"{len(every)} batches of {args.batch_size} under {args.path}: fewer than the {world} ranks")
    return every[rank::world][:common]


def load_batch(item, args, gen, device):
    if item is None:
        return torch.randn(args.batch_size, 3, args.size, args.size, generator=gen).to(device)
    f, i = item
    return torch.from_numpy(np.ascontiguousarray(np.load(f, mmap_mode="r")[i:i + args.batch_size])).float().to(device)


NORMS = {"half": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),                       # extract_code.py:52
         "imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))}       # train_vqvae.py:154


def data_is_uint8(args, plan):
    if not args.path:
        return args.dtype == "uint8"
    return np.load(plan[0][0], mmap_mode="r").dtype == np.uint8


def host_u8_batches(args, plan, epochs, gen):
    """Host side of the 8-bit path: every batch of every remaining epoch, in the order the loop consumes them."""
    for _ in range(epochs):
        for item in plan:
            if item is None:
                yield torch.randint(0, 256, (args.batch_size, args.size, args.size, 3), dtype=torch.uint8, generator=gen)
            else:
                f, i = item
                yield np.load(f, mmap_mode="r")[i:i + args.batch_size]      # copied once, into pinned memory


def plan_val_batches(args, rank, world):
    """Every image under --val_path in batches of at most --batch_size (a file's ragged tail is a short batch, as in
    examples/eval_stage1.py), dealt round-robin; ranks may get one batch more or less (the totals are summed)."""
    every = []
    for f in sorted(glob.glob(os.path.join(args.val_path, "*.npy"))):
        rows = np.load(f, mmap_mode="r").shape[0]
        every += [(f, i) for i in range(0, rows, args.batch_size)]
    if not every:
        raise SystemExit(f"no images under {args.val_path}")
    return every[rank::world]


def val_batches(args, plan, device):
    for f, i in plan:
        a = np.ascontiguousarray(np.load(f, mmap_mode="r")[i:i + args.batch_size])
        t = torch.from_numpy(a)
        yield (t if a.dtype == np.uint8 else t.float()).to(device)


def print_validation(epoch, i, r, restarted=None):
    print(f"epoch: {epoch + 1}; it {i}; val images: {r['images']}; val mse: {r['mse']:.5f}; val latent: {r['latent']:.3f}; "
          f"perplexity t/b: {r['perplexity_t']:.1f}/{r['perplexity_b']:.1f}; "
          f"used codes t/b: {r['used_t']}/{r['used_b']} of {r['n_embed']}"
          + (f"; psnr: {r['psnr']:.2f} dB; ssim: {r['ssim']:.4f}" if "psnr" in r else "") + restarted_text(restarted), flush=True)


def restarted_text(totals):
    return "" if totals is None else "; restarted codes: " + "/".join(str(v) for v in totals)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_gpu", type=int, default=1)            # kept for CLI parity; world size comes from the launcher
    ap.add_argument("--dist_url", default="env://")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--epoch", type=int, default=560)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--sched", type=str)
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--resume", "-r", default="", type=str)
    ap.add_argument("--path", type=str, default="")
    ap.add_argument("--iters", type=int, default=100, help="synthetic batches per epoch when --path is not given")
    ap.add_argument("--out", default="checkpoint")
    ap.add_argument("--norm", choices=sorted(NORMS), default="half", help="statistics for uint8 data")
    ap.add_argument("--dtype", choices=("float32", "uint8"), default="float32", help="what the synthetic run draws")
    ap.add_argument("--val_path", type=str, default="", help="held-out batches, same file format as --path")
    ap.add_argument("--eval_every", type=int, default=0, help="steps between evaluations of --val_path (0 = never)")
    ap.add_argument("--sample_every", type=int, default=0, help="steps between sample grids under sample/ (0 = never)")
    ap.add_argument("--image_metrics", action="store_true",
                    help="with --val_path: also PSNR and SSIM of the 8-bit reconstructions of the held-out set")
    ap.add_argument("--clip_grad_norm", type=float, default=None, help="clip the global gradient norm to this value")
    ap.add_argument("--ema_decay", type=float, default=None, help="decay of the Polyak-averaged weights")
    ap.add_argument("--code_restart", type=float, default=None, metavar="THRESHOLD",
                    help="restart codes whose EMA cluster size falls below THRESHOLD from encoder outputs (default: off)")
    ap.add_argument("--code_restart_start", type=int, default=0, metavar="STEPS", help="first step that may restart a code")
    args = ap.parse_args(argv)
    if args.eval_every and not args.val_path:
        raise SystemExit("--eval_every needs --val_path")
    return args


def main(argv=None):
    args = parse_args(argv)

    rank, local_rank, world = dist.bringup("nccl")             # launch.py:52-92 (RCCL group + device binding)
    device = torch.device("cuda", local_rank)

    # every rank may build its model from its own RNG state: the trainer broadcasts rank 0's (DDP, train_vqvae.py:166-171)
    model = vqvae2_amd.VQVAE().to(device)
    plan = plan_batches(args, rank, world)
    u8 = data_is_uint8(args, plan)
    # (float batches are already normalised: the normaliser then only says which statistics the sample grid inverts)
    normalizer = vqvae2_amd.ImageNormalizer(*NORMS[args.norm], layout="hwc", crop=(args.size, args.size)) \
        if (u8 or args.sample_every or args.eval_every) else None
    val_plan = plan_val_batches(args, rank, world) if args.eval_every else None
    trainer = vqvae2_amd.Stage1Trainer(model, lr=args.lr, sched=args.sched, n_iter=len(plan) * args.epoch,
                                       normalizer=normalizer, clip_grad_norm=args.clip_grad_norm, ema_decay=args.ema_decay)
    if args.code_restart is not None:
        trainer.set_code_restart(args.code_restart, start=args.code_restart_start)
    restarted = (lambda: trainer.restarted_codes()) if args.code_restart is not None else (lambda: None)
    first_epoch = 0
    if args.resume:                                            # train_vqvae.py:173-182
        sd = torch.load(args.resume, map_location=device, weights_only=True)
        trainer.load_state_dict(sd)                            # bare model state_dict or a trainer checkpoint
        first_epoch = int(sd.get("epoch", 0)) if "model" in sd else 0
        if dist.is_primary():
            print(f"==> loaded checkpoint {args.resume} (epoch {first_epoch})")

    gen = torch.Generator(device="cpu").manual_seed(1234 + rank)
    feed = vqvae2_amd.HostBatchPrefetcher(host_u8_batches(args, plan, args.epoch - first_epoch, gen), device) if u8 else None
    for epoch in range(first_epoch, args.epoch):
        mse_sum = torch.zeros(2, device=device)                # (sum of recon * batch, count)
        for i, item in enumerate(plan):
            img = next(feed) if u8 else load_batch(item, args, gen, device)
            out = trainer.step(img)
            mse_sum[0] += out["recon"] * img.shape[0]
            mse_sum[1] += img.shape[0]
            if args.eval_every and (i + 1) % args.eval_every == 0:       # every rank: result() sums over the group
                evaluate = trainer.evaluate_image_metrics if args.image_metrics else trainer.evaluate
                r = evaluate(val_batches(args, val_plan, device))
                if dist.is_primary():
                    print_validation(epoch, i, r, restarted())
                if args.ema_decay is not None:
                    with trainer.averaged_weights():
                        r = evaluate(val_batches(args, val_plan, device))
                    if dist.is_primary():
                        print("averaged weights -- ", end="")
                        print_validation(epoch, i, r, restarted())
            if args.sample_every and i % args.sample_every == 0 and dist.is_primary():   # train_vqvae.py:120-139
                grid = trainer.sample_grid(img[:min(img.shape[0], 25)].contiguous())
                os.makedirs("sample", exist_ok=True)
                vqvae2_amd.save_u8_image(grid, f"sample/{str(epoch + 1).zfill(5)}_{str(i).zfill(5)}.png", "hwc")
            if i % 25 == 0:
                agg = mse_sum.clone()
                dist.all_reduce(agg)                           # replaces the pickled all_gather of train_vqvae.py:93-100
                if dist.is_primary():
                    lr = trainer.optimizer.param_groups[0]["lr"]
                    print(f"epoch: {epoch + 1}; it {i}; mse: {float(out['recon']):.5f}; "
                          f"latent: {float(out['latent']):.3f}; avg mse: {float(agg[0] / agg[1]):.5f}; lr: {lr:.5f}"
                          + (f"; gnorm: {float(out['grad_norm']):.5f}" if "grad_norm" in out else "")
                          + restarted_text(restarted()), flush=True)
        if dist.is_primary() and (epoch % 10 == 0 or epoch == args.epoch - 1):   # train_vqvae.py:205-206
            os.makedirs(args.out, exist_ok=True)
            tag = str(epoch + 1).zfill(3)
            torch.save(model.state_dict(), os.path.join(args.out, f"vqvae_{tag}.pt"))       # the reference's file
            if args.ema_decay is not None:
                torch.save(trainer.averaged_state_dict(), os.path.join(args.out, f"vqvae_{tag}_ema.pt"))
            full = trainer.state_dict()
            full["epoch"] = epoch + 1
            torch.save(full, os.path.join(args.out, f"trainer_{tag}.pt"))                   # exact-resume extras
    if dist.is_primary() and args.clip_grad_norm is not None:
        print(f"skipped steps (non-finite gradient norm): {trainer.skipped_steps()}")
    if feed is not None:
        feed.close()
    dist.synchronize()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
