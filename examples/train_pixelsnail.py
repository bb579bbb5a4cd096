"""Train a PixelSNAIL prior on extracted codes: the reference's train_pixelsnail.py on one MI355X or several.

    python examples/train_pixelsnail.py --hier top    [--batch 32 --epoch 420 --lr 3e-4 --sched cycle ...] CODES
    python examples/train_pixelsnail.py --hier bottom [...] CODES
    python -m torch.distributed.run --nproc-per-node N examples/train_pixelsnail.py [...] CODES

CODES is what examples/extract_code.py wrote (vqvae2_amd.codes.CodeDataset reads it).  The command line is the
reference's; `--amp` is accepted only as O0; `--precision bf16` (and bf16_wgrad, bf16_attn) is this path's reduced precision (bf16 conv and attention operands, see --help).  The reference wraps the model in nn.DataParallel; here
data parallelism is one process per GPU under torch.distributed.run: every rank takes its shard of each epoch (--batch is
per rank), Stage2Trainer all-reduces the gradients, and only the primary rank prints and saves.  Every epoch whose number
is 1 modulo 10, and the last, saves {'model': state_dict, 'args': args} as <ckpt_dir>/pixelsnail_<hier>_<NNN>.pt, the
reference's file, and beside it trainer_<hier>_<NNN>.pt: Stage2Trainer.state_dict() plus the epoch, which --resume
continues from exactly (model, Adam moments, schedule position).

Extra arguments of this script (all default to the reference's fixed values): --size H W of the top codes (the bottom codes
are twice that), --n_class, --n_block, --kernel_size, --max_steps to stop early, --ckpt_dir, --workers, --seed (the torch
generator is seeded with seed + rank: it draws the shuffle and the dropout seeds), --resume FILE, and --val_path CODES with
--eval_every N: every N steps each rank scores its share of the held-out codes (Stage2Trainer.evaluate: eval mode, no
dropout seed drawn, the training run itself unchanged) and the primary rank prints the totals.  N = 0, the default, is off.
--clip_grad_norm X clips the global gradient norm to X on the device (the printed line gains gnorm:, the norm before
clipping; a step whose norm is not finite is skipped and counted, the count is printed at the end).  --ema_decay D keeps
Polyak-averaged weights: every save also writes pixelsnail_<hier>_<NNN>_ema.pt, the same file with the averaged weights
(sample.py and eval_pixelsnail.py load it like any checkpoint), and the held-out line is printed for both sets of weights.
--n_label N (0, the default: off) trains a class-conditional prior: the label of a row is the directory part of its stored
file name (class_dir/name.png), the class names are sorted as ImageFolder numbers them (at most N of them) and written into
the checkpoint's args as class_names; the held-out codes use the same list, a class it does not hold gets label -1."""
import argparse
import os
import sys

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--batch', type=int, default=32)
    parser.add_argument('--epoch', type=int, default=420)
    parser.add_argument('--hier', type=str, default='top', choices=['top', 'bottom'])
    parser.add_argument('--lr', type=float, default=3e-4)
    parser.add_argument('--channel', type=int, default=256)
    parser.add_argument('--n_res_block', type=int, default=4)
    parser.add_argument('--n_res_channel', type=int, default=256)
    parser.add_argument('--n_out_res_block', type=int, default=0)
    parser.add_argument('--n_cond_res_block', type=int, default=3)
    parser.add_argument('--dropout', type=float, default=0.1)
    parser.add_argument('--amp', type=str, default='O0', choices=['O0'])
    parser.add_argument('--sched', type=str, choices=['cycle'])
    parser.add_argument('--ckpt', type=str)
    parser.add_argument('path', type=str)
    # not in the reference
    parser.add_argument('--size', type=int, nargs=2, default=[32, 32], metavar=('H', 'W'))
    parser.add_argument('--n_class', type=int, default=512)
    parser.add_argument('--n_block', type=int, default=4)
    parser.add_argument('--kernel_size', type=int, default=5)
    parser.add_argument('--max_steps', type=int, default=0)
    parser.add_argument('--ckpt_dir', type=str, default='checkpoint')
    parser.add_argument('--workers', type=int, default=4)
    parser.add_argument('--seed', type=int, default=None)
    parser.add_argument('--resume', type=str, default=None)
    parser.add_argument('--val_path', type=str, default=None)
    parser.add_argument('--eval_every', type=int, default=0)
    parser.add_argument('--clip_grad_norm', type=float, default=None)
    parser.add_argument('--ema_decay', type=float, default=None)
    parser.add_argument('--n_label', type=int, default=0)
    parser.add_argument('--precision', type=str, default='fp32', choices=['fp32', 'bf16', 'bf16_wgrad', 'bf16_attn'],
                        help='fp32 (default), or bf16: the eligible conv forwards and data gradients multiply bf16-rounded operands and accumulate in fp32; weight gradients, weights, optimizer state and every stored tensor stay fp32 (no loss scaling); the counterpart of --amp O1 of the reference; bf16_wgrad: as bf16, and the eligible weight gradients (input and output channels both multiples of 16) multiply bf16-rounded x and dy as well, bias gradients stay fp32 sums; bf16_attn: as bf16_wgrad, and the attention cores with heads of 16, 32, 48 or 64 channels multiply bf16-rounded q, k, v, probabilities and gradients as well (softmax and the three projections stay fp32)')
    return parser.parse_args(argv)


def build_model(args):
    import vqvae2_amd
    h, w = args.size
    if args.hier == 'top':
        return vqvae2_amd.PixelSNAIL([h, w], args.n_class, args.channel, args.kernel_size, args.n_block, args.n_res_block,
                                     args.n_res_channel, dropout=args.dropout, n_out_res_block=args.n_out_res_block,
                                     n_label=getattr(args, 'n_label', 0))
    return vqvae2_amd.PixelSNAIL([2 * h, 2 * w], args.n_class, args.channel, args.kernel_size, args.n_block, args.n_res_block,
                                 args.n_res_channel, attention=False, dropout=args.dropout,
                                 n_cond_res_block=args.n_cond_res_block, cond_res_channel=args.n_res_channel,
                                 n_label=getattr(args, 'n_label', 0))


def main(argv=None):
    args = parse_args(argv)
    import vqvae2_amd
    from vqvae2_amd import distributed as dist_fn
    rank, _, world = dist_fn.bringup()       # joins the launcher's job; a no-op without one
    primary = dist_fn.is_primary()
    if primary:
        print(args)
    if args.seed is not None:
        torch.manual_seed(args.seed + rank)
    device = 'cuda'
    dataset = vqvae2_amd.codes.CodeDataset(args.path)
    distributed = dist_fn.get_world_size() > 1
    sampler = dist_fn.data_sampler(dataset, shuffle=True, distributed=distributed)
    # (the DistributedSampler pads every shard to the same length and drop_last cuts whole batches: every rank takes the
    # same number of steps)
    loader = DataLoader(dataset, batch_size=args.batch, sampler=sampler, num_workers=args.workers, drop_last=True)
    val_loader, eval_every = None, args.eval_every
    if args.val_path is not None and eval_every > 0:
        # every image once: rank r takes the rows r, r + world, ... (a DistributedSampler would repeat rows to pad the shards)
        held_out = vqvae2_amd.codes.CodeDataset(args.val_path)
        share = torch.utils.data.Subset(held_out, range(rank, len(held_out), max(world, 1)))
        val_loader = DataLoader(share, batch_size=args.batch, shuffle=False, num_workers=0)
    # (--resume keeps this command line: give the run's own arguments again)
    clip_grad_norm, ema_decay = args.clip_grad_norm, args.ema_decay     # of THIS command line, like --resume
    precision = args.precision
    resume = torch.load(args.resume, map_location='cpu', weights_only=False) if args.resume is not None else None
    ckpt = {}
    if args.ckpt is not None:
        ckpt = torch.load(args.ckpt, weights_only=False)
        args = ckpt['args']
    n_label = getattr(args, 'n_label', 0)
    if n_label > 0:
        from vqvae2_amd.codes import class_names, labels_of
        if not getattr(args, 'class_names', None):
            args.class_names = class_names(dataset)
        if len(args.class_names) > n_label:
            raise SystemExit(f"--n_label {n_label}: the codes hold {len(args.class_names)} classes")

    def labels(filenames):
        return labels_of(filenames, args.class_names).to(device) if n_label > 0 else None

    def labelled(batches):      # (top, bottom, filename) -> (top, bottom, label) for Stage2Trainer.evaluate
        return ((top, bottom, labels_of(names, args.class_names)) for top, bottom, names in batches) if n_label > 0 else batches

    model = build_model(args)
    if 'model' in ckpt:
        model.load_state_dict(ckpt['model'])
    model = model.to(device).train()
    trainer = vqvae2_amd.Stage2Trainer(model, args.hier, lr=args.lr, sched=args.sched, n_iter=len(loader) * args.epoch,
                                       clip_grad_norm=clip_grad_norm, ema_decay=ema_decay)
    if precision != 'fp32':
        trainer.set_precision(precision)
    first_epoch = 0
    if resume is not None:
        trainer.load_state_dict(resume['trainer'] if 'trainer' in resume else resume)
        first_epoch = int(resume.get('epoch', 0))
    if primary:
        os.makedirs(args.ckpt_dir, exist_ok=True)
    steps = 0
    for i in range(first_epoch, args.epoch):
        if distributed:
            sampler.set_epoch(i)
        for top, bottom, names in loader:
            r = trainer.step(top.to(device), bottom.to(device) if args.hier == 'bottom' else None, labels(names))
            steps += 1
            if primary:
                gnorm = f"; gnorm: {r['grad_norm'].item():.5f}" if 'grad_norm' in r else ''
                print(f"epoch: {i + 1}; loss: {r['loss'].item():.5f}; acc: {r['accuracy'].item():.5f}; lr: {r['lr']:.5f}{gnorm}")
            if val_loader is not None and steps % eval_every == 0:
                held = trainer.evaluate(labelled(val_loader))
                if primary:
                    print(f"step: {steps}; held-out {vqvae2_amd.PriorEvaluator.summary(held)}")
                if ema_decay is not None:
                    with trainer.averaged_weights():
                        held = trainer.evaluate(labelled(val_loader))
                    if primary:
                        print(f"step: {steps}; held-out (averaged weights) {vqvae2_amd.PriorEvaluator.summary(held)}")
            if args.max_steps and steps >= args.max_steps:
                break
        done = bool(args.max_steps and steps >= args.max_steps)
        if primary and (i % 10 == 0 or i >= args.epoch - 1 or done):
            tag = f'{args.hier}_{str(i + 1).zfill(3)}.pt'
            torch.save({'model': model.state_dict(), 'args': args}, os.path.join(args.ckpt_dir, 'pixelsnail_' + tag))
            if ema_decay is not None:
                torch.save({'model': trainer.averaged_state_dict(), 'args': args},
                           os.path.join(args.ckpt_dir, 'pixelsnail_' + tag[:-3] + '_ema.pt'))
            torch.save({'trainer': trainer.state_dict(), 'args': args, 'epoch': i + 1},
                       os.path.join(args.ckpt_dir, 'trainer_' + tag))
        if done:
            break
    if primary and clip_grad_norm is not None:
        print(f"skipped steps (non-finite gradient norm): {trainer.skipped_steps()}")
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        dist_fn.synchronize()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
