"""Score held-out codes under a saved PixelSNAIL prior: nats and bits per code, perplexity, accuracy and top-k accuracy,
the mean predictive entropy, and the entropy of the codes' own histogram (what the best context-free model reaches).

    python examples/eval_pixelsnail.py --ckpt checkpoint/pixelsnail_top_001.pt --hier top [--batch 32 --top_k 5] CODES
    python examples/eval_pixelsnail.py --ckpt checkpoint/pixelsnail_bottom_001.pt --hier bottom --dump_map nll.npy CODES
    python -m torch.distributed.run --nproc-per-node N examples/eval_pixelsnail.py [...] CODES

--ckpt is a pixelsnail_<hier>_<NNN>.pt as examples/train_pixelsnail.py (or the reference) saves it; the model is rebuilt
from the checkpoint's 'args'.  CODES is what examples/extract_code.py wrote.  With one process per GPU every rank scores
the rows rank, rank + world, ... and PriorEvaluator.result() sums over the group; the primary rank prints one line.
--dump_map FILE.npy saves the mean nll per position as a float64 [H,W] array.  A class-conditional checkpoint (trained with
--n_label) is recognised by its args: every row is scored under the label of its directory in the checkpoint's class_names."""
import argparse
import os
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader, Subset

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--ckpt', type=str, required=True)
    parser.add_argument('--hier', type=str, default='top', choices=['top', 'bottom'])
    parser.add_argument('--batch', type=int, default=32)
    parser.add_argument('--top_k', type=int, default=5)
    parser.add_argument('--dump_map', type=str, default=None, metavar='FILE.npy')
    parser.add_argument('--precision', type=str, default='fp32', choices=['fp32', 'bf16', 'bf16_wgrad', 'bf16_attn'],
                        help='fp32 (default), or bf16: the eligible conv forwards and data gradients multiply bf16-rounded operands and accumulate in fp32; weight gradients, weights, optimizer state and every stored tensor stay fp32 (no loss scaling); the counterpart of --amp O1 of the reference; bf16_wgrad is accepted as an alias of bf16 (evaluation has no weight gradient); bf16_attn: bf16 convs, and the eligible attention cores (heads of 16, 32, 48 or 64 channels) on bf16-rounded operands as well')
    parser.add_argument('path', type=str)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    import vqvae2_amd
    from vqvae2_amd import distributed as dist_fn
    rank, _, world = dist_fn.bringup()       # joins the launcher's job; a no-op without one
    device = 'cuda'
    ckpt_dir, name = os.path.split(os.path.abspath(args.ckpt))
    model = vqvae2_amd.load_model('pixelsnail_' + args.hier, name, device, ckpt_dir=ckpt_dir)
    if args.precision != 'fp32':
        vqvae2_amd.set_conv_precision(model, 'bf16')
    if args.precision == 'bf16_attn':
        vqvae2_amd.set_attention_precision(model, 'bf16')
    dataset = vqvae2_amd.codes.CodeDataset(args.path)
    share = Subset(dataset, range(rank, len(dataset), max(world, 1)))
    evaluator = vqvae2_amd.PriorEvaluator(model, args.hier, top_k=args.top_k)
    class_names = None
    if model.n_label > 0:
        saved = torch.load(args.ckpt, map_location='cpu', weights_only=False)['args']
        class_names = saved['class_names'] if isinstance(saved, dict) else saved.class_names
    for top, bottom, names in DataLoader(share, batch_size=args.batch, shuffle=False, num_workers=0):
        label = vqvae2_amd.codes.labels_of(names, class_names).to(device) if class_names is not None else None
        evaluator.update_labelled(label, top.to(device), bottom.to(device) if args.hier == 'bottom' else None)
    r = evaluator.result()
    if dist_fn.is_primary():
        print(vqvae2_amd.PriorEvaluator.summary(r))
        if args.dump_map:
            np.save(args.dump_map, r['nll_map'].numpy())
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        dist_fn.synchronize()
        torch.distributed.destroy_process_group()
    return r


if __name__ == '__main__':
    main()
