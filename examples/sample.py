"""Sample images from the two trained priors and the VQ-VAE: the reference's sample.py on one MI355X.

    python examples/sample.py --vqvae vqvae_560.pt --top pixelsnail_top_420.pt --bottom pixelsnail_bottom_420.pt \\
        [--batch 8 --temp 1.0] sample.png

Top codes are drawn from the top prior, bottom codes from the bottom prior conditioned on them, both are decoded with
VQVAE.decode_code, clamped to [-1, 1] and written as one grid.  The command line is the reference's; checkpoints are looked up
under --ckpt_dir (the reference's fixed 'checkpoint').  The priors are rebuilt from the arguments their checkpoints carry
(what examples/train_pixelsnail.py saves: the reference's plus size / n_class / n_block / kernel_size).

Extra arguments of this script: --ckpt_dir; --seed (torch.manual_seed, which fixes every draw); --vqvae_arg NAME=INT (repeatable)
for a VQVAE that was not built with the defaults (channel, n_res_block, n_res_channel, embed_dim, n_embed), since
examples/train_stage1.py saves a bare state_dict.  A PNG needs PIL; without it the same canvas is written as .npy."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--batch', type=int, default=8)
    parser.add_argument('--vqvae', type=str, required=True)
    parser.add_argument('--top', type=str, required=True)
    parser.add_argument('--bottom', type=str, required=True)
    parser.add_argument('--temp', type=float, default=1.0)
    parser.add_argument('filename', type=str)
    # not in the reference
    parser.add_argument('--ckpt_dir', type=str, default='checkpoint')
    parser.add_argument('--seed', type=int)
    parser.add_argument('--vqvae_arg', action='append', default=[], metavar='NAME=INT')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    import vqvae2_amd
    device = 'cuda'
    if args.seed is not None:
        torch.manual_seed(args.seed)
    vqvae_kw = {k: int(v) for k, v in (a.split('=', 1) for a in args.vqvae_arg)}
    model_vqvae = vqvae2_amd.load_model('vqvae', args.vqvae, device, ckpt_dir=args.ckpt_dir, **vqvae_kw)
    model_top = vqvae2_amd.load_model('pixelsnail_top', args.top, device, ckpt_dir=args.ckpt_dir)
    model_bottom = vqvae2_amd.load_model('pixelsnail_bottom', args.bottom, device, ckpt_dir=args.ckpt_dir)
    top_size = list(model_top.background.shape[2:])
    bottom_size = list(model_bottom.background.shape[2:])
    top_sample = vqvae2_amd.sample_model(model_top, device, args.batch, top_size, args.temp)
    bottom_sample = vqvae2_amd.sample_model(model_bottom, device, args.batch, bottom_size, args.temp, condition=top_sample)
    with torch.no_grad():
        decoded = model_vqvae.decode_code(top_sample, bottom_sample).clamp(-1, 1)
    # the reference's save_image(normalize=True, range=(-1, 1)): (x + 1) / 2 is the inverse of Normalize(0.5, 0.5)
    denorm = vqvae2_amd.ImageDenormalizer([0.5] * decoded.shape[1], [0.5] * decoded.shape[1])
    path = vqvae2_amd.save_u8_image(denorm.grid(decoded, nhwc=False), args.filename)
    print(f"wrote {path}: {args.batch} images of {decoded.shape[2]} x {decoded.shape[3]}")


if __name__ == '__main__':
    main()
