"""Sample images from the two trained priors and the VQ-VAE: the reference's sample.py on one MI355X.

    python examples/sample.py --vqvae vqvae_560.pt --top pixelsnail_top_420.pt --bottom pixelsnail_bottom_420.pt \\
        [--batch 8 --temp 1.0] sample.png

Top codes are drawn from the top prior, bottom codes from the bottom prior conditioned on them, both are decoded with
VQVAE.decode_code, clamped to [-1, 1] and written as one grid.  The command line is the reference's; checkpoints are looked up
under --ckpt_dir (the reference's fixed 'checkpoint').  The priors are rebuilt from the arguments their checkpoints carry
(what examples/train_pixelsnail.py saves: the reference's plus size / n_class / n_block / kernel_size).

Extra arguments of this script: --ckpt_dir; --seed (torch.manual_seed, which fixes every draw); --vqvae_arg NAME=INT (repeatable)
for a VQVAE that was not built with the defaults (channel, n_res_block, n_res_channel, embed_dim, n_embed), since
examples/train_stage1.py saves a bare state_dict.  A PNG needs PIL; without it the same canvas is written as .npy.

Truncated sampling, for both priors: --top_k INT draws from the INT most likely codes only, --top_p FLOAT from the smallest set
of most likely codes that holds FLOAT of the probability (0 and 1.0: off).

--stepping row (the default) recomputes a whole row per drawn code; --stepping pixel computes the drawn column only
(PriorSampler's `stepping`).

--label K draws class K from class-conditional priors (checkpoints of examples/train_pixelsnail.py --n_label N, which carry
n_label and the sorted class names in their args): both priors get the same label for every image.  Such priors need it;
priors trained without labels refuse it.

Completing images: --from_images FILE.npy --keep_rows R.  FILE.npy holds uint8 [B, H, W, 3]; the images are normalised to
[-1, 1], encoded with the VQ-VAE, and the first R rows of their top codes and 2 R rows of their bottom codes are kept; the priors
draw the rest.  The batch size is that of the file."""
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
    parser.add_argument('--top_k', type=int, default=0)
    parser.add_argument('--top_p', type=float, default=1.0)
    parser.add_argument('--stepping', choices=['row', 'pixel'], default='row')
    parser.add_argument('--from_images', type=str, metavar='FILE.npy')
    parser.add_argument('--keep_rows', type=int, default=0)
    parser.add_argument('--label', type=int, default=None, metavar='K')
    return parser.parse_args(argv)


def encode_images(model_vqvae, path, device):
    """The top and bottom codes (int64 [B, Ht, Wt], [B, Hb, Wb]) of the uint8 images [B, H, W, 3] stored at `path`."""
    import numpy as np
    import vqvae2_amd
    images = np.load(path)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
        raise SystemExit(f"--from_images: uint8 [B, H, W, 3] expected, {path} holds {images.dtype} {images.shape}")
    norm = vqvae2_amd.ImageNormalizer([0.5] * 3, [0.5] * 3)
    with torch.no_grad():
        _, _, _, id_t, id_b = model_vqvae.encode(norm.nchw(torch.from_numpy(images).to(device).contiguous()))
    return id_t, id_b


def draw_codes(args, model_vqvae, model_top, model_bottom, device):
    """(top codes, bottom codes) as the command line asks for them: drawn freely, or completed from encoded images."""
    import vqvae2_amd
    top_size = list(model_top.background.shape[2:])
    bottom_size = list(model_bottom.background.shape[2:])
    batch, top_prefix, bottom_prefix = args.batch, None, None
    if args.from_images:
        id_t, id_b = encode_images(model_vqvae, args.from_images, device)
        if list(id_t.shape[1:]) != top_size or list(id_b.shape[1:]) != bottom_size:
            raise SystemExit(f"--from_images: the images encode to {list(id_t.shape[1:])} / {list(id_b.shape[1:])} codes, "
                             f"the priors draw {top_size} / {bottom_size}")
        if not 0 <= args.keep_rows <= top_size[0]:
            raise SystemExit(f"--keep_rows must be in 0..{top_size[0]}")
        batch = id_t.shape[0]
        top_prefix, bottom_prefix = id_t[:, :args.keep_rows].contiguous(), id_b[:, :2 * args.keep_rows].contiguous()
    kw = dict(top_k=args.top_k, top_p=args.top_p, stepping=args.stepping)
    if args.label is not None:
        kw['label'] = args.label
    top_sample = vqvae2_amd.sample_model(model_top, device, batch, top_size, args.temp, prefix=top_prefix, **kw)
    bottom_sample = vqvae2_amd.sample_model(model_bottom, device, batch, bottom_size, args.temp, condition=top_sample,
                                            prefix=bottom_prefix, **kw)
    return top_sample, bottom_sample


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
    top_sample, bottom_sample = draw_codes(args, model_vqvae, model_top, model_bottom, device)
    with torch.no_grad():
        decoded = model_vqvae.decode_code(top_sample, bottom_sample).clamp(-1, 1)
    # the reference's save_image(normalize=True, range=(-1, 1)): (x + 1) / 2 is the inverse of Normalize(0.5, 0.5)
    denorm = vqvae2_amd.ImageDenormalizer([0.5] * decoded.shape[1], [0.5] * decoded.shape[1])
    path = vqvae2_amd.save_u8_image(denorm.grid(decoded, nhwc=False), args.filename)
    print(f"wrote {path}: {decoded.shape[0]} images of {decoded.shape[2]} x {decoded.shape[3]}")


if __name__ == '__main__':
    main()
