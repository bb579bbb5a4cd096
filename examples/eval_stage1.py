"""Evaluate a saved stage-1 checkpoint on held-out data: the reference's running mse (train_vqvae.py:93-100), the
latent loss and the health of both codebooks (codes in use, perplexity), optionally with reconstruction grids in the
form of the reference's samples (train_vqvae.py:120-139: inputs on the top row, reconstructions below).

--ckpt is a checkpoint/vqvae_XXX.pt as examples/train_stage1.py (or the reference) saves it, or a trainer_XXX.pt.
--path is a directory of .npy image batches, uint8 [N,H,W,3] pixels (normalised on the GPU with --norm, centre-cropped
to --size) or float32 [N,3,H,W], already normalised.  --image_metrics adds PSNR and SSIM of the 8-bit reconstructions.

    python examples/eval_stage1.py --ckpt checkpoint/vqvae_001.pt --path /data/ffhq_val_u8 --size 256 --dump recon
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vqvae2_amd  # noqa: E402

NORMS = {"half": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),                       # extract_code.py:52
         "imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))}       # train_vqvae.py:154


def batches(args, device):
    for f in sorted(glob.glob(os.path.join(args.path, "*.npy"))):
        data = np.load(f, mmap_mode="r")
        for i in range(0, data.shape[0], args.batch_size):
            a = np.ascontiguousarray(data[i:i + args.batch_size])
            t = torch.from_numpy(a)
            yield (t if a.dtype == np.uint8 else t.float()).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", type=str, required=True)
    ap.add_argument("--path", type=str, required=True)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--norm", choices=sorted(NORMS), default="half")
    ap.add_argument("--dump", type=str, default="", help="directory for one reconstruction grid per batch")
    ap.add_argument("--dump_images", type=int, default=8, help="images of each batch that go into its grid")
    ap.add_argument("--image_metrics", action="store_true", help="also PSNR and SSIM of the 8-bit reconstructions")
    args = ap.parse_args()

    device = torch.device("cuda", 0)
    sd = torch.load(args.ckpt, map_location="cpu", weights_only=True)
    sd = sd["model"] if "model" in sd and isinstance(sd["model"], dict) else sd
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    model = vqvae2_amd.VQVAE()
    model.load_state_dict(sd)
    model.to(device).eval()

    normalizer = vqvae2_amd.ImageNormalizer(*NORMS[args.norm], layout="hwc", crop=(args.size, args.size))
    ev = vqvae2_amd.Evaluator(model, normalizer, image_metrics=args.image_metrics)
    denorm = normalizer.inverse()
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    for b, img in enumerate(batches(args, device)):
        ev.update(img)
        if args.dump:
            k = min(img.shape[0], args.dump_images)
            part = img[:k].contiguous()
            with torch.no_grad():
                x = normalizer(part) if part.dtype == torch.uint8 else vqvae2_amd.ops.to_nhwc(part)
                dec, _ = model.forward_nhwc(x)
            vqvae2_amd.save_u8_image(denorm.grid([x, dec], nrow=k, nhwc=True), os.path.join(args.dump, f"recon_{b:05d}.png"))
    r = ev.result()
    print(f"images: {r['images']}; mse: {r['mse']:.6f}; latent: {r['latent']:.4f}; "
          f"perplexity t/b: {r['perplexity_t']:.2f}/{r['perplexity_b']:.2f}; "
          f"used codes t/b: {r['used_t']}/{r['used_b']} of {r['n_embed']}"
          + (f"; psnr: {r['psnr']:.2f} dB; ssim: {r['ssim']:.4f}" if args.image_metrics else ""))


if __name__ == "__main__":
    main()
