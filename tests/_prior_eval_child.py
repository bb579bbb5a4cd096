"""Shared by tests/test_gpu_prior_eval.py and its child processes: the held-out set of a golden PixelSNAIL case, and one
gloo rank that scores its share of it.

As a script: `_prior_eval_child.py RANK WORLD PORT OUT CASE` joins a gloo group of WORLD ranks on the one GPU, evaluates the
rows RANK, RANK + WORLD, ... of held_out(CASE) and leaves PriorEvaluator.result() in OUT.rank<RANK>.npz."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _pixelsnail_model_ref as M  # noqa: E402
import _stage2_child as S  # noqa: E402

SCALARS = ("nll", "bits_per_code", "perplexity", "accuracy", "top_k_accuracy", "top_k", "entropy", "unigram_nll", "images", "codes")


def held_out(ci, n, seed):
    """n code maps of golden case ci from a seeded generator: (hier, top [n,...] or None, codes [n,H,W]) on the CPU."""
    g = M.load()
    c = M.cases(g)[ci]
    gen = torch.Generator().manual_seed(seed)
    h, w = c["shape"]
    codes = torch.randint(0, c["n_class"], (n, h, w), generator=gen)
    if "cond" in c:
        return "bottom", torch.randint(0, c["n_class"], (n, *c["cond"]), generator=gen), codes
    return "top", None, codes


def evaluate(amd, model, hier, cond, codes, batches, top_k=3, evaluator=None):
    """PriorEvaluator over the set cut into `batches` (sizes); returns the evaluator (state on the device)."""
    ev = evaluator if evaluator is not None else amd.PriorEvaluator(model, hier, top_k=top_k)
    lo = 0
    for b in batches:
        part = codes[lo:lo + b].cuda()
        if hier == "top":
            ev.update(part)
        else:
            ev.update(cond[lo:lo + b].cuda(), part)
        lo += b
    assert lo == codes.shape[0]
    return ev


def save_result(path, r):
    np.savez(path, nll_map=r["nll_map"].numpy(), nll_rows=np.array(r["nll_rows"]), counts=r["counts"].numpy(),
             **{k: np.array(r[k]) for k in SCALARS})


def main():
    rank, world, port, out, ci = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5])
    import torch.distributed as dist
    import vqvae2_amd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    hier, cond, codes = held_out(ci, 6, 77)
    mine = slice(rank, None, world)
    model = S.build(vqvae2_amd, ci)
    ev = evaluate(vqvae2_amd, model, hier, None if cond is None else cond[mine], codes[mine], [2, 1])
    save_result(f"{out}.rank{rank}.npz", ev.result())
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
