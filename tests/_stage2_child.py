"""Shared by tests/test_gpu_stage2_trainer.py and its child processes: the same seeded Stage2Trainer run on either side.

As a script (started by `python -m torch.distributed.run --nproc-per-node 1` with VQ2_DP_FORCE=1) it runs both golden cases
over the real "nccl" (= RCCL) backend at world size 1 and leaves the state_dicts, losses and bucket facts in argv[1].
gloo_worker() is one of two ranks that share the one GPU of the test box over gloo."""
import json
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

CASES = (0, 1)          # the unconditioned golden model with attention, the conditioned one
N_ITER = 40             # of the 'cycle' schedule: 12 warm-up steps, so the learning rate moves every step


def build(amd, ci, rank=0, dropout=None):
    """The golden model of case ci on the GPU in train mode; rank > 0 perturbs every parameter (what per-process RNG
    initialisation gives a real launch)."""
    g = M.load()
    c = M.cases(g)[ci]
    kw = dict(c["kw"])
    if dropout is not None:
        kw["dropout"] = dropout
    m = amd.PixelSNAIL(c["shape"], c["n_class"], *c["args"], **kw)
    sd = M.state_dict(g, ci)
    if rank:
        gen = torch.Generator().manual_seed(1000 + rank)
        sd = {k: (v if k == "background" else v + 0.05 * torch.randn(v.shape, generator=gen)) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    if dropout is not None:
        # the gated blocks of cond_resnet keep the reference's default dropout of 0.1 whatever the model's is (pixelsnail.py:
        # 311-323): "dropout 0" here means none anywhere, so that no pass draws a seed
        for mod in m.modules():
            if hasattr(mod, "p") and isinstance(mod.p, float):
                mod.p = float(dropout)
    return m.cuda().train()


def batch(ci, variant=0):
    """(hier, step arguments) of case ci; variant > 0: other codes of the same shape."""
    g = M.load()
    c = M.cases(g)[ci]
    t = f"c{ci}.in."
    codes = torch.from_numpy(g[t + "input"])
    cond = torch.from_numpy(g[t + "condition"]) if t + "condition" in g.files else None
    if variant:
        codes = (codes + variant) % c["n_class"]
        cond = None if cond is None else (cond * 2 + variant) % c["n_class"]
    if cond is None:
        return "top", (codes.cuda(),)
    return "bottom", (cond.cuda(), codes.cuda())


def numpy_sd(model):
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


def run(amd, ci, steps, arena=True, sched="cycle", seed=5, rank=0, dropout=None, variant=0, trainer_hook=None):
    """`steps` trainer steps on case ci from a seeded generator -> (state_dict as numpy, losses, trainer)."""
    m = build(amd, ci, rank, dropout)
    hier, args = batch(ci, variant)
    tr = amd.Stage2Trainer(m, hier, lr=1e-3, sched=sched, n_iter=N_ITER, arena=arena)
    if trainer_hook is not None:
        trainer_hook(tr)
    torch.manual_seed(seed)
    losses = [float(tr.step(*args)["loss"]) for _ in range(steps)]
    torch.cuda.synchronize()
    return numpy_sd(m), losses, tr


def bucket_facts(tr):
    return {"early": tr.early_buckets, "dp": tr.dp, "world": tr.world, "bucket_bytes": tr.bucket_bytes,
            "slices": sorted((lo, hi) for _, lo, hi, _ in tr.buckets), "total": tr.arena.flat_g.numel(),
            "per_layer": tr.plan_info["per_layer"]}


def gloo_worker(rank, world, port, out, mode, cases=CASES):
    """mode 'same': both ranks see the same batch from the same seed, three steps; 'split': different batches, dropout 0,
    one step.  Every rank starts from different weights; the trainer brings all of them to rank 0's."""
    import torch.distributed as dist
    import vqvae2_amd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    facts = {}
    for ci in cases:
        if mode == "same":
            sd, losses, tr = run(vqvae2_amd, ci, 3, rank=rank)
        else:
            sd, losses, tr = run(vqvae2_amd, ci, 1, sched=None, rank=rank, dropout=0.0, variant=rank)
        assert tr.dp and tr.world == world
        facts[str(ci)] = dict(bucket_facts(tr), losses=losses)
        np.savez(f"{out}.c{ci}.rank{rank}.npz", **sd)
    with open(f"{out}.rank{rank}.json", "w") as f:
        json.dump(facts, f)
    dist.barrier()
    dist.destroy_process_group()


def main():
    out = sys.argv[1]
    import vqvae2_amd
    rank, local_rank, world = vqvae2_amd.distributed.bringup("nccl")
    assert world == 1 and torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl"
    want_native = os.environ.get("VQ2_COMM") == "capi"
    info = {"data_path": vqvae2_amd.distributed.data_comm().name}
    for ci in CASES:
        sd, losses, tr = run(vqvae2_amd, ci, 3)
        assert tr.dp and tr.comm_stream is not None
        assert isinstance(tr.comm, vqvae2_amd.distributed.NativeComm) == want_native
        info[str(ci)] = dict(bucket_facts(tr), losses=losses)
        np.savez(os.path.join(out, f"c{ci}.npz"), **sd)
    with open(os.path.join(out, "info.json"), "w") as f:
        json.dump(info, f)
    if want_native:
        assert vqvae2_amd._lib.lib.vq2_comm_destroy() == 0
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
