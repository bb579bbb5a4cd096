"""Shared by tests/test_gpu_code_restart_trainer.py and its child processes: a tiny VQVAE (32x32 images, n_embed 64) whose
codebooks can be given dead codes, under Stage1Trainer with set_code_restart.

As a script -- `_code_restart_child.py RANK WORLD PORT OUT SHARE` -- it is one rank of a gloo group (SHARE = 1: the ranks
share GPU 0, else rank r runs on GPU r): half a batch per rank, dead codes present, three steps; it leaves its codebook
buffers, restarted totals and the rows drawn for the last step in OUT.rank<RANK>.npz.  The parent starts one fresh process
per rank, each under its own time limit."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import vqvae_oracle as O  # noqa: E402

CFG, SIZE, BATCH = O.TINY, 32, 4
DEAD_AT, DEAD_SIZE = 1e3, 0.5          # where the moved codes sit, and their cluster size (below the threshold 1.0)
TWO_RANK_SEED, TWO_RANK_STEPS = 5, 3


def moved_columns(k):
    return torch.arange(0, k, 2)


def build(amd, seed, dead, device="cuda"):
    """The tiny model from seeded state; dead: every second code of both levels moved to DEAD_AT, where no encoder output
    selects it, with embed_avg = embed * cluster_size as the invariant wants."""
    m = amd.VQVAE(channel=CFG.channel, n_res_block=CFG.n_res_block, n_res_channel=CFG.n_res_channel, embed_dim=CFG.embed_dim,
                  n_embed=CFG.n_embed)
    st = O.make_state(CFG, seed)
    if dead:
        for level in ("t", "b"):
            cols = moved_columns(CFG.n_embed)
            st[f"quantize_{level}.embed"][:, cols] = DEAD_AT
            st[f"quantize_{level}.cluster_size"][cols] = DEAD_SIZE
            st[f"quantize_{level}.embed_avg"][:, cols] = DEAD_AT * DEAD_SIZE
    m.load_state_dict(st)
    return m.to(device)


def images(n_steps, seed=700):
    return [O.make_images(BATCH, SIZE, seed + s) for s in range(n_steps)]


def snapshot(tr):
    """Everything a step changes, on the host: the model's state_dict (codebook buffers included) and the trainer's."""
    torch.cuda.synchronize()
    to_host = lambda v: v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v
    sd = tr.state_dict()
    return {"model": {k: to_host(v) for k, v in tr.model.state_dict().items()},
            "trainer": {k: ({kk: to_host(vv) for kk, vv in v.items()} if isinstance(v, dict) else to_host(v))
                        for k, v in sd.items()}}


def same(a, b, path=""):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), f"{path} differs"
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), (path, sorted(a), sorted(b))
        for k in a:
            same(a[k], b[k], f"{path}.{k}")
    else:
        assert a == b, f"{path}: {a!r} != {b!r}"


def main():
    rank, world, port, out, share = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5])
    import torch.distributed as dist
    import vqvae2_amd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0 if share else rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = build(vqvae2_amd, 40 + 100 * rank, dead=True)         # every rank its own state: the trainer brings rank 0's
    tr = vqvae2_amd.Stage1Trainer(m, lr=3e-4)
    tr.set_code_restart(1.0, start=0, seed=TWO_RANK_SEED)
    assert tr.dp and tr.world == world
    per = BATCH // world
    for img in images(TWO_RANK_STEPS):
        r = tr.step(img[rank * per:(rank + 1) * per].contiguous().cuda())
    torch.cuda.synchronize()
    res = {"restarted": r["restarted"].cpu().numpy(), "totals": np.asarray(tr.restarted_codes(), dtype=np.int64)}
    for slot, q in enumerate(tr.quantizers):
        # the rows the last step drew, asked again with picks: the draw reads no data, only (seed, step, slot, k, M, world)
        rows = q.restart_cand.numel() // q.dim
        m_rank = per * (SIZE // (8 if slot == 0 else 4)) ** 2
        x = torch.zeros((m_rank, 1, 1, q.dim), device="cuda")
        picks = torch.empty(rows, device="cuda", dtype=torch.int64)
        vqvae2_amd.ops.vq_restart_candidates(x, q.n_embed, torch.empty(rows * q.dim, device="cuda"), TWO_RANK_SEED,
                                             TWO_RANK_STEPS - 1, slot, rank, world, picks)
        res[f"picks{slot}"], res[f"m{slot}"] = picks.cpu().numpy(), np.int64(m_rank)
        for name in ("embed", "cluster_size", "embed_avg"):
            res[f"{slot}.{name}"] = getattr(q, name).cpu().numpy()
    np.savez(f"{out}.rank{rank}.npz", **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
