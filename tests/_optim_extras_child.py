"""Shared by tests/test_gpu_optim_extras.py and its child processes: seeded Stage2Trainer / Stage1Trainer runs with
clip_grad_norm / ema_decay, on the golden models of tests/_stage2_child.py and tests/_train_cases.py.

As a script -- `_optim_extras_child.py RANK WORLD PORT OUT CASE` -- it is one rank of a gloo group whose ranks share the
one GPU: a split batch (every rank its own codes, dropout 0), both features on, two steps; it leaves its parameter arena,
average, reduced gradient arena and grad_norm in OUT.rank<RANK>.npz.  The parent starts one fresh process per rank, each
under its own time limit."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _stage2_child as S  # noqa: E402

TWO_RANK_CLIP, TWO_RANK_DECAY, TWO_RANK_STEPS = 1.0, 0.5, 2


def stage2(amd, ci, rank=0, dropout=None, sched="cycle", **extras):
    """(trainer, step arguments) of golden case ci."""
    hier, args = S.batch(ci)
    return amd.Stage2Trainer(S.build(amd, ci, rank, dropout), hier, lr=1e-3, sched=sched, n_iter=S.N_ITER, **extras), args


def stage1(amd, sched=None, **extras):
    """(trainer, batches) of the tiny stage-1 case: one batch per step, a few more than any test takes."""
    import _train_cases as T
    from oracle import vqvae_oracle as O
    cfg, size, batch, _, seed = T.CASES["tiny"]
    m = amd.VQVAE(channel=cfg.channel, n_res_block=cfg.n_res_block, n_res_channel=cfg.n_res_channel,
                  embed_dim=cfg.embed_dim, n_embed=cfg.n_embed)
    m.load_state_dict(O.make_state(cfg, seed))
    m.cuda()
    tr = amd.Stage1Trainer(m, lr=3e-4, sched=sched, n_iter=40, **extras)
    return tr, [O.make_images(batch, size, seed + s).cuda() for s in range(6)]


def snapshot(tr):
    """Everything a step changes, as numpy: the model's state_dict, both moments and (if kept) the average."""
    torch.cuda.synchronize()
    out = {"model." + k: v.detach().cpu().numpy() for k, v in tr.model.state_dict().items()}
    out["adam_m"], out["adam_v"] = tr.optimizer._m.cpu().numpy(), tr.optimizer._v.cpu().numpy()
    if tr.optimizer._avg is not None:
        out["avg"] = tr.optimizer._avg.cpu().numpy()
    return out


def same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


def main():
    rank, world, port, out, ci = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5])
    import torch.distributed as dist
    import vqvae2_amd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    hier, args = S.batch(ci, variant=rank)
    tr = vqvae2_amd.Stage2Trainer(S.build(vqvae2_amd, ci, rank, 0.0), hier, lr=1e-3, sched=None,
                                  clip_grad_norm=TWO_RANK_CLIP, ema_decay=TWO_RANK_DECAY)
    assert tr.dp and tr.world == world and tr.optimizer.grad_scale == 1.0 / world
    for _ in range(TWO_RANK_STEPS):
        r = tr.step(*args)
    torch.cuda.synchronize()
    np.savez(f"{out}.rank{rank}.npz", flat_p=tr.arena.flat_p.cpu().numpy(), avg=tr.optimizer._avg.cpu().numpy(),
             gp=tr.arena.gp.cpu().numpy(), ctl=tr.optimizer.ctl.cpu().numpy(), grad_norm=r["grad_norm"].cpu().numpy(),
             skipped=np.int64(tr.skipped_steps()))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
