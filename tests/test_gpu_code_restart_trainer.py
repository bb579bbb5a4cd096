"""GPU: dead-code restart through Quantize and Stage1Trainer on a tiny VQVAE (32x32 images, batch 4, n_embed 64): off and
threshold 0 are the same run bit for bit, dead codes come back, `start` holds them, resume is exact, mismatched
checkpoints are refused, evaluation between steps changes nothing, and two ranks stay identical."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _code_restart_child as X
import _code_restart_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAY = 0.99


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def make(amd, dead, restart=None, seed=40, **kw):
    tr = amd.Stage1Trainer(X.build(amd, seed, dead), lr=3e-4, **kw)
    if restart is not None:
        tr.set_code_restart(**restart)
    return tr


def run(tr, imgs):
    return [tr.step(img.cuda()) for img in imgs]


def losses(results):
    torch.cuda.synchronize()
    return [float(r["loss"]) for r in results]


def test_threshold_zero_is_the_run_without_the_feature(amd):
    imgs = X.images(4)
    plain, zero = make(amd, True), make(amd, True, dict(threshold=0.0))
    r_plain, r_zero = run(plain, imgs), run(zero, imgs)
    assert sorted(r_plain[-1]) == ["latent", "loss", "recon"] and sorted(r_zero[-1]) == ["latent", "loss", "recon", "restarted"]
    assert losses(r_plain) == losses(r_zero)
    a, b = X.snapshot(plain), X.snapshot(zero)
    assert "code_restart" not in a["trainer"]
    assert b["trainer"].pop("code_restart") == {"threshold": 0.0, "start": 0, "seed": 0, "totals": [0, 0]}
    X.same(a, b, "threshold 0")
    assert zero.restarted_codes() == [0, 0] and plain.restarted_codes() == [0, 0]
    assert r_zero[-1]["restarted"].tolist() == [0, 0]
    # turning it off again gives the keys the step had
    zero.set_code_restart(None)
    assert sorted(zero.step(imgs[0].cuda())) == ["latent", "loss", "recon"] and "code_restart" not in zero.state_dict()


def test_dead_codes_come_back_and_start_holds_them(amd):
    imgs = X.images(3)
    cols = X.moved_columns(X.CFG.n_embed)
    on = make(amd, True, dict(threshold=1.0, start=0))
    r = run(on, imgs)
    torch.cuda.synchronize()
    totals = on.restarted_codes()
    print("restarted totals after 3 steps:", totals, "last step:", r[-1]["restarted"].tolist())
    assert all(t > 0 for t in totals) and len(totals) == 2
    for q in on.quantizers:
        assert float(q.embed[:, cols.cuda()].abs().max()) < 1e2
        assert bool(torch.isfinite(q.embed).all())
    # start = 10: nothing restarts in 3 steps.  The moved codes never receive a vector (counts = 0, sums = 0), so each step
    # multiplies their cluster_size and embed_avg by decay: after 3 steps embed_avg = 1e3 * 0.5 * decay^3 (three fp32
    # roundings: 2^-22 relative), cluster_size = 0.5 * decay^3 = 0.485, and embed = embed_avg / ((cs + eps) / (n + K eps) * n)
    # lies between 1e3 * cs / (cs + eps) > 1e3 * (1 - 2.1e-5) and 1e3 * (n + K eps) / n < 1e3 * (1 + 4.2e-5)
    # (n >= the 32 moved codes' 0.485 = 15.5, K eps = 6.4e-4): inside 1e3 * (1 +- 1e-4).
    late = make(amd, True, dict(threshold=1.0, start=10))
    r = run(late, imgs)
    torch.cuda.synchronize()
    assert late.restarted_codes() == [0, 0] and r[-1]["restarted"].tolist() == [0, 0]
    for q in late.quantizers:
        ea, cs, e = q.embed_avg[:, cols.cuda()], q.cluster_size[cols.cuda()], q.embed[:, cols.cuda()]
        assert float((ea / (X.DEAD_AT * X.DEAD_SIZE * DECAY ** 3) - 1).abs().max()) < 2.0 ** -20
        assert float((cs / (X.DEAD_SIZE * DECAY ** 3) - 1).abs().max()) < 2.0 ** -20
        assert float((e / X.DEAD_AT - 1).abs().max()) < 1e-4


def test_resume_continues_exactly(amd):
    imgs = X.images(6)
    restart = dict(threshold=1.0, start=0, seed=3)
    whole = make(amd, True, restart)
    l_whole = losses(run(whole, imgs))
    first = make(amd, True, restart)
    l_first = losses(run(first, imgs[:3]))
    ck = first.state_dict()
    assert ck["code_restart"] == dict(restart, totals=first.restarted_codes()) and ck["adam_t"] == 3
    assert all(t > 0 for t in ck["code_restart"]["totals"])
    second = make(amd, False, restart, seed=41)              # a fresh model and trainer, from another state
    second.load_state_dict(ck)
    assert second.restarted_codes() == ck["code_restart"]["totals"]
    l_second = losses(run(second, imgs[3:]))
    assert l_first + l_second == l_whole
    X.same(X.snapshot(second), X.snapshot(whole), "resumed")
    assert second.restarted_codes() == whole.restarted_codes()


def test_mismatched_checkpoints_are_refused_before_anything_changes(amd):
    imgs = X.images(1)
    with_it, without = make(amd, True, dict(threshold=1.0)), make(amd, True)
    run(with_it, imgs), run(without, imgs)
    ck_with, ck_without = with_it.state_dict(), without.state_dict()
    for trainer, ck, word in ((make(amd, False, seed=41), ck_with, "with"),
                              (make(amd, False, dict(threshold=1.0), seed=41), ck_without, "without"),
                              (make(amd, False, dict(threshold=2.0), seed=41), ck_with, "differ")):
        before = X.snapshot(trainer)
        with pytest.raises(RuntimeError, match=word):
            trainer.load_state_dict(ck)
        X.same(X.snapshot(trainer), before, "refused load")
    # the model alone (the reference's file) loads into either
    make(amd, False, dict(threshold=1.0), seed=41).load_state_dict(ck_without["model"])
    make(amd, False, seed=41).load_state_dict(ck_with["model"])


def test_evaluation_between_two_steps_changes_nothing(amd):
    imgs = X.images(6)
    val = X.images(1, seed=999)[0].cuda()

    def go(evaluate):
        tr = make(amd, True, dict(threshold=1.0, seed=2))
        m = tr.model
        run(tr, imgs[:3])
        if evaluate:
            torch.cuda.synchronize()
            before = {k: v.clone() for k, v in m.state_dict().items()}
            slots, cand, counters = tr.arena.extra.clone(), tr._restart_cand.clone(), tr._restart_counters.clone()
            steps = [q.restart_step for q in tr.quantizers]
            preps = [q._prep for q in tr.quantizers]
            prep_vals = [(p[0].clone(), p[1].clone()) for p in preps]
            keys = [q._prep_key for q in tr.quantizers]
            r = tr.evaluate([val, val])
            torch.cuda.synchronize()
            assert r["images"] == 8 and np.isfinite(r["mse"]) and m.training
            X.same(before, dict(m.state_dict()), "model")
            assert torch.equal(slots, tr.arena.extra), "EMA statistics slots were written by evaluate()"
            assert torch.equal(cand, tr._restart_cand) and torch.equal(counters, tr._restart_counters)
            assert steps == [q.restart_step for q in tr.quantizers]
            for q, p, pv, key in zip(tr.quantizers, preps, prep_vals, keys):
                assert q._prep is p and q._prep_key == key and q._prepared() is p
                assert torch.equal(p[0], pv[0]) and torch.equal(p[1], pv[1])
        run(tr, imgs[3:])
        return X.snapshot(tr)

    X.same(go(True), go(False), "evaluated")


def test_drop_in_quantize_restarts_without_a_trainer(amd):
    """Quantize alone (statistics and candidates in one buffer, update inside forward): a dead code lands on the row the
    reference draws, eval mode draws nothing."""
    d, k = 16, 64
    g = torch.Generator().manual_seed(5)
    q = amd.Quantize(d, k)
    embed = torch.randn(d, k, generator=g)
    embed[:, 7] = 1e3
    cs = torch.full((k,), 4.0)
    cs[7] = 0.5
    q.load_state_dict({"embed": embed, "cluster_size": cs, "embed_avg": embed * cs[None, :]})
    q.cuda().train()
    q.enable_code_restart(1.0, seed=11, slot=3)
    q.restart_step = 20
    x = torch.randn(2, 8, 8, d, generator=g).cuda()
    q.eval()
    with torch.no_grad():
        q(x)
    assert q.restart_step == 20 and q.restart_counter is None
    q.train()
    q(x)
    torch.cuda.synchronize()
    assert q.restart_step == 21 and q.restart_counter.tolist() == [1, 1]
    row = x.reshape(-1, d)[R.draw(11, 20, 3, 7, 128)]
    assert float(q.cluster_size[7]) == 1.0 and torch.equal(q.embed_avg[:, 7], row)
    assert float((q.embed[:, 7] / row - 1).abs().max()) < 1e-3
    assert q._prepared() is not None and torch.equal(q._prepared()[0], q.embed.t())


# ----------------------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_ranks(tmp_path, share):
    out, port = str(tmp_path / "two"), _free_port()
    child = os.path.join(ROOT, "tests", "_code_restart_child.py")
    procs = [subprocess.Popen([sys.executable, child, str(rank), "2", str(port), out, str(int(share))], cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in (0, 1)]
    logs = []
    try:
        for proc in procs:                                                   # each rank under its own time limit
            logs.append(proc.communicate(timeout=240)[0])
    finally:
        for proc in procs:
            if proc.poll() is None:
                proc.kill()
                proc.wait()
    assert [p.returncode for p in procs] == [0, 0], "\n".join(log[-3000:] for log in logs)
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    assert sorted(r0.files) == sorted(r1.files)
    for key in r0.files:
        assert np.array_equal(r0[key], r1[key]), f"{key}: the ranks differ"
    assert (r0["totals"] > 0).all()
    for slot in (0, 1):
        m = int(r0[f"m{slot}"])
        want = R.picks(X.TWO_RANK_SEED, X.TWO_RANK_STEPS - 1, slot, X.CFG.n_embed, 2 * m)
        owners = want // m
        assert (owners == 0).any() and (owners == 1).any(), "the seed must draw rows of both ranks"
        assert np.array_equal(r0[f"picks{slot}"], want)
        cols = X.moved_columns(X.CFG.n_embed).numpy()
        assert np.abs(r0[f"{slot}.embed"][:, cols]).max() < 1e2


def test_two_ranks_hold_identical_codebooks(tmp_path):
    """One process per GPU."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _two_ranks(tmp_path, share=False)


def test_two_ranks_sharing_one_gpu_hold_identical_codebooks(tmp_path):
    """The same two ranks on GPU 0 (as tests/test_gpu_dp.py runs its ranks): runs wherever one GPU is visible."""
    _two_ranks(tmp_path, share=True)
