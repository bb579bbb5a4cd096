"""GPU checks of the prior's held-out evaluation: the two kernels of csrc/vq2_eval.hip (prior_eval_rows_kernel,
prior_eval_accumulate_kernel) against tests/_prior_eval_ref.py, and PriorEvaluator / score_codes / Stage2Trainer.evaluate
on the golden PixelSNAIL models of tests/golden/pixelsnail_model.npz against tests/_pixelsnail_model_ref.py in float64.
Floating-point results are bounded by 4 x the error of the same formula in float32 torch (the rule of
tests/test_gpu_prior_kernels.py, ratios printed); integers and everything the design makes order-independent are exact."""
import ctypes
import glob
import math
import os
import re
import socket
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import _pixelsnail_model_ref as M
import _prior_eval_child as K
import _prior_eval_ref as E
import _stage2_child as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 1.0e30        # what the lanes beyond n_class hold: a kernel that read one as data would show it


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def ceil4(c):
    return (c + 3) // 4 * 4


def rows_on_device(logits, extra=0):
    """[M, C] -> NHWC [1, M, 1, ceil4(C)] on the GPU with PAD in the pad lanes; extra > 0: a channel slice of a tensor
    `extra` floats wider, so that the row stride is larger than ceil4(C)."""
    m, c = logits.shape
    full = torch.full((1, m, 1, ceil4(c) + extra), PAD, dtype=torch.float32)
    full[0, :, 0, :c] = logits
    return full.cuda()[..., :ceil4(c)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def xent_rows(amd, x, target, n_class):
    """row_ok and the hit count of vq2_xent_fwd on the same logits."""
    m = target.numel()
    dev = x.device
    stat = torch.empty((m, 2), device=dev)
    nll = torch.empty(m, device=dev)
    ok = torch.empty(m, device=dev, dtype=torch.int32)
    loss, acc = torch.empty((), device=dev), torch.empty((), device=dev)
    count = torch.empty((), device=dev, dtype=torch.int32)
    amd._lib.check(amd._lib.lib.vq2_xent_fwd(_p(x), amd.ops.ld_of(x), _p(target), m, n_class, _p(stat), _p(nll), _p(ok), _p(loss),
                                             _p(acc), _p(count), amd.ops._stream()), "xent_fwd")
    return ok.cpu(), int(count)


# ----------------------------------------------------------------------------------------------- 1. the rows kernel
@pytest.mark.parametrize("m", [1, 5, 67])
@pytest.mark.parametrize("n_class", [1, 6, 512, 513, 16384])
def test_rows_kernel_against_fp64(amd, n_class, m):
    g = torch.Generator().manual_seed(zlib.crc32(f"rows-{n_class}-{m}".encode()))
    logits = (torch.randn(m, n_class, generator=g) * 3).float()
    target = torch.randint(0, n_class, (m,), generator=g)
    n64, h64, r64 = E.row_quantities(logits, target, torch.float64)
    n32, h32, _ = E.row_quantities(logits, target, torch.float32)
    x = rows_on_device(logits)
    nll, entropy, rank = amd.ops.prior_eval_rows(x, target.cuda().view(1, m, 1), n_class)
    torch.cuda.synchronize()
    assert nll.dtype == torch.float32 and entropy.dtype == torch.float32 and rank.dtype == torch.int32
    assert nll.shape == (m,) and entropy.shape == (m,) and rank.shape == (m,)
    assert torch.equal(rank.cpu().long(), r64)
    if n_class == 1:
        assert float(nll.abs().max()) == 0.0 and float(entropy.abs().max()) == 0.0
    E.bound(f"rows nll C={n_class} M={m}", nll.cpu(), n64, n32)
    E.bound(f"rows entropy C={n_class} M={m}", entropy.cpu(), h64, h32)
    ok, count = xent_rows(amd, x, target.cuda(), n_class)
    assert torch.equal(rank.cpu() == 0, ok == 1) and int((rank == 0).sum()) == count
    again = amd.ops.prior_eval_rows(x, target.cuda().view(1, m, 1), n_class)
    assert all(torch.equal(a, b) for a, b in zip(again, (nll, entropy, rank)))


def test_rows_kernel_reads_a_strided_view_in_place(amd):
    n_class, m = 513, 67
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(m, n_class, generator=g) * 3).float()
    target = torch.randint(0, n_class, (m,), generator=g)
    x = rows_on_device(logits, extra=8)
    assert amd.ops.ld_of(x) == ceil4(n_class) + 8 and not x.is_contiguous()
    assert amd.ops.as_nhwc(x).data_ptr() == x.data_ptr()                     # no packed copy is made on the way in
    nll, entropy, rank = amd.ops.prior_eval_rows(x, target.cuda().view(1, m, 1), n_class)
    dense = amd.ops.prior_eval_rows(rows_on_device(logits), target.cuda().view(1, m, 1), n_class)
    assert all(torch.equal(a, b) for a, b in zip(dense, (nll, entropy, rank)))
    n64, h64, r64 = E.row_quantities(logits, target, torch.float64)
    n32, h32, _ = E.row_quantities(logits, target, torch.float32)
    assert torch.equal(rank.cpu().long(), r64)
    E.bound("strided nll", nll.cpu(), n64, n32)
    E.bound("strided entropy", entropy.cpu(), h64, h32)
    # the model's own output form: a channels-last [B, n_class, H, W] view goes through to_nhwc without a copy
    out = torch.randn(2, 3, 5, 8, device="cuda")
    v = amd.ops.to_nhwc(amd.ops.from_nhwc(out, 8))
    assert v.data_ptr() == out.data_ptr()
    t = torch.randint(0, 8, (2, 3, 5), device="cuda")
    got = amd.ops.prior_eval_rows(v, t, 8)
    want = E.row_quantities(out.cpu().reshape(-1, 8), t.cpu().reshape(-1))
    assert torch.equal(got[2].cpu().long(), want[2]) and float((got[0].cpu().double() - want[0]).abs().max()) <= 1e-5


def test_rows_kernel_ties_and_out_of_range_targets(amd):
    n_class = 513
    logits = torch.full((6, n_class), -1.0)
    logits[0, [2, 5, 9]] = 4.0                     # classes 2, 5, 9 share the target's value, target 5: class 2 is ahead
    logits[1] = 0.0                                # all equal, target t: rank t
    logits[2] = 0.0
    logits[3, [100, 300]] = 2.0                    # a tie across lanes
    logits[4, [256, 512]] = 3.0                    # a tie between a lane's first and a later group
    logits[5, [6, 7]] = 1.0                        # a tie inside one float4 group
    target = torch.tensor([5, 0, 512, 300, 512, 7])
    x = rows_on_device(logits)
    _, _, rank = amd.ops.prior_eval_rows(x, target.cuda().view(1, 6, 1), n_class)
    assert rank.tolist() == [1, 0, 512, 1, 1, 1]
    assert torch.equal(rank.cpu().long(), E.brute_rank(logits, target))
    ok, count = xent_rows(amd, x, target.cuda(), n_class)
    assert ok.tolist() == [0, 1, 0, 0, 0, 0] and count == 1
    for c in (6, 513):
        g = torch.Generator().manual_seed(c)
        lg = torch.randn(4, c, generator=g)
        tg = torch.tensor([1, -1, c, 2 ** 40])
        nll, entropy, rank = amd.ops.prior_eval_rows(rows_on_device(lg), tg.cuda().view(1, 4, 1), c)
        torch.cuda.synchronize()
        n64, h64, r64 = E.row_quantities(lg, tg)
        assert rank.tolist() == [int(r64[0]), -1, -1, -1] and nll[1:].tolist() == [0.0, 0.0, 0.0]
        E.bound(f"entropy beside a bad target C={c}", entropy.cpu(), h64, E.row_quantities(lg, tg, torch.float32)[1])


def test_rows_refusals(amd):
    ops = amd.ops
    x = torch.zeros(1, 2, 2, 8, device="cuda")
    t = torch.zeros(1, 2, 2, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):
        ops.prior_eval_rows(x, t.int(), 6)
    with pytest.raises(RuntimeError):
        ops.prior_eval_rows(x, t[:, :1], 6)
    with pytest.raises(RuntimeError):
        ops.prior_eval_rows(x, t, 12)                      # 8 stored lanes are not ceil4(12)
    with pytest.raises(RuntimeError):
        ops.prior_eval_rows(x.double(), t, 6)


# ----------------------------------------------------------------------------------------------- 2. accumulate
@pytest.mark.parametrize("top_k", [1, 5, 600])
@pytest.mark.parametrize("shape", [(1, 1), (3, 6), (2, 72), (3, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_accumulate_equals_the_ordered_double_loop(amd, shape, top_k):
    n, length = shape
    n_class = 6
    rng = np.random.default_rng(zlib.crc32(f"acc-{n}-{length}-{top_k}".encode()))
    dev_state = {k: torch.from_numpy(v).cuda() for k, v in E.new_state(length).items()}
    ref = E.new_state(length)
    for call in range(2):                                   # the second call accumulates on the first
        nll = (rng.random(n * length, dtype=np.float32) * np.float32(12.0)) * np.float32(10.0) ** rng.integers(-12, 1, n * length).astype(np.float32)
        ent = rng.random(n * length, dtype=np.float32) * np.float32(np.log(n_class))
        rank = rng.integers(-1, n_class, n * length).astype(np.int32)
        want_image = E.accumulate(ref, nll, ent, rank, n, length, top_k)
        args = (torch.from_numpy(nll).cuda(), torch.from_numpy(ent).cuda(), torch.from_numpy(rank).cuda(), n, top_k,
                dev_state["pos_nll"], dev_state["pos_entropy"], dev_state["pos_hit1"], dev_state["pos_hitk"], dev_state["counters"])
        image = amd.ops.prior_eval_accumulate(*args, return_image_nll=(call == 0))
        torch.cuda.synchronize()
        if call == 0:
            assert image.dtype == torch.float32 and image.cpu().numpy().tobytes() == want_image.tobytes()
        else:
            assert image is None                            # a NULL image_nll is accepted
        for k in ref:
            assert dev_state[k].cpu().numpy().tobytes() == ref[k].tobytes(), (k, call)
    assert ref["counters"][0] == 2 * n


def test_accumulate_refusals(amd):
    f = lambda n, dt=torch.float32: torch.zeros(n, device="cuda", dtype=dt)      # noqa: E731
    good = dict(pos_nll=f(3, torch.float64), pos_entropy=f(3, torch.float64), pos_hit1=f(3, torch.int64),
                pos_hitk=f(3, torch.int64), counters=f(2, torch.int64))
    acc = amd.ops.prior_eval_accumulate
    acc(f(6), f(6), f(6, torch.int32), 2, 1, **good)
    with pytest.raises(RuntimeError):
        acc(f(6), f(6), f(6, torch.int64), 2, 1, **good)
    with pytest.raises(RuntimeError):
        acc(f(6), f(6), f(6, torch.int32), 4, 1, **good)
    with pytest.raises(RuntimeError):
        acc(f(6), f(6), f(6, torch.int32), 2, 0, **good)
    with pytest.raises(RuntimeError):
        acc(f(6), f(6), f(6, torch.int32), 2, 1, **dict(good, pos_nll=f(3)))
    with pytest.raises(RuntimeError):
        acc(f(6), f(6), f(6, torch.int32), 2, 1, **dict(good, counters=f(3, torch.int64)))


# ----------------------------------------------------------------------------------------------- 3. batching
@pytest.mark.parametrize("ci", S.CASES, ids=["attention", "conditioned"])
def test_batches_of_5_3_1_leave_the_state_of_one_batch_of_9(amd, ci):
    hier, cond, codes = K.held_out(ci, 9, 31 + ci)
    model = S.build(amd, ci)
    whole = K.evaluate(amd, model, hier, cond, codes, [9])
    parts = K.evaluate(amd, model, hier, cond, codes, [5, 3, 1])
    torch.cuda.synchronize()
    assert whole._state.dtype == torch.int64 and whole._state.numel() == 4 * codes[0].numel() + 2 + whole.n_class + 1
    assert torch.equal(whole._state, parts._state)
    assert int(whole._state[4 * codes[0].numel()]) == 9
    with pytest.raises(ValueError):
        if hier == "top":
            parts.update(codes[:1, :-1].cuda())
        else:
            parts.update(cond[:1, :-1].cuda(), codes[:1, :-2].cuda())
    assert torch.equal(whole._state, parts._state)
    parts.reset()
    assert int(parts._state.abs().sum()) == 0 and parts.result()["images"] == 0
    assert all(m.training for m in model.modules())            # the model came in train mode and leaves in it


# ----------------------------------------------------------------------------------------------- 4. against fp64
REF_SEED = {0: 100, 1: 101}     # seeds at which the float64 and the float32 reference agree on every rank (asserted below)


@pytest.mark.parametrize("ci", S.CASES, ids=["attention", "conditioned"])
def test_evaluator_and_score_codes_against_fp64(amd, ci):
    """nll, entropy, nll_map and score_codes within 4 x the error of the float32 run of tests/_pixelsnail_model_ref.py, both
    against its float64 run; each run is in its own precision throughout (tests/_prior_eval_ref.totals)."""
    g = M.load()
    c = M.cases(g)[ci]
    hier, cond, codes = K.held_out(ci, 3, REF_SEED[ci])
    sd = M.state_dict(g, ci)
    top_k = 3
    ref = E.model_rows(M, sd, codes, c["n_class"], c["attention"], cond, torch.float64)
    ref32 = E.model_rows(M, sd, codes, c["n_class"], c["attention"], cond, torch.float32)
    assert torch.equal(ref[2], ref32[2]), "the two references disagree on a rank: choose another seed"
    want, want32 = E.totals(*ref, top_k), E.totals(*ref32, top_k)
    model = S.build(amd, ci)
    ev = K.evaluate(amd, model, hier, cond, codes, [2, 1], top_k=top_k)
    r = ev.result()
    assert r["images"] == 3 and r["codes"] == codes.numel() and r["top_k"] == top_k
    missed = []
    errs = [E.bound(f"case {ci} nll", r["nll"], want["nll"], want32["nll"], missed),
            E.bound(f"case {ci} entropy", r["entropy"], want["entropy"], want32["entropy"], missed),
            E.bound(f"case {ci} nll_map", r["nll_map"].reshape(-1), want["nll_map"], want32["nll_map"], missed)]
    args = (codes.cuda(),) if cond is None else (codes.cuda(), cond.cuda())
    logp = amd.score_codes(model, *args)
    assert logp.dtype == torch.float32 and logp.shape == (3,) and logp.is_cuda
    errs.append(E.bound(f"case {ci} score_codes", logp.cpu(), -want["image_nll"], -want32["image_nll"], missed))
    assert not missed, missed
    assert max(errs) > 0
    assert want32["nll"].dtype == torch.float32 and want["nll"].dtype == torch.float64
    assert r["accuracy"] == want["accuracy"] and r["top_k_accuracy"] == want["top_k_accuracy"]
    assert r["bits_per_code"] == r["nll"] / math.log(2.0) and r["perplexity"] == math.exp(r["nll"])
    counts = torch.bincount(codes.reshape(-1), minlength=c["n_class"])
    assert torch.equal(r["counts"], counts)
    assert r["unigram_nll"] == math.log(amd.perplexity_from_counts(counts))
    assert r["nll_map"].shape == tuple(codes.shape[1:]) and len(r["nll_rows"]) == codes.shape[1]
    assert r["nll_rows"] == [float(v) for v in r["nll_map"].mean(1)]
    # return_image_nll is the same per-image sum that score_codes negates
    ev2 = amd.PriorEvaluator(model, hier, top_k=top_k)
    image = ev2.update(*((codes.cuda(),) if cond is None else (cond.cuda(), codes.cuda())), return_image_nll=True)
    assert torch.equal(image, -logp)
    assert all(m.training for m in model.modules())
    # a target outside the classes is reported by result()
    bad = codes.clone()
    bad[0, 0, 0] = c["n_class"]
    ev2.update(*((bad.cuda(),) if cond is None else (cond.cuda(), bad.cuda())))
    with pytest.raises(RuntimeError, match="outside"):
        ev2.result()


# ----------------------------------------------------------------------------------------------- 5. training is left alone
def _flat(sd, prefix=""):
    out = {}
    for k, v in sd.items():
        if isinstance(v, dict):
            out.update(_flat(v, prefix + k + "."))
        else:
            out[prefix + k] = v.detach().cpu().numpy().tobytes() if torch.is_tensor(v) else v
    return out


@pytest.mark.parametrize("ci", S.CASES, ids=["attention", "conditioned"])
def test_evaluation_between_steps_changes_nothing(amd, ci):
    hier, args = S.batch(ci)
    _, cond, codes = K.held_out(ci, 3, 55)
    batches = [(codes[:2], codes[:2], "a") if cond is None else (cond[:2], codes[:2], "a"),
               (codes[2:], codes[2:]) if cond is None else (cond[2:], codes[2:])]

    def run(evaluate):
        model = S.build(amd, ci, dropout=0.1)
        model.horizontal.eval()                       # a module of its own mode: evaluate() has to give it back as it was
        tr = amd.Stage2Trainer(model, hier, lr=1e-3, sched="cycle", n_iter=S.N_ITER)
        torch.manual_seed(17)
        losses = [float(tr.step(*args)["loss"]) for _ in range(2)]
        held = None
        if evaluate:
            flags = [m.training for m in model.modules()]
            rng = torch.get_rng_state()
            held = tr.evaluate(batches, top_k=2)
            assert [m.training for m in model.modules()] == flags and not all(flags) and any(flags)
            assert torch.equal(torch.get_rng_state(), rng)                 # no dropout seed was drawn
            assert held["images"] == 3 and held["top_k"] == 2 and np.isfinite(held["nll"])
        losses += [float(tr.step(*args)["loss"]) for _ in range(2)]
        torch.cuda.synchronize()
        return _flat(model.state_dict()), _flat(tr.state_dict()), losses, held, tr

    sd_a, tr_a, loss_a, _, _ = run(False)
    sd_b, tr_b, loss_b, held, tr = run(True)
    assert loss_a == loss_b
    assert sd_a.keys() == sd_b.keys() and all(sd_a[k] == sd_b[k] for k in sd_a), [k for k in sd_a if sd_a[k] != sd_b[k]]
    assert tr_a.keys() == tr_b.keys() and all(tr_a[k] == tr_b[k] for k in tr_a), [k for k in tr_a if tr_a[k] != tr_b[k]]
    # what evaluate() scored is the parameters as they were between the steps: the same trainer, evaluated now, differs
    assert tr.evaluate(batches, top_k=2)["nll"] != held["nll"]


# ----------------------------------------------------------------------------------------------- 6. two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_equal_one_rank(amd, tmp_path):
    """Two gloo ranks (two fresh child processes on the one GPU) score the rows 0, 2, 4 and 1, 3, 5; this process scores all
    six.  Integers are equal.  A float64 total of the group is the sum of two doubles, each the exact running sum one rank
    took in its own order, where the single process adds the six rows in one chain: the two differ by the rounding of a few
    additions of like-signed terms, a relative 2^-53 each -- 1e-12 leaves three decimal orders of room."""
    ci = 0
    out = str(tmp_path / "ev")
    port = _free_port()
    env = dict(os.environ, PYTHONPATH=ROOT)
    child = os.path.join(ROOT, "tests", "_prior_eval_child.py")
    procs = [subprocess.Popen([sys.executable, child, str(rank), "2", str(port), out, str(ci)], cwd=ROOT, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in (0, 1)]
    logs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(log[-3000:] for log in logs)
    hier, cond, codes = K.held_out(ci, 6, 77)
    one = K.evaluate(amd, S.build(amd, ci), hier, cond, codes, [4, 2]).result()
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    for r in (r0, r1):
        for k in ("images", "codes", "top_k", "accuracy", "top_k_accuracy", "unigram_nll"):
            assert r[k] == one[k], k
        assert np.array_equal(r["counts"], one["counts"].numpy())
        for k in ("nll", "entropy", "bits_per_code", "perplexity"):
            assert abs(float(r[k]) - one[k]) <= 1e-12 * abs(one[k]), k
        assert np.all(np.abs(r["nll_map"] - one["nll_map"].numpy()) <= 1e-12 * np.abs(one["nll_map"].numpy()))
    assert all(r0[k].tobytes() == r1[k].tobytes() for k in r0.files)
    assert int(one["images"]) == 6


# ----------------------------------------------------------------------------------------------- 7. example scripts
def _write_codes(amd, path, n, seed):
    g = torch.Generator().manual_seed(seed)
    tops = torch.randint(0, 6, (n, 4, 5), generator=g)
    bottoms = torch.randint(0, 6, (n, 8, 10), generator=g)
    with amd.codes.CodeStore(str(path), "w", backend="sqlite") as store:
        end = amd.codes.write_code_rows(store, tops, bottoms, [f"{i}.png" for i in range(n)])
        store.put(b"length", str(end).encode())
    return tops


def test_example_scripts_train_with_validation_then_evaluate(amd, tmp_path):
    _write_codes(amd, tmp_path / "train.db", 8, 1)
    tops = _write_codes(amd, tmp_path / "val.db", 5, 2)            # batches of 2, 2 and a ragged 1
    env = dict(os.environ, PYTHONPATH=ROOT)
    model_args = ["--hier", "top", "--size", "4", "5", "--n_class", "6", "--channel", "64", "--n_res_block", "1",
                  "--n_res_channel", "8", "--n_block", "1", "--kernel_size", "3", "--batch", "2"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_pixelsnail.py"), *model_args, "--epoch", "1",
                        "--max_steps", "4", "--workers", "0", "--seed", "3", "--ckpt_dir", "ckpt", "--val_path", "val.db",
                        "--eval_every", "2", "train.db"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    held = [l for l in r.stdout.splitlines() if "held-out" in l]
    assert len(held) == 2 and held[0].startswith("step: 2; held-out images: 5;") and held[1].startswith("step: 4;"), r.stdout
    assert len([l for l in r.stdout.splitlines() if l.startswith("epoch: 1; loss:")]) == 4
    ckpt = tmp_path / "ckpt" / "pixelsnail_top_001.pt"
    assert ckpt.exists()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "eval_pixelsnail.py"), "--ckpt", str(ckpt), "--hier", "top",
                        "--batch", "2", "--top_k", "5", "--dump_map", "map.npy", "val.db"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("images: ")]
    assert len(line) == 1, r.stdout
    model = amd.load_model("pixelsnail_top", "pixelsnail_top_001.pt", "cuda", ckpt_dir=str(tmp_path / "ckpt"))
    ev = amd.PriorEvaluator(model, "top", top_k=5)
    for lo in (0, 2, 4):
        ev.update(tops[lo:lo + 2].cuda())
    direct = ev.result()
    assert line[0] == amd.PriorEvaluator.summary(direct)
    assert np.load(tmp_path / "map.npy").tobytes() == direct["nll_map"].numpy().tobytes()
    # the run's own last validation saw the parameters the checkpoint holds
    assert held[1] == "step: 4; held-out " + line[0]


# ----------------------------------------------------------------------------------------------- 8. registers
def test_prior_eval_kernels_do_not_spill():
    """The compiler's resource report of csrc/vq2_eval.hip (written by csrc/build.sh): no spilled register and no scratch
    in the two kernels of the prior's evaluation."""
    files = glob.glob(os.path.join(ROOT, "vq-vae-2-pytorch_amd", "csrc", "_obj", "vq2_eval.res"))
    assert files, "csrc/_obj/vq2_eval.res is missing: csrc/build.sh lists vq2_eval and writes the report with the object"
    hot = re.compile(r"prior_eval_rows_kernel|prior_eval_accumulate_kernel")
    seen, name = 0, None
    for line in open(files[0]):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen += bool(hot.search(name))
            continue
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name and hot.search(name):
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
    assert seen == 2, f"{seen} kernels found in the report, expected 2"
