"""GPU: the table-driven weight-norm kernels against the per-layer ones (bit for bit, sentinels around every slot), and
Stage2Trainer's arena path -- against arena=False, through a checkpoint, over RCCL at world size 1 and with two ranks over
gloo -- always bit for bit: the same kernels see the same numbers in the same order on either side."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _stage2_child as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.5

# (rows, cols, kh, kw, mask_from); several numels are no multiple of 4, the last entry has a multi-row kernel and no mask
ENTRIES = [(1, 1, 1, 1, 1), (3, 63, 1, 1, 1), (64, 64, 1, 1, 1), (65, 65, 1, 1, 1), (5, 130, 1, 1, 1), (6, 7 * 9, 3, 3, 1),
           (4, 5 * 15, 3, 5, 2), (2, 3 * 3, 1, 3, 1), (7, 2 * 6, 2, 3, 3)]


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _ceil4(n):
    return (n + 3) // 4 * 4


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def table(amd):
    """One arena [g0 v0 g1 v1 ...] and one flat weight buffer, every slot on a 16-byte boundary, sentinels everywhere
    else; the table in device memory.  Leaves everything as built: the tests work on clones."""
    L = amd._lib
    gen = torch.Generator().manual_seed(3)
    arr = (L.WnEntry * (len(ENTRIES) + 1))()
    off = w_off = row_start = 0
    for i, (rows, cols, kh, kw, mask_from) in enumerate(ENTRIES):
        e = arr[i]
        e.rows, e.cols, e.kh, e.kw, e.mask_from, e.row_start = rows, cols, kh, kw, mask_from, row_start
        e.g_off = off
        off += _ceil4(rows)
        e.v_off = off
        off += _ceil4(rows * cols)
        e.w_off = w_off
        w_off += _ceil4(rows * cols)
        row_start += rows
    arr[len(ENTRIES)].row_start = row_start
    params = torch.full((off,), SENTINEL)
    dw = torch.full((w_off,), SENTINEL)
    for e in list(arr)[:-1]:
        n = e.rows * e.cols
        params[e.g_off:e.g_off + e.rows] = torch.randn(e.rows, generator=gen)
        params[e.v_off:e.v_off + n] = torch.randn(n, generator=gen)
        dw[e.w_off:e.w_off + n] = torch.randn(n, generator=gen)
    dev = amd.ops._upload_structs(arr, "cuda")
    return dict(entries=list(arr)[:-1], dev=dev, params=params.cuda(), dw=dw.cuda(), n_p=off, n_w=w_off)


def _masked(e, v):
    """weight_v [rows, cols] of entry e with the 'causal' zeros in it."""
    v = v.clone().view(e.rows, e.cols // (e.kh * e.kw), e.kh, e.kw)
    v[:, :, -1, e.mask_from:] = 0
    return v.view(e.rows, e.cols)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_table_forward_equals_the_per_layer_kernel(amd, table):
    lib, check = amd._lib.lib, amd._lib.check
    params, w = table["params"].clone(), torch.full((table["n_w"],), SENTINEL, device="cuda")
    want_p, want_w = table["params"].clone(), w.clone()
    for e in table["entries"]:
        n = e.rows * e.cols
        v = _masked(e, table["params"][e.v_off:e.v_off + n]).contiguous()
        g = table["params"][e.g_off:e.g_off + e.rows].clone()
        ref = torch.empty_like(v)
        check(lib.vq2_weight_norm_fwd(_p(v), _p(g), _p(ref), e.rows, e.cols, _stream()), "weight_norm_fwd")
        want_p[e.v_off:e.v_off + n] = v.view(-1)
        want_w[e.w_off:e.w_off + n] = ref.view(-1)
        if e.mask_from < e.kw:
            assert int((v == 0).sum()) == e.rows * (e.cols // (e.kh * e.kw)) * (e.kw - e.mask_from)    # exactly the masked ones
    check(lib.vq2_wn_table_fwd(_p(table["dev"]), len(ENTRIES), _p(params), _p(w), _stream()), "wn_table_fwd")
    torch.cuda.synchronize()
    assert torch.equal(w, want_w)           # every row bit for bit, every pad float still the sentinel
    assert torch.equal(params, want_p)      # zeros exactly where the mask is; g, the rest of v and the pads untouched
    assert not torch.equal(params, table["params"])


@pytest.mark.parametrize("first,last", [(0, len(ENTRIES)), (0, 0), (2, 3), (3, len(ENTRIES))])
def test_table_backward_equals_the_per_layer_kernel(amd, table, first, last):
    lib, check = amd._lib.lib, amd._lib.check
    params = table["params"].clone()
    for e in table["entries"]:              # the parameters as the forward leaves them
        n = e.rows * e.cols
        params[e.v_off:e.v_off + n] = _masked(e, params[e.v_off:e.v_off + n]).view(-1)
    dw = table["dw"].clone()
    grads = torch.full((table["n_p"],), SENTINEL, device="cuda")
    want = grads.clone()
    for e in table["entries"][first:last]:
        n = e.rows * e.cols
        v, g = params[e.v_off:e.v_off + n].clone(), params[e.g_off:e.g_off + e.rows].clone()
        d = dw[e.w_off:e.w_off + n].clone()
        dv, dg = torch.empty_like(v), torch.empty_like(g)
        check(lib.vq2_weight_norm_bwd(_p(d), _p(v), _p(g), _p(dv), _p(dg), e.rows, e.cols, _stream()), "weight_norm_bwd")
        want[e.v_off:e.v_off + n] = dv
        want[e.g_off:e.g_off + e.rows] = dg
    p0, d0 = params.clone(), dw.clone()
    check(lib.vq2_wn_table_bwd(_p(table["dev"]), first, last, _p(params), _p(dw), _p(grads), _stream()), "wn_table_bwd")
    torch.cuda.synchronize()
    assert torch.equal(grads, want)         # the range bit for bit; everything outside it and every pad: the sentinel
    assert torch.equal(params, p0) and torch.equal(dw, d0)
    assert (first == last) == bool((grads == SENTINEL).all())


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def plain(amd):
    """Three steps of the arena path in this process, per golden case: what every other way of running it must equal."""
    return {ci: S.run(amd, ci, 3) for ci in S.CASES}


@pytest.mark.parametrize("ci", S.CASES, ids=["attention", "conditioned"])
def test_arena_path_equals_the_per_layer_path(amd, plain, ci):
    sd_new, loss_new, tr_new = plain[ci]
    sd_old, loss_old, tr_old = S.run(amd, ci, 3, arena=False)
    n_wn = sum(1 for k in sd_new if k.endswith("weight_g"))
    assert tr_new.plan_info["entries"] == n_wn and tr_new.plan_info["per_layer"] == 0      # every layer took the table path
    assert tr_old.plan_info["entries"] == 0 and tr_old.plan_info["per_layer"] == n_wn
    assert tr_new.arena is not None and tr_old.arena is None and not tr_new.dp
    assert loss_new == loss_old
    _same(sd_new, sd_old, f"case {ci}")
    assert tr_new.arena.grads_ready()


@pytest.mark.parametrize("ci", S.CASES, ids=["attention", "conditioned"])
def test_resume_continues_exactly(amd, ci):
    hier, args = S.batch(ci)

    def trainer(sched="cycle"):
        return amd.Stage2Trainer(S.build(amd, ci), hier, lr=1e-3, sched=sched, n_iter=S.N_ITER)

    def steps(tr, n, seed):
        torch.manual_seed(seed)
        return [float(tr.step(*args)["loss"]) for _ in range(n)]

    whole = trainer()
    l_whole = steps(whole, 2, 21) + steps(whole, 2, 22)
    first = trainer()
    l_first = steps(first, 2, 21)
    ck = first.state_dict()
    assert sorted(ck) == ["adam_m", "adam_t", "adam_v", "betas", "lr", "model", "scheduler"]
    assert sorted(ck["model"]) == sorted(first.model.state_dict()) and ck["adam_t"] == 2 and ck["scheduler"] == {"t": 2}
    assert ck["adam_m"].numel() == sum(p.numel() for p in first.model.parameters())
    ck = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ck.items()}
    ck["model"] = {k: v.cpu() for k, v in ck["model"].items()}
    second = trainer()
    with torch.no_grad():
        for p in second.model.parameters():     # a fresh model would differ: make sure the checkpoint is what counts
            p.add_(0.25)
    second.load_state_dict(ck)
    l_second = steps(second, 2, 22)
    torch.cuda.synchronize()
    assert l_first + l_second == l_whole
    _same(S.numpy_sd(second.model), S.numpy_sd(whole.model), f"case {ci}")
    # a bare model dict, with DataParallel's prefix too: weights load, the optimizer starts fresh
    bare = trainer()
    bare.load_state_dict({"module." + k: v for k, v in ck["model"].items()})
    _same(S.numpy_sd(bare.model), {k: v.numpy() for k, v in ck["model"].items()}, "bare")
    assert bare.optimizer._t == 0
    bare.load_state_dict(ck["model"])
    with pytest.raises(RuntimeError, match="sched"):
        trainer(sched=None).load_state_dict(ck)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _check_slices(facts):
    lo_hi = [tuple(s) for s in facts["slices"]]
    assert len(lo_hi) == 2 and lo_hi[0][0] == 0 and lo_hi[0][1] == lo_hi[1][0] and lo_hi[1][1] == facts["total"]
    assert sorted(facts["bucket_bytes"]) == ["early", "late"] and sum(facts["bucket_bytes"].values()) == 4 * facts["total"]


@pytest.mark.parametrize("comm", ["torch", "capi"])
def test_world1_over_rccl_equals_plain_run(amd, plain, tmp_path, comm):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VQ2_DP_FORCE="1", VQ2_COMM=comm)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "_stage2_child.py"), str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    info = json.load(open(tmp_path / "info.json"))
    assert info["data_path"] == ("libvq2 vq2_comm" if comm == "capi" else "torch.distributed")
    for ci in S.CASES:
        sd, losses, tr = plain[ci]
        facts = info[str(ci)]
        assert facts["dp"] and facts["world"] == 1 and facts["per_layer"] == 0
        assert facts["early"] >= 3, "the early slice must go out from the backward hook every step"
        _check_slices(facts)
        assert facts["losses"] == losses
        _same(dict(np.load(tmp_path / f"c{ci}.npz")), sd, f"case {ci} over RCCL")


def test_two_ranks_same_batch_equal_the_plain_run(amd, plain, tmp_path):
    """Both ranks see the same batch and draw the same dropout seeds, from different initial weights: after the initial
    broadcast both compute rank 0's gradient g, and (g + g) * 0.5 is g exactly."""
    out = str(tmp_path / "same")
    mp.spawn(S.gloo_worker, args=(2, _free_port(), out, "same"), nprocs=2, join=True)
    facts = [json.load(open(f"{out}.rank{r}.json")) for r in (0, 1)]
    for ci in S.CASES:
        sd, losses, _ = plain[ci]
        for r in (0, 1):
            f = facts[r][str(ci)]
            assert f["losses"] == losses and f["early"] >= 3 and f["world"] == 2
            _check_slices(f)
            _same(dict(np.load(f"{out}.c{ci}.rank{r}.npz")), sd, f"case {ci} rank {r}")


@pytest.mark.parametrize("ci", S.CASES, ids=["attention", "conditioned"])
def test_two_ranks_split_batch_equal_the_summed_gradients(amd, tmp_path, ci):
    """Different batches per rank, dropout 0, one step: both ranks end equal, and equal to one process that back-propagates
    both batches on the per-layer path, adds the two gradients in torch (a two-operand fp32 sum has one value in either
    order) and lets Adam halve the sum."""
    from vqvae2_amd.optim import FusedAdam
    out = str(tmp_path / "split")
    mp.spawn(S.gloo_worker, args=(2, _free_port(), out, "split", (ci,)), nprocs=2, join=True)
    r0, r1 = dict(np.load(f"{out}.c{ci}.rank0.npz")), dict(np.load(f"{out}.c{ci}.rank1.npz"))
    _same(r0, r1, f"case {ci}: replicas")
    m = S.build(amd, ci, dropout=0.0)
    grads = []
    for variant in (0, 1):
        hier, args = S.batch(ci, variant)
        m.zero_grad(set_to_none=True)
        logits, _ = m(args[0]) if hier == "top" else m(args[1], condition=args[0])
        loss, _ = amd.prior_loss(logits, args[-1])
        loss.backward()
        grads.append([p.grad.clone() for p in m.parameters()])
    for p, ga, gb in zip(m.parameters(), *grads):
        p.grad = ga + gb
    opt = FusedAdam(m.parameters(), lr=1e-3)
    opt.grad_scale = 0.5
    opt.step()
    torch.cuda.synchronize()
    _same(r0, S.numpy_sd(m), f"case {ci}: against the summed gradients")
