"""The bf16-operand weight gradient (VQ2_ALLOW_BF16 in the flags of vq2_conv_wgrad, ConvSpec.bf16_wgrad) on the GPU, against
the references of tests/_wgrad_bf16_cases.py: dw within the project's tolerance of the fp64 gradient of the bf16-ROUNDED
operands and outside it of the unrounded one, db within it of the fp64 sum of the UNROUNDED dy; reproducible; nothing read
or written beyond the tensors; the layer that is not eligible and every spec without the permission unchanged; the deferred
path bit for bit the immediate one; the _ex entry points with flag 0 the old ones."""
import ctypes as C
import dataclasses
import functools

import pytest
import torch

import _wgrad_bf16_cases as W
from test_gpu_dispatch import launched, sliced

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT, GUARD = -1234.5, 64      # guard floats behind dw, db and the workspace
ALL = W.CASES + [W.NOT_ELIGIBLE]


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


@functools.lru_cache(maxsize=None)
def _refs(name):
    """Inputs and the fp64 references of a case, computed once: dw of the rounded and of the unrounded operands for both
    ReLU settings, db."""
    c = W.BY_NAME[name]
    d = W.make_inputs(c)
    return d, {(r, rounded): W.dw_ref(c, d, r, rounded=rounded) for r in (False, True) for rounded in (False, True)}, W.db_ref(c, d)


def _spec(amd, c, permission=True):
    from vqvae2_amd import ops
    return dataclasses.replace(ops.ConvSpec.geom(*c[1:7]), bf16_wgrad=permission)


def _wgrad_labels(seen):
    return [s for s in seen if s.startswith("wgrad")]


def _run(amd, c, spec, relu_in, bias=True, x=None, dy=None):
    from vqvae2_amd import ops
    d = _refs(c[0])[0]
    x = d["x"].to(DEV) if x is None else x
    dy = d["dy"].to(DEV) if dy is None else dy
    wt, b = d["w"].to(DEV), (d["b"].to(DEV) if bias else None)
    (dw, db), seen = launched(amd, lambda: ops.conv_wgrad(spec, x, dy, relu_in, wt, b))
    return dw, db, _wgrad_labels(seen)


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c[0])
def test_dw_matches_fp64_of_the_rounded_operands_and_db_of_the_unrounded_dy(amd, c):
    d, dws, rb = _refs(c[0])
    for relu_in in (False, True):
        for bias in (True, False):
            dw, db, labels = _run(amd, c, _spec(amd, c), relu_in, bias)
            assert len(labels) == 1 and labels[0].startswith("wgrad<") and labels[0].endswith(",bf16"), labels
            assert ("S=" in labels[0]) and (",k%d," % c[3]) in labels[0]
            ref, exact = dws[(relu_in, True)], dws[(relu_in, False)]
            tol = W.tolerance(c, ref)
            err = float((dw.cpu().double() - ref).abs().max())
            gap = float((dw.cpu().double() - exact).abs().max())
            print("%s relu_in=%d bias=%d %s: dw err %.3e tol %.3e; against the unrounded reference %.3e (tol %.3e)"
                  % (c[0], relu_in, bias, labels[0], err, tol, gap, W.tolerance(c, exact)))
            assert err <= tol
            assert gap > W.tolerance(c, exact), "dw is inside the tolerance of the UNROUNDED reference"
            if bias:
                berr = float((db.cpu().double() - rb).abs().max())
                print("    db err %.3e tol %.3e" % (berr, W.tolerance(c, rb)))
                assert berr <= W.tolerance(c, rb)
            else:
                assert db is None
            # a second call gives the same bits
            dw2, db2, _ = _run(amd, c, _spec(amd, c), relu_in, bias)
            assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2))
    assert "S=1," not in _run(amd, W.BY_NAME["e"], _spec(amd, W.BY_NAME["e"]), False)[2][0]      # (e) is split


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c[0])
def test_sliced_operands_neighbours_unread(amd, c):
    """x and dy as channel slices of wider buffers (ldx, ldy past the channel counts): the same bits as from dense tensors,
    and filling the neighbouring channels with NaN changes nothing."""
    d = _refs(c[0])[0]
    dw, db, _ = _run(amd, c, _spec(amd, c), True)
    xw, xs = sliced(d["x"], DEV)
    gw, gs = sliced(d["dy"], DEV)
    dw1, db1, labels = _run(amd, c, _spec(amd, c), True, x=xs, dy=gs)
    assert labels[0].endswith(",bf16") and torch.equal(dw, dw1) and torch.equal(db, db1)
    for wide, cdim in ((xw, d["x"].shape[3]), (gw, d["dy"].shape[3])):
        wide[..., :4] = float("nan")
        wide[..., 4 + cdim:] = float("nan")
    dw2, db2, _ = _run(amd, c, _spec(amd, c), True, x=xs, dy=gs)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c[0])
def test_guards_behind_dw_db_and_workspace_are_untouched(amd, c):
    """The C entry point on sentinel-filled buffers: dw, db and the workspace of exactly the size the library asks for,
    GUARD floats behind each."""
    from vqvae2_amd import ops
    lib = amd._lib.lib
    d = _refs(c[0])[0]
    spec = _spec(amd, c)
    x, dy = d["x"].to(DEV), d["dy"].to(DEV)
    desc = ops._desc(spec, c[7], c[8], c[9], spec.ci, spec.co)
    flags = ops.VQ2_ALLOW_BF16 | ops.VQ2_RELU_IN
    nbytes = lib.vq2_conv_wgrad_workspace_bytes_ex(C.byref(desc), flags)
    assert nbytes % 4 == 0
    nw, nb = d["w"].numel(), d["b"].numel()
    bufs = [torch.full((n + GUARD,), SENT, device=DEV) for n in (nw, nb, nbytes // 4)]
    rc = lib.vq2_conv_wgrad(C.byref(desc), flags, x.data_ptr(), dy.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(),
                            bufs[2].data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vq2_last_error()
    torch.cuda.synchronize()
    for buf, n in zip(bufs, (nw, nb, nbytes // 4)):
        assert bool((buf[n:] == SENT).all())
    assert not bool((bufs[2][:nbytes // 4] == SENT).any()), "part of the workspace was left unwritten"
    dw, db, _ = _run(amd, c, spec, True)
    assert torch.equal(bufs[0][:nw].view_as(dw), dw) and torch.equal(bufs[1][:nb], db)
    # a workspace one float short is refused before any launch
    rc = lib.vq2_conv_wgrad(C.byref(desc), flags, x.data_ptr(), dy.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(),
                            bufs[2].data_ptr(), nbytes - 4, torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"workspace too small" in lib.vq2_last_error()


def test_the_layer_that_is_not_eligible_runs_the_fp32_kernel(amd):
    c = W.NOT_ELIGIBLE
    for relu_in in (False, True):
        dw, db, labels = _run(amd, c, _spec(amd, c, True), relu_in)
        dw0, db0, labels0 = _run(amd, c, _spec(amd, c, False), relu_in)
        assert labels == labels0 and not labels[0].endswith(",bf16"), labels
        assert torch.equal(dw, dw0) and torch.equal(db, db0)


@pytest.mark.parametrize("c", ALL, ids=lambda c: c[0])
def test_without_the_permission_nothing_changes(amd, c):
    """bf16_wgrad=False, with or without the forward's bf16 permission, is a spec that never had the field set."""
    from vqvae2_amd import ops
    plain = ops.ConvSpec.geom(*c[1:7])
    dw0, db0, labels0 = _run(amd, c, plain, True)
    assert not labels0[0].endswith(",bf16")
    for spec in (_spec(amd, c, False), dataclasses.replace(plain, bf16=True)):
        dw, db, labels = _run(amd, c, spec, True)
        assert labels == labels0 and torch.equal(dw, dw0) and torch.equal(db, db0)
    tol = W.tolerance(c, _refs(c[0])[1][(True, False)])
    assert float((dw0.cpu().double() - _refs(c[0])[1][(True, False)]).abs().max()) <= tol      # the fp32 gradient, unrounded


@pytest.mark.parametrize("c", [W.BY_NAME[n] for n in ("a", "e", "g", "i", "n")], ids=lambda c: c[0])
def test_deferred_weight_gradient_equals_the_immediate_one_bitwise(amd, c):
    """Inside an active StepContext, with arena slots on weight and bias, conv_wgrad writes only the slabs
    (vq2_conv_wgrad_partial); flush() reduces them with the batched reduction into the slots: the same bits as the
    immediate call, under the same weight-gradient label."""
    from vqvae2_amd import ops
    d = _refs(c[0])[0]
    x, dy = d["x"].to(DEV), d["dy"].to(DEV)
    for permission in (True, False):
        spec = _spec(amd, c, permission)
        for relu_in in (True, False):
            dw, db, labels = _run(amd, c, spec, relu_in)
            assert labels[0].endswith(",bf16") == (permission and c[0] != "n")
            w2, b2 = d["w"].to(DEV), d["b"].to(DEV)
            w2._vq2_grad, b2._vq2_grad = torch.full_like(w2, 7.0), torch.full_like(b2, 7.0)      # the slots of a ParamArena
            ctx = ops.StepContext(torch.cuda.Stream())
            w2._vq2_ctx = b2._vq2_ctx = ctx

            def deferred():
                ctx.active = True
                try:
                    out = ops.conv_wgrad(spec, x, dy, relu_in, w2, b2)
                finally:
                    ctx.active = False
                assert float(w2._vq2_grad[0, 0, 0, 0]) == 7.0                # nothing reduced yet
                torch.cuda.current_stream().wait_stream(ctx.stream)          # all slabs written
                ctx.batch.flush()
                return out
            (dw2, db2), seen = launched(amd, deferred)
            assert _wgrad_labels(seen) == labels, seen      # (the reductions carry no profiler label: the bits below say which ran)
            assert dw2.data_ptr() == w2._vq2_grad.data_ptr() and db2.data_ptr() == b2._vq2_grad.data_ptr()
            assert torch.equal(dw, dw2) and torch.equal(db, db2), (c[0], permission, relu_in)


def test_one_weight_under_both_precisions_keeps_two_entries(amd):
    """WgradBatch keys its entry on the permission: the same weight launched with and without it gets two workspaces and
    two jobs, each the right size."""
    from vqvae2_amd import ops
    c = W.BY_NAME["g"]          # the fp32 plan (wino) and the bf16 plan differ in workspace and job
    d = _refs(c[0])[0]
    x, dy = d["x"].to(DEV), d["dy"].to(DEV)
    w2, b2 = d["w"].to(DEV), d["b"].to(DEV)
    w2._vq2_grad, b2._vq2_grad = torch.zeros_like(w2), torch.zeros_like(b2)
    batch, side = ops.WgradBatch(), torch.cuda.Stream()
    for permission in (True, False, True):
        spec = _spec(amd, c, permission)
        batch.launch(spec, x, dy, False, w2, b2, True, side)
        torch.cuda.current_stream().wait_stream(side)
        batch.flush()
        torch.cuda.synchronize()
        dw, db, _ = _run(amd, c, spec, False)
        assert torch.equal(w2._vq2_grad, dw) and torch.equal(b2._vq2_grad, db), permission
    assert len(batch.entries) == 2
    assert len({e["job"].swapped for e in batch.entries.values()}) == 2


@pytest.mark.parametrize("c", ALL, ids=lambda c: c[0])
def test_ex_entry_points_with_flag_zero_are_the_old_ones(amd, c):
    from vqvae2_amd import ops
    lib = amd._lib.lib
    spec = _spec(amd, c)
    desc = ops._desc(spec, c[7], c[8], c[9], spec.ci, spec.co)
    assert lib.vq2_conv_wgrad_workspace_bytes_ex(C.byref(desc), 0) == lib.vq2_conv_wgrad_workspace_bytes(C.byref(desc)) > 0
    ws = torch.empty(16, device=DEV)
    jobs = [amd._lib.WgradJob(), amd._lib.WgradJob()]
    C.memset(C.byref(jobs[0]), 0xA5, C.sizeof(jobs[0]))
    C.memset(C.byref(jobs[1]), 0xA5, C.sizeof(jobs[1]))
    assert lib.vq2_wgrad_job_init_ex(C.byref(desc), 0, ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), C.byref(jobs[0])) == 0
    assert lib.vq2_wgrad_job_init(C.byref(desc), ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), C.byref(jobs[1])) == 0
    assert bytes(jobs[0]) == bytes(jobs[1])
