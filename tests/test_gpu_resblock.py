"""The fused ResBlock kernels called through the C API, against fp64 at their tile edges (csrc/vq2_resblock.hip:
resblock_fwd_kernel, resblock_bwd_data_kernel<SAME_LD> with and without the 1x1 weight-gradient workspace; csrc/vq2_rbwino.hip:
rbw_fwd_kernel).  tests/_resblock_ref.py has the operands, the fp64 reference, the tolerances and the case table; tests/
test_resblock_ref_cpu.py shows on the CPU that the reference is the module's gradient and that the tolerance bites.

What is asserted per launch: the profiler label (family and M), every output against fp64 at the project's tolerance (5e-6 *
max|ref| for r, y, dh, dx; 1e-5 * max|ref| for dw2, db2; rtol 0; 0 for the "integer" operands), the sentinel in every float the
launch does not own (neighbouring channels of a wider buffer, 16 guard pixels on both ends), and the same bits on a second call.
The backward takes r and x as operands, so both ReLU masks are exact: no allowance for flipped masks anywhere.

Which layout reaches which instantiation of the backward (SAME_LD is ldg == ldx == lddx, decided in vq2_resblock_bwd_data):
    same128, same136    resblock_bwd_data_kernel<true>      workspace null | given
    mixed               resblock_bwd_data_kernel<false>     workspace null | given
The label is resblock_bwd_data| for all four; test_census_of_labels_and_instantiations runs every one of them.

With a workspace the launch leaves per-workgroup partial 1x1 weight and bias gradients; vq2_resblock_w2_job_init describes them
and ONE vq2_wgrad_reduce_batched launch reduces them.  The workspace is pre-filled with NaN: a float the kernel does not write
shows in dw2 / db2 (and in the workspace itself, which is checked too).

VQ2_FORMS=direct (a child process: the library reads the variable once) runs the forward cases again; every case, the
Winograd-eligible ones included, must then carry resblock_fwd|.

Every case meets the project's rule as it stands (no case needs a measured, wider tolerance).  Largest error as a share of the
tolerance on the MI355X when this was written, "normal" operands: r 0.17, y 0.06, dh 0.10, dx 0.05, dw2 0.02, db2 0.02; the
"integer" operands gave 0 everywhere."""
import ctypes as C
import os
import subprocess
import sys
import time

import pytest
import torch

import _resblock_ref as R

pytestmark = pytest.mark.gpu

FORMS = os.environ.get("VQ2_FORMS", "all")
SENT, GUARD = 7.0, 16
KINDS = ("normal", "integer")

# name: (ldx, offset of x), (ldy, offset of y), (ldr, offset of r) -- offsets in floats, multiples of 4 (16-byte aligned slices)
FWD_LAYOUTS = {
    "dense": ((128, 0), (128, 0), (32, 0)),
    "wide": ((136, 4), (140, 8), (40, 4)),
}
# name: g, x, dx, r, dh as (pixel stride, offset)
BWD_LAYOUTS = {
    "same128": ((128, 0), (128, 0), (128, 0), (32, 0), (32, 0)),
    "same136": ((136, 4), (136, 8), (136, 0), (36, 4), (40, 8)),
    "mixed": ((136, 8), (128, 0), (140, 12), (40, 4), (36, 4)),
}


def same_ld(layout):
    (ldg, _), (ldx, _), (lddx, _) = BWD_LAYOUTS[layout][:3]
    return ldg == ldx == lddx


assert same_ld("same128") and same_ld("same136") and not same_ld("mixed")


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _dev():
    return torch.device("cuda:0")


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


class In:
    """[N,H,W,c] CPU values as channels [off, off + c) of a device buffer with pixel stride ld (the rest random)"""

    def __init__(self, a, ld, off):
        c = a.shape[-1]
        self.buf = torch.randn((a.numel() // c, ld), generator=torch.Generator().manual_seed(ld * 131 + c)).to(_dev())
        self.buf[:, off:off + c] = a.reshape(-1, c).to(_dev())
        self.ld, self.ptr = ld, _ptr(self.buf, off)


class Out:
    """Sentinel-filled allocation: GUARD pixels, npix pixels of stride ld that own channels [off, off + c), GUARD pixels"""

    def __init__(self, npix, c, ld, off):
        self.npix, self.c, self.ld, self.off = npix, c, ld, off
        self.flat = torch.empty(((npix + 2 * GUARD) * ld,), device=_dev())
        self.ptr = _ptr(self.flat, GUARD * ld + off)
        self.reset()

    def reset(self):
        self.flat.fill_(SENT)

    def owned(self):
        return self.flat.view(-1, self.ld)[GUARD:GUARD + self.npix, self.off:self.off + self.c]

    def untouched(self, what):
        rest = self.flat.clone().view(-1, self.ld)
        rest[GUARD:GUARD + self.npix, self.off:self.off + self.c] = SENT
        assert bool((rest == SENT).all()), "%s: %d floats outside the owned channels were written" % (what, int((rest != SENT).sum()))


def packed(ops, spec, wt, which):
    """vq2_pack_weight of a reference-layout weight"""
    d = ops._desc(spec, 1, max(spec.k, 2), max(spec.k, 2), spec.ci, spec.co)
    buf = torch.empty(spec.ci * spec.co * spec.taps, device=_dev())
    ops.check(ops.lib.vq2_pack_weight(C.byref(d), which, _ptr(wt), _ptr(buf), ops._stream()), "pack_weight")
    return buf


_REF = {}


def reference(c, kind):
    """(operands, fp64 references) of a case: computed once, shared by every test, never modified"""
    key = (R.case_id(c), kind)
    if key not in _REF:
        n, h, w, _ = c
        d = R.operands("rb", n, h, w, kind)
        r, y = R.fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], False)
        dh, dx, dw2, db2 = R.bwd(d["g"], d["r"], d["x"], d["w1"], d["w2"])
        _REF[key] = (d, {"r": r, "y0": y, "y1": torch.relu(y), "dh": dh, "dx": dx, "dw2": dw2, "db2": db2})
    return _REF[key]


def compare(what, kind, name, got, ref):
    rule = {"y0": "y", "y1": "y"}.get(name, name)
    tol = R.tolerances({rule: ref}, kind)[rule]
    got = got.cpu().double().reshape(ref.shape)
    err = float((got - ref).abs().max())
    print("%s %s: max err %.3e  tolerance %.3e  max|ref| %.3e" % (what, name, err, tol, float(ref.abs().max())))
    assert not bool(torch.isnan(got).any()), "%s.%s: NaN" % (what, name)
    assert err <= tol, "%s.%s: err %.3e > tolerance %.3e" % (what, name, err, tol)


def launched(amd, fn):
    """Run fn with every instrumented launch bracketed; returns (result, one kernel label per launch).  (launched of
    tests/test_gpu_dispatch.py, with the launch count of each report line kept.)"""
    lib = amd._lib.lib
    lib.vq2_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.vq2_prof_enable(0)
    buf = C.create_string_buffer(1 << 16)
    lib.vq2_prof_report(buf, len(buf))
    seen = []
    for ln in buf.value.decode().splitlines():
        name, count = ln.split()[:2]
        seen += [name] * int(count)
    return out, seen


def rb_labels(seen):
    return [s for s in seen if s.startswith("resblock")]


def expected_fwd_label(c):
    fam = c[3] if FORMS == "all" else R.DIRECT
    return "%s|M=%d,C=128,Cm=32" % (fam, c[0] * c[1] * c[2])


SPEC1 = dict(transposed=False, cin=128, cout=32, k=3, stride=1, pad=1)
SPEC2 = dict(transposed=False, cin=32, cout=128, k=1, stride=1, pad=0)

_FWD, _BWD = {}, {}


def run_fwd(amd, c, kind, layout, relu_out):
    """One forward case on the GPU against fp64 (cached for the census).  Returns the resblock labels of the launch."""
    key = (R.case_id(c), kind, layout, relu_out)
    if key in _FWD:
        return _FWD[key]
    from vqvae2_amd import ops
    lib = ops.lib
    n, h, w, _ = c
    npix = n * h * w
    what = "fwd %s %s %s relu_out=%d" % key
    d, ref = reference(c, kind)
    (ldx, ox), (ldy, oy), (ldr, orr) = FWD_LAYOUTS[layout]
    x = In(d["x"], ldx, ox)
    r, y = Out(npix, 32, ldr, orr), Out(npix, 128, ldy, oy)
    w1, b1, w2, b2 = (d[k].to(_dev()) for k in ("w1", "b1", "w2", "b2"))
    w1p = packed(ops, ops.ConvSpec(**SPEC1), w1, ops.PACK_FWD)
    w2p = packed(ops, ops.ConvSpec(**SPEC2), w2, ops.PACK_FWD)
    torch.cuda.synchronize()

    def call():
        ops.check(lib.vq2_resblock_fwd(n, h, w, 128, 32, ops.VQ2_RELU_OUT if relu_out else 0, x.ptr, ldx, _ptr(w1p), _ptr(b1),
                                       _ptr(w2p), _ptr(b2), r.ptr, ldr, y.ptr, ldy, ops._stream()), "resblock_fwd")
    _, seen = launched(amd, call)
    labels = rb_labels(seen)
    print("%s: %s" % (what, labels))
    first = (r.flat.clone(), y.flat.clone())
    r.untouched(what + " r")
    y.untouched(what + " y")
    compare(what, kind, "r", r.owned(), ref["r"])
    compare(what, kind, "y%d" % relu_out, y.owned(), ref["y%d" % relu_out])
    r.reset()
    y.reset()
    call()
    torch.cuda.synchronize()
    assert torch.equal(r.flat, first[0]) and torch.equal(y.flat, first[1]), what + ": a second call gives other bits"
    _FWD[key] = labels
    return labels


def w2_job(ops, n, h, w, ws, dw, db):
    """The job of the 1x1 weight gradient as a one-entry device table (ops.WgradBatch.flush builds the trainers' tables so)"""
    WgradJob = ops.WgradJob
    job = WgradJob()
    ops.check(ops.lib.vq2_resblock_w2_job_init(n, h, w, 128, 32, _ptr(ws), _ptr(dw), _ptr(db), C.byref(job)), "resblock_w2_job_init")
    assert (job.O, job.I, job.Or, job.Ir, job.taps, job.S) == (128, 32, 128, 32, 1, R.direct_grid(n, h, w))
    assert (job.n_units_w, job.n_units_b, job.swapped, job.bias_splits) == (128, 4, 0, 0)
    job.unit_offset = 0
    arr = (WgradJob * 1)()
    arr[0] = job
    return ops._upload_structs(arr, _dev()), job.n_units_w + job.n_units_b


def run_bwd(amd, c, kind, layout, with_ws):
    """One backward case on the GPU against fp64 (cached for the census).  Returns the resblock labels of the launch."""
    key = (R.case_id(c), kind, layout, with_ws)
    if key in _BWD:
        return _BWD[key]
    from vqvae2_amd import ops
    lib = ops.lib
    n, h, w, _ = c
    npix, grid = n * h * w, R.direct_grid(n, h, w)
    what = "bwd %s %s %s ws=%d" % key
    d, ref = reference(c, kind)
    (ldg, og), (ldx, ox), (lddx, odx), (ldr, orr), (lddh, odh) = BWD_LAYOUTS[layout]
    g, x, r = In(d["g"], ldg, og), In(d["x"], ldx, ox), In(d["r"], ldr, orr)
    dh, dx = Out(npix, 32, lddh, odh), Out(npix, 128, lddx, odx)
    w1, w2 = d["w1"].to(_dev()), d["w2"].to(_dev())
    w1d = packed(ops, ops.ConvSpec(**SPEC1), w1, ops.PACK_DGRAD)
    w2d = packed(ops, ops.ConvSpec(**SPEC2), w2, ops.PACK_DGRAD)
    nbytes = lib.vq2_resblock_w2_workspace_bytes(n, h, w, 128, 32)
    assert nbytes == grid * (128 * 32 + 128) * 4, (nbytes, grid)
    ws = dw2 = db2 = tab = None
    units = 0
    if with_ws:
        ws = torch.empty(nbytes // 4, device=_dev())
        dw2, db2 = torch.empty((128, 32, 1, 1), device=_dev()), torch.empty((128,), device=_dev())
        tab, units = w2_job(ops, n, h, w, ws, dw2, db2)

    def refill():
        dh.reset()
        dx.reset()
        if with_ws:
            for t in (ws, dw2, db2):
                t.fill_(float("nan"))

    def call():
        ops.check(lib.vq2_resblock_bwd_data(n, h, w, 128, 32, g.ptr, ldg, r.ptr, ldr, x.ptr, ldx, _ptr(w2d), _ptr(w1d), dh.ptr, lddh,
                                            dx.ptr, lddx, _ptr(ws) if with_ws else None, ops._stream()), "resblock_bwd_data")
        if with_ws:
            ops.check(lib.vq2_wgrad_reduce_batched(_ptr(tab), 1, units, ops._stream()), "wgrad_reduce_batched")
    refill()
    torch.cuda.synchronize()
    _, seen = launched(amd, call)
    labels = rb_labels(seen)
    print("%s (SAME_LD=%s, grid %d): %s" % (what, same_ld(layout), grid, labels))
    first = [t.clone() for t in (dh.flat, dx.flat) + ((ws, dw2, db2) if with_ws else ())]
    dh.untouched(what + " dh")
    dx.untouched(what + " dx")
    compare(what, kind, "dh", dh.owned(), ref["dh"])
    compare(what, kind, "dx", dx.owned(), ref["dx"])
    if with_ws:
        assert not bool(torch.isnan(ws).any()), "%s: %d floats of the workspace were not written" % (what, int(torch.isnan(ws).sum()))
        compare(what, kind, "dw2", dw2, ref["dw2"])
        compare(what, kind, "db2", db2, ref["db2"])
    refill()
    call()
    torch.cuda.synchronize()
    second = (dh.flat, dx.flat) + ((ws, dw2, db2) if with_ws else ())
    assert all(torch.equal(a, b) for a, b in zip(first, second)), what + ": a second call gives other bits"
    _BWD[key] = labels
    return labels


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", sorted(FWD_LAYOUTS))
@pytest.mark.parametrize("relu_out", (0, 1))
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_forward_case_runs_its_kernel_and_matches_fp64(amd, c, relu_out, layout, kind):
    labels = run_fwd(amd, c, kind, layout, relu_out)
    assert labels == [expected_fwd_label(c)], (labels, expected_fwd_label(c))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_ws", (0, 1), ids=("nows", "ws"))
@pytest.mark.parametrize("layout", sorted(BWD_LAYOUTS))
@pytest.mark.parametrize("c", R.BWD_CASES, ids=R.case_id)
def test_backward_case_runs_its_kernel_and_matches_fp64(amd, c, layout, with_ws, kind):
    labels = run_bwd(amd, c, kind, layout, with_ws)
    assert labels == ["resblock_bwd_data|M=%d,C=128,Cm=32" % (c[0] * c[1] * c[2])], labels


def test_census_of_labels_and_instantiations(amd):
    """Both forward families, and resblock_bwd_data in all four instantiations (SAME_LD x workspace), each over every case of
    its table and both kinds of operands."""
    fams = set()
    for c in R.CASES:
        for layout in FWD_LAYOUTS:
            for kind in KINDS:
                for relu_out in (0, 1):
                    fams |= {s.split("|")[0] for s in run_fwd(amd, c, kind, layout, relu_out)}
    assert fams == ({R.DIRECT, R.WINO} if FORMS == "all" else {R.DIRECT}), fams
    inst = {}
    for c in R.BWD_CASES:
        for layout in BWD_LAYOUTS:
            for with_ws in (0, 1):
                for kind in KINDS:
                    labels = run_bwd(amd, c, kind, layout, with_ws)
                    inst.setdefault((same_ld(layout), bool(with_ws)), set()).update(s.split("|")[0] for s in labels)
    print("backward instantiations (SAME_LD, workspace): %s" % sorted(inst))
    assert inst == {(s, v): {"resblock_bwd_data"} for s in (True, False) for v in (True, False)}, inst


# Wall time on the MI355X machine when this was written: this module without the child 3.1 s (226 tests, the fp64 references
# included), the forward cases in a child process with VQ2_FORMS=direct 4.3 s, most of it the start of the interpreter.
# CHILD_SECONDS is that figure with room for a cold start; the child gets three times as long.
CHILD_SECONDS = 20


def test_forward_cases_on_the_direct_kernel():
    """The direct forward at the Winograd-eligible shapes: every forward case again in ONE fresh child process with
    VQ2_FORMS=direct; expected_fwd_label() then asks for resblock_fwd| in every case."""
    env = dict(os.environ, VQ2_FORMS="direct")
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        "-k", "forward_case_runs_its_kernel"], env=env, capture_output=True, text=True, timeout=3 * CHILD_SECONDS)
    print("VQ2_FORMS=direct child: %.1f s" % (time.time() - t0))
    want = "%d passed" % (len(R.CASES) * 2 * len(FWD_LAYOUTS) * len(KINDS))
    assert r.returncode == 0 and want in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, \
        r.stdout[-3000:] + r.stderr[-2000:]


def test_refusals_return_before_any_launch(amd):
    """Argument checks of the three entry points: the return code and vq2_last_error for each refused argument, no launch
    (no label), and a valid call right after each refusal gives the bits of the first valid call."""
    from vqvae2_amd import ops
    lib = ops.lib
    INVALID, UNSUPPORTED = 1, 2
    c = (2, 3, 5, R.DIRECT)
    n, h, w, _ = c
    npix = n * h * w
    d, ref = reference(c, "normal")
    x, g, r_in = In(d["x"], 128, 0), In(d["g"], 128, 0), In(d["r"], 32, 0)
    r, y, dh, dx = Out(npix, 32, 32, 0), Out(npix, 128, 128, 0), Out(npix, 32, 32, 0), Out(npix, 128, 128, 0)
    w1, b1, w2, b2 = (d[k].to(_dev()) for k in ("w1", "b1", "w2", "b2"))
    s1, s2 = ops.ConvSpec(**SPEC1), ops.ConvSpec(**SPEC2)
    w1p, w2p = packed(ops, s1, w1, ops.PACK_FWD), packed(ops, s2, w2, ops.PACK_FWD)
    w1d, w2d = packed(ops, s1, w1, ops.PACK_DGRAD), packed(ops, s2, w2, ops.PACK_DGRAD)
    ws = torch.zeros(lib.vq2_resblock_w2_workspace_bytes(n, h, w, 128, 32) // 4 + 4, device=_dev())

    def fwd(**kw):
        a = dict(N=n, H=h, W=w, C=128, Cm=32, flags=0, x=x.ptr, ldx=128, r=r.ptr, ldr=32, y=y.ptr, ldy=128)
        a.update(kw)
        return lib.vq2_resblock_fwd(a["N"], a["H"], a["W"], a["C"], a["Cm"], a["flags"], a["x"], a["ldx"], _ptr(w1p), _ptr(b1),
                                    _ptr(w2p), _ptr(b2), a["r"], a["ldr"], a["y"], a["ldy"], ops._stream())

    def bwd(**kw):
        a = dict(N=n, H=h, W=w, C=128, Cm=32, g=g.ptr, ldg=128, r=r_in.ptr, ldr=32, x=x.ptr, ldx=128, dh=dh.ptr, lddh=32,
                 dx=dx.ptr, lddx=128, ws=None)
        a.update(kw)
        return lib.vq2_resblock_bwd_data(a["N"], a["H"], a["W"], a["C"], a["Cm"], a["g"], a["ldg"], a["r"], a["ldr"], a["x"],
                                         a["ldx"], _ptr(w2d), _ptr(w1d), a["dh"], a["lddh"], a["dx"], a["lddx"], a["ws"], ops._stream())

    def valid(fn, outs):
        for o in outs:
            o.reset()
        assert fn() == 0, lib.vq2_last_error()
        torch.cuda.synchronize()
        return [o.flat.clone() for o in outs]

    good_f, good_b = valid(fwd, (r, y)), valid(bwd, (dh, dx))
    compare("refusals fwd", "normal", "y0", y.owned(), ref["y0"])
    compare("refusals bwd", "normal", "dx", dx.owned(), ref["dx"])
    off = lambda o: C.c_void_p(o.ptr.value + 4)       # 4 bytes past a 16-byte boundary
    F_REFUSED = [
        (dict(C=64), UNSUPPORTED, "built for channel=128"), (dict(Cm=16), UNSUPPORTED, "built for channel=128"),
        (dict(ldx=124), INVALID, "pixel strides"), (dict(ldy=124), INVALID, "pixel strides"), (dict(ldr=28), INVALID, "pixel strides"),
        (dict(ldx=130), INVALID, "pixel strides"), (dict(ldy=134), INVALID, "pixel strides"), (dict(ldr=34), INVALID, "pixel strides"),
        (dict(x=off(x)), INVALID, "16-byte aligned"), (dict(r=off(r)), INVALID, "16-byte aligned"), (dict(y=off(y)), INVALID, "16-byte aligned"),
        (dict(flags=ops.VQ2_RELU_IN), INVALID, "only VQ2_RELU_OUT"), (dict(flags=ops.VQ2_RELU_IN | ops.VQ2_RELU_OUT), INVALID, "only VQ2_RELU_OUT"),
        (dict(flags=4), INVALID, "only VQ2_RELU_OUT"),
        (dict(N=0), INVALID, "empty tensor"), (dict(H=0), INVALID, "empty tensor"), (dict(W=0), INVALID, "empty tensor"),
    ]
    B_REFUSED = [
        (dict(C=64), UNSUPPORTED, "built for channel=128"), (dict(Cm=16), UNSUPPORTED, "built for channel=128"),
        (dict(ldg=124), INVALID, "pixel strides"), (dict(ldx=124), INVALID, "pixel strides"), (dict(lddx=124), INVALID, "pixel strides"),
        (dict(ldr=28), INVALID, "pixel strides"), (dict(lddh=28), INVALID, "pixel strides"),
        (dict(ldg=130), INVALID, "pixel strides"), (dict(ldx=134), INVALID, "pixel strides"), (dict(lddx=138), INVALID, "pixel strides"),
        (dict(ldr=34), INVALID, "pixel strides"), (dict(lddh=38), INVALID, "pixel strides"),
        (dict(g=off(g)), INVALID, "16-byte aligned"), (dict(r=off(r_in)), INVALID, "16-byte aligned"), (dict(x=off(x)), INVALID, "16-byte aligned"),
        (dict(dh=off(dh)), INVALID, "16-byte aligned"), (dict(dx=off(dx)), INVALID, "16-byte aligned"),
        (dict(ws=_ptr(ws, 1)), INVALID, "workspace must be 16-byte aligned"),
        (dict(N=0), INVALID, "empty tensor"), (dict(H=0), INVALID, "empty tensor"), (dict(W=0), INVALID, "empty tensor"),
    ]
    for fn, table, outs, good in ((fwd, F_REFUSED, (r, y), good_f), (bwd, B_REFUSED, (dh, dx), good_b)):
        for kw, code, text in table:
            for o in outs:
                o.reset()
            rc, seen = launched(amd, lambda: fn(**kw))
            msg = lib.vq2_last_error().decode(errors="replace")
            assert rc == code and text in msg, (fn.__name__, kw, rc, msg)
            assert rb_labels(seen) == [], (kw, seen)
            assert all(bool((o.flat == SENT).all()) for o in outs), (kw, "an output was written")
            again = valid(fn, outs)
            assert all(torch.equal(a, b) for a, b in zip(again, good)), (kw, "the valid call after the refusal differs")
    for shape in ((n, h, w, 64, 32), (n, h, w, 128, 16), (0, h, w, 128, 32), (n, 0, w, 128, 32), (n, h, 0, 128, 32)):
        assert lib.vq2_resblock_w2_workspace_bytes(*shape) == 0, shape
