"""torch.autograd.Function wrappers over the C ABI of libvq2.so (include/vq2.h).

Activations inside this module are NHWC tensors of shape [N,H,W,C] whose last dim is
contiguous and whose pixel stride `ld = t.stride(2)` may exceed C (a channel slice of a
wider buffer).  PyTorch is used for device memory, streams and autograd bookkeeping only;
every FLOP and every byte moved on this path is a libvq2 kernel.
"""
from dataclasses import dataclass, field
import contextlib
import ctypes as C
import os

import torch
from torch.autograd import Function

from ._lib import lib, check, AttnDesc, ConvDesc, OneHotDesc, PackJob, WgradJob, WnEntry

VQ2_RELU_IN = 1
VQ2_RELU_OUT = 2
VQ2_MASK_AFTER_RESIDUAL = 4
VQ2_ALLOW_BF16 = 16
PACK_FWD = 0
PACK_DGRAD = 1
PACK_FWD_BF16 = 2
PACK_DGRAD_BF16 = 3

# There is NO process-global mutable state on the autograd path (SURVEY 8b threading row): what a step shares hangs on the
# tensors, so two trainers or models can coexist in one process and back-propagate on different autograd threads:
#   _vq2_packs  packed-weight cache {which: (version, buffer)}: set by packed_weight / PackPlan.run, read by packed_weight
#   _vq2_epoch  count of raw-pointer weight updates (no _version bump): set by touch_weights, read through weight_epoch
#               (_pack_version, the sampler's snapshot)
#   _vq2_ctx    the owning trainer's StepContext (deferred reduction, side stream): set by the trainer, read by _step_ctx
#   _vq2_grad   slot in a flat gradient buffer: set by ParamArena (parameters) and planned_weight (a WeightNormPlan's
#               effective weight), read by slot_of / landed alone
#   _vq2_wn     the WeightNormPlan that forms this weight_v's effective weight: set by the plan, read by plan_ready


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# `with (torch.cuda.stream(side) if ... else _THIS_STREAM):` -- one launch written once, on the side stream or on the
# current one (nullcontext holds no state: one object serves every call and every thread)
_THIS_STREAM = contextlib.nullcontext()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ceil4(c):
    return (c + 3) // 4 * 4


def _require_cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError(f"vqvae2_amd: {what} must be a float32 tensor on the MI355X (got "
                           f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '?')}); "
                           "this package has no CPU path")


def is_nhwc_dense(t):
    """[N,H,W,C] with contiguous channels and a uniform pixel stride, 16-byte aligned."""
    if t.dim() != 4 or t.stride(3) != 1:
        return False
    n, h, w, c = t.shape
    ld = t.stride(2)
    if w == 1:
        ld = t.stride(1) if h > 1 else (t.stride(0) if n > 1 else c)
    return (ld >= c and ld % 4 == 0 and (w == 1 or t.stride(2) == ld) and (h == 1 or t.stride(1) == w * ld)
            and (n == 1 or t.stride(0) == h * w * ld) and t.data_ptr() % 16 == 0)


def ld_of(t):
    n, h, w, c = t.shape
    if w > 1:
        return t.stride(2)
    if h > 1:
        return t.stride(1)
    if n > 1:
        return t.stride(0)
    return c


def as_nhwc(t):
    """Return t if it already is a dense NHWC view (any pixel stride), else a packed copy."""
    _require_cuda(t, "activation")
    if is_nhwc_dense(t):
        return t
    return t.contiguous()  # exotic layout handed in by foreign code; never hit on the stage-1 path


def packed(t):
    """Dense NHWC view -> pixel stride == C (slice-copy kernel when it is a channel slice)."""
    if t.is_contiguous():
        return t
    t = as_nhwc(t)
    if t.is_contiguous():
        return t
    n, h, w, c = t.shape
    out = torch.empty((n, h, w, c), device=t.device, dtype=torch.float32)
    check(lib.vq2_slice_copy(_p(t), ld_of(t), _p(out), c, n * h * w, c, 0, _stream()), "slice_copy")
    return out


# ----------------------------------------------------------------------------- conv plumbing
@dataclass(frozen=True)
class ConvSpec:
    """A conv layer as vq2_conv_desc (include/vq2.h) states it, without the batch.  ConvSpec(transposed, cin, cout, k, stride,
    pad) is the square kernel with the same padding on every side of the stage-1 layers; ConvSpec.geom() the stride-1
    kh x kw kernel with top / left padding and an output the size of the input (WNConv2d / CausalConv2d of the stage-2 prior)."""
    transposed: bool
    cin: int
    cout: int
    k: int                    # kernel rows
    stride: int
    pad: int                  # top padding
    kw: int = 0               # kernel columns and left padding; without same_size always k and pad (__post_init__)
    pad_left: int = 0
    same_size: bool = False   # vq2_conv_desc.same_size
    # The two permissions are keyword-only: a positional argument can never land on the wrong one.  (`bf16` stays the last
    # field, as tests/test_conv_bf16_cpu.py pins it.)
    # the weight gradient rounds x and dy to bf16 where conv_wgrad_bf16_eligible
    bf16_wgrad: bool = field(default=False, kw_only=True)
    # forward and data gradient round their operands to bf16 where conv_bf16_eligible
    bf16: bool = field(default=False, kw_only=True)

    def __post_init__(self):
        if not self.same_size:
            object.__setattr__(self, "kw", self.k)
            object.__setattr__(self, "pad_left", self.pad)

    @classmethod
    def geom(cls, cin, cout, kh, kw, pad_top, pad_left):
        """A stride-1 conv with a kh x kw kernel that reads from row h - pad_top and column w - pad_left on."""
        return cls(False, cin, cout, kh, 1, pad_top, kw, pad_left, True)

    @property
    def pad_top(self):
        return self.pad

    @property
    def taps(self):
        return self.k * self.kw

    @property
    def ci(self):
        return ceil4(self.cin)

    @property
    def co(self):
        return ceil4(self.cout)

    def out_hw(self, h, w):
        if self.transposed:
            return 2 * h, 2 * w
        if self.same_size:
            return h, w
        return (h + 2 * self.pad - self.k) // self.stride + 1, (w + 2 * self.pad - self.k) // self.stride + 1


def conv_bf16_eligible(spec, dgrad=False):
    """The host mirror of vq2_conv_bf16_eligible (include/vq2.h): a same_size layer whose depth-side channel count (the
    padded input channels for the forward, output channels for the data gradient) is a multiple of 16.  A spec with
    `bf16` set takes the bf16-operand kernel, and packs the bf16 panel, exactly where this holds."""
    return bool(spec.same_size) and (spec.co if dgrad else spec.ci) % 16 == 0


def conv_wgrad_bf16_eligible(spec):
    """The host mirror of vq2_conv_wgrad_bf16_eligible (include/vq2.h): a same_size layer whose padded input AND output channel
    counts are multiples of 16.  A spec with `bf16_wgrad` set takes the bf16-operand weight gradient exactly where this holds."""
    return bool(spec.same_size) and spec.ci % 16 == 0 and spec.co % 16 == 0


def _wgrad_flags(spec, relu_in):
    """The flags of a weight-gradient launch of `spec`; workspace size and reduction job are asked with the same ones."""
    bf16 = spec.bf16_wgrad and conv_wgrad_bf16_eligible(spec)
    return (VQ2_RELU_IN if relu_in else 0) | (VQ2_ALLOW_BF16 if bf16 else 0)


def _desc(spec, n, h, w, ldx, ldy):
    d = ConvDesc()
    d.N, d.H, d.W, d.Ci, d.Co = n, h, w, spec.ci, spec.co
    d.KH, d.KW, d.stride, d.pad_top, d.pad_left = spec.k, spec.kw, spec.stride, spec.pad, spec.pad_left
    d.transposed, d.same_size = int(spec.transposed), int(spec.same_size)
    d.ldx, d.ldy = ldx, ldy
    d.Cir, d.Cor = spec.cin, spec.cout
    return d


def touch_weights(params):
    """Tell the packed-weight caches that `params` were updated through raw pointers (vq2_adam_step), which
    does not bump tensor._version."""
    for p in params:
        p._vq2_epoch = weight_epoch(p) + 1


def weight_epoch(param):
    """How often touch_weights reported a raw-pointer update of `param` (a cache of its values compares this too)."""
    return getattr(param, "_vq2_epoch", 0)


def _pack_version(spec, weight):
    return (weight.data_ptr(), weight._version, weight_epoch(weight), spec)


def _upload_structs(arr, device):
    """A ctypes array of job structs as a uint8 tensor on `device`, byte for byte."""
    import numpy as np
    return torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(device)


def packed_weight(spec, weight, which):
    """Kernel-layout copy of a reference-layout weight, cached ON the weight until it changes."""
    packs = weight.__dict__.setdefault("_vq2_packs", {})
    ver = _pack_version(spec, weight)
    hit = packs.get(which)
    if hit is not None and hit[0] == ver:
        return hit[1]
    _require_cuda(weight, "weight")
    wsrc = weight.detach()
    if not wsrc.is_contiguous():
        wsrc = wsrc.contiguous()
    n = spec.ci * spec.co * spec.taps
    buf = hit[1] if (hit is not None and hit[1].numel() == n and hit[1].device == weight.device) else \
        torch.empty(n, device=weight.device, dtype=torch.float32)
    d = _desc(spec, 1, max(spec.k, 2), max(spec.k, 2), spec.ci, spec.co)
    check(lib.vq2_pack_weight(C.byref(d), which, _p(wsrc), _p(buf), _stream()), "pack_weight")
    packs[which] = (ver, buf)
    return buf


class PackPlan:
    """Every (layer, fwd|dgrad) weight panel of a model re-packed by ONE launch per step
    (vq2_pack_weights_batched) instead of one launch per panel; feeds the same cache that
    packed_weight() reads, so the conv wrappers need no change."""

    def __init__(self, layers):
        """layers: iterable of (ConvSpec, weight Parameter, needs_dgrad)."""
        jobs = []
        for spec, weight, needs_dgrad in layers:
            for which in ((PACK_FWD, PACK_DGRAD) if needs_dgrad else (PACK_FWD,)):
                jobs.append((spec, weight, which))
        n = sum(s.ci * s.co * s.taps for s, _, _ in jobs)
        dev = jobs[0][1].device
        self.flat = torch.empty(n, device=dev, dtype=torch.float32)
        self.entries = []
        arr = (PackJob * len(jobs))()
        off = 0
        for i, (spec, weight, which) in enumerate(jobs):
            numel = spec.ci * spec.co * spec.taps
            buf = self.flat[off:off + numel]
            d = _desc(spec, 1, max(spec.k, 2), max(spec.k, 2), spec.ci, spec.co)
            if not weight.is_contiguous():
                raise RuntimeError("PackPlan: weights must be contiguous")
            check(lib.vq2_pack_job_init(C.byref(d), which, _p(weight), _p(buf), C.byref(arr[i])), "pack_job_init")
            arr[i].offset = off
            assert arr[i].numel == numel
            self.entries.append((spec, weight, which, buf))
            off += numel
        self.total = off
        self.jobs_dev = _upload_structs(arr, dev)
        self.njobs = len(jobs)
        self._ptrs = [w.data_ptr() for _, w, _, _ in self.entries]

    def run(self):
        if any(w.data_ptr() != p for (_, w, _, _), p in zip(self.entries, self._ptrs)):
            raise RuntimeError("PackPlan: a parameter was re-allocated; rebuild the plan")
        check(lib.vq2_pack_weights_batched(_p(self.jobs_dev), self.njobs, self.total, _stream()), "pack_batched")
        for spec, weight, which, buf in self.entries:
            weight.__dict__.setdefault("_vq2_packs", {})[which] = (_pack_version(spec, weight), buf)


def conv_forward(spec, x, weight, bias, flags=0, residual=None, out=None):
    n, h, w, c = x.shape
    if c != spec.ci:
        raise RuntimeError(f"conv_forward: input has {c} channels, expected {spec.ci}")
    ho, wo = spec.out_hw(h, w)
    if out is None:
        out = torch.empty((n, ho, wo, spec.co), device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (n, ho, wo, spec.co) or not is_nhwc_dense(out):
        raise RuntimeError("conv_forward: bad `out` buffer")
    d = _desc(spec, n, h, w, ld_of(x), ld_of(out))
    if spec.bf16 and conv_bf16_eligible(spec):
        flags |= VQ2_ALLOW_BF16
        wp = packed_weight(spec, weight, PACK_FWD_BF16)
    else:
        wp = packed_weight(spec, weight, PACK_FWD)
    ldres = ld_of(residual) if residual is not None else 0
    check(lib.vq2_conv_fwd(C.byref(d), flags, _p(x), _p(wp), _p(bias), _p(residual), ldres, _p(out), _stream()),
          "conv_fwd")
    return out


def conv_dgrad(spec, xshape, dy, weight, mask=None, residual=None, out=None, mask_after=False):
    n, h, w, _ = xshape
    if out is None:
        out = torch.empty((n, h, w, spec.ci), device=dy.device, dtype=torch.float32)
    d = _desc(spec, n, h, w, spec.ci, ld_of(dy))
    flags = VQ2_MASK_AFTER_RESIDUAL if mask_after else 0
    if spec.bf16 and conv_bf16_eligible(spec, dgrad=True):
        flags |= VQ2_ALLOW_BF16
        wp = packed_weight(spec, weight, PACK_DGRAD_BF16)
    else:
        wp = packed_weight(spec, weight, PACK_DGRAD)
    check(lib.vq2_conv_dgrad(C.byref(d), flags, _p(dy), _p(wp), _p(mask),
                             ld_of(mask) if mask is not None else 0, _p(residual),
                             ld_of(residual) if residual is not None else 0, _p(out), ld_of(out), _stream()),
          "conv_dgrad")
    return out


def slot_of(param):
    """THE SLOT RULE (truth tables: DESIGN §3).  The slot `_vq2_grad` that a weight-gradient launch may write for `param`
    now, or None: it exists with param's shape, contiguous (the kernels write numel() floats through its pointer), and
    param is a leaf whose .grad is None -- a second backward (accumulation) must not overwrite the first, it gets a fresh
    tensor that autograd adds -- or no leaf: a WeightNormPlan's effective weight, which has no .grad to ask and whose slot,
    the plan's dW buffer, is written once per step (PlannedWeightFn.backward refuses a second backward itself).
    The deferred branch of conv_wgrad and ResBlockFn's w2 job need both slots, weight and bias.  The deferred branch keeps
    bias.numel() == spec.cout too: its job writes spec.cout floats through the raw slot pointer at flush(), after autograd
    has checked what it was handed, so a bias of another length would have the reduction end in the neighbouring slot or
    short of its own.  One site differs: OneHotConvFn keeps no weight and decides in forward, where a leaf's .grad says
    nothing about the time of backward, so it takes the slot of a non-leaf weight only (a leaf's goes to a fresh tensor)."""
    slot = getattr(param, "_vq2_grad", None) if param is not None else None
    ok = slot is not None and (not param.is_leaf or param.grad is None) and slot.shape == param.shape and slot.is_contiguous()
    return slot if ok else None


def _grad_slot(param):
    """Where the gradient of `param` is written: a view of slot_of(param), a fresh tensor object so that autograd can adopt
    it as .grad without a copy, else a fresh contiguous tensor."""
    slot = slot_of(param)
    if slot is not None:
        return slot.view_as(slot)
    return None if param is None else torch.empty_like(param, memory_format=torch.contiguous_format)


def landed(param):
    """True when `param.grad` is its slot (starts where `_vq2_grad` does): what ParamArena.grads_ready, FusedAdam.step and
    the trainers' early buckets ask before they read the flat gradient buffer."""
    slot, grad = getattr(param, "_vq2_grad", None), param.grad
    return slot is not None and grad is not None and grad.data_ptr() == slot.data_ptr()


class WgradBatch:
    """Deferred weight-gradient reduction for a whole backward pass: every conv_wgrad writes only its
    split-K slabs into a persistent per-layer workspace; flush() reduces ALL layers with one launch
    (vq2_wgrad_reduce_batched) straight into the ParamArena gradient slots."""

    def __init__(self):
        self.entries = {}
        self.order = []
        self.tables = {}
        self.dirty = True

    def _entry(self, key, device, create):
        """The entry of `key`; made on first use from create() -> (workspace bytes, dw slot, db slot, job_init(ws, dw, db, job))"""
        ent = self.entries.get(key)
        if ent is None:
            nbytes, dw, db, job_init = create()
            ws = torch.empty(max(nbytes // 4, 4), device=device, dtype=torch.float32)
            job = WgradJob()
            job_init(_p(ws), _p(dw), _p(db), C.byref(job))
            ent = self.entries[key] = {"ws": ws, "nbytes": nbytes, "job": job, "dw": dw, "db": db, "used": False}
            self.dirty = True
        return ent

    def _mark_used(self, key, ent):
        if not ent["used"]:
            ent["used"] = True
            self.order.append(key)

    def launch(self, spec, x, dy, relu_in, weight, bias, want_db, side):
        n, h, w, _ = x.shape
        flags = _wgrad_flags(spec, relu_in)
        key = (id(weight), n, h, w, ld_of(x), ld_of(dy), relu_in, flags & VQ2_ALLOW_BF16)   # workspace and job differ with the bit
        d = _desc(spec, n, h, w, ld_of(x), ld_of(dy))
        ent = self._entry(key, x.device, lambda: (
            lib.vq2_conv_wgrad_workspace_bytes_ex(C.byref(d), flags), slot_of(weight), slot_of(bias) if want_db else None,
            lambda *a: check(lib.vq2_wgrad_job_init_ex(C.byref(d), flags, *a), "wgrad_job_init")))
        # off the backward critical path: overlaps the next layers' data gradients.  A launch that fills the chip by
        # itself gains nothing from a second stream.
        on_side = n * h * w <= WGRAD_STREAM_MAX_PIXELS
        if on_side:
            side.wait_event(torch.cuda.current_stream().record_event())
        with (torch.cuda.stream(side) if on_side else _THIS_STREAM):
            check(lib.vq2_conv_wgrad_partial(C.byref(d), flags, _p(x), _p(dy), _p(ent["db"]),
                                             _p(ent["ws"]), ent["nbytes"], _stream()), "conv_wgrad_partial")
        if on_side:
            x.record_stream(side)
            dy.record_stream(side)
        self._mark_used(key, ent)
        dw, db = ent["dw"], ent["db"]
        return dw.view_as(dw), (None if db is None else db.view_as(db))

    def resblock_w2(self, n, h, w, c, cm, weight, bias):
        """Workspace for the 1x1 weight/bias gradient that vq2_resblock_bwd_data leaves per workgroup; its job
        joins the batched reduction like any other layer's slabs.  Returns (workspace tensor, dw view, db view)."""
        key = (id(weight), n, h, w, "rbw2")
        ent = self._entry(key, weight.device, lambda: (
            lib.vq2_resblock_w2_workspace_bytes(n, h, w, c, cm), slot_of(weight), slot_of(bias),
            lambda *a: check(lib.vq2_resblock_w2_job_init(n, h, w, c, cm, *a), "resblock_w2_job_init")))
        self._mark_used(key, ent)
        return ent["ws"], ent["dw"].view_as(ent["dw"]), ent["db"].view_as(ent["db"])

    def flush(self):
        if not self.order:
            return
        sig = tuple(self.order)
        if self.dirty:
            self.tables = {}
            self.dirty = False
        tab = self.tables.get(sig)
        if tab is None:   # job table of this subset of layers: built and uploaded once, then reused every step
            arr = (WgradJob * len(self.order))()
            off = 0
            for i, key in enumerate(self.order):
                job = self.entries[key]["job"]
                job.unit_offset = off
                arr[i] = job
                off += job.n_units_w + job.n_units_b
            tab = (_upload_structs(arr, self.entries[self.order[0]]["ws"].device), off)
            self.tables[sig] = tab
        check(lib.vq2_wgrad_reduce_batched(_p(tab[0]), len(self.order), tab[1], _stream()), "wgrad_reduce_batched")
        for key in self.order:
            self.entries[key]["used"] = False
        self.order = []


class StepContext:
    """What one Stage1Trainer's backward pass shares between its layers: the deferred split-K reduction
    (WgradBatch) and the side stream for weight gradients.  Hung on the trainer's own parameters as
    `_vq2_ctx`; `active` only while that trainer's backward runs (a stand-alone .backward() on the same model
    takes the immediate per-layer path).  Weight gradients are off the backward critical path (only the optimizer
    consumes them), so on a side stream they overlap the next layers' data-gradient launches; only legal when
    they land in arena slots that nobody reads before the trainer joins the streams."""

    def __init__(self, wgrad_stream):
        self.batch = WgradBatch()
        self.stream = wgrad_stream
        self.active = False


def _step_ctx(weight):
    ctx = getattr(weight, "_vq2_ctx", None)
    return ctx if (ctx is not None and ctx.active) else None


# Only launches too small to fill the chip go to the side stream (measured on MI355X, batch 32: the 32x32-resolution
# layers, <= 32,768 pixels: 7.19 -> 7.13 ms per step; every weight gradient there: 7.34 -- two chip-filling kernels
# of different streams do not share CUs usefully)
WGRAD_STREAM_MAX_PIXELS = 40000


def conv_wgrad(spec, x, dy, relu_in, weight, bias=None, want_dw=True, want_db=True):
    """(dw, db) in the reference layouts; the bias gradient is fused into the same launches."""
    n, h, w, _ = x.shape
    d = _desc(spec, n, h, w, ld_of(x), ld_of(dy))
    flags = _wgrad_flags(spec, relu_in)
    nbytes = lib.vq2_conv_wgrad_workspace_bytes_ex(C.byref(d), flags)
    sc = _step_ctx(weight)
    in_slot = sc is not None and slot_of(weight) is not None
    # deferred: both slots writable (slot_of), and the bias exactly as long as the job's reduction writes
    if in_slot and (bias is None or (slot_of(bias) is not None and bias.numel() == spec.cout)):
        dw, db = sc.batch.launch(spec, x, dy, relu_in, weight, bias, want_db, sc.stream)
        return (dw if want_dw else None), db
    dw = _grad_slot(weight)
    db = _grad_slot(bias) if (bias is not None and want_db) else None
    side = None   # the side stream only for a gradient that lands in its arena slot (see StepContext)
    if in_slot:
        side = sc.stream
        side.wait_event(torch.cuda.current_stream().record_event())
    with (torch.cuda.stream(side) if side is not None else _THIS_STREAM):
        ws = torch.empty(max(nbytes // 4, 4), device=x.device, dtype=torch.float32)
        check(lib.vq2_conv_wgrad(C.byref(d), flags, _p(x), _p(dy), _p(dw), _p(db), _p(ws), nbytes,
                                 _stream()), "conv_wgrad")
    if side is not None:
        x.record_stream(side)   # keep the caching allocator from recycling these while the side stream reads
        dy.record_stream(side)
    return (dw if want_dw else None), db


def relu_bwd(dy, y):
    """g = dy * (y > 0) for dense NHWC operands of any pixel stride."""
    n, h, w, c = dy.shape
    g = torch.empty((n, h, w, c), device=dy.device, dtype=torch.float32)
    check(lib.vq2_relu_bwd(_p(dy), ld_of(dy), _p(y), ld_of(y), _p(g), c, n * h * w, c, _stream()), "relu_bwd")
    return g


def add_(a, b, alpha=1.0):
    """a + alpha*b into a fresh packed tensor (own kernel; used for autograd fan-out sums)."""
    a, b = packed(a), packed(b)
    out = torch.empty_like(a)
    check(lib.vq2_axpby(_p(a), _p(b), float(alpha), _p(out), a.numel(), _stream()), "axpby")
    return out


# ----------------------------------------------------------------------------- layout boundary
class NchwToNhwc(Function):
    """[N,C,H,W] (any strides) -> packed NHWC [N,H,W,ceil4(C)] (zero padded)."""

    @staticmethod
    def forward(ctx, x):
        _require_cuda(x, "input")
        n, c, h, w = x.shape
        ctx.c = c
        xc = x if x.is_contiguous() else x.contiguous()
        out = torch.empty((n, h, w, ceil4(c)), device=x.device, dtype=torch.float32)
        check(lib.vq2_nchw_to_nhwc(_p(xc), _p(out), n, c, h, w, ceil4(c), _stream()), "nchw_to_nhwc")
        return out

    @staticmethod
    def backward(ctx, g):
        g = as_nhwc(g)
        n, h, w, cp = g.shape
        out = torch.empty((n, ctx.c, h, w), device=g.device, dtype=torch.float32)
        check(lib.vq2_nhwc_to_nchw(_p(g), _p(out), n, ctx.c, h, w, ld_of(g), _stream()), "nhwc_to_nchw")
        return out


class NhwcToNchw(Function):
    """NHWC [N,H,W,Cp] -> contiguous NCHW [N,C,H,W] dropping padded channels."""

    @staticmethod
    def forward(ctx, x, c):
        n, h, w, cp = x.shape
        ctx.cp = cp
        out = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
        check(lib.vq2_nhwc_to_nchw(_p(x), _p(out), n, c, h, w, ld_of(x), _stream()), "nhwc_to_nchw")
        return out

    @staticmethod
    def backward(ctx, g):
        n, c, h, w = g.shape
        gc = g if g.is_contiguous() else g.contiguous()
        out = torch.empty((n, h, w, ctx.cp), device=g.device, dtype=torch.float32)
        check(lib.vq2_nchw_to_nhwc(_p(gc), _p(out), n, c, h, w, ctx.cp, _stream()), "nchw_to_nhwc")
        return out, None


def to_nhwc(x):
    """Module-boundary input: NCHW tensor -> internal NHWC (zero-copy when x is channels-last)."""
    _require_cuda(x, "input")
    if x.dim() != 4:
        raise RuntimeError("expected a 4-D NCHW tensor")
    c = x.shape[1]
    if c % 4 == 0:
        v = x.permute(0, 2, 3, 1)
        if is_nhwc_dense(v):
            return v
    return NchwToNhwc.apply(x)


U8_LAYOUTS = {"hwc": 0, "chw": 1}   # VQ2_U8_HWC / VQ2_U8_CHW of include/vq2.h


def u8_to_nhwc4(img, lut, layout, box=None):
    """uint8 image batch ([N,Hs,Ws,C] for "hwc", [N,C,Hs,Ws] for "chw") -> the internal NHWC tensor [N,H,W,4] of
    lut[c][byte] (pad lanes 0): ToTensor + Normalize + crop + layout change in one launch (vq2_u8_to_nhwc4).
    lut: device float32 [C,256]; box = (y0, x0, H, W), default the whole image."""
    if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8):
        raise RuntimeError(f"vqvae2_amd: 8-bit image batch must be a uint8 tensor on the MI355X (got "
                           f"{getattr(img, 'dtype', type(img))} on {getattr(img, 'device', '?')}); "
                           "this package has no CPU path")
    if layout not in U8_LAYOUTS:
        raise ValueError(f"layout must be 'hwc' or 'chw', not {layout!r}")
    if img.dim() != 4 or not img.is_contiguous():
        raise RuntimeError("expected a contiguous 4-D uint8 batch")
    n, hs, ws, c = img.shape if layout == "hwc" else (img.shape[0], img.shape[2], img.shape[3], img.shape[1])
    _require_cuda(lut, "normalisation table")
    if tuple(lut.shape) != (c, 256) or not lut.is_contiguous() or lut.device != img.device:
        raise RuntimeError(f"normalisation table of shape {tuple(lut.shape)} for a batch of {c} channels")
    y0, x0, h, w = (0, 0, hs, ws) if box is None else box
    out = torch.empty((n, h, w, 4), device=img.device, dtype=torch.float32)
    check(lib.vq2_u8_to_nhwc4(_p(img), U8_LAYOUTS[layout], n, c, hs, ws, y0, x0, h, w, _p(lut), _p(out), _stream()),
          "u8_to_nhwc4")
    return out


def nhwc_to_u8(x, c, inv_s, mean, layout, canvas=None, cols=1, pad=0):
    """Internal NHWC tensor [N,H,W,>=c] -> 8-bit pixels (vq2_nhwc_to_u8): byte = trunc(clamp((x / inv_s[ch] + mean[ch])
    * 255 + 0.5, 0, 255)), every operation in fp32.  inv_s / mean: sequences of c Python floats already rounded to fp32.
    canvas None: a fresh batch, [N,H,W,c] for "hwc" or [N,c,H,W] for "chw".  canvas given (uint8, contiguous,
    [Hc,Wc,c] or [c,Hc,Wc]): image k is written at make_grid's origin of cell (k // cols, k % cols) with `pad` pixels
    around every cell; the other bytes of the canvas are left alone."""
    _require_cuda(x, "activation")
    if layout not in U8_LAYOUTS:
        raise ValueError(f"layout must be 'hwc' or 'chw', not {layout!r}")
    if not is_nhwc_dense(x):
        raise RuntimeError("nhwc_to_u8: expected a dense NHWC tensor")
    n, h, w, cp = x.shape
    if not 1 <= c <= min(cp, 4) or len(inv_s) != c or len(mean) != c:
        raise RuntimeError(f"nhwc_to_u8: {c} channels with {len(inv_s)} / {len(mean)} statistics from a tensor of {cp} lanes")
    hwc = layout == "hwc"
    if canvas is None:
        out = torch.empty((n, h, w, c) if hwc else (n, c, h, w), device=x.device, dtype=torch.uint8)
        hc, wc, cols, pad, image_pitch = h, w, 1, 0, h * w * c
    else:
        out = canvas
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.device == x.device and out.dim() == 3
                and out.is_contiguous() and out.shape[2 if hwc else 0] == c):
            raise RuntimeError(f"nhwc_to_u8: the canvas must be a contiguous uint8 tensor on {x.device} with {c} channels "
                               f"in layout '{layout}'")
        hc, wc = (out.shape[0], out.shape[1]) if hwc else (out.shape[1], out.shape[2])
        image_pitch = 0
    fa = (C.c_float * c)(*inv_s)
    fm = (C.c_float * c)(*mean)
    check(lib.vq2_nhwc_to_u8(_p(x), ld_of(x), n, c, h, w, fa, fm, _p(out), U8_LAYOUTS[layout], hc, wc,
                             wc * (c if hwc else 1), int(cols), int(pad), image_pitch, _stream()), "nhwc_to_u8")
    return out


def sse_per_image(a, b):
    """One fp32 sum of squared differences per image of two dense NHWC tensors of the same shape and pixel stride
    (vq2_sse_per_image; lanes beyond the real channels must agree, as the zero pad lane of NHWC4 does)."""
    _require_cuda(a, "reconstruction")
    _require_cuda(b, "target")
    if a.shape != b.shape or not (is_nhwc_dense(a) and is_nhwc_dense(b)) or ld_of(a) != ld_of(b) or ld_of(a) != a.shape[3]:
        raise RuntimeError("sse_per_image: two packed NHWC tensors of one shape expected")
    n, h, w, ld = a.shape
    out = torch.empty(n, device=a.device, dtype=torch.float32)
    nbytes = lib.vq2_sse_workspace_bytes(n, h, w, ld)
    ws = torch.empty(max(nbytes // 4, 1), device=a.device, dtype=torch.float32)
    check(lib.vq2_sse_per_image(_p(a), _p(b), n, h, w, ld, _p(out), _p(ws), nbytes, _stream()), "sse_per_image")
    return out


def index_hist(idx, counts, flag):
    """counts[idx] += 1 (vq2_index_hist): idx int64 of any shape, counts int64 [K] accumulated across calls, flag int32
    [1] set to 1 by an index outside [0, K) (which is counted nowhere)."""
    if not (idx.is_cuda and idx.dtype == torch.int64 and counts.dtype == torch.int64 and flag.dtype == torch.int32
            and counts.is_contiguous() and counts.device == idx.device and flag.device == idx.device):
        raise RuntimeError("index_hist: int64 indices and counts and an int32 flag on one GPU expected; no CPU path")
    ic = idx if idx.is_contiguous() else idx.contiguous()
    check(lib.vq2_index_hist(_p(ic), ic.numel(), counts.numel(), _p(counts), _p(flag), _stream()), "index_hist")


def eval_accumulate(sse, elems_per_image, diff, acc):
    """acc (float64 [4]: sse total, elements, latent total, images) += this batch, on the device (vq2_eval_accumulate)."""
    if not (acc.dtype == torch.float64 and acc.numel() == 4 and acc.is_contiguous() and acc.is_cuda):
        raise RuntimeError("eval_accumulate: the accumulator is a float64 [4] tensor on the GPU")
    d = diff.detach().reshape(-1)
    if d.numel() != 1 or d.dtype != torch.float32:
        raise RuntimeError("eval_accumulate: the latent loss is one float32 value")
    check(lib.vq2_eval_accumulate(_p(sse), sse.numel(), int(elems_per_image), _p(d), _p(acc), _stream()), "eval_accumulate")


def image_metrics(a, b, c, inv_s, mean):
    """Per image, between the 8-bit images nhwc_to_u8 would write from a (reconstruction) and b (target), dense NHWC
    tensors [N,H,W,>=c] (vq2_image_metrics): sse_u8 int64 [N], the exact sum of squared byte differences over the
    H * W * c elements, and ssim float64 [N], Gaussian-window SSIM (11x11, sigma 1.5, valid region, data range 255) in
    fp64.  inv_s / mean as for nhwc_to_u8.  Nothing is read back."""
    _require_cuda(a, "reconstruction")
    _require_cuda(b, "target")
    if not (is_nhwc_dense(a) and is_nhwc_dense(b)) or a.shape[:3] != b.shape[:3] or a.device != b.device:
        raise RuntimeError("image_metrics: two dense NHWC tensors of one [N,H,W] on one GPU expected")
    n, h, w, _ = a.shape
    if not 1 <= c <= min(a.shape[3], b.shape[3], 4) or len(inv_s) != c or len(mean) != c:
        raise RuntimeError(f"image_metrics: {c} channels with {len(inv_s)} / {len(mean)} statistics from tensors of "
                           f"{a.shape[3]} and {b.shape[3]} lanes")
    sse = torch.empty(n, device=a.device, dtype=torch.int64)
    ssim = torch.empty(n, device=a.device, dtype=torch.float64)
    nbytes = lib.vq2_image_metrics_workspace_bytes(n, c, h, w)
    ws = torch.empty(max(nbytes // 8, 1), device=a.device, dtype=torch.float64)
    fa = (C.c_float * c)(*inv_s)
    fm = (C.c_float * c)(*mean)
    check(lib.vq2_image_metrics(_p(a), ld_of(a), _p(b), ld_of(b), n, c, h, w, fa, fm, _p(sse), _p(ssim), _p(ws), nbytes,
                                _stream()), "image_metrics")
    return sse, ssim


def image_metrics_accumulate(sse_u8, ssim, acc_i, acc_d):
    """acc_i (int64 [1]) += sum of sse_u8; acc_d (float64 [1]) += ssim[0], then ssim[1], ... in image order, on the
    device (vq2_image_metrics_accumulate)."""
    if not (sse_u8.is_cuda and sse_u8.dtype == torch.int64 and ssim.dtype == torch.float64 and ssim.device == sse_u8.device
            and sse_u8.is_contiguous() and ssim.is_contiguous() and sse_u8.dim() == 1 and sse_u8.shape == ssim.shape):
        raise RuntimeError("image_metrics_accumulate: int64 [N] squared errors and float64 [N] SSIM values on one GPU "
                           "expected; no CPU path")
    if not (acc_i.dtype == torch.int64 and acc_d.dtype == torch.float64 and acc_i.numel() == 1 and acc_d.numel() == 1
            and acc_i.device == ssim.device and acc_d.device == ssim.device):
        raise RuntimeError("image_metrics_accumulate: the accumulators are an int64 [1] and a float64 [1] tensor on the GPU")
    check(lib.vq2_image_metrics_accumulate(_p(sse_u8), _p(ssim), sse_u8.numel(), _p(acc_i), _p(acc_d), _stream()),
          "image_metrics_accumulate")


def prior_eval_rows(out_nhwc, target, n_class):
    """Per pixel of the prior's NHWC logits [N,H,W,ceil4(n_class)] (any dense pixel stride, read in place) against int64
    targets [N,H,W] (vq2_prior_eval_rows) -> (nll float32 [N*H*W], entropy float32 [N*H*W], rank int32 [N*H*W]): the
    cross-entropy term, the entropy of the predicted distribution (both in nats) and the number of classes that beat the
    target (0: the hit of prior_loss, the lowest index winning a tie).  A target outside [0, n_class) gives nll 0 and
    rank -1.  Not an autograd function."""
    x = _rows(out_nhwc.detach(), n_class)
    target = _require_codes(target, "target")
    n, h, w, _ = x.shape
    m = n * h * w
    if target.numel() != m or target.device != x.device:
        raise RuntimeError("prior_eval_rows: one target per pixel, on the logits' GPU, expected")
    if not 1 <= n_class <= ONEHOT_MAX_CLASSES:
        raise NotImplementedError(f"vqvae2_amd: n_class must be in 1..{ONEHOT_MAX_CLASSES}, got {n_class}")
    nll = torch.empty(m, device=x.device, dtype=torch.float32)
    entropy = torch.empty(m, device=x.device, dtype=torch.float32)
    rank = torch.empty(m, device=x.device, dtype=torch.int32)
    check(lib.vq2_prior_eval_rows(_p(x), ld_of(x), _p(target), m, n_class, _p(nll), _p(entropy), _p(rank), _stream()),
          "prior_eval_rows")
    return nll, entropy, rank


def prior_eval_accumulate(nll, entropy, rank, n_images, top_k, pos_nll, pos_entropy, pos_hit1, pos_hitk, counters,
                          return_image_nll=False):
    """Fold the rows of one batch ([n_images, L] in image order, from prior_eval_rows) into the running state on the
    device (vq2_prior_eval_accumulate): pos_nll / pos_entropy float64 [L] += the rows of each position in image order,
    pos_hit1 / pos_hitk int64 [L] += the rows of rank 0 / of rank in [0, top_k), counters int64 [2] += (n_images, rows of
    rank -1).  No atomics: the state after batches of 5, 3 and 1 is bit for bit that after one batch of 9.
    return_image_nll: also the float32 [n_images] sums of nll over each image's positions."""
    m = nll.numel()
    if not (nll.is_cuda and nll.dtype == torch.float32 and entropy.dtype == torch.float32 and rank.dtype == torch.int32
            and entropy.numel() == m and rank.numel() == m and entropy.device == nll.device and rank.device == nll.device
            and nll.is_contiguous() and entropy.is_contiguous() and rank.is_contiguous()):
        raise RuntimeError("prior_eval_accumulate: float32 nll and entropy and int32 rank of one length on one GPU expected; "
                           "no CPU path")
    n_images, top_k = int(n_images), int(top_k)
    if n_images < 1 or m % n_images or top_k < 1:
        raise RuntimeError(f"prior_eval_accumulate: {m} rows are not {n_images} images, or top_k {top_k} < 1")
    length = m // n_images
    for t, dtype, size, what in ((pos_nll, torch.float64, length, "pos_nll"), (pos_entropy, torch.float64, length, "pos_entropy"),
                                 (pos_hit1, torch.int64, length, "pos_hit1"), (pos_hitk, torch.int64, length, "pos_hitk"),
                                 (counters, torch.int64, 2, "counters")):
        if not (t.dtype == dtype and t.numel() == size and t.is_contiguous() and t.device == nll.device):
            raise RuntimeError(f"prior_eval_accumulate: {what} must be a contiguous {dtype} [{size}] tensor on {nll.device}")
    image_nll = torch.empty(n_images, device=nll.device, dtype=torch.float32) if return_image_nll else None
    check(lib.vq2_prior_eval_accumulate(_p(nll), _p(entropy), _p(rank), n_images, length, top_k, _p(pos_nll), _p(pos_entropy),
                                        _p(pos_hit1), _p(pos_hitk), _p(counters),
                                        _p(image_nll) if image_nll is not None else None, _stream()), "prior_eval_accumulate")
    return image_nll


def from_nhwc(y, c):
    """Internal NHWC -> NCHW-shaped result (zero-copy channels-last view when C % 4 == 0)."""
    if y.shape[3] == c:
        return y.permute(0, 3, 1, 2)
    return NhwcToNchw.apply(y, c)


class ReluFn(Function):
    """Stand-alone ReLU (only used when a ReLU cannot be fused into a neighbouring conv)."""

    @staticmethod
    def forward(ctx, x):
        x = as_nhwc(x)
        y = relu_bwd(x, x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return relu_bwd(as_nhwc(g), y)


# ----------------------------------------------------------------------------- fused conv op
class GradStash:
    """Side channel for a tensor that is consumed twice (enc_b -> enc_t and the concat, vqvae.py:225,233):
    the consumer that back-propagates FIRST (CatViewFn) parks its gradient here instead of returning it,
    the one that runs LAST (the first conv of enc_t) adds it in its dgrad epilogue -- the sum autograd would
    form with a separate add kernel (+ a slice copy) happens inside a launch that exists anyway.  Either
    order is correct: a stash that was already taken refuses the put and the gradient flows normally."""

    def __init__(self, strict=False):
        self.tensor = None
        self.closed = False
        self.strict = strict   # the taker also applies a ReLU mask to the sum: falling back would be wrong, so raise

    def put(self, t):
        if self.closed:
            return False
        self.tensor = t
        return True

    def take(self):
        t, self.tensor, self.closed = self.tensor, None, True
        return t


class ConvFn(Function):
    """y = [relu]( conv|convT([relu] x) + b [+ residual] ), NHWC."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, spec, flags, out, grad_stash=None, mask_input=False, premasked=False):
        """mask_input: x is the output of a fused trailing ReLU and this op is the one that applies that ReLU's
        backward mask (to its complete input gradient); premasked: the consumers of y do the same for this op's
        own VQ2_RELU_OUT, so the incoming gradient is already masked."""
        ctx.grad_stash, ctx.mask_input, ctx.premasked = grad_stash, mask_input, premasked
        x = as_nhwc(x)
        if residual is not None:
            residual = as_nhwc(residual)
        y = conv_forward(spec, x, weight, bias, flags, residual, out)
        ctx.spec, ctx.flags = spec, flags
        ctx.has_res = residual is not None
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, y if (flags & VQ2_RELU_OUT) else None, bias)
        if out is not None:
            y = y.view_as(y)  # fresh tensor object aliasing the caller's buffer
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y, bias = ctx.saved_tensors
        spec, flags = ctx.spec, ctx.flags
        g = as_nhwc(dy)
        if (flags & VQ2_RELU_OUT) and not ctx.premasked:
            g = relu_bwd(g, y)
        relu_in = bool(flags & VQ2_RELU_IN)
        dx = dw = db = dres = None
        if ctx.needs_input_grad[0]:
            other = ctx.grad_stash.take() if ctx.grad_stash is not None else None   # gradient of x's second consumer
            dx = conv_dgrad(spec, x.shape, g, weight, mask=x if (relu_in or ctx.mask_input) else None, residual=other,
                            mask_after=ctx.mask_input)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = conv_wgrad(spec, x, g, relu_in, weight, bias, ctx.needs_input_grad[1],
                                ctx.has_bias and ctx.needs_input_grad[2])
        if ctx.has_res and ctx.needs_input_grad[3]:
            dres = g
        return dx, dw, db, dres, None, None, None, None, None, None


def conv_op(x, weight, bias, spec, relu_in=False, relu_out=False, residual=None, out=None, grad_stash=None,
            mask_input=False, premasked=False):
    flags = (VQ2_RELU_IN if relu_in else 0) | (VQ2_RELU_OUT if relu_out else 0)
    if grad_stash is not None and relu_in and not mask_input:
        grad_stash.closed = True      # the epilogue would mask before it adds
        grad_stash = None
    return ConvFn.apply(x, weight, bias, residual, spec, flags, out, grad_stash, mask_input, premasked)


# VQ2_FORMS (read once per process, like the library: csrc/vq2_common.h): "all" (default) or "direct" keep the fused
# kernels; "general" runs only the general kernels, and with them the ResBlock as separate conv launches
_FORMS = os.environ.get("VQ2_FORMS", "all")
if _FORMS not in ("all", "direct", "general"):
    raise ValueError(f"VQ2_FORMS={_FORMS!r}: expected all, direct or general")

# one-launch ResBlock forward (csrc/vq2_resblock.hip) where the channel counts allow it
RESBLOCK_FUSED = [_FORMS != "general"]


class ResBlockFn(Function):
    """vqvae.py:81-96 as two launches forward and four backward:
        r = relu(conv3x3(relu(x)) + b1)            (ReLU in + ReLU out fused)
        y = [relu]( conv1x1(r) + b2 + x )          (residual, optional trailing ReLU fused)
    backward fuses both ReLU masks and the skip-path add into the dgrad epilogues."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, spec1, spec2, relu_out, out, premasked=False):
        ctx.premasked = premasked
        x = as_nhwc(x)
        n, h, w, c = x.shape
        if RESBLOCK_FUSED[0] and lib.vq2_resblock_supported(c, spec1.co) and spec1.k == 3 and spec2.k == 1:
            r = torch.empty((n, h, w, spec1.co), device=x.device, dtype=torch.float32)
            y = out if out is not None else torch.empty((n, h, w, c), device=x.device, dtype=torch.float32)
            if tuple(y.shape) != (n, h, w, c) or not is_nhwc_dense(y):
                raise RuntimeError("ResBlock: bad `out` buffer")
            check(lib.vq2_resblock_fwd(n, h, w, c, spec1.co, VQ2_RELU_OUT if relu_out else 0, _p(x), ld_of(x),
                                       _p(packed_weight(spec1, w1, PACK_FWD)), _p(b1),
                                       _p(packed_weight(spec2, w2, PACK_FWD)), _p(b2), _p(r), ld_of(r), _p(y), ld_of(y),
                                       _stream()), "resblock_fwd")
        else:
            r = conv_forward(spec1, x, w1, b1, VQ2_RELU_IN | VQ2_RELU_OUT)
            y = conv_forward(spec2, r, w2, b2, VQ2_RELU_OUT if relu_out else 0, residual=x, out=out)
        ctx.spec1, ctx.spec2, ctx.relu_out = spec1, spec2, relu_out
        ctx.save_for_backward(x, r, w1, w2, y if relu_out else None, b1, b2)
        if out is not None:
            y = y.view_as(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, r, w1, w2, y, b1, b2 = ctx.saved_tensors
        s1, s2 = ctx.spec1, ctx.spec2
        g = as_nhwc(dy)
        if ctx.relu_out and not ctx.premasked:
            g = relu_bwd(g, y)
        n, h, w, c = x.shape
        if RESBLOCK_FUSED[0] and ctx.needs_input_grad[0] and lib.vq2_resblock_supported(c, s1.co) and s1.k == 3 and s2.k == 1:
            # both data gradients in one launch (dh is recomputed on each tile's halo and kept in LDS)
            dh = torch.empty((n, h, w, s1.co), device=x.device, dtype=torch.float32)
            dx = torch.empty((n, h, w, c), device=x.device, dtype=torch.float32)
            # with the deferred reduction active the same launch also produces the 1x1 conv's weight/bias gradient
            # partials (it holds g and r anyway): no separate wgrad launch for conv[3]
            sc = _step_ctx(w2)
            w2_ws = None
            if (sc is not None and ctx.needs_input_grad[3] and ctx.needs_input_grad[4] and
                    slot_of(w2) is not None and slot_of(b2) is not None):
                w2_ws, dw2, db2 = sc.batch.resblock_w2(n, h, w, c, s1.co, w2, b2)
            check(lib.vq2_resblock_bwd_data(n, h, w, c, s1.co, _p(g), ld_of(g), _p(r), ld_of(r), _p(x), ld_of(x),
                                            _p(packed_weight(s2, w2, PACK_DGRAD)), _p(packed_weight(s1, w1, PACK_DGRAD)),
                                            _p(dh), ld_of(dh), _p(dx), ld_of(dx), _p(w2_ws), _stream()), "resblock_bwd_data")
            if w2_ws is not None:
                dw1, db1 = conv_wgrad(s1, x, dh, True, w1, b1, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
                return dx, dw1, db1, dw2, db2, None, None, None, None, None
        else:
            # through conv1x1 and the inner ReLU (mask r > 0)
            dh = conv_dgrad(s2, r.shape, g, w2, mask=r)
            # through conv3x3 and the outer ReLU (mask x > 0), plus the skip gradient
            dx = conv_dgrad(s1, x.shape, dh, w1, mask=x, residual=g) if ctx.needs_input_grad[0] else None
        dw2, db2 = conv_wgrad(s2, r, g, False, w2, b2, ctx.needs_input_grad[3], ctx.needs_input_grad[4])
        dw1, db1 = conv_wgrad(s1, x, dh, True, w1, b1, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return dx, dw1, db1, dw2, db2, None, None, None, None, None


class CatViewFn(Function):
    """torch.cat([a, b], channel) where a and b were *produced into* adjacent channel slices
    of `buf` (vqvae.py:218,233): forward is free, backward hands out slices of the gradient."""

    @staticmethod
    def forward(ctx, a, b, buf, stash=None):
        ctx.ca = a.shape[3]
        ctx.stash = stash
        return buf.view_as(buf)

    @staticmethod
    def backward(ctx, g):
        g = as_nhwc(g)
        gb = g[..., ctx.ca:]
        if ctx.stash is not None:
            if ctx.stash.put(gb):
                gb = None      # b's other consumer adds it inside its own dgrad launch (GradStash)
            elif ctx.stash.strict:
                raise RuntimeError("GradStash: the consumer that applies b's ReLU mask ran before this gradient arrived")
        return g[..., :ctx.ca], gb, None, None


class CatFn(Function):
    """torch.cat([a, b], channel) of two NHWC tensors that already exist (vqvae_deep.py:276,298: the operands are
    handed in by the caller, so they cannot be produced into slices of one buffer like CatViewFn's): two
    slice-copy launches forward, slices of the gradient backward."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = as_nhwc(a), as_nhwc(b)
        n, h, w, ca = a.shape
        cb = b.shape[3]
        if tuple(b.shape[:3]) != (n, h, w):
            raise RuntimeError("CatFn: spatial sizes differ")
        out = torch.empty((n, h, w, ca + cb), device=a.device, dtype=torch.float32)
        pix = n * h * w
        check(lib.vq2_slice_copy(_p(a), ld_of(a), _p(out), ca + cb, pix, ca, 0, _stream()), "slice_copy")
        check(lib.vq2_slice_copy(_p(b), ld_of(b), _p(out[..., ca:]), ca + cb, pix, cb, 0, _stream()), "slice_copy")
        ctx.ca = ca
        return out

    @staticmethod
    def backward(ctx, g):
        g = as_nhwc(g)
        return g[..., :ctx.ca], g[..., ctx.ca:]


class AdaINFn(Function):
    """vqvae_deep.py:99-109 (+ the F.relu_ that follows it at :129,131 when relu=True):
    y = [relu]((1 + gamma) * instance_norm(x) + beta) with (gamma | beta) = h [N, 2C] = fc(style)."""

    @staticmethod
    def forward(ctx, x, h, relu, eps):
        x = as_nhwc(x)
        n, hh, w, c = x.shape
        _require_cuda(h, "AdaIN style projection")
        h2 = h.reshape(n, 2 * c)
        if not h2.is_contiguous():
            h2 = h2.contiguous()
        mean = torch.empty((n, c), device=x.device, dtype=torch.float32)
        rstd = torch.empty((n, c), device=x.device, dtype=torch.float32)
        y = torch.empty((n, hh, w, c), device=x.device, dtype=torch.float32)
        check(lib.vq2_instnorm_stats(_p(x), ld_of(x), n, hh * w, c, float(eps), _p(mean), _p(rstd), _stream()), "instnorm_stats")
        check(lib.vq2_adain_fwd(_p(x), ld_of(x), _p(mean), _p(rstd), _p(h2), n, hh * w, c, VQ2_RELU_OUT if relu else 0,
                                _p(y), c, _stream()), "adain_fwd")
        ctx.save_for_backward(x, mean, rstd, h2, y if relu else None)
        ctx.h_shape = h.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, h2, y = ctx.saved_tensors
        n, hh, w, c = x.shape
        g = as_nhwc(dy)
        dh = torch.empty((n, 2 * c), device=x.device, dtype=torch.float32)
        dx = torch.empty((n, hh, w, c), device=x.device, dtype=torch.float32)
        check(lib.vq2_adain_bwd(_p(g), ld_of(g), _p(y), c, _p(x), ld_of(x), _p(mean), _p(rstd), _p(h2), n, hh * w, c,
                                _p(dh), _p(dx), c, _stream()), "adain_bwd")
        return dx, dh.reshape(ctx.h_shape), None, None


class FanOutFn(Function):
    """One tensor consumed twice (enc_b -> enc_t and the concat, vqvae.py:225,233; quant_t ->
    dec_t and upsample_t, vqvae.py:232,217).  Forward: two aliases; backward: one add kernel."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, g1, g2):
        if g1 is None:
            return g2
        if g2 is None:
            return g1
        return add_(as_nhwc(g1), as_nhwc(g2))


class AddScalarsFn(Function):
    """diff_t + diff_b (vqvae.py:240) on the device without an ATen launch."""

    @staticmethod
    def forward(ctx, a, b):
        out = torch.empty(1, device=a.device, dtype=torch.float32)
        check(lib.vq2_axpby(_p(a), _p(b), 1.0, _p(out), 1, _stream()), "axpby")
        return out

    @staticmethod
    def backward(ctx, g):
        return g.reshape(()), g.reshape(())


# ----------------------------------------------------------------------------- causal attention (stage-2 prior)
ATTN_BQ = 64   # query / key tile lengths of csrc/vq2_attn.hip (AT_BQ, AT_BK): tests place their lengths around them
ATTN_BK = 64


def attn_check_geometry(channel, n_head):
    """The geometries vq2_causal_attn_* accept: dim_head = channel / n_head a multiple of 4 in 4..64."""
    if n_head < 1 or channel < 1 or channel % n_head:
        raise NotImplementedError(f"vqvae2_amd causal attention: channel ({channel}) must be a positive multiple of "
                                  f"n_head ({n_head})")
    dh = channel // n_head
    if not (4 <= dh <= 64 and dh % 4 == 0):
        raise NotImplementedError(f"vqvae2_amd causal attention: dim_head must be a multiple of 4 in 4..64 (got {dh})")
    return dh


def attn_bf16_eligible(channel, n_head):
    """Whether CausalAttnFn(..., bf16=True) takes the bf16-operand kernels at this geometry (vq2_causal_attn_bf16_eligible):
    dim_head = channel / n_head is 16, 32, 48 or 64.  Elsewhere the permission changes nothing."""
    d = AttnDesc()
    d.B, d.L, d.n_head, d.dim_head = 1, 1, n_head, attn_check_geometry(channel, n_head)
    return bool(lib.vq2_causal_attn_bf16_eligible(C.byref(d)))


def _attn_desc(b, l, n_head, dh, q, k, v, o, p, seed):
    d = AttnDesc()
    d.B, d.L, d.n_head, d.dim_head = b, l, n_head, dh
    d.ldq, d.ldk, d.ldv, d.ldo = ld_of(q), ld_of(k), ld_of(v), ld_of(o)
    d.p_drop, d.seed = float(p), int(seed) & 0xFFFFFFFFFFFFFFFF
    return d


def _attn_operand(t, what):
    """A dense NHWC [B,H,W,channel] tensor is the [B, L, channel] matrix with row stride ld the kernels take."""
    _require_cuda(t, what)
    return as_nhwc(t)


class CausalAttnFn(Function):
    """pixelsnail.py:220-228 for projected q, k, v ([B,H,W,n_head * dim_head] NHWC): strictly causal softmax(QK^T /
    sqrt(dim_head)) V over the H * W positions, dropout p on the probabilities keyed by `seed`.  Saves q, k, v and
    one log-sum-exp per (b, h, i); nothing of size L^2 exists in either pass.  bf16=True is the permission VQ2_ALLOW_BF16
    (include/vq2.h, vq2_causal_attn_fwd_ex): where attn_bf16_eligible holds the four matrix products take operands rounded
    to bfloat16 and accumulate in fp32, every tensor stays fp32; the backward runs the precision of its forward."""

    @staticmethod
    def forward(ctx, q, k, v, n_head, p, seed, bf16=False):
        q, k, v = _attn_operand(q, "q"), _attn_operand(k, "k"), _attn_operand(v, "v")
        b, hh, w, c = q.shape
        if k.shape != q.shape or v.shape != q.shape:
            raise RuntimeError("CausalAttnFn: q, k and v must have one shape")
        dh = attn_check_geometry(c, n_head)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"dropout probability must be in [0, 1), got {p}")
        l = hh * w
        o = torch.empty((b, hh, w, c), device=q.device, dtype=torch.float32)
        lse = torch.empty((b, n_head, l), device=q.device, dtype=torch.float32)
        d = _attn_desc(b, l, n_head, dh, q, k, v, o, p, seed)
        flags = VQ2_ALLOW_BF16 if bf16 else 0
        check(lib.vq2_causal_attn_fwd_ex(C.byref(d), flags, _p(q), _p(k), _p(v), _p(o), _p(lse), _stream()), "causal_attn_fwd")
        ctx.save_for_backward(q, k, v, lse)   # the backward kernels recompute P and need neither o nor anything of size L^2
        ctx.n_head, ctx.p, ctx.seed, ctx.flags = n_head, p, seed, flags
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, lse = ctx.saved_tensors
        b, hh, w, c = q.shape
        l = hh * w
        do = _attn_operand(do, "dO")
        dq, dk, dv = (torch.empty((b, hh, w, c), device=q.device, dtype=torch.float32) for _ in range(3))
        delta = torch.empty_like(lse)
        d = _attn_desc(b, l, ctx.n_head, c // ctx.n_head, q, k, v, dq, ctx.p, ctx.seed)
        check(lib.vq2_causal_attn_bwd_ex(C.byref(d), ctx.flags, _p(q), _p(k), _p(v), _p(lse), _p(do), ld_of(do), _p(dq), c,
                                         _p(dk), c, _p(dv), c, _p(delta), _stream()), "causal_attn_bwd")
        return dq, dk, dv, None, None, None, None


def causal_attn_keep_mask(b, n_head, l, p, seed, device):
    """The dropout keep decisions of CausalAttnFn for (p, seed) as a bool tensor [B, n_head, L, L] (the causal mask is
    not applied).  For tests at small L: this IS of size L^2."""
    mask = torch.empty((b, n_head, l, l), device=device, dtype=torch.uint8)
    d = AttnDesc()
    d.B, d.L, d.n_head, d.dim_head = b, l, n_head, 4
    d.ldq = d.ldk = d.ldv = d.ldo = 4 * n_head
    d.p_drop, d.seed = float(p), int(seed) & 0xFFFFFFFFFFFFFFFF
    check(lib.vq2_causal_attn_keep_mask(C.byref(d), _p(mask), _stream()), "causal_attn_keep_mask")
    return mask.bool()


class WeightNormFn(Function):
    """weight_norm(nn.Linear) (pixelsnail.py:17-18): w = g * v / ||v||_2 per output row; v [out, in], g [out, 1]."""

    @staticmethod
    def forward(ctx, v, g):
        _require_cuda(v, "weight_v")
        _require_cuda(g, "weight_g")
        rows, cols = v.shape
        if g.numel() != rows:
            raise RuntimeError("WeightNormFn: weight_g must hold one value per output row")
        vc = v if v.is_contiguous() else v.contiguous()
        gc = g if g.is_contiguous() else g.contiguous()
        w = torch.empty_like(vc)
        check(lib.vq2_weight_norm_fwd(_p(vc), _p(gc), _p(w), rows, cols, _stream()), "weight_norm_fwd")
        ctx.save_for_backward(vc, gc)
        return w

    @staticmethod
    def backward(ctx, dw):
        v, g = ctx.saved_tensors
        rows, cols = v.shape
        dwc = dw if dw.is_contiguous() else dw.contiguous()
        dv = torch.empty_like(v)
        dg = torch.empty_like(g)
        check(lib.vq2_weight_norm_bwd(_p(dwc), _p(v), _p(g), _p(dv), _p(dg), rows, cols, _stream()), "weight_norm_bwd")
        return dv, dg


class WeightNormPlan:
    """Every weight-normed tensor of a model whose parameters live in a ParamArena, formed and differentiated by ONE launch
    each (vq2_wn_table_fwd / vq2_wn_table_bwd) instead of one per layer and pass.  The plan owns the device table (built
    once, offsets only), a flat buffer of effective weights and one of their gradients; each layer's effective weight is
    a view of the first whose `_vq2_grad` is the matching view of the second, so the weight-gradient launches write there.

    The layers take their weight from the plan (planned_weight) only while it is `active` (its trainer's step is running) and
    `current` (prepare() ran after the last change of the parameters); otherwise they run the per-layer kernels as before.
    Entries are in arena order, so a contiguous slice of the gradient arena is a contiguous range of entries."""

    @staticmethod
    def layers(model):
        """[(name, module holding weight_v / weight_g, kh, kw, mask_from)] in registration order.  mask_from < kw only for a
        CausalConv2d(padding='causal'): the first kernel column of the last kernel row that it zeroes."""
        causal = {id(m.conv.conv): m.causal for m in model.modules()
                  if getattr(m, "padding", None) == "causal" and hasattr(m, "causal")}
        out = []
        for name, mod in model.named_modules():
            prm = mod._parameters
            if prm.get("weight_v") is None or prm.get("weight_g") is None:
                continue
            v = mod.weight_v
            kh, kw = (int(v.shape[2]), int(v.shape[3])) if v.dim() == 4 else (1, 1)
            out.append((name, mod, kh, kw, causal.get(id(mod), kw)))
        return out

    @classmethod
    def entries(cls, model, offset):
        """The table as a list of dicts (name, rows, cols, kh, kw, mask_from, v_off, g_off, w_off, row_start), in arena
        order, plus the names of the layers that stay on the per-layer kernels (a weight_v or weight_g outside the arena,
        or not contiguous).  offset: {id(parameter): offset in floats}, ParamArena.offset or ParamArena.layout()[1].
        Needs no device."""
        rows_of, skipped = [], []
        for name, mod, kh, kw, mask_from in cls.layers(model):
            v, g = mod.weight_v, mod.weight_g
            if id(v) not in offset or id(g) not in offset or not v.is_contiguous() or not g.is_contiguous() or \
                    g.numel() != v.shape[0]:
                skipped.append(name)
                continue
            rows = int(v.shape[0])
            rows_of.append(dict(name=name, module=mod, rows=rows, cols=v.numel() // rows, kh=kh, kw=kw, mask_from=mask_from,
                                v_off=offset[id(v)], g_off=offset[id(g)]))
        rows_of.sort(key=lambda e: e["v_off"])
        w_off = row_start = 0
        for e in rows_of:
            e["w_off"], e["row_start"] = w_off, row_start
            w_off += ceil4(e["rows"] * e["cols"])       # 16-byte slots, as in the arena
            row_start += e["rows"]
        return rows_of, skipped

    def __init__(self, model, arena):
        self.arena = arena
        self.table, self.skipped = self.entries(model, arena.offset)
        if not self.table:
            raise ValueError("WeightNormPlan: the model has no weight-normed layer inside the arena")
        n = self.n = len(self.table)
        total = sum(ceil4(e["rows"] * e["cols"]) for e in self.table)
        dev = arena.flat_p.device
        self.w = torch.zeros(total, device=dev, dtype=torch.float32)
        self.dw = torch.zeros(total, device=dev, dtype=torch.float32)
        arr = (WnEntry * (n + 1))()
        self.index, self.vg, self.w_views, self.dw_views = {}, [], [], []
        for i, e in enumerate(self.table):
            for k in ("v_off", "g_off", "w_off", "rows", "cols", "kh", "kw", "mask_from", "row_start"):
                setattr(arr[i], k, e[k])
            mod = e["module"]
            numel = e["rows"] * e["cols"]
            shape = (e["rows"], e["cols"] // (e["kh"] * e["kw"]), e["kh"], e["kw"])
            self.index[id(mod.weight_v)] = i
            self.vg.append((mod.weight_v, mod.weight_g))
            self.w_views.append(self.w[e["w_off"]:e["w_off"] + numel].view(shape))
            self.dw_views.append(self.dw[e["w_off"]:e["w_off"] + numel].view(shape))
            mod.weight_v._vq2_wn = self
        arr[n].row_start = self.table[-1]["row_start"] + self.table[-1]["rows"]      # the terminator: total rows
        self.table_dev = _upload_structs(arr, dev)
        self._ptrs = [(v.data_ptr(), g.data_ptr()) for v, g in self.vg]
        self.active = False
        self.current = False

    def first_entry_at(self, lo):
        """Index of the first entry whose parameters start at arena offset >= lo (entries are in arena order)."""
        return sum(1 for e in self.table if e["v_off"] < lo)

    def prepare(self):
        """One launch: the 'causal' zeros into weight_v, every effective weight into the flat buffer."""
        a = self.arena
        if any((v.data_ptr(), g.data_ptr()) != p for (v, g), p in zip(self.vg, self._ptrs)):
            raise RuntimeError("WeightNormPlan: a parameter was re-allocated; rebuild the trainer")
        check(lib.vq2_wn_table_fwd(_p(self.table_dev), self.n, _p(a.flat_p), _p(self.w), _stream()), "wn_table_fwd")
        self.current = True

    def backward(self, first, last):
        """One launch: dv, dg of the entries [first, last) from their dW, into the gradient arena."""
        a = self.arena
        check(lib.vq2_wn_table_bwd(_p(self.table_dev), first, last, _p(a.flat_p), _p(self.dw), _p(a.gp), _stream()),
              "wn_table_bwd")

    def invalidate(self):
        """The parameters changed (optimizer step, load_state_dict, broadcast): the flat buffer is stale."""
        self.current = False


class PlannedWeightFn(Function):
    """The autograd link between a layer and its WeightNormPlan.  Forward: the prepared view, no launch.  Backward: dW is
    already in its slot when the weight-gradient kernel honoured `_vq2_grad` (one copy if it could not); the gradients
    handed to weight_v and weight_g are their arena slots, whose values vq2_wn_table_bwd writes before anything reads them."""

    @staticmethod
    def forward(ctx, v, g, plan, i):
        ctx.plan, ctx.i = plan, i
        w = plan.w_views[i]
        return w.view_as(w)

    @staticmethod
    def backward(ctx, dw):
        plan, i = ctx.plan, ctx.i
        slot = plan.dw_views[i]
        if dw.data_ptr() != slot.data_ptr() or not dw.is_contiguous():
            slot.copy_(dw)
        v, g = plan.vg[i]
        if v.grad is not None or g.grad is not None:
            raise RuntimeError("WeightNormPlan: a second backward inside one trainer step (arena.zero_grad() first)")
        return _grad_slot(v), _grad_slot(g), None, None


def plan_ready(weight_v):
    """The WeightNormPlan that serves this weight_v right now, or None."""
    plan = getattr(weight_v, "_vq2_wn", None)
    if plan is not None and plan.active and plan.current and id(weight_v) in plan.index:
        return plan
    return None


def planned_weight(weight_v, weight_g):
    """The effective weight [out, in, kh, kw] from the layer's plan, or None when the layer has to form it itself."""
    plan = plan_ready(weight_v)
    if plan is None:
        return None
    i = plan.index[id(weight_v)]
    w = PlannedWeightFn.apply(weight_v, weight_g, plan, i)
    w._vq2_grad = plan.dw_views[i]
    return w


# ----------------------------------------------------------------------------- GatedResBlock pieces (stage-2 prior)
def _rows(t, c):
    """Dense NHWC operand of an elementwise kernel: real channels c, ceil4(c) stored."""
    t = as_nhwc(t)
    if t.shape[3] != ceil4(c):
        raise RuntimeError(f"expected {ceil4(c)} stored channels for {c} real ones, got {t.shape[3]}")
    return t


class EluFn(Function):
    """y = ELU(x) (alpha 1) over NHWC with `c` real channels; pad lanes of y are 0.  Saves y only: the backward is
    dx = dy * (y > 0 ? 1 : y + 1)."""

    @staticmethod
    def forward(ctx, x, c):
        x = _rows(x, c)
        n, h, w, cp = x.shape
        y = torch.empty((n, h, w, cp), device=x.device, dtype=torch.float32)
        check(lib.vq2_elu_fwd(_p(x), ld_of(x), _p(y), cp, n * h * w, c, _stream()), "elu_fwd")
        ctx.save_for_backward(y)
        ctx.c = c
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _rows(dy, ctx.c)
        n, h, w, cp = y.shape
        dx = torch.empty_like(y)
        check(lib.vq2_elu_bwd(_p(dy), ld_of(dy), _p(y), cp, _p(dx), cp, n * h * w, ctx.c, _stream()), "elu_bwd")
        return dx, None


class EluDropoutFn(Function):
    """y = dropout(ELU(x)) in one pass (pixelsnail.py:167-168): keep decisions are a function of (seed, flat index of the
    element in the unpadded tensor) alone, survivors are scaled by 1 / (1 - p).  Saves x: the backward recomputes the
    decisions and the derivative exp(x) from it."""

    @staticmethod
    def forward(ctx, x, c, p, seed):
        x = _rows(x, c)
        n, h, w, cp = x.shape
        y = torch.empty((n, h, w, cp), device=x.device, dtype=torch.float32)
        check(lib.vq2_elu_dropout_fwd(_p(x), ld_of(x), _p(y), cp, n * h * w, c, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                      _stream()), "elu_dropout_fwd")
        ctx.save_for_backward(x)
        ctx.c, ctx.p, ctx.seed = c, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _rows(dy, ctx.c)
        n, h, w, cp = x.shape
        dx = torch.empty((n, h, w, cp), device=x.device, dtype=torch.float32)
        check(lib.vq2_elu_dropout_bwd(_p(dy), ld_of(dy), _p(x), ld_of(x), _p(dx), cp, n * h * w, ctx.c, ctx.p, ctx.seed,
                                      _stream()), "elu_dropout_bwd")
        return dx, None, None, None


def dropout_keep_mask(pixels, c, p, seed, device):
    """The keep decisions of EluDropoutFn for (p, seed) as a bool tensor [pixels, c] (for tests)."""
    mask = torch.empty((pixels, c), device=device, dtype=torch.uint8)
    check(lib.vq2_dropout_keep_mask(_p(mask), pixels, c, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()),
          "dropout_keep_mask")
    return mask.bool()


class GluResFn(Function):
    """out = t[..., :ch] * sigmoid(t[..., ch:2ch]) + res (pixelsnail.py:176-177), t with 2 * ch real channels, res and out
    with ch.  Saves t; the backward recomputes the sigmoid and hands dout on as the gradient of res."""

    @staticmethod
    def forward(ctx, t, res, ch):
        t, res = _rows(t, 2 * ch), _rows(res, ch)
        n, h, w, _ = t.shape
        if tuple(res.shape[:3]) != (n, h, w):
            raise RuntimeError("GluResFn: t and res must cover the same pixels")
        out = torch.empty((n, h, w, ceil4(ch)), device=t.device, dtype=torch.float32)
        check(lib.vq2_glu_res_fwd(_p(t), ld_of(t), _p(res), ld_of(res), _p(out), ceil4(ch), n * h * w, ch, _stream()),
              "glu_res_fwd")
        ctx.save_for_backward(t)
        ctx.ch = ch
        return out

    @staticmethod
    def backward(ctx, dout):
        (t,) = ctx.saved_tensors
        dout = _rows(dout, ctx.ch)
        n, h, w, cp = t.shape
        dt = None
        if ctx.needs_input_grad[0]:
            dt = torch.empty((n, h, w, cp), device=t.device, dtype=torch.float32)
            check(lib.vq2_glu_res_bwd(_p(dout), ld_of(dout), _p(t), ld_of(t), _p(dt), cp, n * h * w, ctx.ch, _stream()),
                  "glu_res_bwd")
        return dt, (dout if ctx.needs_input_grad[1] else None), None


def require_labels(label, batch, device):
    """`label` as the label kernels read it: int64 [batch], contiguous, on `device`."""
    if not (isinstance(label, torch.Tensor) and label.dtype == torch.int64 and label.device == device and label.dim() == 1
            and label.shape[0] == batch):
        raise RuntimeError(f"vqvae2_amd: label must be an int64 tensor [{batch}] on {device} (got "
                           f"{getattr(label, 'dtype', type(label))} {tuple(getattr(label, 'shape', ()))} on "
                           f"{getattr(label, 'device', '?')})")
    return label if label.is_contiguous() else label.contiguous()


class GluResLabelFn(Function):
    """GluResFn with the class label: [a | b] = t + embed[label[image]], out = a * sigmoid(b) + res.  embed is the fp32 table
    [n_label, 2 * ch], label int64 [N] on the device; a label outside [0, n_label) adds nothing and receives no gradient.
    Saves t (the conv output, as GluResFn) and label; the backward recomputes the sum and the sigmoid, writes dt
    (vq2_glu_res_label_bwd) and sums it per image and label row into the table's gradient slot (vq2_label_embed_grad, fixed
    order)."""

    @staticmethod
    def forward(ctx, t, res, ch, embed, label):
        t, res = _rows(t, 2 * ch), _rows(res, ch)
        n, h, w, _ = t.shape
        if tuple(res.shape[:3]) != (n, h, w):
            raise RuntimeError("GluResLabelFn: t and res must cover the same pixels")
        if embed.dim() != 2 or embed.shape[1] != 2 * ch or embed.dtype != torch.float32 or not embed.is_contiguous():
            raise RuntimeError(f"GluResLabelFn: a contiguous float32 table [n_label, {2 * ch}] expected")
        label = require_labels(label, n, t.device)
        out = torch.empty((n, h, w, ceil4(ch)), device=t.device, dtype=torch.float32)
        check(lib.vq2_glu_res_label_fwd(_p(t), ld_of(t), _p(res), ld_of(res), _p(embed), 2 * ch, _p(label), n, h * w, _p(out),
                                        ceil4(ch), n * h * w, ch, embed.shape[0], _stream()), "glu_res_label_fwd")
        ctx.save_for_backward(t, label)
        ctx.ch, ctx.embed = ch, embed
        return out

    @staticmethod
    def backward(ctx, dout):
        t, label = ctx.saved_tensors
        embed, ch = ctx.embed, ctx.ch
        dout = _rows(dout, ch)
        n, h, w, cp = t.shape
        dt = dE = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[3]:
            dt = torch.empty((n, h, w, cp), device=t.device, dtype=torch.float32)
            check(lib.vq2_glu_res_label_bwd(_p(dout), ld_of(dout), _p(t), ld_of(t), _p(embed), 2 * ch, _p(label), n, h * w,
                                            _p(dt), cp, n * h * w, ch, embed.shape[0], _stream()), "glu_res_label_bwd")
        if ctx.needs_input_grad[3]:
            dE = _grad_slot(embed)
            nbytes = lib.vq2_label_embed_grad_workspace_bytes(n, h * w, 2 * ch)
            ws = torch.empty(max(nbytes // 4, 4), device=t.device, dtype=torch.float32)
            check(lib.vq2_label_embed_grad(_p(dt), cp, _p(label), n, h * w, 2 * ch, embed.shape[0], _p(dE), _p(ws), nbytes,
                                           _stream()), "label_embed_grad")
        return (dt if ctx.needs_input_grad[0] else None), (dout if ctx.needs_input_grad[1] else None), None, dE, None


# ----------------------------------------------------------------------------- the two ends of PixelSNAIL (stage-2 prior)
ONEHOT_MAX_CLASSES = 16384


def _require_codes(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64):
        raise RuntimeError(f"vqvae2_amd: {what} must be an int64 tensor on the MI355X (got "
                           f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '?')})")
    return t if t.is_contiguous() else t.contiguous()


def onehot_check_geometry(n_class, kh, kw):
    """What vq2_onehot_conv_* accept: kernel sides in 1..7 with at most 32 taps, 1..16,384 classes."""
    if not (1 <= kh <= 7 and 1 <= kw <= 7 and kh * kw <= 32):
        raise NotImplementedError(f"vqvae2_amd one-hot conv: kernel sides in 1..7 with at most 32 taps, got {kh} x {kw}")
    if not 1 <= n_class <= ONEHOT_MAX_CLASSES:
        raise NotImplementedError(f"vqvae2_amd: n_class must be in 1..{ONEHOT_MAX_CLASSES}, got {n_class}")


def _onehot_desc(n, h, w, cout, n_class, geom, shift, ldy):
    d = OneHotDesc()
    d.N, d.H, d.W, d.Co, d.n_class = n, h, w, cout, n_class
    d.KH, d.KW, d.pad_top, d.pad_left = geom
    d.shift_down, d.shift_right = shift
    d.ldy = ldy
    return d


class OneHotConvFn(Function):
    """shift(conv_at(one_hot(idx), weight, bias, pad_top, pad_left)) [+ acc] over integer codes idx [N,H,W] (pixelsnail.py:
    401-406): no one-hot tensor, no separate shift or add pass.  weight [Co, n_class, KH, KW] is the effective (already
    weight-normed) weight; geom = (KH, KW, pad_top, pad_left); shift = (shift_down, shift_right), each 0 or 1 -- the row /
    column that enters is 0, bias included; acc: an NHWC tensor [N,H,W,ceil4(Co)] added everywhere, or None.  Returns NHWC
    [N,H,W,ceil4(Co)].  An index outside [0, n_class) contributes nothing (the reference's F.one_hot raises; this does
    not).  Backward: the dense weight gradient (exact zeros for absent classes), the bias gradient over the pixels that
    were not shifted in, and dy itself for acc; no gradient for the integer input."""

    @staticmethod
    def forward(ctx, idx, weight, bias, geom, shift, acc):
        idx = _require_codes(idx, "codes")
        _require_cuda(weight, "weight")
        if idx.dim() != 3 or weight.dim() != 4 or tuple(weight.shape[2:]) != tuple(geom[:2]):
            raise RuntimeError("OneHotConvFn: codes [N,H,W] and weight [Co, n_class, KH, KW] expected")
        n, h, w = idx.shape
        cout, n_class, kh, kw = weight.shape
        onehot_check_geometry(n_class, kh, kw)
        wsrc = weight.detach()
        wsrc = wsrc if wsrc.is_contiguous() else wsrc.contiguous()
        cp = ceil4(cout)
        wp = torch.empty(kh * kw * n_class * cp, device=idx.device, dtype=torch.float32)
        check(lib.vq2_onehot_pack_weight(_p(wsrc), _p(wp), cout, n_class, kh, kw, _stream()), "onehot_pack_weight")
        if acc is not None:
            acc = _rows(acc, cout)
            if tuple(acc.shape[:3]) != (n, h, w):
                raise RuntimeError("OneHotConvFn: acc must cover the same pixels")
        y = torch.empty((n, h, w, cp), device=idx.device, dtype=torch.float32)
        d = _onehot_desc(n, h, w, cout, n_class, geom, shift, cp)
        check(lib.vq2_onehot_conv_fwd(C.byref(d), _p(idx), _p(wp), _p(bias), _p(acc), ld_of(acc) if acc is not None else 0,
                                      _p(y), _stream()), "onehot_conv_fwd")
        ctx.save_for_backward(idx)
        ctx.geom, ctx.shift, ctx.wshape, ctx.has_bias = tuple(geom), tuple(shift), tuple(weight.shape), bias is not None
        # where the gradients go: a plan's dW slot for the weight (decided here, the weight is not kept: non-leaf only, see
        # slot_of), the arena slot for the bias (None: fresh tensors)
        ctx.dw_slot, ctx.bias = (None if weight.is_leaf else slot_of(weight)), bias
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        n, h, w = idx.shape
        cout, n_class, kh, kw = ctx.wshape
        dy = _rows(dy, cout)
        dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            d = _onehot_desc(n, h, w, cout, n_class, ctx.geom, ctx.shift, ld_of(dy))
            slot = ctx.dw_slot
            dw = slot.view_as(slot) if slot is not None else torch.empty(ctx.wshape, device=dy.device, dtype=torch.float32)
            ws = nbytes = None
            if ctx.has_bias and ctx.needs_input_grad[2]:
                db = _grad_slot(ctx.bias)
                nbytes = lib.vq2_onehot_conv_wgrad_workspace_bytes(C.byref(d))
                ws = torch.empty(max(nbytes // 8, 1), device=dy.device, dtype=torch.float64)
            check(lib.vq2_onehot_conv_wgrad(C.byref(d), _p(idx), _p(dy), _p(dw), _p(db), _p(ws), nbytes or 0, _stream()),
                  "onehot_conv_wgrad")
        return None, dw, db, None, None, (dy if ctx.needs_input_grad[5] else None)


def onehot_conv(idx, weight, bias, geom, shift=(0, 0), acc=None):
    return OneHotConvFn.apply(idx, weight, bias, tuple(geom), tuple(shift), acc)


class Upsample2Fn(Function):
    """Nearest x2 upsample of an NHWC tensor with `c` real channels (F.interpolate(condition, scale_factor=2),
    pixelsnail.py:422); backward: the sum of each 2x2 block in a fixed order."""

    @staticmethod
    def forward(ctx, x, c):
        x = _rows(x, c)
        n, h, w, cp = x.shape
        y = torch.empty((n, 2 * h, 2 * w, cp), device=x.device, dtype=torch.float32)
        check(lib.vq2_upsample2_fwd(_p(x), ld_of(x), _p(y), cp, n, h, w, c, _stream()), "upsample2_fwd")
        ctx.c, ctx.shape = c, (n, h, w, cp)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _rows(dy, ctx.c)
        n, h, w, cp = ctx.shape
        dx = torch.empty((n, h, w, cp), device=dy.device, dtype=torch.float32)
        check(lib.vq2_upsample2_bwd(_p(dy), ld_of(dy), _p(dx), cp, n, h, w, ctx.c, _stream()), "upsample2_bwd")
        return dx, None


class CrossEntropyFn(Function):
    """(mean cross-entropy, accuracy, hit count) of NHWC logits [N,H,W,ceil4(n_class)] against int64 targets [N,H,W]
    (nn.CrossEntropyLoss and out.max(1), train_pixelsnail.py:39,46-48).  One pass reads each row for the loss, the hit and
    the two saved row values (maximum, log of the sum of exponentials); the backward writes the gradient from the logits
    and those.  The lowest index wins an arg-max tie.  A target outside [0, n_class) gives its row no loss term, no hit and
    no gradient, and still counts in the mean (the reference raises there)."""

    @staticmethod
    def forward(ctx, x, target, n_class):
        x = _rows(x, n_class)
        target = _require_codes(target, "target")
        n, h, w, _ = x.shape
        m = n * h * w
        if target.numel() != m:
            raise RuntimeError("prior_loss: one target per pixel expected")
        if not 1 <= n_class <= ONEHOT_MAX_CLASSES:
            raise NotImplementedError(f"vqvae2_amd: n_class must be in 1..{ONEHOT_MAX_CLASSES}, got {n_class}")
        dev = x.device
        stat = torch.empty((m, 2), device=dev, dtype=torch.float32)
        nll = torch.empty(m, device=dev, dtype=torch.float32)
        ok = torch.empty(m, device=dev, dtype=torch.int32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        acc = torch.empty((), device=dev, dtype=torch.float32)
        count = torch.empty((), device=dev, dtype=torch.int32)
        check(lib.vq2_xent_fwd(_p(x), ld_of(x), _p(target), m, n_class, _p(stat), _p(nll), _p(ok), _p(loss), _p(acc),
                               _p(count), _stream()), "xent_fwd")
        ctx.save_for_backward(x, target, stat)
        ctx.n_class = n_class
        ctx.mark_non_differentiable(acc, count)
        return loss, acc, count

    @staticmethod
    def backward(ctx, g, _gacc, _gcount):
        x, target, stat = ctx.saved_tensors
        n, h, w, cp = x.shape
        _require_cuda(g, "loss gradient")
        gc = g.reshape(1)
        gc = gc if gc.is_contiguous() else gc.contiguous()
        dx = torch.empty((n, h, w, cp), device=x.device, dtype=torch.float32)
        check(lib.vq2_xent_bwd(_p(x), ld_of(x), _p(target), _p(stat), _p(gc), n * h * w, ctx.n_class, _p(dx), cp, _stream()),
              "xent_bwd")
        return dx, None, None


def prior_loss(out, target, return_count=False):
    """(loss, accuracy) of PixelSNAIL's output `out` [B,n_class,H,W] against the codes `target` [B,H,W]: both 0-dim device
    tensors, the loss differentiable, accuracy = hits / target.numel() (train_pixelsnail.py:39,46-48).  The channels-last
    view the model returns is read in place.  The lowest class index wins an arg-max tie; 1 <= n_class <= 16,384; a target
    outside [0, n_class) is skipped as CrossEntropyFn describes."""
    _require_cuda(out, "out")
    if out.dim() != 4 or target.dim() != 3 or out.shape[0] != target.shape[0] or tuple(out.shape[2:]) != tuple(target.shape[1:]):
        raise RuntimeError("prior_loss: out [B,n_class,H,W] and target [B,H,W] expected")
    loss, acc, count = CrossEntropyFn.apply(to_nhwc(out), target, out.shape[1])
    return (loss, acc, count) if return_count else (loss, acc)


class CatNFn(Function):
    """torch.cat(parts, channel) of NHWC tensors whose stored widths are multiples of 4 and of which only the LAST may carry
    pad lanes (PixelBlock's [input, out, background]: 256 + 256 + 2 real channels in 516 stored): one slice copy per part
    forward, slices of the gradient backward."""

    @staticmethod
    def forward(ctx, *parts):
        parts = [as_nhwc(t) for t in parts]
        n, h, w, _ = parts[0].shape
        if any(tuple(t.shape[:3]) != (n, h, w) for t in parts):
            raise RuntimeError("CatNFn: spatial sizes differ")
        widths = [t.shape[3] for t in parts]
        total = sum(widths)
        out = torch.empty((n, h, w, total), device=parts[0].device, dtype=torch.float32)
        off = 0
        for t, c in zip(parts, widths):
            check(lib.vq2_slice_copy(_p(t), ld_of(t), _p(out[..., off:]), total, n * h * w, c, 0, _stream()), "slice_copy")
            off += c
        ctx.widths = widths
        return out

    @staticmethod
    def backward(ctx, g):
        g = as_nhwc(g)
        outs, off = [], 0
        for i, c in enumerate(ctx.widths):
            outs.append(g[..., off:off + c] if ctx.needs_input_grad[i] else None)
            off += c
        return tuple(outs)


# ----------------------------------------------------------------------------- Quantize
def vq_prepare(embed):
    d, k = embed.shape
    embed_t = torch.empty((k, d), device=embed.device, dtype=torch.float32)
    enorm = torch.empty(k, device=embed.device, dtype=torch.float32)
    check(lib.vq2_vq_prepare(_p(embed), _p(embed_t), _p(enorm), d, k, _stream()), "vq_prepare")
    return embed_t, enorm


# The EMA statistics of one quantizer (vqvae.py:55-56) travel as ONE flat fp32 buffer
#     [counts (K) | zero pad to a multiple of 4 floats | sumsT (K*D)]
# so that sumsT starts on a 16-byte boundary for every K (no pad, i.e. today's [counts | sumsT], when K % 4 == 0).
# The pad is written once, when the buffer is allocated: the statistics kernels never touch it and it rides through
# the all-reduce as zeros.  Everything that slices such a buffer goes through these three functions.
def vq_stats_numel(k, d):
    return (k + 3) // 4 * 4 + k * d


def vq_stats_views(stats, k, d):
    """(counts [K], sumsT [K*D]) views of a statistics buffer."""
    if stats.numel() != vq_stats_numel(k, d) or not stats.is_contiguous():
        raise RuntimeError(f"vq statistics buffer must be contiguous with {vq_stats_numel(k, d)} floats (K={k}, D={d})")
    off = (k + 3) // 4 * 4
    return stats[:k], stats[off:]


def vq_stats_alloc(k, d, device):
    stats = torch.empty(vq_stats_numel(k, d), device=device, dtype=torch.float32)
    if k % 4:
        stats[k:(k + 3) // 4 * 4].zero_()
    return stats


class QuantizeFn(Function):
    """vqvae.py:42-75 minus the EMA update (done by the module after the all-reduce).
    Returns (ste_out [N,H,W,D], diff 0-dim, idx int64 [N,H,W], stats) where stats is the flat
    fp32 statistics buffer of vqvae.py:55-56 in the layout of vq_stats_views (None in eval mode)."""

    @staticmethod
    def forward(ctx, x, embed, want_stats, stats_buf, out_buf, prep=None, stats_stream=None, restart=None):
        """prep: (embedT, enorm) of `embed` if the caller already holds them (Quantize caches what
        vq2_vq_ema_update_prepare leaves), else they are computed here.
        stats_stream: side stream for the EMA statistics when their consumer is far away (Stage1Trainer applies the
        EMA update after backward): five small latency-bound launches that then run beside the matrix-bound
        forward / backward kernels instead of between them.  The caller joins the stream before it reads stats_buf.
        restart: None, or (cand [K*D], seed, step, slot, rank, world) of the dead-code restart: with want_stats the
        candidate rows are gathered from the same x right after the statistics, on their stream (vq_restart_candidates)."""
        x = as_nhwc(x)
        n, h, w, d = x.shape
        k = embed.shape[1]
        m = n * h * w
        embed_t, enorm = prep if prep is not None else vq_prepare(embed)
        idx = torch.empty((n, h, w), device=x.device, dtype=torch.int64)
        if out_buf is None:
            out = torch.empty((n, h, w, d), device=x.device, dtype=torch.float32)
        else:
            if tuple(out_buf.shape) != (n, h, w, d) or not is_nhwc_dense(out_buf):
                raise RuntimeError("QuantizeFn: bad output buffer")
            out = out_buf.view_as(out_buf)
        part = torch.empty(lib.vq2_vq_fwd_workspace_floats(m, d, k), device=x.device, dtype=torch.float32)
        check(lib.vq2_vq_fwd(_p(x), ld_of(x), _p(embed), _p(embed_t), _p(enorm), m, d, k, _p(idx), _p(out), ld_of(out),
                             _p(part), _stream()), "vq_fwd")
        stats = None
        if want_stats:
            if stats_buf is not None:
                stats = stats_buf.view_as(stats_buf)
            else:
                stats = vq_stats_alloc(k, d, x.device)
            counts, sums_t = vq_stats_views(stats, k, d)
            # every count and sum is written (deterministic sort + ordered sums, no atomics, no zeroing)
            nbytes = lib.vq2_vq_stats_workspace_bytes(m, d, k)
            ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.int32)
            if stats_stream is not None and stats_buf is not None:
                stats_stream.wait_event(torch.cuda.current_stream().record_event())
                with torch.cuda.stream(stats_stream):
                    check(lib.vq2_vq_stats(_p(x), ld_of(x), _p(idx), m, d, k, _p(counts), _p(sums_t), _p(ws), nbytes,
                                           _stream()), "vq_stats")
                    if restart is not None:
                        vq_restart_candidates(x, k, *restart)
                for tns in (x, idx, ws):
                    tns.record_stream(stats_stream)
            else:
                check(lib.vq2_vq_stats(_p(x), ld_of(x), _p(idx), m, d, k, _p(counts), _p(sums_t), _p(ws), nbytes,
                                       _stream()), "vq_stats")
                if restart is not None:
                    vq_restart_candidates(x, k, *restart)
        diff = torch.empty((), device=x.device, dtype=torch.float32)
        check(lib.vq2_vq_loss(_p(part), m, d, _p(diff), _stream()), "vq_loss")
        ctx.save_for_backward(x, idx, embed_t)
        ctx.k = k
        ctx.set_materialize_grads(False)   # no zero-filled gradients for idx / stats (two fill launches per call)
        ctx.mark_non_differentiable(idx)
        if stats is not None:
            ctx.mark_non_differentiable(stats)
        return out, diff, idx, stats

    @staticmethod
    def backward(ctx, g_out, g_diff, _gi, _gs):
        x, idx, embed_t = ctx.saved_tensors
        n, h, w, d = x.shape
        if g_out is None and g_diff is None:
            return None, None, None, None, None, None, None, None
        if g_out is not None:
            g_out = as_nhwc(g_out)
        if g_diff is not None and not g_diff.is_contiguous():
            g_diff = g_diff.contiguous()
        dx = torch.empty((n, h, w, d), device=x.device, dtype=torch.float32)
        check(lib.vq2_vq_bwd(_p(g_out), ld_of(g_out) if g_out is not None else d, _p(g_diff), _p(x), ld_of(x),
                             _p(idx), _p(embed_t), n * h * w, d, ctx.k, _p(dx), d, _stream()), "vq_bwd")
        return dx, None, None, None, None, None, None, None


def vq_ema_update(embed, cluster_size, embed_avg, stats, decay, eps, prep_out=None):
    """prep_out: (embedT [K,D], enorm [K]) buffers that receive the prepared form of the UPDATED codebook (same launch)."""
    d, k = embed.shape
    counts, sums_t = vq_stats_views(stats, k, d)
    scratch = torch.empty(4, device=embed.device, dtype=torch.float32)
    if prep_out is not None:
        check(lib.vq2_vq_ema_update_prepare(_p(embed), _p(cluster_size), _p(embed_avg), _p(counts), _p(sums_t), d, k,
                                            float(decay), float(eps), _p(scratch), _p(prep_out[0]), _p(prep_out[1]),
                                            _stream()), "vq_ema_update_prepare")
        return True
    check(lib.vq2_vq_ema_update(_p(embed), _p(cluster_size), _p(embed_avg), _p(counts), _p(sums_t), d, k,
                                float(decay), float(eps), _p(scratch), _stream()), "vq_ema_update")
    return False


def vq_restart_candidates(x, k, cand, seed, step, slot, rank=0, world=1, picks=None):
    """cand [K*D] <- the candidate row of every code from this rank's x [..., D] (NHWC latents, as vq2_vq_stats reads them),
    zeros for rows another rank owns; picks (int64 [K], optional) <- the global rows drawn.  On the current stream."""
    n, h, w, d = x.shape
    m = n * h * w
    if cand.numel() != k * d or not cand.is_contiguous() or cand.dtype != torch.float32:
        raise RuntimeError(f"vq_restart_candidates: cand must be {k * d} contiguous floats (K={k}, D={d})")
    if picks is not None and (picks.numel() != k or picks.dtype != torch.int64 or not picks.is_contiguous()):
        raise RuntimeError(f"vq_restart_candidates: picks must be {k} contiguous int64")
    check(lib.vq2_vq_restart_candidates(_p(x), ld_of(x), m, d, k, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1),
                                        int(slot), int(rank), int(world), _p(cand), _p(picks), _stream()),
          "vq_restart_candidates")


def vq_ema_update_restart(embed, cluster_size, embed_avg, stats, cand, decay, eps, threshold, counter, prep_out=None):
    """vq_ema_update with dead-code restarts: a code whose new size is below `threshold` and whose candidate row in
    cand [K*D] is finite restarts from it.  counter: int64 [2] on the device, {restarted by this call, running total}."""
    d, k = embed.shape
    counts, sums_t = vq_stats_views(stats, k, d)
    if counter.dtype != torch.int64 or counter.numel() != 2 or not counter.is_contiguous() or counter.device != embed.device:
        raise RuntimeError("vq_ema_update_restart: counter must be 2 contiguous int64 on the codebook's device")
    scratch = torch.empty(4 + k, device=embed.device, dtype=torch.float32)    # n, then the dead mask
    et, en = prep_out if prep_out is not None else (None, None)
    check(lib.vq2_vq_ema_update_restart(_p(embed), _p(cluster_size), _p(embed_avg), _p(counts), _p(sums_t), _p(cand), d, k,
                                        float(decay), float(eps), float(threshold), _p(scratch), _p(et), _p(en),
                                        _p(counter), _stream()), "vq_ema_update_restart")
    return prep_out is not None


def vq_gather(idx, embed, prep=None):
    """embed_code (vqvae.py:77-78): idx [...] int64 -> [..., D]."""
    d, k = embed.shape
    embed_t, _ = prep if prep is not None else vq_prepare(embed)
    idx_c = idx.contiguous()
    m = idx_c.numel()
    out = torch.empty((*idx.shape, d), device=embed.device, dtype=torch.float32)
    check(lib.vq2_vq_gather(_p(idx_c), _p(embed_t), m, d, k, _p(out), d, _stream()), "vq_gather")
    return out


# ----------------------------------------------------------------------------- loss
def _scale_by(src, scalar, alpha=1.0):
    """src * scalar[0] * alpha with the scalar read on the device (no host sync)."""
    out = torch.empty_like(src)
    sc = scalar.reshape(1) if scalar.is_contiguous() else scalar.contiguous().reshape(1)
    check(lib.vq2_scale(_p(src), _p(sc), float(alpha), _p(out), src.numel(), _stream()), "scale")
    return out


class MseLossFn(Function):
    """nn.MSELoss() (train_vqvae.py:31,83); the gradient 2(a-b)/n is produced in the same pass."""

    @staticmethod
    def forward(ctx, a, b):
        _require_cuda(a, "mse input")
        ac = a if a.is_contiguous() else a.contiguous()
        bc = b if b.is_contiguous() else b.contiguous()
        n = ac.numel()
        loss = torch.empty((), device=a.device, dtype=torch.float32)
        grad = torch.empty_like(ac) if ctx.needs_input_grad[0] else None
        ws = torch.empty(lib.vq2_mse_workspace_bytes(n) // 4, device=a.device, dtype=torch.float32)
        check(lib.vq2_mse_fwd_bwd(_p(ac), _p(bc), n, n, None, _p(loss), _p(grad), _p(ws), ws.numel() * 4, _stream()),
              "mse_fwd_bwd")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (None if grad is None else _scale_by(grad, g)), None


def mse_loss(a, b):
    return MseLossFn.apply(a, b)


def stage1_loss_and_seeds(dec, diff, img, weight, denom):
    """Trainer fast path of Stage1LossFn: the loss values AND the gradients of (dec, diff) for a backward
    seed of exactly 1 (what loss.backward() means), so the pass can start with
    torch.autograd.backward((dec, diff), seeds) -- no ones_like fill, no gradient re-scaling launches.
    Returns (loss, recon, latent, d_dec, d_diff)."""
    dc, ic = dec.detach(), img.detach()
    if not (dc.is_contiguous() and ic.is_contiguous()) or diff.numel() != 1:
        raise RuntimeError("stage1_loss_and_seeds: contiguous dec/img and the [1]-shaped latent loss expected")
    n = dc.numel()
    recon = torch.empty((), device=dc.device, dtype=torch.float32)
    loss = torch.empty((), device=dc.device, dtype=torch.float32)
    grad = torch.empty_like(dc)
    latent = diff.detach().reshape(())
    ws = torch.empty(lib.vq2_mse_workspace_bytes(n) // 4, device=dc.device, dtype=torch.float32)
    check(lib.vq2_stage1_loss(_p(dc), _p(ic), n, int(denom), _p(latent), float(weight), _p(recon), _p(loss), _p(grad),
                              _p(ws), ws.numel() * 4, _stream()), "stage1_loss")
    key = (dc.device, float(weight), tuple(diff.shape))
    seed = _DIFF_SEEDS.get(key)
    if seed is None:
        seed = _DIFF_SEEDS[key] = torch.full(tuple(diff.shape), float(weight), device=dc.device, dtype=torch.float32)
    return loss, recon, latent, grad, seed


_DIFF_SEEDS = {}


class Stage1LossFn(Function):
    """loss = MSE(dec, img) + 0.25 * diff.mean()  (train_vqvae.py:83-85) -> (loss, recon, latent)."""

    @staticmethod
    def forward(ctx, dec, diff, img, weight, denom=None):
        """`denom`: number of real elements when dec/img carry zero padding (NHWC4 image layout)."""
        _require_cuda(dec, "dec")
        dc = dec if dec.is_contiguous() else dec.contiguous()
        ic = img if img.is_contiguous() else img.contiguous()
        n = dc.numel()
        denom = n if denom is None else int(denom)
        recon = torch.empty((), device=dec.device, dtype=torch.float32)
        grad = torch.empty_like(dc) if ctx.needs_input_grad[0] else None
        ws = torch.empty(lib.vq2_mse_workspace_bytes(n) // 4, device=dec.device, dtype=torch.float32)
        check(lib.vq2_mse_fwd_bwd(_p(dc), _p(ic), n, denom, None, _p(recon), _p(grad), _p(ws), ws.numel() * 4,
                                  _stream()), "mse_fwd_bwd")
        if diff.numel() != 1:
            raise RuntimeError("stage1 loss expects the [1]-shaped latent loss of VQVAE.forward")
        latent = diff.detach().reshape(())  # mean of a single element
        loss = torch.empty((), device=dec.device, dtype=torch.float32)
        check(lib.vq2_axpby(_p(recon), _p(latent.contiguous()), float(weight), _p(loss), 1, _stream()), "axpby")
        ctx.save_for_backward(grad)
        ctx.weight = weight
        ctx.diff_shape = diff.shape
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(recon, latent)
        return loss, recon, latent

    @staticmethod
    def backward(ctx, g, _gr, _gl):
        (grad,) = ctx.saved_tensors
        if g is None:
            return None, None, None, None, None
        d_dec = None if grad is None else _scale_by(grad, g)
        d_diff = _scale_by(torch.ones(ctx.diff_shape, device=g.device), g, ctx.weight) if ctx.needs_input_grad[1] else None
        return d_dec, d_diff, None, None, None
