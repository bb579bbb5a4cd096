"""Sampling from a trained PixelSNAIL prior (drop-in for the reference's sample.py: sample_model, load_model).

The reference draws pixel (i, j) from model(row[:, :i + 1])[..., i, j]: H * W forward passes over ever more rows.  Every layer
of the model is causal in raster order, so rows < i never change.  PriorSampler computes row i only:

    row-local layers     (ELU, GLU, 1x1 convs, the concatenations with the coordinate planes, the condition) run the
                         library's kernels on a dense [B, 1, W, C] row
    'causal' convs       keep their input rows in a history [H, B, W, C] and compute output row i with vq2_conv_fwd_row
    CausalAttention      keeps the projected keys and values [H, B, W, C / 2]; row i's W queries go through
                         vq2_causal_attn_fwd_rows
    the input convs      run vq2_onehot_conv_fwd on the band of code rows that ends at row i (-1 above the image: such a code
                         contributes nothing); at row 0 the shifted-down branch is left out, because the row a shift brings in
                         is 0 without the bias
    the condition        cond_resnet and the x2 upsample run once per call

Histories are row-outer so that every row slice is dense.  Effective weights (g * v / ||v|| after the 'causal' zeroing) and
their packed panels are formed once, when the sampler is built; the launches of a row are recorded once per (batch, rows) as a
list of library calls with their arguments and replayed W times, without autograd, dropout or a host synchronisation.  Step
(i, j) recomputes the whole row: columns <= j are exact, later ones are placeholders nothing reads.  The integer code map
is moved by torch copies once per row (band of row i + 1 from band of row i); everything else is a libvq2 kernel.

PriorSampler(model, stepping='pixel') computes column j only at step (i, j): the same histories, dense [B, C] column
buffers, every row-local kernel with pixels = B (into a history through the pixel stride W * C), every 'causal' conv through
vq2_conv_fwd_col, the attention with one query.

The recording is written once.  A _Recorder writes the calls of one step of row i into a _Program against a step geometry,
which states all that the two modes differ in: _RowStep (the whole row, B * W pixels per call) or _ColumnStep (column j, B
pixels).  An activation is a _View (tensor, channels, pixel stride, elements per column): a scratch buffer stays; a history,
background or condition row seen through _ColumnStep moves, and its pointer is recorded as a _Moving argument that gets j at
replay, as do the integers `col` and `q0`.  A _Plan holds the buffers and, per row, the program of a step and the program
that fills a given row from all its codes; under _RowStep the two are one program."""
import ctypes as C
import dataclasses
import os
import weakref

import torch

from . import ops
from ._lib import lib, check, AttnDesc
from .evaluate import eval_mode
from .pixelsnail import CausalConv2d, GatedResBlock, PixelSNAIL, WNConv2d, _WNLinear

VQ2_ROW_CAUSAL_TAPS = 8
_MASK64 = 0xFFFFFFFFFFFFFFFF


def _ptr(t, offset=0):
    """Device pointer `offset` elements into t."""
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


class _Moving:
    """An argument of a recorded call that moves with the column: base + j * step, a device address or an integer."""
    __slots__ = ("base", "step", "pointer")

    def __init__(self, base, step, pointer=True):
        self.base, self.step, self.pointer = base, step, pointer

    def at(self, j):
        v = self.base + j * self.step
        return C.c_void_p(v) if self.pointer else v


class _Program:
    """Library calls recorded with their arguments; run(j) replays them in order with the _Moving arguments taken at column j.
    calls holds (fn, args, what, ((index, _Moving), ...)); a call without a moving argument is replayed as it was recorded."""

    def __init__(self):
        self.calls = []

    def add(self, what, fn, *args):
        for a in args:
            if type(a) is _Moving:
                args = list(args)       # run() patches these places
                moving = tuple((k, a) for k, a in enumerate(args) if type(a) is _Moving)
                break
        else:
            moving = ()
        self.calls.append((fn, args, what, moving))

    def run(self, j=0):
        for fn, args, what, moving in self.calls:
            for k, a in moving:
                args[k] = a.at(j)
            rc = fn(*args)
            if rc:
                check(rc, what)


class _View:
    """An activation as the recording passes it around: float32 tensor `t` (which keeps the memory and gives the base address),
    `c` stored channels per pixel, pixels `ld` elements apart; it moves by `step` elements per column (0: it stays)."""
    __slots__ = ("t", "c", "ld", "step")

    def __init__(self, t, c, ld, step=0):
        self.t, self.c, self.ld, self.step = t, c, ld, step

    def ptr(self, offset=0):
        a = self.t.data_ptr() + 4 * offset
        return _Moving(a, 4 * self.step) if self.step else C.c_void_p(a)


class _RowStep:
    """Step (i, j) computes the whole of row i: a row-local call covers B * W pixels."""
    prefix = ""                          # name space of the scratch buffers [B, 1, w, c]

    def __init__(self, batch, width):
        self.W, self.w, self.pixels = width, width, batch * width          # w: the pixels of one image in a step
        self.workspace_query = lib.vq2_conv_fwd_row_workspace_bytes

    def row(self, t):
        """A row [B, W, C] of a history, the background or the condition: all of it."""
        return _View(t, t.shape[2], t.shape[2])

    def band_row(self, t):
        """A row [B, W, c] out of the band [B, R, W, c], image by image (ld is the image stride): runs of W * c."""
        return _View(t, self.W * t.shape[2], t.stride(0))

    def column(self, j):
        """The pixel of a scratch buffer at which column j stands."""
        return j

    def conv_rows(self, conv, row):
        """The call of a conv over several rows and the arguments that say where."""
        return "conv_fwd_row", lib.vq2_conv_fwd_row, (row,)

    def queries(self, row):
        return row * self.W, self.W      # q0, nq


class _ColumnStep:
    """Step (i, j) computes column j of row i: a row-local call covers B pixels, and what is read from or written into a row
    is its column 0, moving by the row's channels per column."""
    prefix = "px."

    def __init__(self, batch, width):
        self.W, self.w, self.pixels = width, 1, batch
        self.workspace_query = lib.vq2_conv_fwd_col_workspace_bytes

    def row(self, t):
        return _View(t, t.shape[2], self.W * t.shape[2], t.shape[2])

    def band_row(self, t):
        return _View(t, t.shape[2], t.stride(0), t.shape[2])

    def column(self, j):
        return 0

    def conv_rows(self, conv, row):
        assert conv.row_flags == VQ2_ROW_CAUSAL_TAPS        # row `row` holds columns <= j only
        return "conv_fwd_col", lib.vq2_conv_fwd_col, (row, _Moving(0, 1, pointer=False))

    def queries(self, row):
        return _Moving(row * self.W, 1, pointer=False), 1


_STEPS = {'row': _RowStep, 'pixel': _ColumnStep}


class _Conv:
    """One weight-normed conv with its effective weight, formed and packed once."""

    def __init__(self, mod, pack=True):
        causal_cols = None
        if isinstance(mod, CausalConv2d):
            if mod.padding == 'causal':
                causal_cols = mod.causal
            mod = mod.conv
        if isinstance(mod, WNConv2d):
            if mod.elu:
                raise NotImplementedError("vqvae2_amd.PriorSampler: a WNConv2d with an activation of its own")
            par, self.spec = mod.conv, mod.spec
        elif isinstance(mod, _WNLinear):
            par, self.spec = mod, mod.spec
        else:
            raise NotImplementedError(f"vqvae2_amd.PriorSampler: cannot step through {type(mod).__name__}")
        if self.spec.bf16 or self.spec.bf16_wgrad:   # the row kernels are fp32: the sampler's copy of a spec drops the bf16 permissions
            self.spec = dataclasses.replace(self.spec, bf16=False, bf16_wgrad=False)
        s = self.spec
        v = par.weight_v.detach().clone().contiguous()
        if causal_cols is not None:
            v[:, :, -1, causal_cols:] = 0
        g = par.weight_g.detach().contiguous()
        w = torch.empty_like(v)
        check(lib.vq2_weight_norm_fwd(ops._p(v), ops._p(g), ops._p(w), s.cout, v.numel() // s.cout, ops._stream()), "weight_norm_fwd")
        self.kh, self.kw = s.k, s.kw
        self.weight = w.view(s.cout, s.cin, self.kh, self.kw)
        self.bias = None if par.bias is None else par.bias.detach()
        self.row_flags = VQ2_ROW_CAUSAL_TAPS if causal_cols is not None else 0
        if self.kh > 1 and not (s.same_size and s.pad_top == self.kh - 1):
            raise NotImplementedError("vqvae2_amd.PriorSampler: a conv over several rows must end at its output row")
        self.wp = ops.packed_weight(s, self.weight, ops.PACK_FWD) if pack else None
        self.hist = None

    def row_desc(self, batch, rows, width):
        return ops._desc(self.spec, batch, rows, width, self.spec.ci, self.spec.co)

    def workspace_bytes(self, batch, rows, width, query):
        if self.kh == 1:
            return 0
        return query(C.byref(self.row_desc(batch, rows, width)), self.row_flags)


class _Recorder:
    """Records the library calls of one step of row `row` under the step geometry `geo`: prog is the program, logits the view
    in which a step leaves its logits."""

    def __init__(self, plan, geo, row):
        self.plan, self.geo, self.row, self.prog = plan, geo, row, _Program()
        self.s, self.B, self.H, self.W, self.R, self.stream = plan.s, plan.B, plan.H, plan.W, plan.R, plan.stream
        cond = None if plan.cond_rows is None else geo.row(plan.cond_rows[row])
        self.logits = self.body(self.input_stage(), geo.row(plan.bg_rows[row]), cond)

    def buf(self, name, c):
        """A scratch buffer of this geometry: dense, and it stays."""
        return _View(self.plan.tensor(self.geo.prefix + name, (self.B, 1, self.geo.w, c)), c, c)

    def hist(self, name, c):
        return self.plan.tensor(name, (self.H, self.B, self.W, c))

    def hist_row(self, hist):
        """Where this step writes its part of a history [H, B, W, C]."""
        return self.geo.row(hist[self.row])

    def add(self, what, fn, *args):
        self.prog.add(what, fn, *args, self.stream)

    def body(self, x, bg, cond):
        """Everything after the input stage; returns the logits buffer."""
        s, m = self.s, self.s.model
        for bi, block in enumerate(m.blocks):
            x = self.pixel_block(f"b{bi}", block, x, bg, cond)
        n_out = len(m.out) - 2
        for k in range(n_out):
            x = self.gated(f"o{k}", m.out[k], x)
        e = self.buf("head.elu", m.channel)
        self.elu(x, m.channel, e)
        logits = self.buf("head.logits", ops.ceil4(m.n_class))
        self.conv(s.conv_of[m.out[n_out + 1]], e, None, logits)
        return logits

    def elu(self, x, c, out):
        self.add("elu_fwd", lib.vq2_elu_fwd, x.ptr(), x.ld, out.ptr(), out.ld, self.geo.pixels, c)

    def copy(self, src, dst, dst_off):
        self.add("slice_copy", lib.vq2_slice_copy, src.ptr(), src.ld, dst.ptr(dst_off), dst.ld, self.geo.pixels, src.c, 0)

    def conv_input(self, name, conv):
        """Where the input of `conv` is to be written: its history's row, or a plain scratch buffer."""
        if conv.kh > 1:
            return self.hist_row(self.hist(name + ".hist", conv.spec.ci))
        return self.buf(name + ".in", conv.spec.ci)

    def conv(self, conv, x, residual, out, name=None):
        sp = conv.spec
        res, ldres = (residual.ptr(), residual.ld) if residual is not None else (None, 0)
        if conv.kh == 1:
            d = ops._desc(sp, self.B, 1, self.geo.w, x.ld, out.ld)
            self.add("conv_fwd", lib.vq2_conv_fwd, d, 0, x.ptr(), _ptr(conv.wp), ops._p(conv.bias), res, ldres, out.ptr())
            return
        hist = self.hist(name + ".hist", sp.ci)
        want = self.hist_row(hist)          # the conv reads its history: x must be this step's part of row `row` of it
        assert (x.t.data_ptr(), x.ld, x.step) == (want.t.data_ptr(), want.ld, want.step) and (out.ld, out.step) == (sp.co, 0)
        what, fn, where = self.geo.conv_rows(conv, self.row)
        self.add(what, fn, conv.row_desc(self.B, self.H, self.W), *where, self.W * sp.ci, self.B * self.W * sp.ci, conv.row_flags,
                 _ptr(hist), _ptr(conv.wp), ops._p(conv.bias), res, ldres, out.ptr(), _ptr(self.plan.ws), self.plan.ws_bytes)

    def input_stage(self):
        cp = ops.ceil4(self.s.model.channel)
        src = self.geo.band_row(self.input_band()[:, self.R - 1])      # the band's last row of every image, B runs
        x = self.buf("in.x", cp)
        self.add("slice_copy", lib.vq2_slice_copy, src.ptr(), src.ld, x.ptr(), src.c, self.B, src.c, 0)
        return x

    def input_band(self):
        """The two one-hot convs over the band of code rows that ends at this row: [B, R, W, cp], the last row is the row's."""
        s, m, i = self.s, self.s.model, self.row
        cp = ops.ceil4(m.channel)
        band = self.plan.bands[i]
        acc = None
        if i > 0:       # at row 0 the shift brings in a row of zeros (no bias); the band would give the bias
            acc = self.plan.tensor("in.h", (self.B, self.R, self.W, cp))
            sp = s.horizontal.spec
            d = ops._onehot_desc(self.B, self.R, self.W, sp.cout, sp.cin, (sp.k, sp.kw, sp.pad_top, sp.pad_left), (1, 0), cp)
            self.add("onehot_conv_fwd", lib.vq2_onehot_conv_fwd, d, _ptr(band), _ptr(s.horizontal_wp), ops._p(s.horizontal.bias),
                     None, 0, _ptr(acc))
        y = self.plan.tensor("in.v", (self.B, self.R, self.W, cp))
        sp = s.vertical.spec
        d = ops._onehot_desc(self.B, self.R, self.W, sp.cout, sp.cin, (sp.k, sp.kw, sp.pad_top, sp.pad_left), (0, 1), cp)
        self.add("onehot_conv_fwd", lib.vq2_onehot_conv_fwd, d, _ptr(band), _ptr(s.vertical_wp), ops._p(s.vertical.bias),
                 ops._p(acc), cp if acc is not None else 0, _ptr(y))
        return y

    def gated(self, name, block, x, aux=None, cond=None):
        s = self.s
        conv1, conv2 = s.conv_of[block.conv1], s.conv_of[block.conv2]
        r = None
        if aux is not None:
            ea = self.buf(name + ".ea", aux.c)
            self.elu(aux, block.auxiliary_channel, ea)
            r = self.buf(name + ".aux", conv1.spec.co)
            self.conv(s.conv_of[block.aux_conv], ea, None, r)
        e = self.conv_input(name + ".c1", conv1)
        self.elu(x, block.in_channel, e)
        h = self.buf(name + ".h", conv1.spec.co)
        self.conv(conv1, e, r, h, name + ".c1")
        e2 = self.conv_input(name + ".c2", conv2)
        self.elu(h, block.channel, e2)
        r = None
        if cond is not None:
            r = self.buf(name + ".cond", conv2.spec.co)
            self.conv(s.conv_of[block.condition], cond, None, r)
        t = self.buf(name + ".t", conv2.spec.co)
        self.conv(conv2, e2, r, t, name + ".c2")
        out = self.buf(name + ".out", ops.ceil4(block.in_channel))
        if block.n_label > 0:       # image b's pixels of a step are geo.w consecutive ones: the row's W, or the column's one
            e = s.label_embed[block]
            self.add("glu_res_label_fwd", lib.vq2_glu_res_label_fwd, t.ptr(), t.ld, x.ptr(), x.ld, _ptr(e), e.shape[1],
                     _ptr(self.plan.labels), self.B, self.geo.w, out.ptr(), out.ld, self.geo.pixels, block.in_channel, e.shape[0])
            return out
        self.add("glu_res_fwd", lib.vq2_glu_res_fwd, t.ptr(), t.ld, x.ptr(), x.ld, out.ptr(), out.ld, self.geo.pixels,
                 block.in_channel)
        return out

    def cat(self, name, parts):
        out = self.buf(name, sum(p.c for p in parts))
        off = 0
        for p in parts:
            self.copy(p, out, off)
            off += p.c
        return out

    def pixel_block(self, name, block, x, bg, cond):
        s = self.s
        out = x
        for k, rb in enumerate(block.resblocks):
            out = self.gated(f"{name}.r{k}", rb, out, cond=cond)
        if not block.attention:
            o = self.buf(name + ".o", s.conv_of[block.out].spec.co)
            self.conv(s.conv_of[block.out], self.cat(name + ".cat", [out, bg]), None, o)
            return o
        key = self.gated(name + ".key", block.key_resblock, self.cat(name + ".kcat", [x, out, bg]))
        query = self.gated(name + ".query", block.query_resblock, self.cat(name + ".qcat", [out, bg]))
        att = block.causal_attention
        ch = att.channel
        q = self.buf(name + ".q", ch)
        kh, vh = self.hist(name + ".khist", ch), self.hist(name + ".vhist", ch)
        self.conv(s.conv_of[att.query], query, None, q)
        self.conv(s.conv_of[att.key], key, None, self.hist_row(kh))
        self.conv(s.conv_of[att.value], key, None, self.hist_row(vh))
        o = self.buf(name + ".att", ch)
        d = AttnDesc()
        d.B, d.L, d.n_head, d.dim_head = self.B, self.H * self.W, att.n_head, att.dim_head
        d.ldq = d.ldk = d.ldv = d.ldo = ch
        q0, nq = self.geo.queries(self.row)
        self.add("causal_attn_fwd_rows", lib.vq2_causal_attn_fwd_rows, d, q0, nq, self.W, self.W * ch, self.B * self.W * ch,
                 q.ptr(), _ptr(kh), _ptr(vh), o.ptr())
        return self.gated(name + ".outb", block.out_resblock, out, aux=o)


class _Plan:
    """Buffers, histories and the recorded programs of every row for one (batch, rows, condition?) on one stream, under the
    step geometry `step`.  step_programs[i].run(j) is step (i, j); row_programs[i].run() fills row i when all its codes are
    given (a `prefix` row costs one run, not W).  Under _RowStep they are the same programs, and nothing of a column is
    recorded or allocated; under _ColumnStep both kinds fill the same histories."""

    def __init__(self, sampler, step, batch, rows, with_condition):
        self.s, self.B, self.H, self.W = sampler, batch, rows, sampler.width
        self.dev = sampler.device
        self.stream = ops._stream()
        self.stream_id = torch.cuda.current_stream().cuda_stream
        self.bufs = {}
        m = sampler.model
        self.step = step(batch, self.W)
        fill = self.step if step is _RowStep else _RowStep(batch, self.W)
        self.ws_bytes = max([c.workspace_bytes(batch, rows, self.W, g.workspace_query) for g in {self.step, fill} for c in sampler.convs]
                            + [16])
        self.ws = torch.empty((self.ws_bytes + 3) // 4, device=self.dev, dtype=torch.float32)
        self.R = sampler.band_rows
        # band i: code rows i - R + 1 .. i as the input convs see them at row i; -1 above the image
        self.bands = torch.empty((rows, batch, self.R, self.W), device=self.dev, dtype=torch.int64)
        # the class labels the recorded gates read (a class-conditional model): filled once per call, -1 adds nothing
        self.labels = torch.full((batch,), -1, device=self.dev, dtype=torch.int64) if m.n_label > 0 else None
        self.cond_rows = None
        if with_condition:
            self.cond_rows = torch.empty((rows, batch, self.W, ops.ceil4(m.cond_res_channel)), device=self.dev, dtype=torch.float32)
        bg = m._background(batch, rows)                                   # [B, rows, W, 4]
        self.bg_rows = torch.empty((rows, batch, self.W, 4), device=self.dev, dtype=torch.float32)
        self.to_row_outer(bg, self.bg_rows)
        recorded = [_Recorder(self, fill, i) for i in range(rows)]
        self.row_programs = self.step_programs = [r.prog for r in recorded]
        if self.step is not fill:
            recorded = [_Recorder(self, self.step, i) for i in range(rows)]
            self.step_programs = [r.prog for r in recorded]
        self.logits = recorded[-1].logits

    def logits_at(self, j):
        """Where the logits of step (i, j) stand once it has run: (pointer to image 0's, elements between images)."""
        v = self.logits
        return v.ptr(self.step.column(j) * v.c), self.step.w * v.c

    def tensor(self, name, shape):
        t = self.bufs.get(name)
        if t is None:
            t = self.bufs[name] = torch.empty(shape, device=self.dev, dtype=torch.float32)
        return t

    def to_row_outer(self, src, dst):
        """NHWC [B, >= rows, W, C] -> [rows, B, W, C]: one slice copy per row (an image's row is one run of W * C floats)."""
        b, h, w, c = src.shape
        for i in range(self.H):
            check(lib.vq2_slice_copy(_ptr(src, i * w * c), h * w * c, _ptr(dst, i * b * w * c), w * c, b, w * c, 0, self.stream),
                  "slice_copy")

    def reset_codes(self):
        self.bands.zero_()
        for r in range(self.R - 1):
            self.bands[:self.R - 1 - r, :, r].fill_(-1)

    def end_row(self, i):
        if i + 1 < self.H:
            self.bands[i + 1, :, :self.R - 1].copy_(self.bands[i, :, 1:])

    def codes(self):
        return self.bands[:, :, self.R - 1].permute(1, 0, 2).contiguous()


class PriorSampler:
    """PriorSampler(model, stepping='row'): an incremental sampler over a vqvae2_amd.PixelSNAIL on the GPU.

    stepping   'row' (the default): step (i, j) recomputes row i, M = B * W pixels per launch.  'pixel': step (i, j) computes
               column j only, M = B; every conv over several rows must then be a 'causal' one.  Both give what the model
               gives, to rounding; the draws of one seed may differ between them where a logit's last bits decide.  Anything
               else is a ValueError.

    sample(batch, temperature=1.0, condition=None, seed=None, rows=None, *, top_k=0, top_p=1.0, prefix=None,
        return_logp=False) -> int64 [B, rows, W] on the device.  condition: the
        int64 top codes [B, H / 2, W / 2] for a model built with a condition network.  seed None takes one integer from torch's
        default CPU generator (as the dropout layers do), so torch.manual_seed makes a run repeatable.  The code of pixel (i, j)
        of image b is drawn by vq2_sample_categorical at position i * W + j, row b.  Keyword only:
        top_k, top_p   draw from the top_k most likely codes (0: off; above n_class: n_class) and, of those, from the smallest
                       set of most likely codes that holds top_p of the mass (1.0: off); ties at a cut are kept.  The draw is
                       then vq2_sample_filtered (include/vq2.h has the exact rule), still one launch per step.
        prefix         int64 [B, r0, W] on the device, 0 <= r0 <= rows: the first r0 rows of the result are these codes and
                       drawing starts at (r0, 0).  A given row costs one run of its row program, not W.  Draws keep their
                       position i * W + j, so a prefix taken from sample(seed=s) is completed to that very map.
        return_logp    returns (codes, logp): logp float32 [B, rows, W], the log-probability of each drawn code under the
                       tempered, truncated distribution it was drawn from; 0 at prefix positions.
        label          for a class-conditional model (PixelSNAIL(..., n_label > 0)), which needs it: an int (every image) or
                       an int64 [B] tensor on the device.  It is written once per call into the buffer the recorded gates
                       (vq2_glu_res_label_fwd, pixels_per_image = W in row stepping, 1 in pixel stepping) read; a label
                       outside [0, n_label) adds nothing.  A model built with n_label=0 refuses it.
        With these at their defaults the calls and their arguments are what they were without them.
    logits_given(codes, condition=None, label=None) -> [B, n_class, H, W]: the same stepping with `codes` written where sample() draws;
        entry (i, j) is what step (i, j) saw, which by causality is the model's own output for those codes.
    The weights are those of the moment of construction: a model whose parameters changed since is refused until refresh().
    One set of histories and recorded launches is kept, for the last (batch, rows, condition or not, stream): a call with
    another combination frees it and builds a new one (alternating sample() and logits_given() of different sizes rebuilds
    every time).  The sampler holds device pointers: it cannot be pickled or deep-copied, and nothing of it is stored on the
    model."""

    def __init__(self, model, stepping='row', _weak=False):
        if not isinstance(model, PixelSNAIL):
            raise TypeError("vqvae2_amd.PriorSampler: a vqvae2_amd.PixelSNAIL expected")
        if stepping not in _STEPS:
            raise ValueError(f"vqvae2_amd.PriorSampler: stepping must be 'row' or 'pixel', got {stepping!r}")
        self.stepping, self.step = stepping, _STEPS[stepping]
        # _weak: sample_model's cache is keyed weakly by the model; its samplers must not keep the model alive themselves
        self._model_ref = weakref.ref(model)
        self._model = None if _weak else model
        self.refresh()

    @property
    def model(self):
        m = self._model_ref()
        if m is None:
            raise RuntimeError("vqvae2_amd.PriorSampler: the model is gone")
        return m

    def refresh(self):
        m = self.model
        par = next(m.parameters())
        ops._require_cuda(par, "the model's parameters")
        self.device = par.device
        self.width = m.background.shape[3]
        with torch.no_grad():
            self.conv_of = {}
            self.label_embed = {mod: mod.label_embed.detach().clone().contiguous() for mod in self._gated_blocks()
                                if mod.n_label > 0}
            for mod in self._gated_blocks():
                names = ["conv1", "conv2"] + (["aux_conv"] if mod.auxiliary_channel > 0 else []) + \
                        (["condition"] if mod.condition_dim > 0 else [])
                for n in names:
                    self.conv_of[getattr(mod, n)] = _Conv(getattr(mod, n))
            for block in m.blocks:
                if block.attention:
                    for lin in (block.causal_attention.query, block.causal_attention.key, block.causal_attention.value):
                        self.conv_of[lin] = _Conv(lin)
                else:
                    self.conv_of[block.out] = _Conv(block.out)
            self.conv_of[m.out[-1]] = _Conv(m.out[-1])
            self.convs = list(self.conv_of.values())
            if self.stepping == 'pixel':
                for c in self.convs:
                    if (c.kh > 1 and not c.row_flags) or (c.kh == 1 and c.kw > 1):
                        raise NotImplementedError("vqvae2_amd.PriorSampler: pixel stepping takes 1 x 1 and 'causal' convs only")
            self.horizontal, self.vertical = _Conv(m.horizontal, pack=False), _Conv(m.vertical, pack=False)
            self.horizontal_wp, self.vertical_wp = self._onehot_panel(self.horizontal), self._onehot_panel(self.vertical)
        self.band_rows = max(self.horizontal.kh + 1, self.vertical.kh)
        self._versions = self._snapshot()
        self._plan = None

    def _gated_blocks(self):
        """The gated blocks the stepping runs (cond_resnet's run through the module itself, once per call)."""
        for block in self.model.blocks:
            yield from block.resblocks
            if block.attention:
                yield from (block.key_resblock, block.query_resblock, block.out_resblock)
        yield from list(self.model.out)[:-2]

    def _onehot_panel(self, conv):
        cout, n_class, kh, kw = conv.weight.shape
        wp = torch.empty(kh * kw * n_class * ops.ceil4(cout), device=self.device, dtype=torch.float32)
        check(lib.vq2_onehot_pack_weight(ops._p(conv.weight), ops._p(wp), cout, n_class, kh, kw, ops._stream()), "onehot_pack_weight")
        return wp

    def _snapshot(self):
        return [(p.data_ptr(), p._version, ops.weight_epoch(p)) for p in self.model.parameters()]

    def _plan_for(self, batch, rows, condition, label=None):
        if self._snapshot() != self._versions:
            raise RuntimeError("vqvae2_amd.PriorSampler: the model's parameters changed since the sampler was built; call refresh()")
        m = self.model
        if not 1 <= rows <= m.background.shape[2]:
            raise RuntimeError(f"PriorSampler: {rows} rows do not fit the model's {m.background.shape[2]}")
        key = (batch, rows, condition is not None, torch.cuda.current_stream().cuda_stream)
        if self._plan is None or self._plan[0] != key:
            self._plan = None       # free the old histories before the new ones are allocated
            self._plan = (key, _Plan(self, self.step, batch, rows, condition is not None))
        plan = self._plan[1]
        if condition is not None:
            if not hasattr(m, "cond_resnet"):
                raise RuntimeError("PriorSampler: condition given to a model built without a condition network")
            condition = ops._require_codes(condition, "condition")
            if condition.dim() != 3 or condition.shape[0] != batch or 2 * condition.shape[1] < rows or 2 * condition.shape[2] != self.width:
                raise RuntimeError("PriorSampler: condition [B, H / 2, W / 2] of int64 codes expected")
            with eval_mode(m.cond_resnet):
                cond = ops.Upsample2Fn.apply(m.cond_resnet.nhwc(condition), m.cond_res_channel)
            plan.to_row_outer(cond, plan.cond_rows)
        if (label is not None) != (m.n_label > 0):
            raise RuntimeError(f"PriorSampler: a model built with n_label={m.n_label} needs `label`" if label is None else
                               "PriorSampler: label given to a model built with n_label=0")
        if label is not None:
            if isinstance(label, int):
                plan.labels.fill_(label)
            else:
                plan.labels.copy_(ops.require_labels(label, batch, self.device))
        plan.reset_codes()
        return plan

    @torch.no_grad()
    def sample(self, batch, temperature=1.0, condition=None, seed=None, rows=None, *, top_k=0, top_p=1.0, prefix=None,
               return_logp=False, label=None):
        rows = self.model.background.shape[2] if rows is None else int(rows)
        if not temperature > 0:
            raise ValueError(f"PriorSampler: temperature must be positive, got {temperature}")
        n_class = self.model.n_class
        if int(top_k) != top_k or top_k < 0:
            raise ValueError(f"PriorSampler: top_k must be 0 (off) or a positive integer, got {top_k}")
        if not 0 < top_p <= 1:
            raise ValueError(f"PriorSampler: top_p must be in (0, 1], got {top_p}")
        top_k, top_p = min(int(top_k), n_class), float(top_p)
        batch = int(batch)
        r0 = 0
        if prefix is not None:
            prefix = ops._require_codes(prefix, "prefix")
            if prefix.device != self.device or prefix.dim() != 3 or prefix.shape[0] != batch or prefix.shape[2] != self.width \
                    or prefix.shape[1] > rows:
                raise RuntimeError(f"PriorSampler: prefix [B, r0 <= rows, W] = [{batch}, <= {rows}, {self.width}] of int64 codes on "
                                   f"{self.device} expected, got {tuple(prefix.shape)} on {prefix.device}")
            r0 = prefix.shape[1]
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        seed = int(seed) & _MASK64
        plan = self._plan_for(batch, rows, condition, label)
        b, w, r = plan.B, plan.W, plan.R
        t = float(temperature)
        filtered = top_k > 0 or top_p < 1.0 or return_logp
        # step-outer [rows, W, B]: the draw of step (i, j) writes its B values densely
        logp = torch.zeros((rows, w, b), device=self.device, dtype=torch.float32) if return_logp else None
        for i in range(rows):
            band = plan.bands[i]
            if i < r0:
                # a given row: with all its codes in place one run of the row's program is exact in every column
                band[:, r - 1].copy_(prefix[:, i])
                plan.row_programs[i].run()
                plan.end_row(i)
                continue
            prog = plan.step_programs[i]
            for j in range(w):
                prog.run(j)
                logits, lrow = plan.logits_at(j)
                if filtered:
                    check(lib.vq2_sample_filtered(logits, lrow, b, n_class, t, top_k, top_p, seed, i * w + j,
                                                  _ptr(band, (r - 1) * w + j), r * w,
                                                  _ptr(logp, (i * w + j) * b) if return_logp else None, None, plan.stream),
                          "sample_filtered")
                else:
                    check(lib.vq2_sample_categorical(logits, lrow, b, n_class, t, seed, i * w + j,
                                                     _ptr(band, (r - 1) * w + j), r * w, plan.stream), "sample_categorical")
            plan.end_row(i)
        if return_logp:
            return plan.codes(), logp.permute(2, 0, 1).contiguous()
        return plan.codes()

    @torch.no_grad()
    def logits_given(self, codes, condition=None, label=None):
        codes = ops._require_codes(codes, "codes")
        if codes.dim() != 3 or codes.shape[2] != self.width:
            raise RuntimeError("PriorSampler: codes [B, H, W] of int64 expected")
        batch, rows, w = codes.shape
        plan = self._plan_for(batch, rows, condition, label)
        ld = ops.ceil4(self.model.n_class)
        out = torch.zeros((batch, rows, w, ld), device=self.device, dtype=torch.float32)
        for i in range(rows):
            prog = plan.step_programs[i]
            for j in range(w):
                prog.run(j)
                logits, lrow = plan.logits_at(j)
                check(lib.vq2_slice_copy(logits, lrow, _ptr(out, (i * w + j) * ld), rows * w * ld, batch, ld, 0, plan.stream),
                      "slice_copy")
                plan.bands[i, :, plan.R - 1, j] = codes[:, i, j]
            plan.end_row(i)
        return ops.from_nhwc(out, self.model.n_class)


_SAMPLERS = weakref.WeakKeyDictionary()      # model -> {stepping: its PriorSampler, which refers to the model weakly}


def sample_model(model, device, batch, size, temperature, condition=None, *, top_k=0, top_p=1.0, prefix=None, stepping='row',
                 label=None):
    """The reference's sample_model (sample.py:12-24): int64 codes [batch, size[0], size[1]] on `device`, drawn from `model`
    pixel by pixel in raster order.  One PriorSampler per model and stepping is kept in this module, keyed weakly by the model
    (it goes when the model goes, and the model itself carries nothing: it still pickles and deep-copies), and is rebuilt when
    the model's parameters change.  top_k, top_p and prefix (keyword only, not in the reference) are PriorSampler.sample's;
    stepping ('row' or 'pixel') is PriorSampler's, and so is label (a class-conditional model's class: an int or int64 [B])."""
    if stepping not in _STEPS:
        raise ValueError(f"sample_model: stepping must be 'row' or 'pixel', got {stepping!r}")
    if tuple(size)[1] != model.background.shape[3]:
        raise RuntimeError(f"sample_model: width {size[1]} does not fit the model's {model.background.shape[3]}")
    model = model.to(device)
    cache = _SAMPLERS.setdefault(model, {})
    sampler = cache.get(stepping)
    if sampler is None or sampler._snapshot() != sampler._versions:
        sampler = cache[stepping] = PriorSampler(model, stepping, _weak=True)
    return sampler.sample(batch, temperature, condition, rows=int(size[0]), top_k=top_k, top_p=top_p, prefix=prefix, label=label)


def _arg(args, name, default):
    if isinstance(args, dict):
        return args.get(name, default)
    return getattr(args, name, default)


def load_model(model, checkpoint, device, ckpt_dir='checkpoint', **overrides):
    """The reference's load_model (sample.py:27-68): model is 'vqvae', 'pixelsnail_top' or 'pixelsnail_bottom', `checkpoint`
    a file under `ckpt_dir`.  Constructor arguments come from ckpt['args'] where the checkpoint has them (what
    examples/train_pixelsnail.py saves, including its extras size / n_class / n_block / kernel_size / n_label), then from `overrides`.
    Returns the model on `device` in eval mode."""
    from .vqvae import VQVAE
    ckpt = torch.load(os.path.join(ckpt_dir, checkpoint), map_location='cpu', weights_only=False)
    args = ckpt.get('args', {}) if isinstance(ckpt, dict) else {}

    def get(name, default):
        return overrides.get(name, _arg(args, name, default))

    if model == 'vqvae':
        keys = ('in_channel', 'channel', 'n_res_block', 'n_res_channel', 'embed_dim', 'n_embed', 'decay')
        net = VQVAE(**{k: get(k, None) for k in keys if get(k, None) is not None})
    elif model in ('pixelsnail_top', 'pixelsnail_bottom'):
        h, w = get('size', [32, 32])
        n_class, kernel, n_block = get('n_class', 512), get('kernel_size', 5), get('n_block', 4)
        n_label = get('n_label', 0) or 0
        if model == 'pixelsnail_top':
            net = PixelSNAIL([h, w], n_class, get('channel', 256), kernel, n_block, get('n_res_block', 4), get('n_res_channel', 256),
                             dropout=get('dropout', 0.1), n_out_res_block=get('n_out_res_block', 0), n_label=n_label)
        else:
            net = PixelSNAIL([2 * h, 2 * w], n_class, get('channel', 256), kernel, n_block, get('n_res_block', 4),
                             get('n_res_channel', 256), attention=False, dropout=get('dropout', 0.1),
                             n_cond_res_block=get('n_cond_res_block', 3), cond_res_channel=get('n_res_channel', 256),
                             n_label=n_label)
    else:
        raise ValueError(f"load_model: model must be 'vqvae', 'pixelsnail_top' or 'pixelsnail_bottom', got {model!r}")
    if isinstance(ckpt, dict) and 'model' in ckpt:
        ckpt = ckpt['model']
    net.load_state_dict(ckpt)
    return net.to(device).eval()
