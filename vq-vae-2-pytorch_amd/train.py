"""The canonical stage-1 step of /root/reference/train_vqvae.py:83-91 (+166-171, 185-206) as an
object: forward, MSE + 0.25*latent, backward, packed all-reduces (gradients + the EMA sums of both
quantizers) over RCCL on a side stream, deferred EMA update, one-launch Adam, optional CycleScheduler,
and a checkpoint that resumes the run exactly (model in the reference's format + optimizer + schedule).
"""
import os

import torch
from torch import distributed as dist

from . import distributed as dist_fn
from . import ops
from .optim import CycleScheduler, FusedAdam, ParamArena

LATENT_LOSS_WEIGHT = 0.25  # train_vqvae.py:34


def stage1_loss(dec, diff, img, latent_loss_weight=LATENT_LOSS_WEIGHT):
    """(loss, recon_loss, latent_loss) = MSE(dec,img) + w * diff.mean()  (train_vqvae.py:83-85)."""
    return ops.Stage1LossFn.apply(dec, diff, img, latent_loss_weight)


class Stage1Trainer:
    """Replaces `DistributedDataParallel(model)` + `optim.Adam` + the loop body of train_vqvae.py:83-91.

    Data parallelism (one process per GPU): like DDP's constructor (train_vqvae.py:166-171) the trainer first
    broadcasts rank 0's parameters and buffers, so replicas built from different RNG states start identical; every
    step then SUM-all-reduces the flat gradient buffer (Adam divides by the world size) in two buckets.
    VQ2_DP_FORCE=1 takes this path whenever a process group exists, also at world size 1.

    normalizer: a data.ImageNormalizer; step() then also takes uint8 image batches on the device (the loader's
    ToTensor + Normalize + CenterCrop run as one kernel inside the step, train_vqvae.py:149-155)."""

    def __init__(self, model, lr=3e-4, sched=None, n_iter=None, betas=(0.9, 0.999), eps=1e-8, normalizer=None):
        self.model = model
        self.normalizer = normalizer
        live = model.live_parameters() if hasattr(model, "live_parameters") else list(model.parameters())
        self.quantizers = [m for m in model.modules() if type(m).__name__ == "Quantize"]
        extra = sum(ops.vq_stats_numel(q.n_embed, q.dim) for q in self.quantizers)
        # enc_b back-propagates LAST: its parameters go to the end of the arena, so that the gradient buffer reads
        # [EMA statistics | enc_t quantize_conv_t dec_t | quantize_conv_b upsample_t dec | enc_b] and each of the three
        # data-parallel buckets (below) is one contiguous slice
        enc_b = getattr(model, "enc_b", None)
        self.arena = ParamArena(live, extra=extra, last=list(enc_b.parameters()) if enc_b is not None else ())
        off = 0
        for q in self.quantizers:  # EMA statistics ride in the head of the gradient buffer
            n = ops.vq_stats_numel(q.n_embed, q.dim)   # a multiple of 4: every quantizer's slice stays 16-byte aligned
            q.deferred_stats = self.arena.extra[off:off + n]
            off += n
        self.optimizer = FusedAdam(live, lr=lr, betas=betas, eps=eps, arena=self.arena)
        self.scheduler = None
        if sched == "cycle":  # train_vqvae.py:188-195
            self.scheduler = CycleScheduler(self.optimizer, lr, n_iter=n_iter, momentum=None, warmup_proportion=0.05)
        # Stream priorities: the step's main chain should win every CU slot it can use, the side streams (small weight
        # gradients, EMA statistics, early slab reduction, collectives) only what it leaves idle -- mostly the tails of
        # its launches.  HIP knows two levels (0 and -1 = high), so the trainer installs a HIGH-priority stream as this
        # thread's current stream, once (ordered after the work already queued on the previous one), and creates its
        # side streams at the default priority: 6.78 -> 6.74 ms per step.  VQ2_MAIN_PRIO=0 leaves the current stream alone.
        if os.environ.get("VQ2_MAIN_PRIO", "1") != "0" and torch.cuda.current_stream().priority == 0:
            hp = torch.cuda.Stream(priority=-1)
            hp.wait_stream(torch.cuda.current_stream())
            torch.cuda.set_stream(hp)
        # this trainer's backward-pass state hangs on ITS parameters (no process-global state)
        wgrad_stream = torch.cuda.Stream()
        self.ctx = ops.StepContext(wgrad_stream)
        for p in self.arena.params:
            p._vq2_ctx = self.ctx
        for q in self.quantizers:      # the EMA statistics are consumed after backward: off the main stream
            q.stats_stream = wgrad_stream
        # every weight panel (forward and data-gradient layouts) re-packed by one launch per step
        layers = []
        for name, mod in model.named_modules():
            if hasattr(mod, "spec") and hasattr(mod, "weight") and not name.startswith("dec_ir"):
                layers.append((mod.spec, mod.weight, name != "enc_b.blocks.0"))
        self.pack_plan = ops.PackPlan(layers)

        self.world = dist_fn.get_world_size()
        forced = os.environ.get("VQ2_DP_FORCE", "0") != "0" and dist.is_available() and dist.is_initialized()
        self.dp = self.world > 1 or forced
        self.optimizer.grad_scale = 1.0 / self.world  # DDP averages gradients (train_vqvae.py:166-171)
        self.comm_stream = torch.cuda.Stream() if self.dp else None
        self.comm = dist_fn.data_comm() if self.dp else None   # torch.distributed group or libvq2's own communicator
        if self.dp:
            self._sync_initial_state()
        self.pack_plan.run()
        # Overlap (train_vqvae.py:166-171 is DDP's bucketed all-reduce; vqvae.py:58-59 the EMA sums).  The backward pass
        # produces gradients in the order dec, upsample_t, quantize_conv_b | dec_t, quantize_conv_t, enc_t | enc_b, so
        # the gradient buffer goes out in THREE contiguous slices, each all-reduced on the communication stream while
        # the next group is still back-propagating:
        #   tail    [quantize_conv_b upsample_t dec]             when quantize_conv_b's gradient lands   (~60 %)
        #   middle  [EMA statistics | enc_t quantize_conv_t dec_t] when enc_t's first conv's gradient lands
        #   head    [enc_b]                                       after backward: the only exposed part (~1.4 MB)
        # A bucket goes out early only if every parameter of its slice already owns its gradient slot (autograd happens
        # to order the graph this way; nothing else guarantees it) -- whatever was not sent early is sent after backward.
        self.early_buckets = 0      # buckets that went out from a backward hook (all steps)
        self.bucket_bytes = {}      # name -> bytes of the slice (bench line)
        self._sent = []             # [lo, hi) slices of flat_g already handed to the communicator in this step
        self._hooks_seen = {}
        self.buckets = []           # (name, lo, hi, params of the slice)
        split = getattr(model, "quantize_conv_b", None)
        enc_t = getattr(model, "enc_t", None)
        if split is not None and enc_b is not None and enc_t is not None:
            a = self.arena
            off = lambda p: a.n_extra + a.offset[id(p)]
            lo_tail = off(split.weight)
            lo_head = min(off(p) for p in enc_b.parameters())
            total = a.flat_g.numel()
            inside = lambda lo, hi: [p for p in a.params if lo <= off(p) < hi]
            self.buckets = [("tail", lo_tail, lo_head, inside(lo_tail, lo_head)),
                            ("middle", 0, lo_tail, inside(0, lo_tail)),
                            ("head", lo_head, total, inside(lo_head, total))]
            self.bucket_bytes = {name: 4 * (hi - lo) for name, lo, hi, _ in self.buckets}
            for prm in (split.weight, split.bias):
                prm.register_post_accumulate_grad_hook(lambda _p: self._group_done("tail", 2))
            if self.dp:     # (single GPU: one early slab reduction is enough, a second one only adds a launch)
                first = enc_t.blocks[0]
                for prm in (first.weight, first.bias):
                    prm.register_post_accumulate_grad_hook(lambda _p: self._group_done("middle", 2))

    # ------------------------------------------------------------------ data parallel plumbing
    def _sync_initial_state(self):
        """What DistributedDataParallel's constructor does (train_vqvae.py:166-171): rank 0's parameters and
        buffers everywhere.  One broadcast for the whole arena, one per tensor outside it (dead dec_ir, codebooks)."""
        with torch.no_grad():
            self.comm.broadcast(self.arena.flat_p, 0)
            inside = {id(p) for p in self.arena.params}
            for t in list(self.model.parameters()) + list(self.model.buffers()):
                if id(t) not in inside:
                    self.comm.broadcast(t.detach(), 0)     # (detach() shares the version counter; .data does not)
        ops.touch_weights(self.arena.params)
        # the codebooks were just overwritten (NativeComm writes through raw pointers, which no version counter sees):
        # anything a Quantize derived from its OLD codebook is stale now
        for q in self.quantizers:
            q.invalidate_prepared()

    def _group_done(self, name, need):
        """Post-accumulate hook of the LAST layer of a backward group: reduce the split-K slabs produced so far into the
        arena (side stream) and, data parallel, hand the group's slice to the communicator while the next group
        back-propagates."""
        seen = self._hooks_seen[name] = self._hooks_seen.get(name, 0) + 1
        if seen != need:
            return
        _, lo, hi, params = next(b for b in self.buckets if b[0] == name)
        if not all(p.grad is not None and p.grad.data_ptr() == p._vq2_grad.data_ptr() for p in params):
            return      # autograd ordered the graph differently: keep the slice for the collective after backward
        side = self.ctx.stream
        side.wait_event(torch.cuda.current_stream().record_event())
        with torch.cuda.stream(side):
            self.ctx.batch.flush()
            ev = side.record_event()
        if not self.dp:
            return
        with torch.cuda.stream(self.comm_stream):
            self.comm_stream.wait_event(ev)
            self.comm.all_reduce(self.arena.flat_g[lo:hi])
        self._sent.append((lo, hi))
        self.early_buckets += 1

    def _unsent_slices(self):
        """Complement of the slices already sent, as maximal contiguous [lo, hi) ranges of flat_g."""
        out, pos = [], 0
        for lo, hi in sorted(self._sent):
            if lo > pos:
                out.append((pos, lo))
            pos = max(pos, hi)
        if pos < self.arena.flat_g.numel():
            out.append((pos, self.arena.flat_g.numel()))
        return out

    # ------------------------------------------------------------------ the step
    def step(self, img, return_dec=False):
        """One training step on this rank's batch (img: float32 NCHW, or a uint8 batch in the normalizer's layout);
        returns device scalars (no host sync)."""
        model = self.model
        u8 = getattr(img, "dtype", None) == torch.uint8
        if u8 and self.normalizer is None:
            raise TypeError("Stage1Trainer.step: a uint8 batch needs Stage1Trainer(..., normalizer=ImageNormalizer(...))")
        model.train()
        # the EMA statistics slots are fully rewritten by vq2_vq_stats, and their pad floats (ops.vq_stats_views) were
        # zeroed with the arena and are never written: nothing to zero
        self.arena.zero_grad()
        if u8 and hasattr(model, "forward_nhwc"):
            # the same step from 8-bit pixels: x comes normalised out of the conversion launch; the MSE denominator and
            # the channel count are those of the logical (cropped) NCHW image
            x = self.normalizer(img)
            n, channels, h, w = self.normalizer.out_shape(img)
            dec, diff = model.forward_nhwc(x)
            loss, recon, latent, d_dec, d_diff = ops.stage1_loss_and_seeds(dec, diff, x, LATENT_LOSS_WEIGHT, n * channels * h * w)
            roots, seeds = (dec, diff), (d_dec, d_diff)
        elif hasattr(model, "forward_nhwc"):
            # loss evaluated in the kernels' own NHWC4 layout: no layout conversion of the
            # reconstruction or of its gradient (the zero pad lane contributes nothing)
            x = ops.to_nhwc(img)
            channels = img.shape[1]
            dec, diff = model.forward_nhwc(x)
            loss, recon, latent, d_dec, d_diff = ops.stage1_loss_and_seeds(dec, diff, x, LATENT_LOSS_WEIGHT, img.numel())
            roots, seeds = (dec, diff), (d_dec, d_diff)
        else:
            if u8:
                img = self.normalizer.nchw(img)
            dec, diff = model(img)
            loss, recon, latent = stage1_loss(dec, diff, img)
            roots, seeds = (loss,), (None,)
        self._sent, self._hooks_seen = [], {}
        self.ctx.active = True
        try:
            torch.autograd.backward(roots, seeds)
        finally:
            self.ctx.active = False
        torch.cuda.current_stream().wait_stream(self.ctx.stream)   # all slabs written
        self.ctx.batch.flush()   # one launch reduces the split-K slabs of every layer into the arena
        if self.dp:
            if not self.arena.grads_ready():
                raise RuntimeError("Stage1Trainer: a gradient did not land in the flat arena")
            # gradients (SUM; Adam divides by world) and EMA sums (SUM, vqvae.py:58-59) in one collective,
            # issued on a side stream so the host can already enqueue the next step's input work
            ev = torch.cuda.current_stream().record_event()
            with torch.cuda.stream(self.comm_stream):
                self.comm_stream.wait_event(ev)
                for lo, hi in self._unsent_slices():     # normally just enc_b's slice; everything if no hook fired
                    self.comm.all_reduce(self.arena.flat_g[lo:hi])
            torch.cuda.current_stream().wait_stream(self.comm_stream)
        for q in self.quantizers:
            q.apply_deferred_update()
        if self.scheduler is not None:
            self.scheduler.step()
        self.optimizer.step()
        self.pack_plan.run()
        out = {"loss": loss.detach(), "recon": recon, "latent": latent}
        if return_dec:
            d = dec.detach()
            out["dec"] = ops.from_nhwc(d, channels) if hasattr(model, "forward_nhwc") else d
        return out

    # ------------------------------------------------------------------ held-out evaluation
    def evaluate(self, batches, sample=None):
        """Evaluator.result() over an iterable of batches (float32 NCHW, or uint8 with the trainer's normalizer), between
        two steps: eval-mode forwards under no_grad that write no EMA statistics slot, no codebook buffer and no
        parameter, so the steps that follow are bit for bit those of a run that never evaluated; every module's
        train / eval flag is restored.  Data parallel: every rank calls it (result() sums over the group).  sample: a
        batch (same forms) whose grid (sample_grid) is returned under "sample"."""
        return self._evaluate(batches, sample, False)

    def evaluate_image_metrics(self, batches, sample=None):
        """evaluate() with Evaluator(image_metrics=True): the result also holds "psnr", "ssim" and "mse_u8" of the 8-bit
        reconstructions.  Needs the trainer's normalizer; leaves trainer and model alone as evaluate() does."""
        return self._evaluate(batches, sample, True)

    def _evaluate(self, batches, sample, image_metrics):
        from .evaluate import Evaluator
        ev = Evaluator(self.model, self.normalizer, image_metrics=image_metrics)
        for img in batches:
            ev.update(img)
        out = ev.result()
        if sample is not None:
            out["sample"] = self.sample_grid(sample)
        return out

    def sample_grid(self, sample):
        """The reference's sample image (train_vqvae.py:133-139) as one uint8 canvas on the device: the inputs on the top
        row, their eval-mode reconstructions below (nrow = len(sample)), in the normalizer's layout.  No collective:
        one rank may call it alone.  Leaves trainer and model as evaluate() does."""
        if self.normalizer is None:
            raise TypeError("Stage1Trainer.sample_grid needs Stage1Trainer(..., normalizer=ImageNormalizer(...)): its "
                            "statistics are the ones the grid inverts")
        from .evaluate import eval_mode
        model = self.model
        if not hasattr(model, "forward_nhwc"):
            raise TypeError(f"Stage1Trainer.sample_grid: {type(model).__name__} has no forward_nhwc")
        with torch.no_grad():
            x = self.normalizer(sample) if sample.dtype == torch.uint8 else ops.to_nhwc(sample)
            with eval_mode(model):
                dec, _ = model.forward_nhwc(x)
            return self.normalizer.inverse().grid([x, dec], nrow=x.shape[0], nhwc=True)

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self):
        """"model" is exactly what the reference saves (train_vqvae.py:205-206: model.state_dict(), loadable by
        extract_code.py / sample.py); the rest is what the reference lacks for an exact resume: Adam moments and
        step count, learning rate / betas, the schedule position."""
        group = self.optimizer.param_groups[0]
        return {"model": {k: v.detach().clone() for k, v in self.model.state_dict().items()},
                # Adam moments in REGISTRATION order (the arena's internal order is an implementation detail)
                "adam_m": self.arena.canonical(self.optimizer._m), "adam_v": self.arena.canonical(self.optimizer._v),
                "adam_t": self.optimizer._t,
                "lr": group["lr"], "betas": tuple(group["betas"]),
                "scheduler": None if self.scheduler is None else self.scheduler.state_dict()}

    def load_state_dict(self, sd):
        """Inverse of state_dict(); also accepts a bare model state_dict (the reference's --resume file,
        train_vqvae.py:173-182, with or without DDP's "module." prefix): optimizer state then starts fresh."""
        full = "model" in sd and isinstance(sd["model"], dict)
        model_sd = sd["model"] if full else sd
        model_sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in model_sd.items()}
        self.model.load_state_dict(model_sd)          # copies INTO the arena views: parameters stay re-homed
        ops.touch_weights(self.arena.params)
        if full:
            n_real = sum(p.numel() for p in self.arena.params)
            if sd["adam_m"].numel() == self.optimizer._m.numel() and sd["adam_m"].numel() != n_real:
                # a round-2 checkpoint: moments in that arena's padded registration order
                raise RuntimeError("Stage1Trainer.load_state_dict: optimizer state uses the pre-round-3 padded layout; "
                                   "re-save it with that version or resume from the model weights alone")
            if sd["adam_m"].numel() != n_real:
                raise RuntimeError("Stage1Trainer.load_state_dict: optimizer state belongs to a different model")
            dev = self.optimizer._m.device
            self.arena.from_canonical(sd["adam_m"].to(dev), self.optimizer._m)
            self.arena.from_canonical(sd["adam_v"].to(dev), self.optimizer._v)
            self.optimizer._t = int(sd["adam_t"])
            for group in self.optimizer.param_groups:
                group["lr"], group["betas"] = sd["lr"], tuple(sd["betas"])
            if (self.scheduler is None) != (sd.get("scheduler") is None):
                raise RuntimeError("Stage1Trainer.load_state_dict: checkpoint and trainer disagree about --sched")
            if self.scheduler is not None:
                self.scheduler.load_state_dict(sd["scheduler"])
        self.pack_plan.run()


class Stage2Trainer:
    """The train step of the reference's train_pixelsnail.py:20-57 for one PixelSNAIL: zero_grad, forward, cross-entropy with
    accuracy (ops.prior_loss), backward, scheduler step, Adam step.  `hier` is 'top' (the model sees the top codes) or
    'bottom' (the bottom codes, conditioned on the top ones).  step() returns {'loss', 'accuracy'} as 0-dim device tensors
    and 'lr'; nothing is copied to the host.

    arena=True (the default): the parameters live in a ParamArena and an ops.WeightNormPlan forms every effective weight
    with one launch per step and differentiates them with one more, straight into the gradient arena; Adam is one launch.
    Every element goes through the same kernels in the same order as with arena=False (one weight-norm launch per layer and
    pass, one Adam launch per tensor), so losses and parameters are bit for bit the same.

    Data parallelism (one process per GPU, in place of the reference's nn.DataParallel, train_pixelsnail.py:141): as
    Stage1Trainer -- rank 0's parameters and buffers everywhere at construction, the gradient arena SUM-all-reduced in two
    contiguous slices (Adam divides by the world size), the first of them from a backward hook while the rest still
    back-propagates.  VQ2_DP_FORCE=1 takes this path whenever a process group exists, also at world size 1.  Dropout seeds
    come from each rank's own torch generator; the trainer does not touch them."""

    def __init__(self, model, hier="top", lr=3e-4, sched=None, n_iter=None, arena=True):
        if hier not in ("top", "bottom"):
            raise ValueError(f"Stage2Trainer: hier must be 'top' or 'bottom', got {hier!r}")
        if sched not in (None, "cycle"):
            raise ValueError(f"Stage2Trainer: sched must be None or 'cycle', got {sched!r}")
        self.model, self.hier = model, hier
        self.arena = self.plan = None
        self.plan_info = {"entries": 0, "per_layer": len(ops.WeightNormPlan.layers(model)), "per_layer_names": []}
        self.world, self.dp = 1, False
        self.buckets, self.bucket_bytes, self.early_buckets = [], {}, 0
        if arena:
            self._init_arena(lr)
        else:
            if dist_fn.get_world_size() > 1:
                raise RuntimeError("Stage2Trainer: data-parallel training needs the arena path (arena=True)")
            self.optimizer = FusedAdam(model.parameters(), lr=lr)
        self.scheduler = None
        if sched == "cycle":
            self.scheduler = CycleScheduler(self.optimizer, lr, n_iter=n_iter, momentum=None)

    # ------------------------------------------------------------------ the arena path
    @staticmethod
    def _early_modules(model):
        """The modules whose gradients are complete first: the output head and the later half of the blocks (the backward
        pass runs out -> blocks[-1] -> ... -> blocks[0] -> cond_resnet, horizontal, vertical)."""
        blocks = list(getattr(model, "blocks", ()))
        early = blocks[len(blocks) // 2:] if len(blocks) >= 2 else []
        if getattr(model, "out", None) is not None:
            early.append(model.out)
        return early

    def _init_arena(self, lr):
        model = self.model
        live = [p for p in model.parameters() if p.requires_grad]
        # registration order is horizontal vertical blocks[...] cond_resnet out; with the early modules at the end the
        # gradient buffer reads [horizontal vertical blocks[:k] cond_resnet | blocks[k:] out]: the tail is complete first
        early = [p for m in self._early_modules(model) for p in m.parameters() if p.requires_grad]
        if len(early) == len(live):
            early = []
        self.arena = a = ParamArena(live, last=early)
        self.optimizer = FusedAdam(live, lr=lr, arena=a)
        self.plan = ops.WeightNormPlan(model, a)
        self.plan_info = {"entries": self.plan.n, "per_layer": len(self.plan.skipped), "per_layer_names": list(self.plan.skipped),
                          "w_floats": self.plan.w.numel()}
        self.world = dist_fn.get_world_size()
        forced = os.environ.get("VQ2_DP_FORCE", "0") != "0" and dist.is_available() and dist.is_initialized()
        self.dp = self.world > 1 or forced
        self.optimizer.grad_scale = 1.0 / self.world       # the all-reduce sums; DataParallel's loss is a mean over the batch
        self.comm_stream = torch.cuda.Stream() if self.dp else None
        self.comm = dist_fn.data_comm() if self.dp else None
        total = a.flat_g.numel()
        lo = min((a.n_extra + a.offset[id(p)] for p in early), default=total)
        inside = lambda b, e: [p for p in a.params if b <= a.n_extra + a.offset[id(p)] < e]
        # (name, lo, hi, parameters, [first, last) entries of the plan): "early" goes out from the backward hook
        self.buckets = [(name, b, e, inside(b, e), (self.plan.first_entry_at(b), self.plan.first_entry_at(e)))
                        for name, b, e in (("early", lo, total), ("late", 0, lo)) if e > b]
        self.bucket_bytes = {name: 4 * (e - b) for name, b, e, _, _ in self.buckets}
        self._sent, self._seen = [], 0
        if self.dp:
            self._sync_initial_state()
            if len(self.buckets) == 2:
                for prm in self.buckets[0][3]:
                    prm.register_post_accumulate_grad_hook(self._early_hook)

    def _sync_initial_state(self):
        """Rank 0's parameters and buffers everywhere: one broadcast for the arena, one per tensor outside it."""
        with torch.no_grad():
            self.comm.broadcast(self.arena.flat_p, 0)
            inside = {id(p) for p in self.arena.params}
            for t in list(self.model.parameters()) + list(self.model.buffers()):
                if id(t) not in inside:
                    self.comm.broadcast(t.detach(), 0)
        ops.touch_weights(self.arena.params)
        self.plan.invalidate()
        if hasattr(self.model, "_bg"):
            self.model._bg = None       # the repeated coordinate planes were made from the buffer as it was

    def _early_hook(self, _p):
        """Post-accumulate hook of every parameter of the early slice: when the last of them has its gradient, form the
        slice's dv / dg and hand it to the communicator while the rest of the model back-propagates."""
        if not self.plan.active:
            return
        self._seen += 1
        _, lo, hi, params, (first, last) = self.buckets[0]
        if self._seen != len(params):
            return
        if not all(p.grad is not None and p.grad.data_ptr() == p._vq2_grad.data_ptr() for p in params):
            return      # a gradient missed its slot: keep the slice for after backward, where FusedAdam reports it
        self.plan.backward(first, last)
        ev = torch.cuda.current_stream().record_event()
        with torch.cuda.stream(self.comm_stream):
            self.comm_stream.wait_event(ev)
            self.comm.all_reduce(self.arena.flat_g[lo:hi])
        self._sent.append((lo, hi))
        self.early_buckets += 1

    def _step_arena(self, top, bottom):
        a, plan = self.arena, self.plan
        a.zero_grad()
        self._sent, self._seen = [], 0
        plan.prepare()
        plan.active = True
        try:
            if self.hier == "top":
                target = top
                out, _ = self.model(top)
            else:
                target = bottom
                out, _ = self.model(bottom, condition=top)
            loss, accuracy = ops.prior_loss(out, target)
            loss.backward()
        finally:
            plan.active = False
            plan.invalidate()
        # the entries whose slice did not go out early: everything without data parallelism
        plan.backward(0, self.buckets[0][4][0] if self._sent else plan.n)
        if self.dp:
            if not a.grads_ready():
                raise RuntimeError("Stage2Trainer: a gradient did not land in the flat arena")
            ev = torch.cuda.current_stream().record_event()
            with torch.cuda.stream(self.comm_stream):
                self.comm_stream.wait_event(ev)
                pos = 0
                for lo, hi in sorted(self._sent) + [(a.flat_g.numel(), a.flat_g.numel())]:
                    if lo > pos:
                        self.comm.all_reduce(a.flat_g[pos:lo])
                    pos = max(pos, hi)
            torch.cuda.current_stream().wait_stream(self.comm_stream)
        if self.scheduler is not None:
            self.scheduler.step()
        self.optimizer.step()
        return {"loss": loss.detach(), "accuracy": accuracy, "lr": self.optimizer.param_groups[0]["lr"]}

    def step(self, top, bottom=None):
        if self.arena is not None:
            return self._step_arena(top, bottom)
        self.model.zero_grad(set_to_none=True)
        if self.hier == "top":
            target = top
            out, _ = self.model(top)
        else:
            target = bottom
            out, _ = self.model(bottom, condition=top)
        loss, accuracy = ops.prior_loss(out, target)
        loss.backward()
        if self.scheduler is not None:
            self.scheduler.step()
        self.optimizer.step()
        return {"loss": loss.detach(), "accuracy": accuracy, "lr": self.optimizer.param_groups[0]["lr"]}

    # ------------------------------------------------------------------ checkpoint / resume
    def _need_arena(self, what):
        if self.arena is None:
            raise RuntimeError(f"Stage2Trainer.{what} needs the arena path (arena=True)")

    def state_dict(self):
        """As Stage1Trainer.state_dict(): "model" is exactly what the reference saves (train_pixelsnail.py:150-153), then the
        Adam moments in registration order, the step count, learning rate / betas and the schedule position."""
        self._need_arena("state_dict")
        group = self.optimizer.param_groups[0]
        return {"model": {k: v.detach().clone() for k, v in self.model.state_dict().items()},
                "adam_m": self.arena.canonical(self.optimizer._m), "adam_v": self.arena.canonical(self.optimizer._v),
                "adam_t": self.optimizer._t,
                "lr": group["lr"], "betas": tuple(group["betas"]),
                "scheduler": None if self.scheduler is None else self.scheduler.state_dict()}

    def load_state_dict(self, sd):
        """Inverse of state_dict(); also accepts a bare model state_dict (the reference's checkpoint['model'], with or
        without DataParallel's "module." prefix): optimizer state then starts fresh."""
        self._need_arena("load_state_dict")
        model_sd = sd["model"] if isinstance(sd.get("model"), dict) else sd      # (the reference's file: {'model', 'args'})
        full = model_sd is not sd and "adam_m" in sd
        model_sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in model_sd.items()}
        if full and (self.scheduler is None) != (sd.get("scheduler") is None):
            raise RuntimeError("Stage2Trainer.load_state_dict: checkpoint and trainer disagree about --sched")
        if full and sd["adam_m"].numel() != sum(p.numel() for p in self.arena.params):
            raise RuntimeError("Stage2Trainer.load_state_dict: optimizer state belongs to a different model")
        self.model.load_state_dict(model_sd)          # copies INTO the arena views: parameters stay re-homed
        ops.touch_weights(self.arena.params)
        self.plan.invalidate()
        if hasattr(self.model, "_bg"):
            self.model._bg = None
        if full:
            dev = self.optimizer._m.device
            self.arena.from_canonical(sd["adam_m"].to(dev), self.optimizer._m)
            self.arena.from_canonical(sd["adam_v"].to(dev), self.optimizer._v)
            self.optimizer._t = int(sd["adam_t"])
            for group in self.optimizer.param_groups:
                group["lr"], group["betas"] = sd["lr"], tuple(sd["betas"])
            if self.scheduler is not None:
                self.scheduler.load_state_dict(sd["scheduler"])
