"""The canonical stage-1 step of /root/reference/train_vqvae.py:83-91 (+166-171, 185-206) as an
object: forward, MSE + 0.25*latent, backward, packed all-reduces (gradients + the EMA sums of both
quantizers) over RCCL on a side stream, deferred EMA update, one-launch Adam, optional CycleScheduler,
and a checkpoint that resumes the run exactly (model in the reference's format + optimizer + schedule).
Stage2Trainer is the step of train_pixelsnail.py:20-57 for one PixelSNAIL prior.

Both stand on _ArenaTrainer, the host-side machinery of a trainer whose parameters, gradients and Adam moments live in
a ParamArena: the data-parallel set-up and initial broadcast, the gradient buffer cut into contiguous Buckets that go
to the communicator from backward hooks, the all-reduce of whatever did not go out early, and the checkpoint.  A
trainer adds its own step, what "finish this slice of the gradient buffer" means, and which derived state to drop when
the parameters are overwritten behind autograd's back.
"""
import contextlib
import os
from collections import namedtuple

import torch
from torch import distributed as dist

from . import distributed as dist_fn
from . import ops
from .optim import CycleScheduler, FusedAdam, ParamArena

LATENT_LOSS_WEIGHT = 0.25  # train_vqvae.py:34


def stage1_loss(dec, diff, img, latent_loss_weight=LATENT_LOSS_WEIGHT):
    """(loss, recon_loss, latent_loss) = MSE(dec,img) + w * diff.mean()  (train_vqvae.py:83-85)."""
    return ops.Stage1LossFn.apply(dec, diff, img, latent_loss_weight)


# one contiguous slice [lo, hi) of the gradient arena that goes to the communicator in one collective, and its parameters
Bucket = namedtuple("Bucket", "name lo hi params")


def split_checkpoint(sd):
    """(model state_dict without DDP's / DataParallel's "module." prefix, full) of anything load_state_dict accepts: a
    bare model state_dict (train_vqvae.py:173-182), the reference's {'model': ..., 'args': ...} file
    (train_pixelsnail.py:150-153) -- both with full = False: optimizer state starts fresh -- or a trainer's own
    state_dict() (full = True).  Touches no device."""
    wrapped = isinstance(sd.get("model"), dict)
    model_sd = sd["model"] if wrapped else sd
    strip = lambda k: k[len("module."):] if k.startswith("module.") else k
    return {strip(k): v for k, v in model_sd.items()}, wrapped and "adam_m" in sd


class _ArenaTrainer:
    """What Stage1Trainer and Stage2Trainer share; needs self.model, self.arena, self.optimizer and self.scheduler."""

    arena = None

    def _need_arena(self, what):
        if self.arena is None:
            raise RuntimeError(f"{type(self).__name__}.{what} needs the arena path (arena=True)")

    def _params_overwritten(self):
        """The parameters and buffers were written behind autograd's back: drop what was derived from the old ones."""
        raise NotImplementedError

    # ------------------------------------------------------------------ data parallel plumbing
    def _init_data_parallel(self):
        """One process per GPU.  Like DDP's constructor (train_vqvae.py:166-171) rank 0's state goes everywhere first;
        every step then SUM-all-reduces the gradient arena and Adam divides by the world size."""
        self.world = dist_fn.get_world_size()
        forced = os.environ.get("VQ2_DP_FORCE", "0") != "0" and dist.is_available() and dist.is_initialized()
        self.dp = self.world > 1 or forced
        self.optimizer.grad_scale = 1.0 / self.world
        self.comm_stream = torch.cuda.Stream() if self.dp else None
        self.comm = dist_fn.data_comm() if self.dp else None   # torch.distributed group or libvq2's own communicator
        self.buckets = []           # Buckets that tile flat_g, in the order their gradients are complete
        self.bucket_bytes = {}      # name -> bytes of the slice (bench line)
        self.early_buckets = 0      # buckets that went out from a backward hook (all steps)
        self._sent = []             # [lo, hi) slices of flat_g already handed to the communicator in this step
        self._hooks_seen = {}       # bucket name -> watched parameters that have reported in this step
        if self.dp:
            self._sync_initial_state()

    def _sync_initial_state(self):
        """Rank 0's parameters and buffers everywhere: one broadcast for the whole arena, one per tensor outside it
        (dead dec_ir, codebooks, coordinate planes)."""
        with torch.no_grad():
            self.comm.broadcast(self.arena.flat_p, 0)
            inside = {id(p) for p in self.arena.params}
            for t in list(self.model.parameters()) + list(self.model.buffers()):
                if id(t) not in inside:
                    self.comm.broadcast(t.detach(), 0)     # (detach() shares the version counter; .data does not)
        ops.touch_weights(self.arena.params)
        self._params_overwritten()      # (NativeComm writes through raw pointers, which no version counter sees)

    def _set_buckets(self, spans):
        """spans: (name, lo, hi) slices that tile flat_g, in the order their gradients are complete."""
        a = self.arena
        inside = lambda lo, hi: [p for p in a.params if lo <= a.n_extra + a.offset[id(p)] < hi]
        self.buckets = [Bucket(name, lo, hi, inside(lo, hi)) for name, lo, hi in spans]
        self.bucket_bytes = {b.name: 4 * (b.hi - b.lo) for b in self.buckets}

    def _send_when_reported(self, bucket, watched, finish):
        """Post-accumulate hooks on `watched`: when the last of them has reported in a step, `bucket` goes out early."""
        for prm in watched:
            prm.register_post_accumulate_grad_hook(lambda _p: self._reported(bucket, len(watched), finish))

    def _reported(self, bucket, need, finish):
        """finish() completes the bucket's slice of flat_g and returns the event the communicator has to wait for; data
        parallel, the slice is then all-reduced on the communication stream while the rest of the model back-propagates."""
        seen = self._hooks_seen[bucket.name] = self._hooks_seen.get(bucket.name, 0) + 1
        if seen != need:
            return
        if not all(ops.landed(p) for p in bucket.params):
            # a gradient is not in its slot (autograd ordered the graph differently, or it missed the arena, which
            # _reduce_unsent / FusedAdam report): keep the slice for the collective after backward
            return
        ev = finish()
        if not self.dp:
            return
        with torch.cuda.stream(self.comm_stream):
            self.comm_stream.wait_event(ev)
            self.comm.all_reduce(self.arena.flat_g[bucket.lo:bucket.hi])
        self._sent.append((bucket.lo, bucket.hi))
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

    def _reduce_unsent(self):
        """After backward, data parallel: whatever no hook sent goes out now (everything if none fired), on the side
        stream so the host can already enqueue what follows; the main stream waits for all of the step's collectives."""
        if not self.dp:
            return
        if not self.arena.grads_ready():
            raise RuntimeError(f"{type(self).__name__}: a gradient did not land in the flat arena")
        ev = torch.cuda.current_stream().record_event()
        with torch.cuda.stream(self.comm_stream):
            self.comm_stream.wait_event(ev)
            for lo, hi in self._unsent_slices():
                self.comm.all_reduce(self.arena.flat_g[lo:hi])
        torch.cuda.current_stream().wait_stream(self.comm_stream)

    # ------------------------------------------------------------------ clipping, skipped steps, averaged weights
    def _finish_construction(self):
        """Last line of a constructor: the average starts from the parameters every rank now holds."""
        self.optimizer.init_average()

    def _clip_result(self, out):
        """step()'s result gains the pre-clip norm and the coefficient (0-dim device views of optimizer.ctl) when clipping
        is on; otherwise it keeps the keys it has."""
        if self.optimizer.clip_grad_norm is not None:
            out["grad_norm"], out["clip_coef"] = self.optimizer.ctl[0], self.optimizer.ctl[1]
        return out

    def skipped_steps(self):
        """How many steps a non-finite gradient norm has skipped so far: the one host read of optimizer.ctl."""
        ctl = getattr(self.optimizer, "ctl", None)
        return 0 if ctl is None else int(ctl[3].item())

    def _need_average(self, what):
        self._need_arena(what)
        if self.optimizer.ema_decay is None:
            raise RuntimeError(f"{type(self).__name__}.{what} needs averaged weights (ema_decay=...)")

    def _weights_replaced(self):
        """The whole parameter arena was rewritten in place."""
        ops.touch_weights(self.arena.params)
        self._params_overwritten()

    def averaged_state_dict(self):
        """model.state_dict() with every arena parameter replaced by its averaged value; buffers (stage 1's codebooks among
        them) and parameters outside the arena as they are.  Loads wherever the reference's checkpoints load."""
        self._need_average("averaged_state_dict")
        a, avg = self.arena, self.optimizer._avg
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        for name, p in self.model.named_parameters():
            if id(p) in a.offset and name in sd:
                off = a.offset[id(p)]
                sd[name] = avg[off:off + p.numel()].view(p.shape).clone()
        return sd

    @contextlib.contextmanager
    def averaged_weights(self):
        """`with trainer.averaged_weights(): trainer.evaluate(...)`: inside, the model's parameters are the averaged ones.
        The contents of the parameter arena and of the average are exchanged on entry and back on exit (also when the body
        raises); no generator is drawn from, and the steps after the block are bit for bit those of a run that never
        entered.  A forward pass may write the arena (a 'causal' convolution zeroes the masked taps of its weight_v in
        place), so the average goes back from a copy kept aside for the block, not from the arena.  Do not call step()
        inside."""
        self._need_average("averaged_weights")
        p, avg = self.arena.flat_p, self.optimizer._avg
        with torch.no_grad():
            kept = avg.clone()
            avg.copy_(p)
            p.copy_(kept)
        self._weights_replaced()
        try:
            yield self
        finally:
            with torch.no_grad():
                p.copy_(avg)
                avg.copy_(kept)
            self._weights_replaced()

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self):
        """"model" is exactly what the reference saves (train_vqvae.py:205-206, train_pixelsnail.py:150-153:
        model.state_dict(), loadable by extract_code.py / sample.py); the rest is what the reference lacks for an exact
        resume: Adam moments and step count, learning rate / betas, the schedule position.  With ema_decay also "avg" (laid
        out as the moments are) and "ema_decay"; with clip_grad_norm also "clip_grad_norm" and "skipped"."""
        self._need_arena("state_dict")
        opt = self.optimizer
        group = opt.param_groups[0]
        sd = {"model": {k: v.detach().clone() for k, v in self.model.state_dict().items()},
              # Adam moments in REGISTRATION order (the arena's internal order is an implementation detail)
              "adam_m": self.arena.canonical(opt._m), "adam_v": self.arena.canonical(opt._v),
              "adam_t": opt._t,
              "lr": group["lr"], "betas": tuple(group["betas"]),
              "scheduler": None if self.scheduler is None else self.scheduler.state_dict()}
        if opt.ema_decay is not None:
            sd["avg"], sd["ema_decay"] = self.arena.canonical(opt._avg), opt.ema_decay
        if opt.clip_grad_norm is not None:
            sd["clip_grad_norm"], sd["skipped"] = opt.clip_grad_norm, self.skipped_steps()
        return sd

    def load_state_dict(self, sd):
        """Inverse of state_dict(); also accepts what split_checkpoint() calls not full (the reference's files):
        optimizer state then starts fresh.  Averaged weights: a checkpoint's "avg" goes into a trainer with ema_decay; a
        checkpoint without one starts the average from the loaded weights; a checkpoint with one and a trainer without
        ema_decay disagree.  Raises before it changes anything."""
        self._need_arena("load_state_dict")
        who = f"{type(self).__name__}.load_state_dict"
        model_sd, full = split_checkpoint(sd)
        opt = self.optimizer
        n_real = sum(p.numel() for p in self.arena.params)
        if full:
            if (self.scheduler is None) != (sd.get("scheduler") is None):
                raise RuntimeError(f"{who}: checkpoint and trainer disagree about --sched")
            if "avg" in sd and opt.ema_decay is None:
                raise RuntimeError(f"{who}: the checkpoint carries averaged weights and the trainer was built without "
                                   "--ema_decay")
            if "avg" in sd and sd["avg"].numel() != n_real:
                raise RuntimeError(f"{who}: averaged weights belong to a different model")
            n = sd["adam_m"].numel()
            if n != n_real and n == self.optimizer._m.numel():
                # a round-2 checkpoint: moments in that arena's padded registration order
                raise RuntimeError(f"{who}: optimizer state uses the pre-round-3 padded layout; "
                                   "re-save it with that version or resume from the model weights alone")
            if n != n_real:
                raise RuntimeError(f"{who}: optimizer state belongs to a different model")
        self.model.load_state_dict(model_sd)          # copies INTO the arena views: parameters stay re-homed
        ops.touch_weights(self.arena.params)
        if full:
            dev = self.optimizer._m.device
            self.arena.from_canonical(sd["adam_m"].to(dev), self.optimizer._m)
            self.arena.from_canonical(sd["adam_v"].to(dev), self.optimizer._v)
            self.optimizer._t = int(sd["adam_t"])
            for group in self.optimizer.param_groups:
                group["lr"], group["betas"] = sd["lr"], tuple(sd["betas"])
            if self.scheduler is not None:
                self.scheduler.load_state_dict(sd["scheduler"])
            if opt.clip_grad_norm is not None:
                opt.ctl[3] = float(sd.get("skipped", 0))
        if opt.ema_decay is not None:
            if full and "avg" in sd:
                self.arena.from_canonical(sd["avg"].to(opt._avg.device), opt._avg)
            else:
                opt.init_average()
        self._params_overwritten()


class Stage1Trainer(_ArenaTrainer):
    """Replaces `DistributedDataParallel(model)` + `optim.Adam` + the loop body of train_vqvae.py:83-91.

    Data parallelism (one process per GPU): like DDP's constructor (train_vqvae.py:166-171) the trainer first
    broadcasts rank 0's parameters and buffers, so replicas built from different RNG states start identical; every
    step then SUM-all-reduces the flat gradient buffer (Adam divides by the world size) in two buckets.
    VQ2_DP_FORCE=1 takes this path whenever a process group exists, also at world size 1.

    normalizer: a data.ImageNormalizer; step() then also takes uint8 image batches on the device (the loader's
    ToTensor + Normalize + CenterCrop run as one kernel inside the step, train_vqvae.py:149-155)."""

    def __init__(self, model, lr=3e-4, sched=None, n_iter=None, betas=(0.9, 0.999), eps=1e-8, normalizer=None,
                 clip_grad_norm=None, ema_decay=None):
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
        self.optimizer = FusedAdam(live, lr=lr, betas=betas, eps=eps, arena=self.arena, clip_grad_norm=clip_grad_norm,
                                   ema_decay=ema_decay)
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

        self._init_data_parallel()
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
        split = getattr(model, "quantize_conv_b", None)
        enc_t = getattr(model, "enc_t", None)
        if split is not None and enc_b is not None and enc_t is not None:
            a = self.arena
            off = lambda p: a.n_extra + a.offset[id(p)]
            lo_tail = off(split.weight)
            lo_head = min(off(p) for p in enc_b.parameters())
            self._set_buckets([("tail", lo_tail, lo_head), ("middle", 0, lo_tail), ("head", lo_head, a.flat_g.numel())])
            tail, middle, _ = self.buckets
            # each group is watched through its LAST layer; without data parallelism the tail hook still runs, for the
            # early slab reduction (one is enough on a single GPU, a second one only adds a launch)
            self._send_when_reported(tail, (split.weight, split.bias), self._flush_slabs)
            if self.dp:
                first = enc_t.blocks[0]
                self._send_when_reported(middle, (first.weight, first.bias), self._flush_slabs)
        self.code_restart = self._restart_cand = self._restart_counters = None      # set_code_restart()
        self._finish_construction()

    def _params_overwritten(self):
        for q in self.quantizers:       # anything a Quantize derived from its OLD codebook is stale now
            q.invalidate_prepared()

    # ------------------------------------------------------------------ dead-code restart
    def set_code_restart(self, threshold=1.0, start=0, seed=0):
        """Random restart of dead codes in every quantizer (Quantize.enable_code_restart with slot = its index in
        self.quantizers); threshold None turns it off.  The Philox step is this trainer's step count (the optimizer's, which
        the checkpoint holds), so a resumed run draws the rows an uninterrupted one draws.  The candidate rows of all
        quantizers live in ONE flat buffer outside the arena; data parallel it is summed by one collective on the
        communication stream, which the deferred updates wait for.  step() then also returns "restarted"."""
        if threshold is None:
            for q in self.quantizers:
                q.disable_code_restart()
                q.restart_cand = q.restart_counter = None
            self.code_restart = self._restart_cand = self._restart_counters = None
            return
        for slot, q in enumerate(self.quantizers):
            q.enable_code_restart(threshold, start, seed, slot)      # (refuses a bad threshold before anything changes)
        dev = self.arena.flat_p.device
        sizes = [q.n_embed * q.dim for q in self.quantizers]         # multiples of 4: every slice stays 16-byte aligned
        self._restart_cand = torch.zeros(sum(sizes), device=dev, dtype=torch.float32)
        self._restart_counters = torch.zeros((len(sizes), 2), device=dev, dtype=torch.int64)
        off = 0
        for i, (q, n) in enumerate(zip(self.quantizers, sizes)):
            q.restart_cand, q.restart_counter = self._restart_cand[off:off + n], self._restart_counters[i]
            off += n
        self.code_restart = {"threshold": float(threshold), "start": int(start), "seed": int(seed)}

    def restarted_codes(self):
        """Codes restarted so far, one total per quantizer: the one host read of the device counters."""
        if self.code_restart is None:
            return [0] * len(self.quantizers)
        return [int(v) for v in self._restart_counters[:, 1].tolist()]

    def _reduce_candidates(self):
        """Data parallel: the owner of each drawn row wrote it, every other rank zeros; one SUM leaves it everywhere."""
        if self.code_restart is None or not self.dp:
            return
        ev = torch.cuda.current_stream().record_event()
        with torch.cuda.stream(self.comm_stream):
            self.comm_stream.wait_event(ev)
            self.comm.all_reduce(self._restart_cand)

    def _weights_replaced(self):
        super()._weights_replaced()
        self.pack_plan.run()            # the packed panels are made from the weights as they were

    def _flush_slabs(self):
        """Finish a slice: reduce the split-K slabs produced so far into the arena, on the side stream."""
        side = self.ctx.stream
        side.wait_event(torch.cuda.current_stream().record_event())
        with torch.cuda.stream(side):
            self.ctx.batch.flush()
            return side.record_event()

    # ------------------------------------------------------------------ the step
    def step(self, img, return_dec=False):
        """One training step on this rank's batch (img: float32 NCHW, or a uint8 batch in the normalizer's layout);
        returns device scalars (no host sync)."""
        model = self.model
        u8 = getattr(img, "dtype", None) == torch.uint8
        if u8 and self.normalizer is None:
            raise TypeError("Stage1Trainer.step: a uint8 batch needs Stage1Trainer(..., normalizer=ImageNormalizer(...))")
        model.train()
        if self.code_restart is not None:
            for q in self.quantizers:       # the draw of this step: a function of the step count the checkpoint holds
                q.restart_step = self.optimizer._t
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
        # gradients (SUM; Adam divides by world) and EMA sums (SUM, vqvae.py:58-59) travel together; normally only
        # enc_b's slice is left
        self._reduce_candidates()
        self._reduce_unsent()
        for q in self.quantizers:
            q.apply_deferred_update()
        if self.scheduler is not None:
            self.scheduler.step()
        self.optimizer.step()
        self.pack_plan.run()
        out = self._clip_result({"loss": loss.detach(), "recon": recon, "latent": latent})
        if self.code_restart is not None:
            out["restarted"] = self._restart_counters[:, 0]     # per quantizer, this step (a view: the next step rewrites it)
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

    def state_dict(self):
        """_ArenaTrainer.state_dict(), with "code_restart" = {threshold, start, seed, totals} when set_code_restart() is on."""
        sd = super().state_dict()
        if self.code_restart is not None:
            sd["code_restart"] = dict(self.code_restart, totals=self.restarted_codes())
        return sd

    def load_state_dict(self, sd):
        """_ArenaTrainer.load_state_dict(); a full checkpoint and a trainer that disagree about the code restart (one has
        it and the other not, or its threshold / start / seed differ) are refused before anything changes: the steps that
        follow would not be the run's."""
        if split_checkpoint(sd)[1]:
            mine, theirs = self.code_restart, sd.get("code_restart")
            who = "Stage1Trainer.load_state_dict"
            if (mine is None) != (theirs is None):
                raise RuntimeError(f"{who}: the checkpoint was trained {'with' if theirs else 'without'} code restart and the "
                                   f"trainer runs {'with' if mine else 'without'} it (set_code_restart)")
            if mine is not None:
                if any(theirs.get(k) != mine[k] for k in mine):
                    raise RuntimeError(f"{who}: code restart settings differ: checkpoint "
                                       f"{ {k: theirs.get(k) for k in mine} }, trainer {mine} (set_code_restart)")
                if len(theirs.get("totals", ())) != len(self.quantizers):
                    raise RuntimeError(f"{who}: code restart totals belong to a different model")
        super().load_state_dict(sd)
        if self.code_restart is not None and split_checkpoint(sd)[1]:
            totals = torch.tensor(sd["code_restart"]["totals"], dtype=torch.int64)
            self._restart_counters[:, 0].zero_()
            self._restart_counters[:, 1].copy_(totals)
        self.pack_plan.run()


class Stage2Trainer(_ArenaTrainer):
    """The train step of the reference's train_pixelsnail.py:20-57 for one PixelSNAIL: zero_grad, forward, cross-entropy with
    accuracy (ops.prior_loss), backward, scheduler step, Adam step.  `hier` is 'top' (the model sees the top codes) or
    'bottom' (the bottom codes, conditioned on the top ones).  step() returns {'loss', 'accuracy'} as 0-dim device tensors
    and 'lr'; nothing is copied to the host.  step(top, bottom=None, label=None): label is int64 [B] on the device for a
    class-conditional model (PixelSNAIL(..., n_label > 0)); its label_embed tables are ordinary parameters of the arena.

    arena=True (the default): the parameters live in a ParamArena and an ops.WeightNormPlan forms every effective weight
    with one launch per step and differentiates them with one more, straight into the gradient arena; Adam is one launch.
    Every element goes through the same kernels in the same order as with arena=False (one weight-norm launch per layer and
    pass, one Adam launch per tensor), so losses and parameters are bit for bit the same.

    Data parallelism (one process per GPU, in place of the reference's nn.DataParallel, train_pixelsnail.py:141): as
    Stage1Trainer -- rank 0's parameters and buffers everywhere at construction, the gradient arena SUM-all-reduced in two
    contiguous slices (Adam divides by the world size), the first of them from a backward hook while the rest still
    back-propagates.  VQ2_DP_FORCE=1 takes this path whenever a process group exists, also at world size 1.  Dropout seeds
    come from each rank's own torch generator; the trainer does not touch them."""

    def __init__(self, model, hier="top", lr=3e-4, sched=None, n_iter=None, arena=True, clip_grad_norm=None, ema_decay=None):
        if hier not in ("top", "bottom"):
            raise ValueError(f"Stage2Trainer: hier must be 'top' or 'bottom', got {hier!r}")
        if sched not in (None, "cycle"):
            raise ValueError(f"Stage2Trainer: sched must be None or 'cycle', got {sched!r}")
        self.model, self.hier = model, hier
        self.precision = None           # set_precision()
        self.arena = self.plan = None
        self.plan_info = {"entries": 0, "per_layer": len(ops.WeightNormPlan.layers(model)), "per_layer_names": []}
        if arena:
            self._init_arena(lr, clip_grad_norm, ema_decay)
        else:
            if dist_fn.get_world_size() > 1:
                raise RuntimeError("Stage2Trainer: data-parallel training needs the arena path (arena=True)")
            self.world, self.dp = 1, False
            self.buckets, self.bucket_bytes, self.early_buckets = [], {}, 0
            # (FusedAdam refuses clip_grad_norm / ema_decay without an arena)
            self.optimizer = FusedAdam(model.parameters(), lr=lr, clip_grad_norm=clip_grad_norm, ema_decay=ema_decay)
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

    def _init_arena(self, lr, clip_grad_norm=None, ema_decay=None):
        model = self.model
        live = [p for p in model.parameters() if p.requires_grad]
        # registration order is horizontal vertical blocks[...] cond_resnet out; with the early modules at the end the
        # gradient buffer reads [horizontal vertical blocks[:k] cond_resnet | blocks[k:] out]: the tail is complete first
        early = [p for m in self._early_modules(model) for p in m.parameters() if p.requires_grad]
        if len(early) == len(live):
            early = []
        self.arena = a = ParamArena(live, last=early)
        self.optimizer = FusedAdam(live, lr=lr, arena=a, clip_grad_norm=clip_grad_norm, ema_decay=ema_decay)
        self.plan = ops.WeightNormPlan(model, a)
        self.plan_info = {"entries": self.plan.n, "per_layer": len(self.plan.skipped), "per_layer_names": list(self.plan.skipped),
                          "w_floats": self.plan.w.numel()}
        self._init_data_parallel()      # (the all-reduce sums; DataParallel's loss is a mean over the batch)
        total = a.flat_g.numel()
        lo = min((a.n_extra + a.offset[id(p)] for p in early), default=total)
        self._set_buckets([(name, b, e) for name, b, e in (("early", lo, total), ("late", 0, lo)) if e > b])
        # [first, last) entries of the plan that differentiate the "early" slice, the one a backward hook sends
        self._early_entries = (self.plan.first_entry_at(lo), self.plan.first_entry_at(total))
        if self.dp and len(self.buckets) == 2:
            self._send_when_reported(self.buckets[0], self.buckets[0].params, self._finish_early)
        self._finish_construction()

    def set_precision(self, precision):
        """The precision of the run, 'bf16', 'bf16_wgrad', 'bf16_attn' or 'fp32': pixelsnail.set_conv_precision on the model
        (bf16 operands in the eligible conv forwards and data gradients, under 'bf16_wgrad' in the eligible weight gradients
        too; parameters and optimizer state stay fp32), remembered for the checkpoint.  'bf16_attn' is 'bf16_wgrad' plus
        pixelsnail.set_attention_precision(model, 'bf16'): bf16 operands in the eligible attention cores as well; the other
        three levels set the attention back to fp32.  Returns the convs' (eligible_layers, total_layers).  A trainer that was
        never told keeps the model's convs and attention as they are and saves no "precision"."""
        from .pixelsnail import set_conv_precision, set_attention_precision
        attn = precision == "bf16_attn"
        counts = set_conv_precision(self.model, "bf16_wgrad" if attn else precision)      # (refuses anything else)
        set_attention_precision(self.model, "bf16" if attn else "fp32")
        self.precision = precision
        return counts

    def state_dict(self):
        """_ArenaTrainer.state_dict(), with "precision" when set_precision() was called."""
        sd = super().state_dict()
        if self.precision is not None:
            sd["precision"] = self.precision
        return sd

    def load_state_dict(self, sd):
        """_ArenaTrainer.load_state_dict(); a full checkpoint whose precision (absent = 'fp32') differs from this
        trainer's (None = 'fp32') is refused before anything changes: the steps that follow would not be the run's."""
        if split_checkpoint(sd)[1]:
            mine, theirs = self.precision or "fp32", sd.get("precision") or "fp32"
            if mine != theirs:
                raise RuntimeError(f"Stage2Trainer.load_state_dict: the checkpoint was trained with precision {theirs!r}, "
                                   f"the trainer runs {mine!r} (set_precision)")
        super().load_state_dict(sd)

    def _params_overwritten(self):
        self.plan.invalidate()
        if hasattr(self.model, "_bg"):
            self.model._bg = None       # the repeated coordinate planes were made from the buffer as it was

    def _reported(self, bucket, need, finish):
        if self.plan.active:            # a backward pass outside step() sends nothing
            super()._reported(bucket, need, finish)

    def _finish_early(self):
        """Finish the early slice: form its dv / dg while the rest of the model back-propagates."""
        self.plan.backward(*self._early_entries)
        return torch.cuda.current_stream().record_event()

    # ------------------------------------------------------------------ the step
    def _forward_loss(self, top, bottom, label=None):
        kw = {} if label is None else {"label": label}      # (the model refuses a label it has no tables for, and a missing one)
        if self.hier == "top":
            target = top
            out, _ = self.model(top, **kw)
        else:
            target = bottom
            out, _ = self.model(bottom, condition=top, **kw)
        return ops.prior_loss(out, target)

    def step(self, top, bottom=None, label=None):
        plan = self.plan
        if plan is None:                # arena=False: one weight-norm launch per layer and pass, one Adam launch per tensor
            self.model.zero_grad(set_to_none=True)
            loss, accuracy = self._forward_loss(top, bottom, label)
            loss.backward()
        else:
            self.arena.zero_grad()
            self._sent, self._hooks_seen = [], {}
            plan.prepare()
            plan.active = True
            try:
                loss, accuracy = self._forward_loss(top, bottom, label)
                loss.backward()
            finally:
                plan.active = False
                plan.invalidate()
            # the entries whose slice did not go out early: everything without data parallelism
            plan.backward(0, self._early_entries[0] if self._sent else plan.n)
            self._reduce_unsent()
        if self.scheduler is not None:
            self.scheduler.step()
        self.optimizer.step()
        return self._clip_result({"loss": loss.detach(), "accuracy": accuracy, "lr": self.optimizer.param_groups[0]["lr"]})

    # ------------------------------------------------------------------ held-out evaluation
    def evaluate(self, batches, top_k=5):
        """PriorEvaluator.result() over an iterable of (top, bottom) or (top, bottom, filename) code batches -- for a
        class-conditional model (top, bottom, label) with label an int64 tensor [B] -- between two
        steps: eval-mode forwards under no_grad that draw no dropout seed and write no arena slot; the plan is not active,
        so every layer forms its weight from the parameters as they are, and the steps that follow are bit for bit those of
        a run that never evaluated.  Every module's train / eval flag is restored.  Data parallel: every rank calls it
        (result() sums over the group)."""
        from .evaluate import PriorEvaluator
        ev = PriorEvaluator(self.model, self.hier, top_k=top_k)
        device = next(self.model.parameters()).device
        for batch in batches:
            top, bottom = batch[0], batch[1]
            label = batch[2].to(device) if len(batch) > 2 and isinstance(batch[2], torch.Tensor) else None
            ev.update_labelled(label, top.to(device), bottom.to(device) if self.hier == "bottom" else None)
        return ev.result()
