"""Held-out evaluation.  Of a stage-1 model: what the reference's loop reports beside the loss -- the running
`mse_sum / mse_n` of train_vqvae.py:93-100 and the sample grid of :120-139 -- plus the health of both EMA codebooks
(codes in use, perplexity), gathered on the GPU without a host synchronisation per batch.

Evaluator               accumulates reconstruction error, latent loss and both code histograms over batches; with
                        image_metrics=True also the squared error and SSIM of the 8-bit reconstructions (PSNR, SSIM)
PriorEvaluator          accumulates the likelihood of held-out codes under a PixelSNAIL prior: nats and bits per code,
                        accuracy and top-k accuracy, predictive entropy, a per-position map, the targets' histogram
score_codes             log-likelihood of each given code map under a prior (what PriorSampler's return_logp is for drawn ones)
perplexity_from_counts  exp(entropy) of a code histogram, fp64 on the host
psnr_from_mse_u8        10 log10(255^2 / mse) of 8-bit images, fp64 on the host
"""
import contextlib
import math

import torch
from torch import distributed as dist

from . import ops


def perplexity_from_counts(counts):
    """exp(-sum p ln p) with p = counts / sum(counts), in fp64, codes that never occur skipped (0 ln 0 = 0): K for K
    codes used equally often, 1 when a single code takes every vector.  An empty histogram gives nan."""
    c = torch.as_tensor(counts).detach().to("cpu", torch.float64).reshape(-1)
    total = float(c.sum())
    if total <= 0:
        return float("nan")
    p = c[c > 0] / total
    return float(math.exp(-float((p * p.log()).sum())))


def psnr_from_mse_u8(mse_u8):
    """PSNR in dB of 8-bit images (data range 255) from their mean squared error in byte units; inf for identical images."""
    mse_u8 = float(mse_u8)
    if mse_u8 == 0.0:
        return float("inf")
    return 10.0 * math.log10(255.0 ** 2 / mse_u8)


@contextlib.contextmanager
def eval_mode(model):
    """model.eval() for the block, then every module's OWN train / eval flag back: a model whose modules do not all
    share one mode (a frozen Quantize kept in eval mode so that its EMA codebook stands still) leaves as it came."""
    flags = [(mod, mod.training) for mod in model.modules()]
    model.eval()
    try:
        yield
    finally:
        for mod, flag in flags:
            mod.training = flag


class Evaluator:
    """model: a VQVAE (anything with forward_nhwc(x, return_ids=True)); normalizer: a data.ImageNormalizer, needed for
    uint8 batches and for return_u8.

    update(img)   one batch, float32 NCHW or uint8 in the normaliser's layout: eval-mode forward under no_grad, then five
                  small launches on the NHWC tensors the forward already has (per-image squared error: partial sums and
                  their final sum; the two code histograms; one that folds the batch into the device accumulator).
                  Nothing is read back.
                  update(img, return_u8=True) returns the reconstruction as uint8 in the input's layout ([N,C,H,W] for
                  a float batch).  Every module's train / eval flag is restored.
    result()      ONE device-to-host copy -> {"mse", "latent", "images", "perplexity_t", "perplexity_b", "used_t",
                  "used_b", "n_embed", "counts_t", "counts_b"}; mse is the mean over every element of every image seen
                  (train_vqvae.py:83 averaged as :93-100 does), latent the image-weighted mean of the batches' latent
                  losses.  With a process group the totals and the histograms are summed over the ranks first, on
                  float64 / int64 tensors.  Raises RuntimeError if a quantizer ever produced an index outside its codebook.
    reset()       clears the accumulators.

    image_metrics=True (needs the normalizer): the quality of the 8-bit reconstruction, i.e. of the bytes that
    update(..., return_u8=True) returns against the bytes of the input (a uint8 batch returns to its own source bytes
    exactly; a float batch is quantised the same way).  update() adds the launches of vq2_image_metrics and its
    accumulate on the tensors it already holds, and result() gains "mse_u8" (mean squared byte difference over every
    element seen), "psnr" (10 log10(255^2 / mse_u8) dB, inf for mse_u8 == 0) and "ssim" (mean over the images of the
    Gaussian-window SSIM, see include/vq2.h).  They do not depend on the normaliser's statistics in any other way.  The
    integer total is summed over the ranks as int64, the SSIM total as float64."""

    def __init__(self, model, normalizer=None, image_metrics=False):
        if not hasattr(model, "forward_nhwc"):
            raise TypeError(f"Evaluator: {type(model).__name__} has no forward_nhwc (VQVAE_Deep's decoder needs a style "
                            "input that a held-out pass does not have); evaluate a VQVAE")
        if image_metrics and normalizer is None:
            raise TypeError("Evaluator(image_metrics=True) needs normalizer=ImageNormalizer(...): its statistics define the "
                            "8-bit images that PSNR and SSIM compare")
        self.model, self.normalizer, self.image_metrics = model, normalizer, bool(image_metrics)
        self.denormalizer = normalizer.inverse() if normalizer is not None else None
        self.k_t, self.k_b = model.quantize_t.n_embed, model.quantize_b.n_embed
        self._state = None

    def _state_len(self):
        return 4 + self.k_t + self.k_b + 1 + (2 if self.image_metrics else 0)

    def _buffers(self, device):
        """One int64 buffer [accumulator (4 doubles, as bits) | counts_t | counts_b | flag], so that result() is one copy;
        with image_metrics two more words follow: the int64 squared-error total and the SSIM total (a double, as bits)."""
        if self._state is None or self._state.device != device:
            self._state = torch.zeros(self._state_len(), device=device, dtype=torch.int64)
        s = self._state
        hist = 4 + self.k_t + self.k_b
        return (s[:4].view(torch.float64), s[4:4 + self.k_t], s[4 + self.k_t:hist], s[hist:hist + 1].view(torch.int32)[:1])

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    @torch.no_grad()
    def update(self, img, return_u8=False):
        model = self.model
        u8 = getattr(img, "dtype", None) == torch.uint8
        if (u8 or return_u8) and self.normalizer is None:
            raise TypeError("Evaluator.update: uint8 batches and return_u8 need Evaluator(model, normalizer=ImageNormalizer(...))")
        if u8:
            x = self.normalizer(img)
            n, channels, h, w = self.normalizer.out_shape(img)
        else:
            x = ops.to_nhwc(img)
            n, channels, h, w = img.shape
        with eval_mode(model):
            dec, diff, id_t, id_b = model.forward_nhwc(x, return_ids=True)
        acc, counts_t, counts_b, flag = self._buffers(x.device)
        ops.eval_accumulate(ops.sse_per_image(dec, ops.packed(x)), channels * h * w, diff, acc)
        ops.index_hist(id_t, counts_t, flag)
        ops.index_hist(id_b, counts_b, flag)
        if self.image_metrics:
            d = self.denormalizer
            sse_u8, ssim = ops.image_metrics(dec, x, channels, d.inv_s, d.m)
            ops.image_metrics_accumulate(sse_u8, ssim, self._state[-2:-1], self._state[-1:].view(torch.float64))
        if return_u8:
            d = self.denormalizer
            return ops.nhwc_to_u8(dec, channels, d.inv_s, d.m, d.layout if u8 else "chw")
        return None

    def result(self):
        state = self._state
        if state is None:       # no batch yet: empty totals (a rank whose share of the data is empty still joins the sums)
            dev = next(self.model.parameters()).device
            state = self._state = torch.zeros(self._state_len(), device=dev, dtype=torch.int64)
        ints = len(state) - 1 if self.image_metrics else len(state)     # the SSIM total is the last word, a double
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            state = state.clone()
            dist.all_reduce(state[:4].view(torch.float64))       # the four totals, float64
            dist.all_reduce(state[4:ints])                       # both histograms, the flag (and the squared bytes), int64
            if self.image_metrics:
                dist.all_reduce(state[ints:].view(torch.float64))
        host = state.cpu()
        acc = host[:4].view(torch.float64)
        counts_t, counts_b = host[4:4 + self.k_t].clone(), host[4 + self.k_t:4 + self.k_t + self.k_b].clone()
        if int(host[4 + self.k_t + self.k_b]) != 0:
            raise RuntimeError("Evaluator: a quantizer produced a code index outside [0, n_embed) (vq2_index_hist flag)")
        images = int(acc[3])
        out = {"mse": float(acc[0] / acc[1]) if images else float("nan"),
               "latent": float(acc[2] / acc[3]) if images else float("nan"),
               "images": images,
               "perplexity_t": perplexity_from_counts(counts_t), "perplexity_b": perplexity_from_counts(counts_b),
               "used_t": int((counts_t > 0).sum()), "used_b": int((counts_b > 0).sum()),
               "n_embed": self.k_t if self.k_t == self.k_b else (self.k_t, self.k_b), "counts_t": counts_t, "counts_b": counts_b}
        if self.image_metrics:
            nan = float("nan")
            mse_u8 = int(host[-2]) / float(acc[1]) if images else nan
            out["mse_u8"] = mse_u8
            out["psnr"] = psnr_from_mse_u8(mse_u8) if images else nan
            out["ssim"] = float(host[-1:].view(torch.float64)[0] / acc[3]) if images else nan
        return out


def _prior_forward(model, codes, condition, label=None):
    """The logits of an eval-mode forward as the NHWC tensor the row kernels read in place, and the targets' device copy.
    Eval mode draws no dropout seed (p == 0 at every site of pixelsnail.py) and no_grad keeps every gradient slot as it
    is; outside a trainer's step each layer forms its effective weight from the parameters as they are now."""
    ops._require_codes(codes, "codes")
    with eval_mode(model), torch.no_grad():
        kw = {} if condition is None else {"condition": condition}
        if label is not None:       # (a model built with n_label > 0 raises without it, one built without raises with it)
            kw["label"] = label
        out, _ = model(codes, **kw)
        return ops.to_nhwc(out)


class PriorEvaluator:
    """Held-out likelihood of a PixelSNAIL prior: the counterpart of PriorSampler(..., return_logp=True) for GIVEN codes.

    model: a PixelSNAIL; hier 'top' (the model sees the top codes) or 'bottom' (the bottom codes, conditioned on the top
    ones), as Stage2Trainer; top_k: the k of top_k_accuracy (clamped to n_class).

    update(top, bottom=None, return_image_nll=False)
                  one batch of int64 codes on the GPU: eval-mode forward under no_grad, then three launches on the logits
                  where they are -- vq2_prior_eval_rows (per pixel: cross-entropy term, predictive entropy, rank of the
                  target), vq2_prior_eval_accumulate (per-position running totals, no atomics) and one vq2_index_hist of
                  the targets.  Nothing is read back.  return_image_nll=True returns the float32 [B] device tensor of each
                  image's summed negative log-likelihood in nats.  Every module's train / eval flag is restored.
    update_labelled(label, top, bottom=None, return_image_nll=False)
                  update() for a class-conditional model (PixelSNAIL(..., n_label > 0)): label is int64 [B] on the GPU.
    result()      ONE device-to-host copy -> {"nll" (nats per code), "bits_per_code", "perplexity", "accuracy",
                  "top_k_accuracy", "top_k", "entropy" (mean predictive entropy, nats), "unigram_nll" (the entropy of the
                  target histogram: what the best context-free model reaches, the baseline a prior has to beat), "images",
                  "codes", "nll_map" (float64 CPU [H,W], mean nll per position), "nll_rows" (its H row means), "counts"}.
                  With a process group the float64 and the int64 section of the state are summed over the ranks first, on
                  a clone.  Raises RuntimeError if a target was outside [0, n_class).  No batch seen: NaNs and zeros.
    reset()       clears the accumulators.

    The state is one int64 buffer (doubles as bits): [pos_nll (L) | pos_entropy (L) | pos_hit1 (L) | pos_hitk (L) | images |
    bad | target counts (n_class) | hist flag], L = H * W of the first batch; a later batch of another map size raises
    ValueError.  Each position's total is a running fp64 sum in batch order, so the state does not depend on how a set of
    images was cut into batches."""

    def __init__(self, model, hier, top_k=5):
        if hier not in ("top", "bottom"):
            raise ValueError(f"PriorEvaluator: hier must be 'top' or 'bottom', got {hier!r}")
        if int(top_k) < 1:
            raise ValueError(f"PriorEvaluator: top_k must be >= 1, got {top_k}")
        self.model, self.hier = model, hier
        self.n_class = int(model.n_class)
        self.top_k = min(int(top_k), self.n_class)
        self.shape = None
        self._state = None

    @staticmethod
    def state_len(length, n_class):
        return 4 * length + 2 + n_class + 1

    def _buffers(self, device, shape):
        if self._state is None or self._state.device != device:
            self.shape = tuple(shape)
            self._state = torch.zeros(self.state_len(shape[0] * shape[1], self.n_class), device=device, dtype=torch.int64)
        s, n = self._state, self.shape[0] * self.shape[1]
        return (s[:n].view(torch.float64), s[n:2 * n].view(torch.float64), s[2 * n:3 * n], s[3 * n:4 * n], s[4 * n:4 * n + 2],
                s[4 * n + 2:4 * n + 2 + self.n_class], s[-1:].view(torch.int32)[:1])

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def update(self, top, bottom=None, return_image_nll=False):
        return self.update_labelled(None, top, bottom, return_image_nll)

    def update_labelled(self, label, top, bottom=None, return_image_nll=False):
        if self.hier == "top":
            target, condition = top, None
        else:
            if bottom is None:
                raise TypeError("PriorEvaluator(hier='bottom').update needs the bottom codes")
            target, condition = bottom, top
        if target.dim() != 3:
            raise RuntimeError("PriorEvaluator.update: codes [B,H,W] expected")
        if self._state is not None and tuple(target.shape[1:]) != self.shape:
            raise ValueError(f"PriorEvaluator: a batch of {tuple(target.shape[1:])} code maps after batches of {self.shape}")
        x = _prior_forward(self.model, target, condition, label)
        pos_nll, pos_entropy, hit1, hitk, counters, counts, flag = self._buffers(x.device, target.shape[1:])
        nll, entropy, rank = ops.prior_eval_rows(x, target, self.n_class)
        image_nll = ops.prior_eval_accumulate(nll, entropy, rank, target.shape[0], self.top_k, pos_nll, pos_entropy, hit1, hitk,
                                              counters, return_image_nll)
        ops.index_hist(target, counts, flag)
        return image_nll

    @staticmethod
    def finish(host, shape, n_class, top_k):
        """The fp64 host finish of result() on a CPU copy of the state buffer."""
        h, w = shape
        n = h * w
        if host.numel() != PriorEvaluator.state_len(n, n_class):
            raise ValueError(f"PriorEvaluator: a state of {host.numel()} words for {h} x {w} positions and {n_class} classes")
        pos_nll, pos_entropy = host[:n].view(torch.float64), host[n:2 * n].view(torch.float64)
        hit1, hitk = host[2 * n:3 * n], host[3 * n:4 * n]
        images, bad = int(host[4 * n]), int(host[4 * n + 1])
        counts = host[4 * n + 2:4 * n + 2 + n_class].clone()
        if bad != 0 or int(host[-1]) != 0:
            raise RuntimeError(f"PriorEvaluator: {bad} target codes outside [0, {n_class}) "
                               "(vq2_prior_eval_rows rank -1 / vq2_index_hist flag)")
        top_k = min(int(top_k), n_class)
        codes = images * n
        nan = float("nan")
        total_nll = total_entropy = 0.0
        for v in pos_nll.tolist():          # positions ascending
            total_nll += v
        for v in pos_entropy.tolist():
            total_entropy += v
        nll = total_nll / codes if codes else nan
        nll_map = (pos_nll / images if images else torch.full((n,), nan, dtype=torch.float64)).reshape(h, w).clone()
        perplexity = perplexity_from_counts(counts)
        return {"nll": nll, "bits_per_code": nll / math.log(2.0), "perplexity": math.exp(nll) if codes else nan,
                "accuracy": int(hit1.sum()) / codes if codes else nan,
                "top_k_accuracy": int(hitk.sum()) / codes if codes else nan, "top_k": top_k,
                "entropy": total_entropy / codes if codes else nan,
                "unigram_nll": math.log(perplexity) if codes else nan,
                "images": images, "codes": codes, "nll_map": nll_map,
                "nll_rows": [float(v) for v in nll_map.mean(1)] if w else [], "counts": counts}

    @staticmethod
    def summary(r):
        """One line of the scalars of a result()."""
        return (f"images: {r['images']}; codes: {r['codes']}; nll: {r['nll']:.6f}; bits/code: {r['bits_per_code']:.6f}; "
                f"perplexity: {r['perplexity']:.4f}; acc: {r['accuracy']:.6f}; top{r['top_k']}: {r['top_k_accuracy']:.6f}; "
                f"entropy: {r['entropy']:.6f}; unigram nll: {r['unigram_nll']:.6f}")

    def result(self):
        state = self._state
        if state is None:       # no batch yet: empty totals of the model's own map (a rank with no data still joins the sums)
            bg = getattr(self.model, "background", None)
            self.shape = tuple(bg.shape[2:]) if bg is not None else (0, 0)
            dev = next(self.model.parameters()).device
            state = self._state = torch.zeros(self.state_len(self.shape[0] * self.shape[1], self.n_class), device=dev,
                                              dtype=torch.int64)
        n = self.shape[0] * self.shape[1]
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            state = state.clone()
            if n:
                dist.all_reduce(state[:2 * n].view(torch.float64))      # the per-position totals, float64
            dist.all_reduce(state[2 * n:])                              # hits, images, bad, histogram, flag: int64
        return self.finish(state.cpu(), self.shape, self.n_class, self.top_k)


def score_codes(model, codes, condition=None):
    """Log-likelihood of each code map under a PixelSNAIL prior, in nats: float32 [B] on the GPU, minus the per-image sum
    of the cross-entropy terms (PriorEvaluator's image nll), from an eval-mode forward under no_grad.  codes int64 [B,H,W];
    condition: the top codes [B,H/2,W/2] for a bottom prior.  A code outside [0, n_class) adds nothing to its image's
    score, as in prior_loss.  Nothing is read back."""
    return score_codes_labelled(model, codes, None, condition)


def score_codes_labelled(model, codes, label, condition=None):
    """score_codes for a class-conditional model: label is int64 [B] on the GPU (None: score_codes itself)."""
    if codes.dim() != 3:
        raise RuntimeError("score_codes: codes [B,H,W] expected")
    x = _prior_forward(model, codes, condition, label)
    b, length = codes.shape[0], codes.shape[1] * codes.shape[2]
    nll, entropy, rank = ops.prior_eval_rows(x, codes, int(model.n_class))
    state = torch.zeros(4 * length + 2, device=x.device, dtype=torch.int64)
    f = state[:2 * length].view(torch.float64)
    image_nll = ops.prior_eval_accumulate(nll, entropy, rank, b, 1, f[:length], f[length:], state[2 * length:3 * length],
                                          state[3 * length:4 * length], state[4 * length:], True)
    return -image_nll
