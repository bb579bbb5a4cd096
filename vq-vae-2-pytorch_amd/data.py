"""The input half of the training loop for 8-bit images: what the reference's loader does on host workers
(train_vqvae.py:149-155, 199-201; extract_code.py:47-57) -- ToTensor, Normalize, CenterCrop and
`img.to(device)` once per step -- with the arithmetic on the GPU and the transfer off the step's critical path.

ImageNormalizer      uint8 batch on the device -> normalised fp32 in the kernels' NHWC4 layout, one launch
ImageDenormalizer    the way back (train_vqvae.py:22-25, 133-139): normalised fp32 -> uint8 batch or sample grid, one launch
HostBatchPrefetcher  host uint8 batches -> device uint8 batches through pinned memory on a copy stream
"""
import collections
import itertools
import queue
import threading

import numpy as np
import torch

from . import ops


class ImageNormalizer:
    """`ToTensor()` + `Normalize(mean, std)` (+ `CenterCrop(crop)`) of the reference's loader for uint8 batches that
    already sit on the GPU, fused with the conversion to the internal layout (vq2_u8_to_nhwc4).

    A byte has 256 values, so the normalisation is a table per channel, built here with the very fp32 operations the
    reference executes -- `v.float().div(255)` (ToTensor) then `.sub(mean[c]).div(std[c])` with fp32 mean / std
    (Normalize) -- and the kernel only looks values up: the result is bit-identical to that loader for any mean / std.

    layout  "hwc": batches are [N,Hs,Ws,C] (what image decoders produce); "chw": [N,C,Hs,Ws]
    crop    (H, W): the centred window CenterCrop takes, origin y0 = int(round((Hs - H) / 2.0)) and
            x0 = int(round((Ws - W) / 2.0)) as torchvision computes it (Python's round: halves go to the even
            neighbour); None: the whole image.  Resizing stays on the host, as in the reference.

    norm(img) -> NHWC4 fp32 [N,H,W,4] (what ops.to_nhwc gives for a float image; Stage1Trainer.step takes it from
    here); norm.nchw(img) -> the NCHW-shaped fp32 batch [N,C,H,W] the drop-in modules take.  No CPU path."""

    def __init__(self, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), layout="hwc", crop=None):
        if layout not in ops.U8_LAYOUTS:
            raise ValueError(f"layout must be 'hwc' or 'chw', not {layout!r}")
        mean, std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        if len(mean) != len(std) or not 1 <= len(mean) <= 4:
            raise ValueError("mean and std need one entry per channel, 1 to 4 channels")
        if any(s == 0.0 for s in std):
            raise ValueError("std must be non-zero")   # (Normalize refuses it as well)
        if crop is not None:
            crop = (int(crop[0]), int(crop[1]))
            if len(crop) != 2 or min(crop) < 1:
                raise ValueError("crop must be (H, W) with positive sizes")
        self.layout, self.crop, self.channels = layout, crop, len(mean)
        self.mean, self.std = mean, std
        v = torch.arange(256, dtype=torch.uint8).float().div(255)                              # ToTensor
        m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
        self.table = v.unsqueeze(0).repeat(len(mean), 1).sub_(m[:, None]).div_(s[:, None])    # Normalize; [C,256]
        self._device_tables = {}

    @staticmethod
    def crop_origin(source, size):
        """First row (column) of CenterCrop's window of `size` in a side of `source` pixels."""
        return int(round((source - size) / 2.0))

    def box(self, hs, ws):
        """(y0, x0, H, W) of the window taken from an Hs x Ws image."""
        if self.crop is None:
            return 0, 0, hs, ws
        h, w = self.crop
        if h > hs or w > ws:
            raise ValueError(f"crop {h}x{w} is larger than the {hs}x{ws} image")   # (CenterCrop would pad; not supported)
        return self.crop_origin(hs, h), self.crop_origin(ws, w), h, w

    def table_on(self, device):
        t = self._device_tables.get(device)
        if t is None:
            t = self._device_tables[device] = self.table.to(device)
        return t

    def out_shape(self, img):
        """Logical NCHW shape of the normalised (cropped) batch."""
        hs, ws = (img.shape[1], img.shape[2]) if self.layout == "hwc" else (img.shape[2], img.shape[3])
        _, _, h, w = self.box(hs, ws)
        return img.shape[0], self.channels, h, w

    def __call__(self, img):
        if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dtype != torch.uint8:
            raise RuntimeError(f"ImageNormalizer: expected a uint8 tensor on the MI355X (got "
                               f"{getattr(img, 'dtype', type(img))} on {getattr(img, 'device', '?')}); no CPU path")
        if img.dim() != 4 or not img.is_contiguous():
            raise RuntimeError("ImageNormalizer: expected a contiguous 4-D batch")
        c = img.shape[3] if self.layout == "hwc" else img.shape[1]
        if c != self.channels:
            raise RuntimeError(f"ImageNormalizer: batch of shape {tuple(img.shape)} has {c} channels in layout "
                               f"'{self.layout}', the statistics cover {self.channels}")
        hs, ws = (img.shape[1], img.shape[2]) if self.layout == "hwc" else (img.shape[2], img.shape[3])
        return ops.u8_to_nhwc4(img, self.table_on(img.device), self.layout, self.box(hs, ws))

    def nchw(self, img):
        return ops.from_nhwc(self(img), self.channels)

    def inverse(self):
        """The ImageDenormalizer of the same statistics and layout (cropping has no inverse: it yields the cropped size)."""
        return ImageDenormalizer(self.mean, self.std, self.layout)


def grid_layout(n, h, w, nrow=8, padding=2):
    """Geometry of torchvision's make_grid for n images of h x w: (canvas height, canvas width, [(y, x) origin of every
    image]).  Image k sits in cell (k // cols, k % cols) with cols = min(nrow, n); cells are (h + padding) x
    (w + padding) and the canvas has one more `padding` at its bottom and right.  A single image is returned as it is,
    without any border (make_grid's early return).  Pure host arithmetic."""
    n, h, w, nrow, padding = int(n), int(h), int(w), int(nrow), int(padding)
    if n < 1 or h < 1 or w < 1 or nrow < 1 or padding < 0:
        raise ValueError("grid_layout: n, h, w and nrow must be positive and padding non-negative")
    if n == 1:
        return h, w, [(0, 0)]
    cols = min(nrow, n)
    rows = (n + cols - 1) // cols
    origins = [((k // cols) * (h + padding) + padding, (k % cols) * (w + padding) + padding) for k in range(n)]
    return rows * (h + padding) + padding, cols * (w + padding) + padding, origins


def save_u8_image(canvas, path, layout="hwc"):
    """Write a uint8 canvas ([H,W,C] for "hwc", [C,H,W] for "chw"; C = 1, 3 or 4; device or host) as a PNG at `path`
    with PIL where it is importable; otherwise the same array goes to `path` with the extension .npy and a message says
    so.  Returns the path written.  (One device-to-host copy; encoding stays on the host.)"""
    a = canvas.detach().cpu().numpy() if isinstance(canvas, torch.Tensor) else np.asarray(canvas)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError("save_u8_image: a 3-D uint8 canvas expected")
    if layout == "chw":
        a = a.transpose(1, 2, 0)
    elif layout != "hwc":
        raise ValueError(f"layout must be 'hwc' or 'chw', not {layout!r}")
    a = np.ascontiguousarray(a)
    try:
        from PIL import Image
    except ImportError:
        alt = path.rsplit(".", 1)[0] + ".npy"
        np.save(alt, a)
        print(f"PIL is not importable: wrote the canvas as {alt} instead of {path}")
        return alt
    Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).save(path)
    return path


class ImageDenormalizer:
    """Normalised fp32 images -> 8-bit pixels on the GPU (vq2_nhwc_to_u8): the reference's `invTrans`
    (train_vqvae.py:22-25: Normalize(0, 1 / std) then Normalize(-mean, 1)) followed by what torchvision's save_image does
    to a float image (`mul(255).add_(0.5).clamp_(0, 255).to(uint8)`, train_vqvae.py:133-139), in that order and in fp32:

        byte = trunc(clamp((x / inv_s[c] + m[c]) * 255 + 0.5, 0, 255)),  inv_s[c] = fp32(1 / std[c]),  m[c] = fp32(mean[c])

    (the `sub(0)` and `div(1)` of the two stages change nothing, and t - (-m) is t + m).  NaN gives 0.  For the
    statistics the examples ship this maps every value of ImageNormalizer's table back to its byte.

    layout  of the RESULT: "hwc" [N,H,W,C] (what image encoders take) or "chw" [N,C,H,W]
    denorm(x)           x: an internal NHWC tensor [N,H,W,ceil4(C)] (pass nhwc=True where the shape could be read
                        either way) or an NCHW-shaped module output [N,C,H,W]  ->  uint8 batch
    denorm.grid(batches, nrow, padding=2, pad_value=0)   make_grid + the same conversion: ONE uint8 canvas
                        ([Hc,Wc,C] or [C,Hc,Wc]) holding the images of all batches in order.  No CPU path."""

    def __init__(self, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), layout="hwc"):
        if layout not in ops.U8_LAYOUTS:
            raise ValueError(f"layout must be 'hwc' or 'chw', not {layout!r}")
        mean, std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        if len(mean) != len(std) or not 1 <= len(mean) <= 4:
            raise ValueError("mean and std need one entry per channel, 1 to 4 channels")
        if any(s == 0.0 for s in std):
            raise ValueError("std must be non-zero")
        self.layout, self.channels, self.mean, self.std = layout, len(mean), mean, std
        # what Normalize makes of its arguments: torch.as_tensor(python double, dtype=float32)
        self.inv_s = tuple(float(np.float32(1.0 / s)) for s in std)
        self.m = tuple(float(np.float32(m)) for m in mean)

    def _nhwc(self, x, nhwc=None):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            raise RuntimeError(f"ImageDenormalizer: expected a 4-D float32 tensor on the MI355X (got "
                               f"{getattr(x, 'dtype', type(x))} on {getattr(x, 'device', '?')}); no CPU path")
        c = self.channels
        as_nhwc, as_nchw = x.shape[3] == ops.ceil4(c), x.shape[1] == c
        if nhwc is None:
            if as_nhwc and as_nchw:
                raise RuntimeError(f"ImageDenormalizer: a tensor of shape {tuple(x.shape)} reads as NHWC and as NCHW; "
                                   "pass nhwc=True or nhwc=False")
            nhwc = as_nhwc
        if nhwc:
            if not as_nhwc:
                raise RuntimeError(f"ImageDenormalizer: NHWC input of shape {tuple(x.shape)} for {c} channels")
            return ops.as_nhwc(x.detach())
        if not as_nchw:
            raise RuntimeError(f"ImageDenormalizer: input of shape {tuple(x.shape)} is neither [N,H,W,{ops.ceil4(c)}] "
                               f"nor [N,{c},H,W]")
        return ops.to_nhwc(x.detach())

    def __call__(self, x, nhwc=None):
        return ops.nhwc_to_u8(self._nhwc(x, nhwc), self.channels, self.inv_s, self.m, self.layout)

    def grid(self, batches, nrow=8, padding=2, pad_value=0, nhwc=None):
        if isinstance(batches, torch.Tensor):
            batches = [batches]
        xs = [self._nhwc(b, nhwc) for b in batches]
        if not xs or any(x.shape[1:3] != xs[0].shape[1:3] or x.device != xs[0].device for x in xs):
            raise RuntimeError("ImageDenormalizer.grid: one or more batches of images of one size on one GPU expected")
        n, (h, w), c = sum(x.shape[0] for x in xs), xs[0].shape[1:3], self.channels
        hc, wc, _ = grid_layout(n, h, w, nrow, padding)
        cols, pad = (1, 0) if n == 1 else (min(int(nrow), n), int(padding))
        shape = (hc, wc, c) if self.layout == "hwc" else (c, hc, wc)
        canvas = torch.full(shape, int(pad_value), device=xs[0].device, dtype=torch.uint8)
        if len(xs) > 1:     # cells are numbered through all batches: one launch needs them in one tensor
            cp, k = xs[0].shape[3], 0
            joined = torch.empty((n, h, w, cp), device=xs[0].device, dtype=torch.float32)
            for x in xs:
                ops.check(ops.lib.vq2_slice_copy(ops._p(x), ops.ld_of(x), ops._p(joined[k:]), cp, x.shape[0] * h * w, cp, 0,
                                                 ops._stream()), "slice_copy")
                k += x.shape[0]
            xs = [joined]
        return ops.nhwc_to_u8(xs[0], c, self.inv_s, self.m, self.layout, canvas=canvas, cols=cols, pad=pad)


class HostBatchPrefetcher:
    """Iterator over host uint8 batches (numpy arrays or CPU tensors, all of one shape) that yields them as device
    uint8 tensors, the transfer of the next batches running on a copy stream while the consumer works on this one:
    a ring of `depth` pinned staging buffers and `depth` device buffers, one copy per batch.

    Stream ordering (no device or stream synchronise anywhere):
      * `__next__` makes the consumer's stream -- torch.cuda.current_stream() looked up AT THAT CALL, so a
        Stage1Trainer that installed its high-priority stream before or after this object was built is served alike --
        wait for the slot's copy event, and returns the slot's device buffer;
      * the tensor returned is the consumer's until its next `__next__` (or the end of the iteration): there an event
        is recorded on the consumer's current stream, and the copy that refills the slot waits for that event.  Work
        the consumer queued on the batch on OTHER streams must be ordered before that call by the consumer;
      * the one host wait: a pinned buffer is handed back for refilling after `synchronize()` on its own copy event
        (with depth >= 2 that copy finished long before).
    Filling the pinned buffers (a host memcpy, possibly out of an mmap) runs on one worker thread; every GPU call is
    issued from the thread that iterates.  `close()` (also on exhaustion, on an error and on leaving a `with` block)
    joins the worker; an exception raised by the source surfaces from `__next__`, after the batches before it."""

    def __init__(self, batches, device, depth=2):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("HostBatchPrefetcher: the destination must be a GPU; this package has no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if int(depth) < 1:
            raise ValueError("depth must be >= 1")
        self.depth = int(depth)
        self._source = iter(batches)
        self._started = self._source_done = self._closed = False
        self._error = None
        self._worker = None
        self._free_q, self._filled_q = queue.SimpleQueue(), queue.SimpleQueue()
        self._ready = collections.deque()     # slots whose copy is in flight or done, oldest first
        self._held = None                     # slot the consumer works on

    # ------------------------------------------------------------------ worker thread: host memory only
    @staticmethod
    def _as_array(item):
        a = item.numpy() if isinstance(item, torch.Tensor) else np.asarray(item)
        if a.dtype != np.uint8:
            raise TypeError(f"HostBatchPrefetcher: host batches must be uint8, got {a.dtype}")
        return a

    def _fill(self, source):
        try:
            for item in source:
                k = self._free_q.get()
                if k is None:                 # closed
                    return
                a = self._as_array(item)
                if a.shape != self._shape:
                    raise ValueError(f"HostBatchPrefetcher: batch of shape {a.shape} after batches of {self._shape}")
                np.copyto(self._pinned_np[k], a)
                self._filled_q.put(("batch", k))
            self._filled_q.put(("end", None))
        except BaseException as e:            # surfaces from __next__
            self._filled_q.put(("error", e))

    # ------------------------------------------------------------------ consuming thread: every GPU call
    def _start(self):
        self._started = True
        try:
            first = next(self._source)
        except StopIteration:
            self._source_done = True
            return
        self._shape = self._as_array(first).shape
        with torch.cuda.device(self.device):
            self._copy_stream = torch.cuda.Stream()
        self._pinned = [torch.empty(self._shape, dtype=torch.uint8, pin_memory=True) for _ in range(self.depth)]
        self._pinned_np = [t.numpy() for t in self._pinned]
        self._dev = [torch.empty(self._shape, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
        for t in self._dev:
            t.record_stream(self._copy_stream)
        self._copy_done = [torch.cuda.Event() for _ in range(self.depth)]
        self._released = [None] * self.depth
        for k in range(self.depth):
            self._free_q.put(k)
        self._worker = threading.Thread(target=self._fill, args=(itertools.chain([first], self._source),),
                                        name="vq2-prefetch", daemon=True)
        self._worker.start()

    def _release_held(self):
        """The consumer is done ISSUING work on the slot it holds: mark that point on its stream, give the staging
        buffer back to the worker."""
        k, self._held = self._held, None
        if k is None:
            return
        self._released[k] = torch.cuda.current_stream(self.device).record_event()
        self._copy_done[k].synchronize()      # the copy that read pinned[k]; the consumer's stream waited for it long ago
        self._free_q.put(k)

    def _pump(self):
        """Start the copy of every batch the worker has finished; block for one only when nothing is in flight."""
        while not self._source_done:
            try:
                kind, val = self._filled_q.get() if not self._ready else self._filled_q.get_nowait()
            except queue.Empty:
                return
            if kind == "batch":
                if self._released[val] is not None:          # the device buffer's previous consumer
                    self._copy_stream.wait_event(self._released[val])
                with torch.cuda.stream(self._copy_stream):
                    self._dev[val].copy_(self._pinned[val], non_blocking=True)
                    self._copy_done[val].record(self._copy_stream)
                self._ready.append(val)
            else:
                self._source_done = True
                self._error = val

    def __iter__(self):
        return self

    def __next__(self):
        if self._closed:
            raise StopIteration
        if not self._started:
            try:
                self._start()
            except BaseException:
                self.close()
                raise
        self._release_held()
        self._pump()
        if not self._ready:
            err, self._error = self._error, None
            self.close()
            if err is not None:
                raise err
            raise StopIteration
        k = self._ready.popleft()
        stream = torch.cuda.current_stream(self.device)
        stream.wait_event(self._copy_done[k])
        self._dev[k].record_stream(stream)
        self._held = k
        return self._dev[k]

    def close(self):
        """Stop the worker and join it.  Device tensors already handed out stay valid."""
        if self._closed:
            return
        self._closed = True
        if self._worker is not None:
            self._free_q.put(None)
            self._worker.join()
            self._worker = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
