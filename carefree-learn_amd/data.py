"""Input path: `TensorBatcher` with the host-to-device copy off the step's critical path.

The reference's batcher (data/utils.py:255-283) converts every numpy batch to torch tensors and calls a
synchronous `.to(device)` inside `__next__`, i.e. on the compute stream, inside the training step's critical path
(trainer.py:314,333,580).  Same interface here (`__len__`, `__iter__`, `__next__`, `to`, `get_one_batch`,
`get_full_batch`; dict batches, float arrays -> float32, integer arrays -> int64, strings untouched — the
`np_batch_to_tensor` / `cftool.array.to_torch` rules, toolkit.py:1182-1207), but the copy of batch i+1 is issued
on a dedicated HIP stream while the kernels of batch i run, into a ring of pre-allocated device buffers (nothing is
allocated in the steady state; a batch stays valid until the next `__next__`), and `__next__` only makes the compute
stream wait on the copy's event.  With device=None / "cpu" it degrades to the reference behaviour.

Measured on the MI355X box (tools/feed_probe.py, ViT-B/16 batch 128 = 77 MB per batch, PCIe ~50 GB/s): a producer
THREAD with pinned staging buffers — the textbook design — tripled the host's launch time through GIL contention
(46 ms/step against 24 ms resident), so the copy is issued from the consumer thread, straight from the pageable
numpy memory: the driver's own staging path moves it in ~1.6 ms.

`ImageBatcher` (below) is the same batcher for uint8 image batches: the batch crosses PCIe as uint8 HWC, a quarter of the
float32 bytes, and `DeviceImageTransform`'s crop, resize, flip, normalisation and HWC -> CHW transpose run as one HIP launch
(csrc/image.hip) on the copy stream, in front of the event `__next__` waits on.  Measured at the ViT batch
(tools/image_feed_bench.py, profiles/r16/image_feed_ab.txt): 1.16 ms per batch against 2.69 ms for the float32 copy.
"""
import collections
from typing import Any, Dict, Iterator, List, Optional

import numpy as np
import torch
from torch import Tensor


def _to_tensor(v: Any) -> Any:
    """cftool.array.to_torch semantics: floating -> float32, integer / bool -> int64, strings untouched"""
    if isinstance(v, Tensor):
        return v
    if not isinstance(v, np.ndarray) or v.dtype.kind in ("U", "S", "O"):
        return v
    if v.dtype.kind == "f":
        return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64))


class TensorBatcher:
    def __init__(self, loader: Any, device: Any = None, *, depth: int = 1):
        self.loader = loader
        self.depth = max(1, int(depth))  # batches in flight ahead of the consumer
        self.to(device)
        self._dev_slots: List[Dict[str, Tensor]] = []  # device destinations, per ring slot
        self._free_events: Dict[int, Any] = {}         # compute stream is past the work that used the slot's batch
        self._pending: "collections.deque" = collections.deque()
        self._in_use: Optional[int] = None
        self._slot = 0
        self._exhausted = False
        self._copy_stream: Optional[torch.cuda.Stream] = None

    # -- reference interface ------------------------------------------------------------------------
    def __len__(self) -> int:
        return len(self.loader)

    def to(self, device: Any) -> None:
        if device is None:
            device = "cpu"
        if isinstance(device, int):
            device = f"cuda:{device}"
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

    def __iter__(self) -> "TensorBatcher":
        self._it: Iterator = iter(self.loader)
        self._pending.clear()
        self._exhausted = False
        if self.device.type == "cuda":
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(self.device)
            for _ in range(self.depth):
                self._prefetch()
        return self

    def __next__(self) -> Dict[str, Any]:
        if self.device.type != "cuda":
            return {k: _to_tensor(v) for k, v in next(self._it).items()}
        if not self._pending:
            raise StopIteration
        batch, event, slot = self._pending.popleft()
        cur = torch.cuda.current_stream(self.device)
        if self._in_use is not None:
            # everything enqueued so far used the PREVIOUS batch: once the compute stream is past this point its
            # ring slot may be overwritten by the copy stream
            freed = torch.cuda.Event()
            freed.record(cur)
            self._free_events[self._in_use] = freed
        self._in_use = slot
        cur.wait_event(event)
        self._prefetch()  # batch i + depth goes out while the caller launches the kernels of batch i
        return batch

    def get_one_batch(self) -> Dict[str, Any]:
        return self._sync_copy(self.loader.get_one_batch())

    def get_full_batch(self) -> Dict[str, Any]:
        return self._sync_copy(self.loader.get_full_batch())

    # -- internals ------------------------------------------------------------------------------------
    def _sync_copy(self, npd: Dict[str, Any]) -> Dict[str, Any]:
        return {k: (t.to(self.device) if isinstance(t, Tensor) else t)
                for k, t in ((k, _to_tensor(v)) for k, v in npd.items())}

    def _device_buf(self, slot: int, key: str, like: Tensor) -> Tensor:
        """pre-allocated destination of this slot / key (re-allocated when the batch shape changes, e.g. the
        ragged last batch of an epoch)"""
        while len(self._dev_slots) <= slot:
            self._dev_slots.append({})
        buf = self._dev_slots[slot].get(key)
        if buf is None or buf.shape != like.shape or buf.dtype != like.dtype:
            buf = torch.empty(like.shape, dtype=like.dtype, device=self.device)
            self._dev_slots[slot][key] = buf
        return buf

    def _prefetch(self) -> None:
        if self._exhausted:
            return
        try:
            npd = next(self._it)
        except StopIteration:
            self._exhausted = True
            return
        slot = self._slot
        self._slot = (self._slot + 1) % (self.depth + 2)  # `depth` queued + one in use + one being filled
        batch: Dict[str, Any] = {}
        with torch.cuda.stream(self._copy_stream):
            freed = self._free_events.pop(slot, None)
            if freed is not None:
                self._copy_stream.wait_event(freed)  # GPU-side: the consumer of this slot's last batch is done
            for k, v in npd.items():
                t = _to_tensor(v)
                if not isinstance(t, Tensor) or t.is_cuda:
                    batch[k] = t
                    continue
                dst = self._device_buf(slot, k, t)
                dst.copy_(t, non_blocking=True)
                batch[k] = dst
            event = torch.cuda.Event()
            event.record(self._copy_stream)
        self._pending.append((batch, event, slot))


# ---------------------------------------------------------------------------------------------------------
# The uint8 image input path: the batch crosses PCIe as uint8 HWC and becomes the model's f32 / bf16 NCHW tensor in one
# HIP launch on the copy stream (csrc/image.hip, cfhip_image_transform).  Replaces the per-item CPU blocks of the
# reference's data/blocks/cv/: resize.py, crop.py, normalize.py and hwc_to_chw.py.
# ---------------------------------------------------------------------------------------------------------
INPUT_KEY = "input"  # the reference's constants.INPUT_KEY

_MODES = ("resize", "center_crop", "random_resized_crop")


class DeviceImageTransform:
    """out[b, c] = normalize_c(resize(crop(flip(image_b)))): one crop box per sample (drawn on the host), resized to `size` by the
    sampling rule of include/cfhip.h (half-pixel centres, replicate border; not cv2's fixed point), mirrored with probability `flip`,
    then value * a[c] + b[c] with the normalisation folded into a, b.

    normalize: ("static", division) = static_normalize; ("affine", center, scale) = static_normalize(255) then affine_normalize;
    ("imagenet", mean, std) = static_normalize(255) then imagenet_normalize; None = the raw 0 .. 255 values.
    mode: "resize" = the whole image; "center_crop" = the centred box of `size` source pixels (no resampling when it lies on the pixel
    grid); "random_resized_crop" = a box of relative area in `scale` and aspect ratio w / h log-uniform in `ratio`, placed uniformly
    inside the image (ten tries, then the largest centred box whose ratio is allowed).  Box sizes are fractional: area and ratio are
    met exactly, not after rounding to pixels.
    Boxes and flips come from numpy.random.default_rng((seed, epoch, batch_index)): a run is reproducible and a resumed run (set the
    epoch, skip batches) draws the same boxes.  for_inference=True: no flip, and random_resized_crop becomes center_crop."""

    def __init__(self, size, *, mode: str = "resize", scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip: float = 0.0,
                 interpolation: str = "bilinear", normalize=("static", 255.0), out_dtype: torch.dtype = torch.float32, seed: int = 0,
                 for_inference: bool = False):
        self.size = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        if min(self.size) < 1:
            raise ValueError(f"DeviceImageTransform: size {self.size}")
        if mode not in _MODES:
            raise ValueError(f"DeviceImageTransform: mode {mode!r} (one of {_MODES})")
        if interpolation not in ("bilinear", "nearest"):
            raise ValueError(f"DeviceImageTransform: interpolation {interpolation!r} ('bilinear' or 'nearest'; antialiased / area "
                             "resampling is not built)")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"DeviceImageTransform: out_dtype {out_dtype} (float32 or bfloat16)")
        if not (0.0 < scale[0] <= scale[1] <= 1.0) or not (0.0 < ratio[0] <= ratio[1]):
            raise ValueError(f"DeviceImageTransform: scale {scale} must lie in (0, 1], ratio {ratio} must be positive, both ascending")
        if not 0.0 <= flip <= 1.0:
            raise ValueError(f"DeviceImageTransform: flip probability {flip}")
        if normalize is not None and (len(normalize) < 2 or normalize[0] not in ("static", "affine", "imagenet")
                                      or len(normalize) != (2 if normalize[0] == "static" else 3)):
            raise ValueError(f"DeviceImageTransform: normalize {normalize!r}: ('static', division), ('affine', center, scale), "
                             "('imagenet', mean, std) or None")
        self.mode = "center_crop" if for_inference and mode == "random_resized_crop" else mode
        self.flip = 0.0 if for_inference else float(flip)
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.interpolation, self.normalize, self.out_dtype, self.seed = interpolation, normalize, out_dtype, int(seed)
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def scale_bias(self, channels: int) -> List[List[float]]:
        """per-channel (a, b) of out = value * a + b, computed in float64 on the host"""
        n = self.normalize
        if n is None:
            return [[1.0, 0.0]] * channels
        if n[0] == "static":
            return [[1.0 / float(n[1]), 0.0]] * channels
        if n[0] == "affine":
            return [[1.0 / (255.0 * float(n[2])), -float(n[1]) / float(n[2])]] * channels
        mean, std = list(n[1]), list(n[2])
        if len(mean) != channels or len(std) != channels:
            raise ValueError(f"DeviceImageTransform: imagenet mean / std of {len(mean)} / {len(std)} channels for {channels}-channel images")
        return [[1.0 / (255.0 * float(s)), -float(m) / float(s)] for m, s in zip(mean, std)]

    def boxes(self, batch_index: int, B: int, Hs: int, Ws: int, *, epoch: Optional[int] = None):
        """(boxes float32 [B, 4]: y0, x0, h, w in source pixels; flips uint8 [B]) of one batch"""
        rng = np.random.default_rng((self.seed, self.epoch if epoch is None else int(epoch), int(batch_index)))
        ho, wo = self.size
        if self.mode == "resize":
            box = np.tile(np.array([0.0, 0.0, Hs, Ws]), (B, 1))
        elif self.mode == "center_crop":
            box = np.tile(np.array([(Hs - ho) / 2.0, (Ws - wo) / 2.0, ho, wo]), (B, 1))
        else:
            tries = 10
            area = Hs * Ws * rng.uniform(self.scale[0], self.scale[1], (B, tries))
            ar = np.exp(rng.uniform(np.log(self.ratio[0]), np.log(self.ratio[1]), (B, tries)))
            w, h = np.sqrt(area * ar), np.sqrt(area / ar)
            ok = (w <= Ws) & (h <= Hs)
            first = np.where(ok.any(1), ok.argmax(1), 0)
            rows = np.arange(B)
            w, h = w[rows, first], h[rows, first]
            u = rng.uniform(0.0, 1.0, (B, 2))
            box = np.stack([u[:, 0] * (Hs - h), u[:, 1] * (Ws - w), h, w], 1)
            # no try fitted: the largest centred box whose ratio is allowed
            r = min(max(Ws / Hs, self.ratio[0]), self.ratio[1])
            fw, fh = min(Ws, Hs * r), min(Hs, Ws / r)
            box[~ok.any(1)] = [(Hs - fh) / 2.0, (Ws - fw) / 2.0, fh, fw]
        flips = (rng.uniform(0.0, 1.0, B) < self.flip).astype(np.uint8)
        return box.astype(np.float32), flips


class ImageBatcher(TensorBatcher):
    """TensorBatcher whose uint8 image batch under `key` ([B, H, W, C] or [B, H, W]) crosses PCIe as uint8 and is turned into
    `transform`'s [B, C, Ho, Wo] tensor by cfhip_image_transform, issued on the copy stream behind the copy and in front of the event
    `__next__` waits on: `__next__` stays an event wait, no stream is added.  The boxes and flips of the batch (17 bytes per sample)
    follow the image in one small copy of their own -- joining them to the image's copy would cost a host pass over the whole batch.
    Every other key behaves as in TensorBatcher.  Epochs count from 0 per `__iter__` (`set_epoch` for a resumed run).
    There is no CPU fallback: device "cpu" raises."""

    def __init__(self, loader: Any, device: Any, transform: DeviceImageTransform, *, key: str = INPUT_KEY, depth: int = 1):
        super().__init__(loader, device, depth=depth)
        self.transform, self.key = transform, key
        self.epoch = 0
        self._batch_index = 0
        self._tables: Dict[int, Tensor] = {}

    def to(self, device: Any) -> None:
        super().to(device)
        if self.device.type != "cuda":
            raise RuntimeError("ImageBatcher needs a HIP device: the image transform is a HIP kernel and has no CPU fallback")

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __iter__(self) -> "ImageBatcher":
        self._batch_index = 0
        self._epoch_now = self.epoch
        self.epoch += 1
        return super().__iter__()  # type: ignore[return-value]

    def _image(self, v: Any) -> Tensor:
        if not isinstance(v, np.ndarray) or v.dtype != np.uint8 or v.ndim not in (3, 4):
            raise TypeError(f"ImageBatcher: `{self.key}` must be a uint8 array [B, H, W, C] or [B, H, W], got "
                            f"{getattr(v, 'dtype', type(v).__name__)} {getattr(v, 'shape', '')}")
        t = torch.from_numpy(np.ascontiguousarray(v))
        return t if t.dim() == 4 else t.unsqueeze(-1)

    def _transform(self, slot: int, t: Tensor, batch_index: int, epoch: int) -> Tensor:
        """copy `t` (uint8 [B, H, W, C], host) and its boxes into the slot's buffers and launch the transform: current stream"""
        from . import ops

        tf = self.transform
        b, hs, ws, c = t.shape
        boxes, flips = tf.boxes(batch_index, b, hs, ws, epoch=epoch)
        params = torch.from_numpy(np.concatenate([boxes.view(np.uint8).reshape(-1), flips]))
        raw = self._device_buf(slot, self.key + "/uint8", t)
        dev_params = self._device_buf(slot, self.key + "/boxes", params)
        raw.copy_(t, non_blocking=True)
        dev_params.copy_(params, non_blocking=True)
        if c not in self._tables:
            self._tables[c] = ops.image_scale_bias(tf.scale_bias(c), self.device)
        dst = self._device_buf(slot, self.key, torch.empty((b, c, *tf.size), dtype=tf.out_dtype, device="meta"))
        return ops.image_transform(raw, boxes, tf.size, self._tables[c], flips=flips, interpolation=tf.interpolation, out=dst,
                                   out_dtype=tf.out_dtype, dev_boxes=dev_params[:16 * b].view(torch.float32).view(b, 4),
                                   dev_flips=dev_params[16 * b:])

    def _sync_copy(self, npd: Dict[str, Any]) -> Dict[str, Any]:
        out = super()._sync_copy({k: v for k, v in npd.items() if k != self.key})
        if self.key in npd:
            out[self.key] = self._transform(self.depth + 2, self._image(npd[self.key]), 0, self.epoch)  # a slot the ring never uses
        return out

    def _prefetch(self) -> None:
        if self._exhausted:
            return
        try:
            npd = next(self._it)
        except StopIteration:
            self._exhausted = True
            return
        slot = self._slot
        self._slot = (self._slot + 1) % (self.depth + 2)
        batch: Dict[str, Any] = {}
        with torch.cuda.stream(self._copy_stream):
            freed = self._free_events.pop(slot, None)
            if freed is not None:
                self._copy_stream.wait_event(freed)
            for k, v in npd.items():
                if k == self.key:
                    batch[k] = self._transform(slot, self._image(v), self._batch_index, self._epoch_now)
                    continue
                t = _to_tensor(v)
                if not isinstance(t, Tensor) or t.is_cuda:
                    batch[k] = t
                    continue
                dst = self._device_buf(slot, k, t)
                dst.copy_(t, non_blocking=True)
                batch[k] = dst
            event = torch.cuda.Event()
            event.record(self._copy_stream)
        self._batch_index += 1
        self._pending.append((batch, event, slot))
