# Copyright (c) Flashy-AMD authors.
"""Host->device input pipeline for MI355X training loops.

The reference wraps DataLoader for distributed sharding only
(reference flashy/distrib.py:220-243 — see :func:`flashy_amd.distrib.loader`);
the H2D copy of every batch runs on the compute stream, where it
serializes with the step (38 MB/step for ImageNet-shaped batch-64 input,
~0.5-0.7 ms at PCIe speed).  :class:`DevicePrefetcher` moves that copy to
a side HIP stream, double-buffered, so the next batch lands in HBM while
the current step computes — the standard prefetch idiom, graph-replay
friendly (the caller copies device-to-device into its static buffers at
~8 TB/s).

:class:`DeviceAugment` is the other half of a real image pipeline: batches
travel as the uint8 NHWC bytes a decoder produces (a quarter of the fp32
bytes), and one gfx950 kernel crops, flips and normalizes them into the bf16
NHWC tensor the native models take — with the random draw keyed on a device
step counter, so it also varies under HIP-graph replay.
:class:`DeviceResizedCrop` is its ImageNet counterpart: random resized crop
(scale / aspect), flip and normalize as an integer draw plus a fixed-point
bilinear resample, under the same counter, mirror and output contracts.
:class:`DeviceMix` then mixes the ingested batch in place — Mixup / CutMix,
drawn from the same kind of counter — and hands the loss a
:class:`MixedTarget` whose ``lam`` lives in device memory.
"""
from __future__ import annotations

import functools
import math
import struct
import typing as tp

import numpy as np
import torch

from . import ops


class DevicePrefetcher:
    """Wrap an iterator of (tensor, ...) host batches; yields the same
    batches resident on ``device``, with H2D copies issued ``depth`` slots
    ahead on a dedicated stream.

    Contract: the caller consumes (enqueues all reads of) a yielded batch
    on the current stream before requesting the next one — the prefetcher
    records an event on the current stream at each ``__next__`` and makes
    the copy stream wait on it before overwriting the oldest slot, so
    stream ordering guarantees the slot is idle.  On a CPU device this is
    a passthrough.

    Pinned source memory makes the copies truly asynchronous; non-pinned
    batches still work but the H2D enqueue blocks the host.

    Slots are staged with ``empty_like``, so any dtype passes through
    unchanged: uint8 image batches (the input of :class:`DeviceAugment`)
    arrive on the device as uint8.
    """

    def __init__(self, it: tp.Iterable, device: torch.device | str,
                 depth: int = 2):
        self.device = torch.device(device)
        self._it = iter(it)
        self._use_cuda = self.device.type == "cuda"
        if not self._use_cuda:
            return
        assert depth >= 2, depth
        self.depth = depth
        self._stream = torch.cuda.Stream(self.device)
        self._slots: tp.List[tp.Optional[tp.Tuple[torch.Tensor, ...]]] = \
            [None] * depth
        self._ready = [torch.cuda.Event() for _ in range(depth)]
        self._bare = [False] * depth
        self._head = 0          # next slot to hand out
        self._primed = 0
        for _ in range(depth):
            if not self._prime():
                break

    def _prime(self) -> bool:
        """Issue the H2D copy for the next host batch into the next free
        slot on the copy stream."""
        try:
            host = next(self._it)
        except StopIteration:
            return False
        bare = isinstance(host, torch.Tensor)
        if bare:
            host = (host,)
        slot = self._primed % self.depth
        self._bare[slot] = bare
        with torch.cuda.stream(self._stream):
            staged = self._slots[slot]
            if staged is None:
                staged = tuple(
                    torch.empty_like(t, device=self.device) for t in host)
                self._slots[slot] = staged
            for dst, src in zip(staged, host):
                dst.copy_(src, non_blocking=True)
            self._ready[slot].record(self._stream)
        self._primed += 1
        return True

    def __iter__(self):
        if not self._use_cuda:
            yield from self._it
            return
        while self._head < self._primed:
            slot = self._head % self.depth
            torch.cuda.current_stream(self.device).wait_event(
                self._ready[slot])
            batch = self._slots[slot]
            assert batch is not None
            self._head += 1
            yield batch[0] if self._bare[slot] else batch
            # the caller has now ENQUEUED its use of `batch` on the current
            # stream; fence the copy stream behind it before the slot is
            # overwritten by the refill
            fence = torch.cuda.Event()
            fence.record(torch.cuda.current_stream(self.device))
            self._stream.wait_event(fence)
            self._prime()


# ---------------------------------------------------------------------------
# on-device augmentation
# ---------------------------------------------------------------------------

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _mix(z: int) -> int:
    """splitmix64 finalizer on Python integers (mirrors csrc/common.h)."""
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z


def _fp32(x: float) -> float:
    """Round a Python float to the nearest fp32 (what the kernel receives)."""
    return struct.unpack("f", struct.pack("f", x))[0]


class DeviceAugment:
    """Random crop (with padding), horizontal flip and per-channel
    normalization of a uint8 NHWC batch, as one gfx950 kernel.

    ``aug(src_u8)`` maps uint8 ``[N, H, W, 3]`` to bf16 ``[N, OH, OW, 3]``,
    the layout the native models consume directly.  It is torchvision's
    ``RandomCrop(out_size, padding=pad, fill=fill)``,
    ``RandomHorizontalFlip(flip)`` and ``Normalize(mean, std)`` (on the
    0..1 scale) in that order; with ``train=False`` it is the centre crop
    of the padded image, no flip.

    Each sample's ``(dy, dx, flip)`` is a hash of ``(seed, step, sample
    index)``; ``step`` is a device int64 counter the kernel reads and a
    one-thread kernel then advances.  Both launches are capturable, so a
    replayed HIP graph crops differently every step, and the counter —
    not any host-side count — is what :meth:`state_dict` saves.
    :meth:`params_at` evaluates the same hash on the host.

    On a CPU device the same arithmetic runs in torch (the test oracle);
    on CUDA the native extension is required.
    """

    def __init__(self, out_size: tp.Union[int, tp.Tuple[int, int]],
                 pad: int = 0, flip: float = 0.5,
                 mean: tp.Sequence[float] = (0., 0., 0.),
                 std: tp.Sequence[float] = (1., 1., 1.),
                 fill: int = 0, seed: int = 0,
                 device: tp.Union[torch.device, str] = "cuda"):
        if isinstance(out_size, int):
            out_size = (out_size, out_size)
        self.out_size = (int(out_size[0]), int(out_size[1]))
        if len(out_size) != 2 or min(self.out_size) < 1:
            raise ValueError(f"out_size must be positive (OH, OW), got {out_size}")
        if int(pad) != pad or pad < 0:
            raise ValueError(f"pad must be a non-negative int, got {pad}")
        if not 0.0 <= flip <= 1.0:
            raise ValueError(f"flip must be a probability, got {flip}")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError(f"mean and std take 3 channels, got {mean}, {std}")
        if any(s <= 0 for s in std):
            raise ValueError(f"std must be positive, got {std}")
        if int(fill) != fill or not 0 <= fill <= 255:
            raise ValueError(f"fill must be a uint8 value, got {fill}")
        self.pad = int(pad)
        self.flip = float(flip)
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(s) for s in std)
        self.fill = int(fill)
        self.seed = int(seed)
        self.device = torch.device(device)
        # computed in double, rounded once to the fp32 the kernel multiplies by
        self.scale = tuple(_fp32(1.0 / (255.0 * s)) for s in self.std)
        self.bias = tuple(_fp32(-m / s) for m, s in zip(self.mean, self.std))
        self._host_step = 0
        self._step_dev: tp.Optional[torch.Tensor] = None
        if self.device.type == "cuda":
            ops.require()
            self._step_dev = torch.zeros(1, dtype=torch.int64,
                                         device=self.device)

    # -- the draw -----------------------------------------------------------
    def _ranges(self, in_size: tp.Tuple[int, int]) -> tp.Tuple[int, int]:
        H, W = in_size
        OH, OW = self.out_size
        ny = H + 2 * self.pad - OH + 1
        nx = W + 2 * self.pad - OW + 1
        if ny < 1 or nx < 1:
            raise ValueError(
                f"out_size {self.out_size} exceeds the padded source "
                f"{(H + 2 * self.pad, W + 2 * self.pad)}")
        return ny, nx

    def params_at(self, step: int, n: int, in_size: tp.Tuple[int, int]
                  ) -> tp.Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Host mirror of the kernel's draw at counter value ``step`` for
        samples ``0..n-1`` of an ``in_size = (H, W)`` source: CPU tensors
        ``(dy int64, dx int64, flip bool)``, offsets into the padded image."""
        ny, nx = self._ranges(in_size)
        thresh = round(self.flip * (1 << 24))
        key = _mix((self.seed + _GOLDEN * (step + 1)) & _M64)
        dys, dxs, flips = [], [], []
        for i in range(n):
            h1 = _mix((key + _GOLDEN * (i + 1)) & _M64)
            h2 = _mix((h1 + _GOLDEN) & _M64)
            dys.append(((h1 & 0xffffffff) * ny) >> 32)
            dxs.append(((h1 >> 32) * nx) >> 32)
            flips.append((h2 >> 40) < thresh)
        return (torch.tensor(dys, dtype=torch.int64),
                torch.tensor(dxs, dtype=torch.int64),
                torch.tensor(flips, dtype=torch.bool))

    # -- state --------------------------------------------------------------
    @property
    def step(self) -> int:
        """Number of train-mode batches drawn so far (reads the device)."""
        if self._step_dev is not None:
            return int(self._step_dev.item())
        return self._host_step

    def state_dict(self) -> tp.Dict[str, int]:
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state: tp.Mapping[str, int]) -> None:
        self.seed = int(state["seed"])
        self._host_step = int(state["step"])
        if self._step_dev is not None:
            # in place: a captured graph keeps reading this address
            self._step_dev.fill_(self._host_step)

    # -- the op -------------------------------------------------------------
    def _check(self, src: torch.Tensor, out: tp.Optional[torch.Tensor]):
        if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8:
            raise TypeError(
                f"source must be a uint8 tensor, got "
                f"{getattr(src, 'dtype', type(src))}")
        if src.dim() != 4 or src.shape[-1] != 3:
            raise ValueError(
                f"source must be NHWC [N, H, W, 3], got {tuple(src.shape)}")
        if not src.is_contiguous():
            raise ValueError(
                f"source must be contiguous NHWC, got shape "
                f"{tuple(src.shape)} with strides {src.stride()}")
        if src.device.type != self.device.type:
            raise ValueError(
                f"source is on {src.device}, this augment on {self.device}")
        self._ranges((src.shape[1], src.shape[2]))
        shape = (src.shape[0], *self.out_size, 3)
        if out is not None:
            if out.dtype != torch.bfloat16:
                raise TypeError(f"out must be bfloat16, got {out.dtype}")
            if tuple(out.shape) != shape or not out.is_contiguous() \
                    or out.device != src.device:
                raise ValueError(
                    f"out must be contiguous {shape} on {src.device}, got "
                    f"{tuple(out.shape)} on {out.device}")
        return shape

    def __call__(self, src: torch.Tensor,
                 out: tp.Optional[torch.Tensor] = None,
                 train: bool = True) -> torch.Tensor:
        shape = self._check(src, out)
        if out is None:
            out = torch.empty(shape, dtype=torch.bfloat16, device=src.device)
        if self._step_dev is not None:
            ops.image_ingest(src, out, self._step_dev, self.seed, self.pad,
                             self.flip, self.scale, self.bias, self.fill,
                             train)
            return out
        out.copy_(self._reference(src, self._host_step, train))
        if train:
            self._host_step += 1
        return out

    def _reference(self, src: torch.Tensor, step: int,
                   train: bool) -> torch.Tensor:
        """Torch path: gather at the ``params_at`` offsets, then
        ``(u8.double() * scale + bias).float().bfloat16()``."""
        N, H, W, _ = src.shape
        OH, OW = self.out_size
        if train:
            dy, dx, flip = self.params_at(step, N, (H, W))
        else:
            ny, nx = self._ranges((H, W))
            dy = torch.full((N,), (ny - 1) // 2, dtype=torch.int64)
            dx = torch.full((N,), (nx - 1) // 2, dtype=torch.int64)
            flip = torch.zeros(N, dtype=torch.bool)
        ox = torch.arange(OW).expand(N, OW)
        ox = torch.where(flip[:, None], OW - 1 - ox, ox)
        sy = torch.arange(OH)[None, :] + dy[:, None] - self.pad     # [N, OH]
        sx = ox + dx[:, None] - self.pad                            # [N, OW]
        inside = (((sy >= 0) & (sy < H))[:, :, None]
                  & ((sx >= 0) & (sx < W))[:, None, :])             # [N,OH,OW]
        idx_n = torch.arange(N)[:, None, None]
        px = src[idx_n, sy.clamp(0, H - 1)[:, :, None],
                 sx.clamp(0, W - 1)[:, None, :]]                    # [N,OH,OW,3]
        px = torch.where(inside[..., None], px,
                         torch.full_like(px, self.fill))
        scale = torch.tensor(self.scale, dtype=torch.float64)
        bias = torch.tensor(self.bias, dtype=torch.float64)
        return (px.double() * scale + bias).float().bfloat16()


_TABLE = 1024      # quantization levels of the area and of the log-ratio draw
_TRIES = 10        # torchvision's number of attempts before the fallback
_MAX_SIDE = 32767  # (side << 16) must fit the kernel's int32 coordinates


class DeviceResizedCrop:
    """Random resized crop, horizontal flip and per-channel normalization of
    a uint8 NHWC batch, as two gfx950 kernels (draw + bilinear resample).

    ``aug(src_u8)`` maps uint8 ``[N, H, W, 3]`` (one size per batch) to bf16
    ``[N, OH, OW, 3]``.  Train mode is torchvision's
    ``RandomResizedCrop(out_size, scale, ratio, antialias=False)``,
    ``RandomHorizontalFlip(flip)`` and ``Normalize(mean, std)``; eval mode
    (``train=False``) is the centred box of aspect ``OW:OH`` covering
    ``eval_crop`` of the largest such box, resampled to ``out_size`` without
    flip — ``eval_crop = 224 / 256`` is ``Resize(256)`` + ``CenterCrop(224)``
    on a square source.

    The draw follows torchvision's algorithm — ten tries of (area uniform
    in ``scale``, ratio log-uniform in ``ratio``, uniform position), then
    the centred fallback box at the violated ratio bound — with one
    difference: area and ratio are each quantized to 1024 levels, the
    midpoints of 1024 equal bins, whose square roots the host tabulates in
    Q16 at construction.  Everything on the device is then integer
    arithmetic (no ``exp`` / ``log`` / ``sqrt``, whose last bit differs
    from the host's), so :meth:`boxes_at` reproduces every box bit for bit.

    Resampling is bilinear with half-pixel centres (``align_corners=False``)
    in fixed point: Q16 source coordinates, 8-bit weights, an exact integer
    accumulator.  There is NO antialiasing: the source is expected within
    about 2x of the output size, i.e. pre-resized storage.

    As in :class:`DeviceAugment`, a sample's box is a hash of ``(seed,
    step, sample index)`` with ``step`` a device int64 counter that a
    one-thread kernel advances after the resample; all launches are
    capturable, a replayed HIP graph crops differently every step, and
    :meth:`state_dict` saves the counter.  The first two hash levels are
    those of :class:`DeviceAugment`, so one ``seed`` drives both.

    On a CPU device the same arithmetic runs in torch (the test oracle);
    on CUDA the native extension is required.
    """

    def __init__(self, out_size: tp.Union[int, tp.Tuple[int, int]],
                 scale: tp.Sequence[float] = (0.08, 1.0),
                 ratio: tp.Sequence[float] = (3 / 4, 4 / 3),
                 flip: float = 0.5,
                 mean: tp.Sequence[float] = (0., 0., 0.),
                 std: tp.Sequence[float] = (1., 1., 1.),
                 eval_crop: float = 0.875, seed: int = 0,
                 device: tp.Union[torch.device, str] = "cuda"):
        if isinstance(out_size, int):
            out_size = (out_size, out_size)
        self.out_size = (int(out_size[0]), int(out_size[1]))
        if len(out_size) != 2 or min(self.out_size) < 1:
            raise ValueError(f"out_size must be positive (OH, OW), got {out_size}")
        if len(scale) != 2 or not 0.0 < scale[0] <= scale[1] <= 1.0:
            raise ValueError(
                f"scale must satisfy 0 < s0 <= s1 <= 1, got {tuple(scale)}")
        if len(ratio) != 2 or not 0.0 < ratio[0] <= ratio[1] \
                or not 2.0 ** -14 <= ratio[0] or not ratio[1] <= 2.0 ** 14:
            raise ValueError(
                f"ratio must satisfy 0 < r0 <= r1 (within 2^-14 .. 2^14), "
                f"got {tuple(ratio)}")
        if not 0.0 <= flip <= 1.0:
            raise ValueError(f"flip must be a probability, got {flip}")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError(f"mean and std take 3 channels, got {mean}, {std}")
        if any(s <= 0 for s in std):
            raise ValueError(f"std must be positive, got {std}")
        if not 0.0 < eval_crop <= 1.0:
            raise ValueError(f"eval_crop must lie in (0, 1], got {eval_crop}")
        self.scale_range = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        self.flip = float(flip)
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(s) for s in std)
        self.eval_crop = float(eval_crop)
        self.seed = int(seed)
        self.device = torch.device(device)
        self.scale = tuple(_fp32(1.0 / (255.0 * s)) for s in self.std)
        self.bias = tuple(_fp32(-m / s) for m, s in zip(self.mean, self.std))
        # Q16 tables of the draw and Q16 constants of the fallback / eval box
        s0, s1 = self.scale_range
        l0, l1 = math.log(self.ratio[0]), math.log(self.ratio[1])
        self._sa, self._sr, self._sri = [], [], []
        for j in range(_TABLE):
            u = (j + 0.5) / _TABLE
            r = math.exp(l0 + u * (l1 - l0))
            self._sa.append(round(65536 * math.sqrt(s0 + u * (s1 - s0))))
            self._sr.append(round(65536 * math.sqrt(r)))
            self._sri.append(round(65536 / math.sqrt(r)))
        self._r0_q16 = round(65536 * self.ratio[0])
        self._r1_q16 = round(65536 * self.ratio[1])
        self._eval_q16 = round(65536 * self.eval_crop)
        self._host_step = 0
        self._step_dev: tp.Optional[torch.Tensor] = None
        self._tables_dev: tp.Optional[torch.Tensor] = None
        self._boxes: tp.Optional[torch.Tensor] = None
        # device box buffers, one per batch size, never released: a captured
        # graph keeps writing and reading the address it was captured with
        self._boxes_dev: tp.Dict[int, torch.Tensor] = {}
        if self.device.type == "cuda":
            ops.require()
            self._step_dev = torch.zeros(1, dtype=torch.int64,
                                         device=self.device)
            self._tables_dev = torch.tensor(
                [self._sa, self._sr, self._sri], dtype=torch.int32,
                device=self.device)

    def __repr__(self) -> str:
        return (f"DeviceResizedCrop(out_size={self.out_size}, "
                f"scale={self.scale_range}, ratio={self.ratio}, "
                f"flip={self.flip}, eval_crop={self.eval_crop}, "
                f"seed={self.seed}, device={self.device})")

    # -- the draw -----------------------------------------------------------
    def _in_size(self, in_size: tp.Tuple[int, int]) -> tp.Tuple[int, int]:
        H, W = int(in_size[0]), int(in_size[1])
        if min(H, W) < 1 or max(H, W) > _MAX_SIDE:
            raise ValueError(
                f"source sides must lie in 1..{_MAX_SIDE}, got {(H, W)}")
        return H, W

    def _consts(self) -> tp.Tuple[int, int, int, int]:
        """(flip threshold, r0, r1, eval_crop), the last three in Q16."""
        return (round(self.flip * (1 << 24)), self._r0_q16, self._r1_q16,
                self._eval_q16)

    def _rows_at(self, step: int, n: int, in_size: tp.Tuple[int, int],
                 train: bool = True) -> tp.List[tp.List[int]]:
        """The ``[n][8]`` rows ``(y0, x0, h, w, flip, step_y, step_x,
        fallback)`` that ``k_resized_crop_draw`` writes, on Python integers."""
        H, W = self._in_size(in_size)
        OH, OW = self.out_size
        rows = []
        if not train:
            if W * OH >= H * OW:        # source at least as wide as the output
                bh, bw = H << 16, ((H * OW) << 16) // OH
            else:
                bh, bw = ((W * OH) << 16) // OW, W << 16
            h = min(max((bh * self._eval_q16 + (1 << 31)) >> 32, 1), H)
            w = min(max((bw * self._eval_q16 + (1 << 31)) >> 32, 1), W)
            row = [(H - h) // 2, (W - w) // 2, h, w, 0,
                   (h << 16) // OH, (w << 16) // OW, 0]
            return [list(row) for _ in range(n)]
        thresh = round(self.flip * (1 << 24))
        root = math.isqrt((H * W) << 32)
        key = _mix((self.seed + _GOLDEN * (step + 1)) & _M64)
        for i in range(n):
            h0 = _mix((key + _GOLDEN * (i + 1)) & _M64)
            box = None
            for t in range(_TRIES):
                a = _mix((h0 + _GOLDEN * (2 * t + 1)) & _M64)
                b = _mix((h0 + _GOLDEN * (2 * t + 2)) & _M64)
                ja = ((a & 0xffffffff) * _TABLE) >> 32
                jr = ((a >> 32) * _TABLE) >> 32
                side = (root * self._sa[ja]) >> 16
                w = (side * self._sr[jr] + (1 << 31)) >> 32
                h = (side * self._sri[jr] + (1 << 31)) >> 32
                if 1 <= w <= W and 1 <= h <= H:
                    box = [((b & 0xffffffff) * (H - h + 1)) >> 32,
                           ((b >> 32) * (W - w + 1)) >> 32, h, w, 0]
                    break
            if box is None:
                h, w = H, W
                if (W << 16) < self._r0_q16 * H:       # narrower than r0
                    h = ((W << 17) + self._r0_q16) // (2 * self._r0_q16)
                elif (W << 16) > self._r1_q16 * H:     # wider than r1
                    w = (H * self._r1_q16 + (1 << 15)) >> 16
                h, w = min(max(h, 1), H), min(max(w, 1), W)
                box = [(H - h) // 2, (W - w) // 2, h, w, 1]
            y0, x0, h, w, fallback = box
            flip = int((_mix((h0 + _GOLDEN * 21) & _M64) >> 40) < thresh)
            rows.append([y0, x0, h, w, flip, (h << 16) // OH,
                         (w << 16) // OW, fallback])
        return rows

    def boxes_at(self, step: int, n: int, in_size: tp.Tuple[int, int]
                 ) -> tp.Tuple[torch.Tensor, torch.Tensor]:
        """Host mirror of the kernel's train-mode draw at counter value
        ``step`` for samples ``0..n-1`` of an ``in_size = (H, W)`` source:
        CPU tensors ``(int64 [n, 5] of (y0, x0, h, w, flip), bool [n]
        fallback)``; ``fallback`` marks boxes that came from the centred
        fallback after ten rejected tries."""
        rows = torch.tensor(self._rows_at(step, n, in_size),
                            dtype=torch.int64).view(n, 8)
        return rows[:, :5].contiguous(), rows[:, 7] != 0

    @property
    def last_boxes(self) -> tp.Optional[torch.Tensor]:
        """int32 ``[N, 8]`` rows ``(y0, x0, h, w, flip, step_y, step_x,
        fallback)`` of the latest call, on this augment's device; reading
        the attribute does not synchronize.  ``None`` before the first call.

        On CUDA the object keeps one such buffer per batch size for its
        whole life, so the address a captured graph was recorded with stays
        valid when other batch sizes come in between: a replay rewrites the
        buffer of the batch size it was captured at (the tensor this
        attribute returned after the captured call), and ``last_boxes``
        keeps naming the buffer of the latest *call*."""
        return self._boxes

    # -- state --------------------------------------------------------------
    @property
    def step(self) -> int:
        """Number of train-mode batches drawn so far (reads the device)."""
        if self._step_dev is not None:
            return int(self._step_dev.item())
        return self._host_step

    def state_dict(self) -> tp.Dict[str, int]:
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state: tp.Mapping[str, int]) -> None:
        self.seed = int(state["seed"])
        self._host_step = int(state["step"])
        if self._step_dev is not None:
            # in place: a captured graph keeps reading this address
            self._step_dev.fill_(self._host_step)

    # -- the op -------------------------------------------------------------
    def _check(self, src: torch.Tensor, out: tp.Optional[torch.Tensor]):
        if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8:
            raise TypeError(
                f"source must be a uint8 tensor, got "
                f"{getattr(src, 'dtype', type(src))}")
        if src.dim() != 4 or src.shape[-1] != 3:
            raise ValueError(
                f"source must be NHWC [N, H, W, 3], got {tuple(src.shape)}")
        if not src.is_contiguous():
            raise ValueError(
                f"source must be contiguous NHWC, got shape "
                f"{tuple(src.shape)} with strides {src.stride()}")
        if src.device.type != self.device.type:
            raise ValueError(
                f"source is on {src.device}, this augment on {self.device}")
        self._in_size((src.shape[1], src.shape[2]))
        shape = (src.shape[0], *self.out_size, 3)
        if out is not None:
            if out.dtype != torch.bfloat16:
                raise TypeError(f"out must be bfloat16, got {out.dtype}")
            if tuple(out.shape) != shape or not out.is_contiguous() \
                    or out.device != src.device:
                raise ValueError(
                    f"out must be contiguous {shape} on {src.device}, got "
                    f"{tuple(out.shape)} on {out.device}")
        return shape

    def __call__(self, src: torch.Tensor,
                 out: tp.Optional[torch.Tensor] = None,
                 train: bool = True) -> torch.Tensor:
        shape = self._check(src, out)
        if out is None:
            out = torch.empty(shape, dtype=torch.bfloat16, device=src.device)
        N = shape[0]
        if self._step_dev is not None:
            boxes = self._boxes_dev.get(N)
            if boxes is None:
                boxes = torch.zeros(N, 8, dtype=torch.int32,
                                    device=src.device)
                self._boxes_dev[N] = boxes
            self._boxes = boxes
            ops.resized_crop(src, out, self._boxes, self._tables_dev,
                             self._step_dev, self.seed, self._consts(),
                             self.scale, self.bias, train)
            return out
        rows = torch.tensor(
            self._rows_at(self._host_step, N, src.shape[1:3], train),
            dtype=torch.int64).view(N, 8)
        self._boxes = rows.to(torch.int32)
        out.copy_(self._resample(src, rows))
        if train:
            self._host_step += 1
        return out

    def _resample(self, src: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
        """Torch path of ``k_resized_crop`` on int64 tensors: the exact
        integer accumulator, then
        ``(acc.double() * (scale * 2^-16) + bias).float().bfloat16()``."""
        N = src.shape[0]
        OH, OW = self.out_size
        y0, x0, h, w, flip, sy, sx = (rows[:, k:k + 1] for k in range(7))

        def axis(o, lo, size, step):
            p = (lo << 16) + o * step + (step >> 1) - 32768
            p = torch.minimum(torch.maximum(p, lo << 16),
                              (lo + size - 1) << 16)
            i = p >> 16
            return i, torch.minimum(i + 1, lo + size - 1), (p >> 8) & 255

        iy, iy1, fy = axis(torch.arange(OH)[None, :], y0, h, sy)    # [N, OH]
        ox = torch.arange(OW).expand(N, OW)
        ox = torch.where(flip != 0, OW - 1 - ox, ox)
        ix, ix1, fx = axis(ox, x0, w, sx)                           # [N, OW]
        px = src.to(torch.int64)
        idx_n = torch.arange(N)[:, None, None]

        def at(yy, xx):
            return px[idx_n, yy[:, :, None], xx[:, None, :]]     # [N,OH,OW,3]

        fy = fy[:, :, None, None]
        fx = fx[:, None, :, None]
        acc = ((256 - fy) * ((256 - fx) * at(iy, ix) + fx * at(iy, ix1))
               + fy * ((256 - fx) * at(iy1, ix) + fx * at(iy1, ix1)))
        scale = torch.tensor(self.scale, dtype=torch.float64) / 65536.0
        bias = torch.tensor(self.bias, dtype=torch.float64)
        return (acc.double() * scale + bias).float().bfloat16()


# ---------------------------------------------------------------------------
# batch mixing: Mixup / CutMix
# ---------------------------------------------------------------------------

def _betainc_sym(a: float, x: np.ndarray) -> np.ndarray:
    """Regularized incomplete beta ``I_x(a, a)`` for ``0 < x <= 0.5`` in
    double: the continued fraction (modified Lentz), which converges fast
    there because ``x <= (a + 1) / (2a + 2)``."""
    tiny = 1e-300
    c = np.ones_like(x)
    d = 1.0 - 2.0 * a * x / (a + 1.0)
    d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
    h = d.copy()
    for m in range(1, 400):
        m2 = 2 * m
        for num in (m * (a - m) * x / ((a + m2 - 1.0) * (a + m2)),
                    -(a + m) * (2.0 * a + m) * x
                    / ((a + m2) * (a + m2 + 1.0))):
            d = 1.0 + num * d
            d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
            c = 1.0 + num / c
            c = np.where(np.abs(c) < tiny, tiny, c)
            delta = d * c
            h = h * delta
        if float(np.max(np.abs(delta - 1.0))) < 1e-16:
            break
    front = np.exp(math.lgamma(2.0 * a) - 2.0 * math.lgamma(a)
                   + a * (np.log(x) + np.log1p(-x)))
    return front * h / a


@functools.lru_cache(maxsize=32)
def _beta_quantiles(alpha: float, levels: int) -> np.ndarray:
    half = levels // 2
    u = (np.arange(half, dtype=np.float64) + 0.5) / levels
    lo = np.full(half, math.log(1e-300))
    hi = np.full(half, math.log(0.5))
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        below = _betainc_sym(alpha, np.exp(mid)) < u
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    q = np.exp(0.5 * (lo + hi))
    q = np.concatenate([q, 1.0 - q[::-1]])
    q.setflags(write=False)
    return q


def beta_quantiles(alpha: float, levels: int = _TABLE) -> np.ndarray:
    """The quantiles of Beta(alpha, alpha) at ``(j + 0.5) / levels``, in
    double: the midpoints of ``levels`` equal-probability bins.  The lower
    half comes from a bisection (on ``log x``, so tiny quantiles keep their
    relative precision) over the continued fraction of the regularized
    incomplete beta; the upper half is its mirror ``q[levels-1-j] = 1 -
    q[j]``.  math / numpy only; about half a second per new ``alpha``, cached."""
    if not alpha > 0 or levels < 2 or levels % 2:
        raise ValueError(f"need alpha > 0 and an even number of levels, got "
                         f"{alpha}, {levels}")
    return _beta_quantiles(float(alpha), int(levels)).copy()


class MixedTarget(tp.NamedTuple):
    """What :class:`DeviceMix` returns in place of the labels: sample ``i``
    is ``lam`` parts class ``target_a[i]`` and ``1 - lam`` parts class
    ``target_b[i]``.  ``lam`` is a 0-dim fp32 view into the mixer's row
    buffer, so it follows every later draw (and every graph replay);
    :func:`flashy_amd.functional.cross_entropy` takes the tuple as target."""
    target_a: torch.Tensor
    target_b: torch.Tensor
    lam: torch.Tensor


class DeviceMix:
    """Mixup and CutMix of a bf16 NHWC batch in place, as two gfx950 kernels
    (draw + mix), for the whole batch at once.

    ``mixer(x, target)`` mixes sample ``i`` of ``x`` ``[N, H, W, C]`` with
    sample ``N-1-i`` and returns :class:`MixedTarget` ``(target,
    target.flip(0), lam)``.  It is timm's ``Mixup`` in batch mode: with
    probability ``prob`` the batch is mixed; CutMix is chosen with
    probability ``switch_prob`` when both alphas are positive (else the one
    enabled mode); ``lam ~ Beta(alpha, alpha)``; Mixup blends ``lam * x +
    (1 - lam) * x.flip(0)``, CutMix swaps timm's ``rand_bbox`` box and
    corrects ``lam`` to the box's actual area share.  One difference, in the
    manner of :class:`DeviceResizedCrop`: Beta is quantized to the midpoints
    of 1024 equal-probability bins (:func:`beta_quantiles`), tabulated here
    as fp32 ``lam`` for Mixup and Q16 ``sqrt(1 - lam)`` for CutMix, so the
    device draw is integer arithmetic plus one double division and
    :meth:`row_at` reproduces it bit for bit.

    The draw hashes ``(seed, step)`` with ``step`` a device int64 counter
    that a one-thread kernel advances after the mix; all launches are
    capturable, so a replayed HIP graph mixes differently every step, and
    :meth:`state_dict` saves the counter.  The row ``(mode, y0, y1, x0, x1,
    lam as fp32 bits, j, 0)`` (mode 0 none, 1 mixup, 2 cutmix) lives in ONE
    persistent int32 ``[8]`` buffer, :attr:`last_row`; the loss kernel reads
    ``lam`` from it.  The level-one hash key is the augments', the mixer
    uses its batch-level slot, so one ``seed`` can drive an augment and a
    mixer without correlated draws.

    On a CPU device the same arithmetic runs in torch (the test oracle,
    for any float dtype); on CUDA the native extension is required and
    ``x`` must be bf16, contiguous, 4-D, ``target`` int64 ``[N]``.
    """

    def __init__(self, mixup_alpha: float = 0., cutmix_alpha: float = 0.,
                 prob: float = 1., switch_prob: float = 0.5, seed: int = 0,
                 device: tp.Union[torch.device, str] = "cuda"):
        if not mixup_alpha >= 0 or not cutmix_alpha >= 0 \
                or not math.isfinite(mixup_alpha + cutmix_alpha):
            raise ValueError(f"alphas must be non-negative, got "
                             f"{mixup_alpha}, {cutmix_alpha}")
        if mixup_alpha == 0 and cutmix_alpha == 0:
            raise ValueError("at least one of mixup_alpha, cutmix_alpha must "
                             "be positive")
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f"prob must be a probability, got {prob}")
        if not 0.0 <= switch_prob <= 1.0:
            raise ValueError(
                f"switch_prob must be a probability, got {switch_prob}")
        self.mixup_alpha = float(mixup_alpha)
        self.cutmix_alpha = float(cutmix_alpha)
        self.prob = float(prob)
        self.switch_prob = float(switch_prob)
        self.seed = int(seed)
        self.device = torch.device(device)
        # the two tables; None for a disabled mode
        self.lam_table: tp.Optional[np.ndarray] = None      # fp32 [1024]
        self.sq_table: tp.Optional[np.ndarray] = None       # int32 [1024]
        if self.mixup_alpha > 0:
            self.lam_table = beta_quantiles(self.mixup_alpha).astype(
                np.float32)
        if self.cutmix_alpha > 0:
            self.sq_table = np.rint(65536.0 * np.sqrt(
                1.0 - beta_quantiles(self.cutmix_alpha))).astype(np.int32)
        self._host_step = 0
        self._step_dev: tp.Optional[torch.Tensor] = None
        self._lam_dev: tp.Optional[torch.Tensor] = None
        self._sq_dev: tp.Optional[torch.Tensor] = None
        # ONE row buffer for the object's life: a captured graph and every
        # MixedTarget.lam handed out keep reading this address
        self._row = torch.zeros(8, dtype=torch.int32, device=self.device)
        self._row[5:6].view(torch.float32).fill_(1.0)
        self._lam = self._row[5:6].view(torch.float32)[0]
        if self.device.type == "cuda":
            ops.require()
            self._step_dev = torch.zeros(1, dtype=torch.int64,
                                         device=self.device)
            if self.lam_table is not None:
                self._lam_dev = torch.from_numpy(self.lam_table).to(
                    self.device)
            if self.sq_table is not None:
                self._sq_dev = torch.from_numpy(self.sq_table).to(self.device)

    def __repr__(self) -> str:
        return (f"DeviceMix(mixup_alpha={self.mixup_alpha}, "
                f"cutmix_alpha={self.cutmix_alpha}, prob={self.prob}, "
                f"switch_prob={self.switch_prob}, seed={self.seed}, "
                f"device={self.device})")

    # -- the draw -----------------------------------------------------------
    def _in_size(self, in_size: tp.Tuple[int, int]) -> tp.Tuple[int, int]:
        H, W = int(in_size[0]), int(in_size[1])
        if min(H, W) < 1 or max(H, W) > _MAX_SIDE:
            raise ValueError(
                f"image sides must lie in 1..{_MAX_SIDE}, got {(H, W)}")
        return H, W

    def row_at(self, step: int, in_size: tp.Tuple[int, int]) -> tp.List[int]:
        """Host mirror of ``k_batch_mix_draw`` at counter value ``step`` for
        ``in_size = (H, W)`` images: the 8 integers ``(mode, y0, y1, x0, x1,
        lam as fp32 bits, j, 0)``."""
        H, W = self._in_size(in_size)
        key = _mix((self.seed + _GOLDEN * (step + 1)) & _M64)
        hm = _mix(key)
        a = _mix((hm + _GOLDEN) & _M64)
        b = _mix((hm + 2 * _GOLDEN) & _M64)
        c = _mix((hm + 3 * _GOLDEN) & _M64)
        apply = (a >> 40) < round(self.prob * (1 << 24))
        cut = self.sq_table is not None and (
            self.lam_table is None
            or (a & 0xffffff) < round(self.switch_prob * (1 << 24)))
        j = ((b & 0xffffffff) * _TABLE) >> 32
        mode, y0, y1, x0, x1, lam = 0, 0, 0, 0, 0, 1.0
        if apply and not cut:
            mode, lam = 1, float(self.lam_table[j])
        elif apply:
            mode = 2
            sq = int(self.sq_table[j])
            cut_h, cut_w = (H * sq) >> 16, (W * sq) >> 16
            cy = ((c & 0xffffffff) * H) >> 32
            cx = ((c >> 32) * W) >> 32
            y0, y1 = max(cy - cut_h // 2, 0), min(cy + cut_h // 2, H)
            x0, x1 = max(cx - cut_w // 2, 0), min(cx + cut_w // 2, W)
            lam = _fp32(1.0 - ((y1 - y0) * (x1 - x0)) / (H * W))
        bits = struct.unpack("i", struct.pack("f", lam))[0]
        return [mode, y0, y1, x0, x1, bits, j, 0]

    @property
    def last_row(self) -> torch.Tensor:
        """The int32 ``[8]`` row of the latest call (or replay), on this
        mixer's device — always the same buffer; reading the attribute does
        not synchronize."""
        return self._row

    # -- state --------------------------------------------------------------
    @property
    def step(self) -> int:
        """Number of batches drawn so far (reads the device)."""
        if self._step_dev is not None:
            return int(self._step_dev.item())
        return self._host_step

    def state_dict(self) -> tp.Dict[str, int]:
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state: tp.Mapping[str, int]) -> None:
        self.seed = int(state["seed"])
        self._host_step = int(state["step"])
        if self._step_dev is not None:
            # in place: a captured graph keeps reading this address
            self._step_dev.fill_(self._host_step)

    # -- the op -------------------------------------------------------------
    def _check(self, x: torch.Tensor, target: torch.Tensor) -> None:
        if not isinstance(x, torch.Tensor) or not x.is_floating_point():
            raise TypeError(f"x must be a float tensor, got "
                            f"{getattr(x, 'dtype', type(x))}")
        if x.dim() != 4:
            raise ValueError(
                f"x must be NHWC [N, H, W, C], got {tuple(x.shape)}")
        if x.device.type != self.device.type:
            raise ValueError(f"x is on {x.device}, this mixer on {self.device}")
        if self._step_dev is not None:
            if x.dtype != torch.bfloat16:
                raise TypeError(f"x must be bfloat16 on CUDA, got {x.dtype}")
            if not x.is_contiguous():
                raise ValueError(
                    f"x must be contiguous NHWC, got shape {tuple(x.shape)} "
                    f"with strides {x.stride()}")
        if not isinstance(target, torch.Tensor) \
                or target.dtype != torch.int64:
            raise TypeError(f"target must be an int64 tensor, got "
                            f"{getattr(target, 'dtype', type(target))}")
        if tuple(target.shape) != (x.shape[0],) \
                or target.device != x.device:
            raise ValueError(
                f"target must be [{x.shape[0]}] on {x.device}, got "
                f"{tuple(target.shape)} on {target.device}")
        self._in_size((x.shape[1], x.shape[2]))

    def __call__(self, x: torch.Tensor, target: torch.Tensor) -> MixedTarget:
        self._check(x, target)
        mixed = MixedTarget(target, target.flip(0), self._lam)
        if self._step_dev is not None:
            ops.batch_mix_draw(self._row, self._lam_dev, self._sq_dev,
                               self._step_dev, self.seed, x.shape[1:3],
                               self.prob, self.switch_prob)
            ops.batch_mix(x, self._row)
            ops.adam_step_inc(self._step_dev)
            return mixed
        row = self.row_at(self._host_step, x.shape[1:3])
        self._row.copy_(torch.tensor(row, dtype=torch.int32))
        self._reference(x, row)
        self._host_step += 1
        return mixed

    @staticmethod
    def _reference(x: torch.Tensor, row: tp.Sequence[int]) -> None:
        """Torch path of ``k_batch_mix``, in place: fp32 products and sum,
        each rounded on its own, then one rounding to ``x.dtype``; the box
        is clamped into the image as the kernel clamps it."""
        mode = int(row[0])
        H, W = x.shape[1], x.shape[2]
        if mode == 1:
            lam = torch.tensor([int(row[5])], dtype=torch.int32).view(
                torch.float32)[0]
            oml = 1.0 - lam                             # fp32, as the kernel
            xf = x.float()
            x.copy_((xf * lam + xf.flip(0) * oml).to(x.dtype))
        elif mode == 2:
            y0 = min(max(int(row[1]), 0), H)
            y1 = min(max(int(row[2]), y0), H)
            x0 = min(max(int(row[3]), 0), W)
            x1 = min(max(int(row[4]), x0), W)
            x[:, y0:y1, x0:x1] = x[:, y0:y1, x0:x1].flip(0).clone()
