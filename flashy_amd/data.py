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
"""
from __future__ import annotations

import struct
import typing as tp

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
    """splitmix64 finalizer on Python integers (mirrors csrc/ingest.hip)."""
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
