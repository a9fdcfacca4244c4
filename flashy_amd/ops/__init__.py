# Copyright (c) Flashy-AMD authors.
"""CDNA4 (gfx950) kernel wrappers.

The native extension ``_hip_ops`` is built in-tree by
``python -m flashy_amd.ops.build`` (hipcc --offload-arch=gfx950) and loaded
from this package directory.  Wrappers pass raw device pointers and the
current HIP stream handle, so every launch lands on the torch stream and is
captured by HIP graphs like any torch kernel.

Policy: on a GPU box a missing extension is a HARD error (no silent eager
fallback — the HIP path must be the one that runs); pure-CPU runs (CI) use
torch fallbacks provided by the callers (see flashy_amd/optim.py,
flashy_amd/functional.py).
"""
from __future__ import annotations

import importlib.util
import math
import os
import typing as tp
from pathlib import Path

import torch

_ext = None
_load_error: tp.Optional[str] = None


def _find_so() -> tp.Optional[Path]:
    for pattern in ("_hip_ops*.so",):
        hits = sorted(Path(__file__).parent.glob(pattern))
        if hits:
            return hits[0]
    return None


def load_extension():
    """Load (once) and return the native module; raises with build advice."""
    global _ext, _load_error
    if _ext is not None:
        return _ext
    so = _find_so()
    if so is None:
        _load_error = "extension not built"
        raise RuntimeError(
            "flashy_amd._hip_ops is not built. Build it in-tree with:\n"
            "    python -m flashy_amd.ops.build\n"
            "(requires hipcc; cross-compiles for gfx950 without a GPU).")
    spec = importlib.util.spec_from_file_location("flashy_amd.ops._hip_ops", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # type: ignore[union-attr]
    _ext = mod
    return _ext


def available() -> bool:
    try:
        load_extension()
        return True
    except (RuntimeError, ImportError, OSError):
        return False


def require() -> tp.Any:
    """On a CUDA device the native kernels are mandatory: fail loudly."""
    return load_extension()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _is_bf16(t: torch.Tensor) -> bool:
    if t.dtype == torch.bfloat16:
        return True
    if t.dtype == torch.float32:
        return False
    raise TypeError(f"unsupported dtype {t.dtype} (float32/bfloat16 only)")


# ---------------------------------------------------------------------------
# optimizer kernels (flat fp32 buffers — see flashy_amd/optim.py)
# ---------------------------------------------------------------------------

def fused_sgd(p: torch.Tensor, g: torch.Tensor, m: tp.Optional[torch.Tensor],
              lr: float, momentum: float, wd: float, grad_scale: float = 1.0,
              nesterov: bool = False, p_bf16: tp.Optional[torch.Tensor] = None,
              hyper: tp.Optional[torch.Tensor] = None) -> None:
    """hyper: optional device block written by :func:`optim_prepare`; when
    given, the kernel takes ``lr`` from it (the ``lr`` argument is ignored)
    and multiplies ``grad_scale`` by its clip coefficient."""
    ext = require()
    assert p.is_contiguous() and g.is_contiguous()
    ext.fused_sgd(p.data_ptr(), g.data_ptr(),
                  m.data_ptr() if m is not None else 0,
                  p_bf16.data_ptr() if p_bf16 is not None else 0,
                  p.numel(), lr, momentum, wd, grad_scale, nesterov, _stream(),
                  _hyper_ptr(hyper))


def fused_adam(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor,
               v: torch.Tensor, lr: float, beta1: float, beta2: float,
               eps: float, wd: float, step: int, grad_scale: float = 1.0,
               adamw: bool = False,
               p_bf16: tp.Optional[torch.Tensor] = None,
               step_dev: tp.Optional[torch.Tensor] = None,
               hyper: tp.Optional[torch.Tensor] = None) -> None:
    """step_dev: optional int64 device scalar holding the step count — makes
    the bias correction graph-replay-safe (advance it with adam_step_inc).
    hyper: as for :func:`fused_sgd`."""
    ext = require()
    assert p.is_contiguous() and g.is_contiguous()
    ext.fused_adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                   p_bf16.data_ptr() if p_bf16 is not None else 0,
                   step_dev.data_ptr() if step_dev is not None else 0,
                   p.numel(), lr, beta1, beta2, eps, wd, step, grad_scale,
                   adamw, _stream(), _hyper_ptr(hyper))


def adam_step_inc(step_dev: torch.Tensor) -> None:
    require().adam_step_inc(step_dev.data_ptr(), _stream())


# layout of the per-device hyper block (fp32), see csrc/fused_optim.hip
HYPER_LR, HYPER_COEF, HYPER_NORM, HYPER_SIZE = 0, 1, 2, 4


def _hyper_ptr(hyper: tp.Optional[torch.Tensor]) -> int:
    if hyper is None:
        return 0
    assert hyper.dtype == torch.float32 and hyper.numel() >= HYPER_SIZE
    assert hyper.is_cuda and hyper.is_contiguous()
    return hyper.data_ptr()


def grad_sqsum_blocks(n: int) -> int:
    """Number of per-block partials :func:`grad_sqsum` writes for ``n``
    elements."""
    return require().grad_sqsum_blocks(n)


def grad_sqsum(g: torch.Tensor, partials: torch.Tensor) -> int:
    """Sum of squares of the flat fp32 buffer ``g`` into per-block fp32
    partials (no atomics, no pre-zeroing: deterministic for a given size).
    Returns how many leading elements of ``partials`` were written; feed
    those to :func:`optim_prepare`."""
    ext = require()
    assert g.dtype == torch.float32 and partials.dtype == torch.float32
    assert g.is_cuda and partials.is_cuda
    assert g.is_contiguous() and partials.is_contiguous()
    assert g.data_ptr() % 16 == 0, "float4 loads need a 16-byte aligned buffer"
    blocks = ext.grad_sqsum_blocks(g.numel())
    if partials.numel() < blocks:
        raise ValueError(
            f"partials holds {partials.numel()} floats, need {blocks}")
    ext.grad_sqsum(g.data_ptr(), g.numel(), partials.data_ptr(), _stream())
    return blocks


def optim_prepare(hyper: torch.Tensor, schedule: tp.Any, base_lr: float,
                  step_dev: tp.Optional[torch.Tensor] = None,
                  partials: tp.Optional[torch.Tensor] = None,
                  max_norm: float = 0.0) -> None:
    """Write this step's ``lr`` / clip ``coef`` / gradient ``norm`` into the
    device block ``hyper`` (one 1-block kernel, no host read).

    schedule: an :class:`flashy_amd.optim.LRSchedule`; it is evaluated on the
    device at ``step_dev - 1`` (``step_dev``: int64 device scalar holding the
    1-based number of the step about to run; step 0 when absent).
    partials: ALL of it is summed (pass exactly the slice that
    :func:`grad_sqsum` wrote); ``None`` means no clipping: coef 1, norm 0."""
    ext = require()
    assert hyper.dtype == torch.float32 and hyper.numel() >= HYPER_SIZE
    assert hyper.is_cuda and hyper.is_contiguous()
    kind, warmup, start, total, floor, milestones, gamma = \
        schedule.kernel_args()
    n_partials = 0
    if partials is not None:
        assert partials.dtype == torch.float32 and partials.is_contiguous()
        assert partials.is_cuda
        if not max_norm > 0:
            raise ValueError(f"max_norm must be > 0, got {max_norm}")
        n_partials = partials.numel()
    if step_dev is not None:
        assert step_dev.dtype == torch.int64 and step_dev.is_cuda
    ext.optim_prepare(hyper.data_ptr(),
                      partials.data_ptr() if partials is not None else 0,
                      n_partials,
                      step_dev.data_ptr() if step_dev is not None else 0,
                      float(max_norm), kind, float(base_lr), warmup, start,
                      total, floor, list(milestones), gamma, _stream())


# ---------------------------------------------------------------------------
# segmented optimizer path: per-tensor weight decay / lr scale / LARS
# ---------------------------------------------------------------------------

SEG_CHUNK = 4096


def seg_chunks(sizes: tp.Sequence[int], chunk: int = SEG_CHUNK
               ) -> tp.List[tp.Tuple[int, int, int]]:
    """Cut a flat arena holding tensors of ``sizes`` (packed back to back)
    into ``(start, len, tensor)`` chunks: the intersection of each fixed
    window ``[w * chunk, (w + 1) * chunk)`` with each tensor.  Chunks never
    cross a tensor boundary, edges inside a tensor are window edges, and
    there are at most ``ceil(n / chunk) + T - 1`` of them.  Pure host code."""
    if chunk <= 0 or chunk % 4:
        raise ValueError(f"chunk must be a positive multiple of 4: {chunk}")
    out = []
    offset = 0
    for t, size in enumerate(sizes):
        start, end = offset, offset + int(size)
        while start < end:
            stop = min(end, (start // chunk + 1) * chunk)
            out.append((start, stop - start, t))
            start = stop
        offset = end
    return out


class SegTable:
    """Device-resident chunk table and per-tensor hyperparameter arrays of
    one flat arena (built once on the host, see :func:`seg_chunks`).

    ``chunks`` is int32 ``[C, 4]``: 64-bit ``start``, ``len``, ``tensor`` —
    one 16-byte entry per chunk.  ``tensor_chunk`` (int32 ``[T + 1]``) maps a
    tensor to its chunk range; ``wd`` / ``lr_scale`` (fp32) and ``lars_on``
    (int32) hold one value per tensor.  :meth:`set_options` rewrites the
    per-tensor values in place, so a captured step sees them on replay."""

    def __init__(self, sizes: tp.Sequence[int], wd: tp.Sequence[float],
                 lr_scale: tp.Sequence[float], lars_on: tp.Sequence[bool],
                 device: tp.Any, chunk: int = SEG_CHUNK):
        self.sizes = [int(s) for s in sizes]
        self.n = sum(self.sizes)
        self.n_tensors = len(self.sizes)
        self.chunk = chunk
        chunks = seg_chunks(self.sizes, chunk)
        if not chunks:
            raise ValueError("empty arena")
        self.n_chunks = len(chunks)
        # the kernels trust the table: check it covers [0, n) exactly, in
        # order, before it reaches the device
        pos = 0
        for start, length, tensor in chunks:
            assert start == pos and 0 < length <= chunk, (start, length)
            assert 0 <= tensor < self.n_tensors
            pos += length
        assert pos == self.n
        starts = torch.tensor([c[0] for c in chunks], dtype=torch.int64)
        rest = torch.tensor([c[1:] for c in chunks], dtype=torch.int32)
        table = torch.cat([starts.view(torch.int32).reshape(-1, 2), rest], 1)
        self.chunks = table.contiguous().to(device)
        first = [0] * (self.n_tensors + 1)
        for _, _, tensor in chunks:
            first[tensor + 1] += 1
        for t in range(self.n_tensors):
            first[t + 1] += first[t]
        self.tensor_chunk = torch.tensor(first, dtype=torch.int32,
                                         device=device)
        self.wd = torch.empty(self.n_tensors, dtype=torch.float32,
                              device=device)
        self.lr_scale = torch.empty_like(self.wd)
        self.lars_on = torch.empty(self.n_tensors, dtype=torch.int32,
                                   device=device)
        self.set_options(wd, lr_scale, lars_on)

    def set_options(self, wd: tp.Sequence[float],
                    lr_scale: tp.Sequence[float],
                    lars_on: tp.Sequence[bool]) -> None:
        """Overwrite the per-tensor values (one per tensor each) in place."""
        if not len(wd) == len(lr_scale) == len(lars_on) == self.n_tensors:
            raise ValueError(f"need {self.n_tensors} values per option")
        self.wd.copy_(torch.tensor(list(wd), dtype=torch.float32))
        self.lr_scale.copy_(torch.tensor(list(lr_scale), dtype=torch.float32))
        self.lars_on.copy_(torch.tensor([int(bool(x)) for x in lars_on],
                                        dtype=torch.int32))


def _seg_check(table: SegTable, *buffers: tp.Optional[torch.Tensor]) -> None:
    for t in buffers:
        if t is None:
            continue
        assert t.is_cuda and t.is_contiguous() and t.numel() == table.n, \
            "buffer does not match the chunk table"
        assert t.device == table.chunks.device
        # float4 / ushort4 accesses at flat indices that are multiples of 4
        assert t.data_ptr() % (4 * t.element_size()) == 0, \
            "vector accesses need an aligned buffer"


def seg_sqsum(p: torch.Tensor, g: torch.Tensor, table: SegTable,
              partials: torch.Tensor) -> None:
    """Per-chunk ``(sum p^2, sum g^2)`` into the fp32 ``partials [C, 2]`` (no
    atomics, no pre-zeroing: every slot is written, deterministic for a
    given table).  Feed them to :func:`lars_prepare`."""
    ext = require()
    assert p.dtype == torch.float32 and g.dtype == torch.float32
    _seg_check(table, p, g)
    assert partials.dtype == torch.float32 and partials.is_contiguous()
    assert partials.is_cuda and partials.numel() == 2 * table.n_chunks
    ext.seg_sqsum(p.data_ptr(), g.data_ptr(), table.chunks.data_ptr(),
                  table.n_chunks, partials.data_ptr(), _stream())


def lars_prepare(partials: torch.Tensor, table: SegTable,
                 ratio: torch.Tensor, eta: float, eps: float,
                 grad_scale: float = 1.0,
                 hyper: tp.Optional[torch.Tensor] = None) -> None:
    """Write the LARS trust ratio of every tensor of ``table`` into the fp32
    ``ratio [T]``: ``eta * |p| / (|g'| + wd * |p| + eps)`` with
    ``g' = grad_scale * hyper[HYPER_COEF] * g`` where the tensor has LARS on
    and both norms are positive, else 1.  The chunk partials are summed per
    tensor in fixed order in fp64; no host read.  Run it after
    :func:`optim_prepare` when ``hyper`` is given."""
    ext = require()
    assert partials.dtype == torch.float32 and partials.is_contiguous()
    assert partials.is_cuda and partials.numel() == 2 * table.n_chunks
    assert ratio.dtype == torch.float32 and ratio.is_contiguous()
    assert ratio.is_cuda and ratio.numel() == table.n_tensors
    ext.lars_prepare(partials.data_ptr(), table.tensor_chunk.data_ptr(),
                     table.wd.data_ptr(), table.lars_on.data_ptr(),
                     ratio.data_ptr(), table.n_tensors, _hyper_ptr(hyper),
                     grad_scale, float(eta), float(eps), _stream())


def fused_sgd_seg(p: torch.Tensor, g: torch.Tensor,
                  m: tp.Optional[torch.Tensor], lr: float, momentum: float,
                  table: SegTable, grad_scale: float = 1.0,
                  nesterov: bool = False,
                  p_bf16: tp.Optional[torch.Tensor] = None,
                  hyper: tp.Optional[torch.Tensor] = None,
                  ratio: tp.Optional[torch.Tensor] = None) -> None:
    """:func:`fused_sgd` with ``wd`` and ``lr * lr_scale`` taken per tensor
    from ``table`` and, when ``ratio`` (from :func:`lars_prepare`) is given,
    the update scaled by the tensor's trust ratio."""
    ext = require()
    assert p.dtype == torch.float32 and g.dtype == torch.float32
    _seg_check(table, p, g, m, p_bf16)
    if ratio is not None:
        assert ratio.dtype == torch.float32 and ratio.is_cuda
        assert ratio.is_contiguous() and ratio.numel() == table.n_tensors
    ext.fused_sgd_seg(p.data_ptr(), g.data_ptr(),
                      m.data_ptr() if m is not None else 0,
                      p_bf16.data_ptr() if p_bf16 is not None else 0,
                      p.numel(), lr, momentum, grad_scale, nesterov,
                      _hyper_ptr(hyper), table.chunks.data_ptr(),
                      table.n_chunks, table.wd.data_ptr(),
                      table.lr_scale.data_ptr(),
                      ratio.data_ptr() if ratio is not None else 0, _stream())


def fused_adam_seg(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor,
                   v: torch.Tensor, lr: float, beta1: float, beta2: float,
                   eps: float, step: int, table: SegTable,
                   grad_scale: float = 1.0, adamw: bool = False,
                   p_bf16: tp.Optional[torch.Tensor] = None,
                   step_dev: tp.Optional[torch.Tensor] = None,
                   hyper: tp.Optional[torch.Tensor] = None) -> None:
    """:func:`fused_adam` with ``wd`` and ``lr * lr_scale`` taken per tensor
    from ``table``."""
    ext = require()
    assert p.dtype == torch.float32 and g.dtype == torch.float32
    _seg_check(table, p, g, m, v, p_bf16)
    ext.fused_adam_seg(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                       p_bf16.data_ptr() if p_bf16 is not None else 0,
                       step_dev.data_ptr() if step_dev is not None else 0,
                       p.numel(), lr, beta1, beta2, eps, step, grad_scale,
                       adamw, _hyper_ptr(hyper), table.chunks.data_ptr(),
                       table.n_chunks, table.wd.data_ptr(),
                       table.lr_scale.data_ptr(), _stream())


# ---------------------------------------------------------------------------
# input ingest (uint8 NHWC -> bf16 NHWC; see flashy_amd/data.py)
# ---------------------------------------------------------------------------

def image_ingest(src: torch.Tensor, out: torch.Tensor,
                 step_dev: tp.Optional[torch.Tensor], seed: int, pad: int,
                 p_flip: float, scale: tp.Sequence[float],
                 bias: tp.Sequence[float], fill: int = 0,
                 train: bool = True) -> None:
    """Fused crop / horizontal flip / normalize: uint8 NHWC ``src``
    [N, H, W, 3] -> bf16 NHWC ``out`` [N, OH, OW, 3], one launch.

    Train mode draws each sample's crop offset and flip bit from a hash of
    (``seed``, ``step_dev``, sample index) and then advances ``step_dev``
    (int64 device scalar) by one on the same stream, so a captured step
    augments differently on every replay.  Eval mode is the centre crop
    without flip; ``step_dev`` is neither read nor advanced.  ``scale`` /
    ``bias`` are the per-channel fp32 values of ``u8 * scale + bias``."""
    ext = require()
    assert src.dtype == torch.uint8 and out.dtype == torch.bfloat16
    assert src.is_cuda and out.is_cuda and src.device == out.device
    assert src.is_contiguous() and out.is_contiguous()
    assert src.dim() == 4 and out.dim() == 4, (src.shape, out.shape)
    N, H, W, C = src.shape
    OH, OW = out.shape[1], out.shape[2]
    assert C == 3 and out.shape[0] == N and out.shape[3] == 3, \
        (src.shape, out.shape)
    assert pad >= 0 and 1 <= OH <= H + 2 * pad and 1 <= OW <= W + 2 * pad, \
        (src.shape, out.shape, pad)
    assert len(scale) == 3 and len(bias) == 3
    assert 0 <= fill <= 255 and 0.0 <= p_flip <= 1.0
    if train:
        assert step_dev is not None and step_dev.dtype == torch.int64
        assert step_dev.is_cuda and step_dev.numel() == 1
    ext.image_ingest(src.data_ptr(), out.data_ptr(),
                     step_dev.data_ptr() if train else 0, N, H, W, OH, OW,
                     pad, seed & (2 ** 64 - 1), round(p_flip * 2 ** 24),
                     [float(s) for s in scale], [float(b) for b in bias],
                     fill, train, _stream())
    if train:
        ext.adam_step_inc(step_dev.data_ptr(), _stream())


def resized_crop(src: torch.Tensor, out: torch.Tensor, boxes: torch.Tensor,
                 tables: torch.Tensor, step_dev: tp.Optional[torch.Tensor],
                 seed: int, consts: tp.Sequence[int],
                 scale: tp.Sequence[float], bias: tp.Sequence[float],
                 train: bool = True) -> None:
    """Random resized crop / horizontal flip / normalize: uint8 NHWC ``src``
    [N, H, W, 3] -> bf16 NHWC ``out`` [N, OH, OW, 3], as two launches.

    ``k_resized_crop_draw`` writes each sample's row ``(y0, x0, h, w, flip,
    step_y, step_x, fallback)`` into ``boxes`` (int32 [N, 8]) and
    ``k_resized_crop`` resamples the boxes bilinearly.  Train mode hashes
    (``seed``, ``step_dev``, sample index) and then advances ``step_dev``
    (int64 device scalar) by one on the same stream; eval mode takes the
    centred box and neither reads nor advances ``step_dev``.  ``tables`` is
    the int32 [3, 1024] Q16 block of
    :class:`flashy_amd.data.DeviceResizedCrop`, ``consts`` its ``(flip
    threshold, r0, r1, eval_crop)`` integers; ``scale`` / ``bias`` are the
    per-channel fp32 values of ``u8 * scale + bias``."""
    ext = require()
    assert src.dtype == torch.uint8 and out.dtype == torch.bfloat16
    assert src.is_cuda and out.is_cuda and src.device == out.device
    assert src.is_contiguous() and out.is_contiguous()
    assert src.dim() == 4 and out.dim() == 4, (src.shape, out.shape)
    N, H, W, C = src.shape
    OH, OW = out.shape[1], out.shape[2]
    assert C == 3 and out.shape[0] == N and out.shape[3] == 3, \
        (src.shape, out.shape)
    assert 1 <= H <= 32767 and 1 <= W <= 32767 and OH >= 1 and OW >= 1, \
        (src.shape, out.shape)
    assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (N, 8)
    assert boxes.is_contiguous() and boxes.device == src.device
    assert tables.dtype == torch.int32 and tuple(tables.shape) == (3, 1024)
    assert tables.is_contiguous() and tables.device == src.device
    assert len(scale) == 3 and len(bias) == 3 and len(consts) == 4
    thresh, r0, r1, eval_crop = (int(c) for c in consts)
    assert 0 <= thresh <= 2 ** 24 and 0 < r0 <= r1 < 2 ** 31
    assert 0 < eval_crop <= 2 ** 16
    if train:
        assert step_dev is not None and step_dev.dtype == torch.int64
        assert step_dev.is_cuda and step_dev.numel() == 1
    if N:
        ext.resized_crop_draw(boxes.data_ptr(), tables.data_ptr(),
                              step_dev.data_ptr() if train else 0, N, H, W,
                              OH, OW, seed & (2 ** 64 - 1),
                              math.isqrt((H * W) << 32), thresh, r0, r1,
                              eval_crop, train, _stream())
        ext.resized_crop(src.data_ptr(), out.data_ptr(), boxes.data_ptr(), N,
                         H, W, OH, OW, [float(s) for s in scale],
                         [float(b) for b in bias], _stream())
    if train:
        ext.adam_step_inc(step_dev.data_ptr(), _stream())


# ---------------------------------------------------------------------------
# batch mixing (Mixup / CutMix on bf16 NHWC; see flashy_amd/data.py)
# ---------------------------------------------------------------------------

# layout of the int32 [8] mix row, see csrc/mix.hip
MIX_MODE, MIX_Y0, MIX_Y1, MIX_X0, MIX_X1, MIX_LAM, MIX_J = range(7)


def _check_mix_row(row: torch.Tensor) -> None:
    assert row.dtype == torch.int32 and tuple(row.shape) == (8,), \
        (row.dtype, row.shape)
    assert row.is_cuda and row.is_contiguous()
    assert row.data_ptr() % 16 == 0, "the kernels read the row as two int4"


def batch_mix_draw(row: torch.Tensor, lam_table: tp.Optional[torch.Tensor],
                   sq_table: tp.Optional[torch.Tensor],
                   step_dev: torch.Tensor, seed: int,
                   in_size: tp.Tuple[int, int], prob: float,
                   switch_prob: float) -> None:
    """Write the batch's mix row ``(mode, y0, y1, x0, x1, lam as fp32 bits,
    j, 0)`` into ``row`` (int32 [8]) from a hash of (``seed``,
    ``step_dev``); one one-thread launch, ``step_dev`` (int64 device scalar)
    is read, not advanced.  ``lam_table`` (fp32 [1024]) enables mixup,
    ``sq_table`` (int32 [1024], Q16) cutmix: the tables of
    :class:`flashy_amd.data.DeviceMix`; ``in_size`` is the ``(H, W)`` the
    cutmix box is drawn for."""
    ext = require()
    _check_mix_row(row)
    assert lam_table is not None or sq_table is not None
    for table, dtype in ((lam_table, torch.float32), (sq_table, torch.int32)):
        if table is not None:
            assert table.dtype == dtype and tuple(table.shape) == (1024,)
            assert table.is_contiguous() and table.device == row.device
    assert step_dev.dtype == torch.int64 and step_dev.is_cuda
    assert step_dev.numel() == 1
    H, W = int(in_size[0]), int(in_size[1])
    assert 1 <= H <= 32767 and 1 <= W <= 32767, in_size
    assert 0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0
    ext.batch_mix_draw(row.data_ptr(),
                       lam_table.data_ptr() if lam_table is not None else 0,
                       sq_table.data_ptr() if sq_table is not None else 0,
                       step_dev.data_ptr(), H, W, seed & (2 ** 64 - 1),
                       round(prob * 2 ** 24), round(switch_prob * 2 ** 24),
                       lam_table is not None, sq_table is not None, _stream())


def batch_mix(x: torch.Tensor, row: torch.Tensor) -> None:
    """Mix the bf16 NHWC batch ``x`` [N, H, W, C] in place, sample ``i``
    with sample ``N-1-i``, as the int32 [8] device ``row`` says: mode 1
    blends ``bf16(lam*x_i + (1-lam)*x_p)`` (every fp32 operation rounded on
    its own), mode 2 swaps the box ``[y0, y1) x [x0, x1)``, any other mode
    leaves ``x`` alone.  Any row is safe: the kernel clamps the box into the
    image."""
    ext = require()
    _check_mix_row(row)
    assert x.dtype == torch.bfloat16 and x.is_cuda and x.device == row.device
    assert x.dim() == 4 and x.is_contiguous(), (x.shape, x.stride())
    assert x.data_ptr() % 16 == 0, "16-byte vectors need an aligned batch"
    N, H, W, C = x.shape
    assert H <= 32767 and W <= 32767, x.shape
    if x.numel():
        ext.batch_mix(x.data_ptr(), row.data_ptr(), N, H, W, C, _stream())


def maxpool_fwd(x: torch.Tensor, y: torch.Tensor, argmax: torch.Tensor,
                d: "ConvDims") -> None:
    assert d.C % 8 == 0
    require().maxpool_fwd(x.data_ptr(), y.data_ptr(), argmax.data_ptr(), *d,
                          _stream())


def maxpool_bwd(dy: torch.Tensor, argmax: torch.Tensor, dx: torch.Tensor,
                d: "ConvDims") -> None:
    require().maxpool_bwd(dy.data_ptr(), argmax.data_ptr(), dx.data_ptr(), *d,
                          _stream())


# ---------------------------------------------------------------------------
# convolution kernels (NHWC bf16 implicit GEMM; see flashy_amd/nn.py)
# All activation tensors are logical-NHWC [N, H, W, C]; weights [K, R, S, C].
# ---------------------------------------------------------------------------

class ConvDims(tp.NamedTuple):
    N: int; H: int; W: int; C: int
    K: int; R: int; S: int
    Ho: int; Wo: int
    stride: int; pad: int

    @staticmethod
    def infer(x: torch.Tensor, w: torch.Tensor, stride: int, pad: int) -> "ConvDims":
        N, H, W, C = x.shape
        K, R, S, Cw = w.shape
        assert C == Cw, (x.shape, w.shape)
        Ho = (H + 2 * pad - R) // stride + 1
        Wo = (W + 2 * pad - S) // stride + 1
        return ConvDims(N, H, W, C, K, R, S, Ho, Wo, stride, pad)


def _splitk_plan(M: int, ktiles: int, red_stages: int):
    """Split the reduction over grid.z into fp32 workspace slices when (a)
    the single-pass grid underfills the 256-CU chip, or (b) the K loop is
    long (>= 48 stages) — measured: splitting a 72-stage reduction to
    ~14 stages/slice wins 20-25% even on a full grid (shorter serial
    chains, more concurrent waves).  Returns zn (or 0 = single pass)."""
    if red_stages < 4:
        return 0
    blocks64 = ((M + 63) // 64) * ktiles
    if blocks64 >= 208:
        fill = 0
    else:
        fill = max(2, min((256 + blocks64 - 1) // max(1, blocks64),
                          red_stages // 2))
    longk = red_stages // 14 if red_stages >= 48 else 0
    zn = min(max(fill, longk), 8)
    return zn if zn >= 2 else 0


def _underfill_zn(M: int, channels: int, stages: int) -> int:
    """Under-fill forcing for small-M long-reduction layers (r4-class): the
    8-wave grid of 256-row tiles underfills the chip without a K split, so
    slice the reduction until ~160 blocks exist and the 8-wave split-K
    launcher engages.  ``channels`` is the GEMM column count (K for fwd, C
    for dgrad).  Returns zn (0 = leave it single pass)."""
    if stages < 16:
        return 0
    bn8 = 128 if channels % 128 == 0 else 64
    tiles8 = ((M + 255) // 256) * (channels // bn8)
    if not tiles8 or tiles8 >= 160:
        return 0
    zn = min(max(2, -(-160 // tiles8)), 8, stages // 8)
    return 0 if zn < 2 else zn


def conv_fwd(x: torch.Tensor, w: torch.Tensor, y: torch.Tensor, d: ConvDims,
             relu: bool = False,
             want_stats: bool = False) -> tp.Optional[tp.Tuple[torch.Tensor, int]]:
    """Forward conv.  With ``want_stats`` the conv also emits BatchNorm
    partials [2][K][msplit] of its output — from the kernel epilogue
    (single-pass implicit-GEMM kernels) or from the split-K combine, whose
    partials are bitwise those of :func:`bn_stats` on ``y``; returns
    (partials, msplit) for :func:`bn_finalize`, else None (the small-C stem
    kernel emits none)."""
    ext = require()
    if d.C % 8 == 0:
        rsc = d.R * d.S * d.C
        assert d.K % 64 == 0 and rsc % 32 == 0, d
        M = d.N * d.Ho * d.Wo
        stages = (rsc + 63) // 64
        zn = 0
        if not ext.conv8_eligible(*d, False):
            zn = _splitk_plan(M, d.K // 64, stages) or \
                _underfill_zn(M, d.K, stages)
        if zn:
            spz = (stages + zn - 1) // zn
            zeff = (stages + spz - 1) // spz
            ws = torch.empty(zeff * M * d.K, dtype=torch.float32, device=x.device)
            ext.conv_fwd_splitk(x.data_ptr(), w.data_ptr(), ws.data_ptr(), *d,
                                spz, _stream())
            if want_stats:
                # the combine holds every output value: emit the BN partials
                # from it instead of re-reading y in bn_stats (same msplit
                # and summation order, so the partials are bitwise the same)
                assert not relu, "a conv feeding BatchNorm has no fused ReLU"
                msplit = bn_msplit(M, d.K)
                partials = torch.empty(2 * d.K * msplit, dtype=torch.float32,
                                       device=x.device)
                ext.splitk_combine_stats(ws.data_ptr(), y.data_ptr(),
                                         partials.data_ptr(), M, d.K, zeff,
                                         msplit, _stream())
                return partials, msplit
            ext.splitk_combine(ws.data_ptr(), y.data_ptr(), M * d.K, zeff, relu,
                               _stream())
        else:
            stats = None
            bn_ptr = 0
            if want_stats:
                msplit = ext.conv_fwd_msplit(*d)
                partials = torch.empty(2 * d.K * msplit, dtype=torch.float32,
                                       device=x.device)
                stats = (partials, msplit)
                bn_ptr = partials.data_ptr()
            ext.conv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), *d, relu,
                         bn_ptr, _stream())
            return stats
    else:
        assert not relu
        M = d.N * d.Ho * d.Wo
        if d.C == 3 and d.K % 64 == 0 and d.R <= 8 and d.S <= 8 \
                and M >= 100_000:
            return _stem_fwd8(ext, x, w, y, d, want_stats)
        assert d.R * d.S * d.C <= 160 and d.K == 64, d
        ext.conv_stem_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), *d, _stream())
    return None


def _stem_pad_x(ext, x: torch.Tensor, d: ConvDims) -> tp.Tuple[torch.Tensor, int, int]:
    """Zero-padded C'=4 / 8x8-tap copy of the C=3 stem input (see
    csrc/conv_fwd8.hip stem helpers)."""
    Hp = (d.Ho - 1) * d.stride + 8
    Wp = (d.Wo - 1) * d.stride + 8
    xp = torch.empty(d.N, Hp, Wp, 4, dtype=torch.bfloat16, device=x.device)
    ext.stem_pad_x(x.data_ptr(), xp.data_ptr(), d.N, d.H, d.W, Hp, Wp, d.pad,
                   _stream())
    return xp, Hp, Wp


def _stem_fwd8(ext, x, w, y, d: ConvDims, want_stats: bool):
    """Large-M C=3 stem through the 8-wave kernel: pad channels to 4 and
    taps to 8x8 (zero weights), rsc' = 256 — the direct small-C kernel runs
    at ~47 TF/s on the 224px stem; this path reaches the implicit-GEMM rate
    at 147/256 useful work."""
    xp, Hp, Wp = _stem_pad_x(ext, x, d)
    wp = torch.empty(d.K, 8, 8, 4, dtype=torch.bfloat16, device=x.device)
    ext.stem_pad_w(w.data_ptr(), wp.data_ptr(), d.K, d.R, d.S, _stream())
    M = d.N * d.Ho * d.Wo
    mtiles = (M + 255) // 256
    stats = None
    bn_ptr = 0
    if want_stats:
        partials = torch.empty(2 * d.K * mtiles, dtype=torch.float32,
                               device=x.device)
        stats = (partials, mtiles)
        bn_ptr = partials.data_ptr()
    ext.conv_fwd8_direct(xp.data_ptr(), wp.data_ptr(), y.data_ptr(),
                         d.N, Hp, Wp, 4, d.K, 8, 8, d.Ho, d.Wo, d.stride, 0,
                         False, bn_ptr, 64, mtiles, _stream())
    return stats


def conv_stem_dgrad(dout: torch.Tensor, w_krsc: torch.Tensor,
                    dx: torch.Tensor, d: ConvDims) -> None:
    """dX of a small-C edge conv (C <= 8, K == 64); weights in KRSC layout."""
    assert d.C <= 8 and d.K == 64 and d.R * d.S * d.C <= 160, d
    require().conv_stem_dgrad(dout.data_ptr(), w_krsc.data_ptr(),
                              dx.data_ptr(), *d, _stream())


def conv_dgrad(dout: torch.Tensor, w_rsck: torch.Tensor, dx: torch.Tensor,
               d: ConvDims) -> None:
    ext = require()
    assert d.C % 64 == 0 and d.K % 32 == 0, d
    M = d.N * d.H * d.W
    rsk = d.R * d.S * d.K
    stages = (rsk + 63) // 64
    zn = 0
    # stride 2: a form without zero-filled MFMA work (parity classes, 1x1
    # quarter GEMM) runs single pass; split-K is for what that plan declines
    if d.stride == 2 and ext.conv_dgrad_s2_plan(*d)[0]:
        pass
    elif not ext.conv8_eligible(*d, True):
        zn = _splitk_plan(M, d.C // 64, stages)
        if zn == 0 and d.stride == 1:
            zn = _underfill_zn(M, d.C, stages)
    if zn:
        spz = (stages + zn - 1) // zn
        zeff = (stages + spz - 1) // spz
        ws = torch.empty(zeff * M * d.C, dtype=torch.float32, device=dout.device)
        ext.conv_dgrad_splitk(dout.data_ptr(), w_rsck.data_ptr(), ws.data_ptr(),
                              *d, spz, _stream())
        ext.splitk_combine(ws.data_ptr(), dx.data_ptr(), M * d.C, zeff, False,
                           _stream())
    else:
        ext.conv_dgrad(dout.data_ptr(), w_rsck.data_ptr(), dx.data_ptr(), *d,
                       _stream())


DGRAD_S2_FORMS = {"generic": 0, "par8": 1, "par4": 2, "scat2": 3}


def conv_dgrad_s2_plan(d: ConvDims) -> tp.Tuple[str, int]:
    """(form, tile) the stride-2 dgrad plan picks for ``d``: "par8" (8-wave
    parity classes, tile = BN), "par4" (4-wave parity classes, tile = BM),
    "scat2" (1x1 quarter GEMM, tile = BN) or ("none", 0)."""
    form, tile = require().conv_dgrad_s2_plan(*d)
    names = {v: k for k, v in DGRAD_S2_FORMS.items() if v}
    return names.get(form, "none"), tile


def conv_dgrad_s2_form(dout: torch.Tensor, w_rsck: torch.Tensor,
                       dx: torch.Tensor, d: ConvDims, form: str,
                       tile: int) -> None:
    """Stride-2 dgrad through one named form, whatever the plan would pick
    (tests and scripts/dgrad_s2_sweep.py): "par8" / "par4" / "scat2" as in
    :func:`conv_dgrad_s2_plan`, or "generic" (the zero-filled single-pass
    kernels, ``tile`` ignored); raises where the form cannot run the shape."""
    require().conv_dgrad_s2_form(dout.data_ptr(), w_rsck.data_ptr(),
                                 dx.data_ptr(), *d, DGRAD_S2_FORMS[form],
                                 tile, _stream())


def weight_transpose_batched(src: torch.Tensor, dst: torch.Tensor,
                             meta: torch.Tensor, n_convs: int,
                             max_elems: int) -> None:
    require().weight_transpose_batched(src.data_ptr(), dst.data_ptr(),
                                       meta.data_ptr(), n_convs, max_elems,
                                       _stream())


def weight_transpose(w: torch.Tensor, wt: torch.Tensor) -> None:
    ext = require()
    K = w.shape[0]
    rsc = w.numel() // K
    ext.weight_transpose(w.data_ptr(), wt.data_ptr(), K, rsc, _stream())


def conv_wgrad(x: torch.Tensor, dout: torch.Tensor, dw: torch.Tensor,
               d: ConvDims, n_splits: tp.Optional[int] = None) -> None:
    """Accumulates (+=) fp32 weight grads; dw must be zeroed or hold the
    running gradient (matches autograd accumulate semantics)."""
    ext = require()
    rsc = d.R * d.S * d.C
    if d.C % 8 == 0:
        assert d.K % 64 == 0 and rsc % 64 == 0, d
        if n_splits is None:
            forced = os.environ.get("FLASHY_WGRAD_SPLITS")
            if forced:  # e.g. =1 -> deterministic wgrad (no atomic splits)
                n_splits = int(forced)
            else:
                tiles = (d.K // 64) * (rsc // 64)
                n_splits = max(1, min(1024 // tiles if tiles else 1, 128))
                M = d.N * d.Ho * d.Wo
                n_splits = max(1, min(n_splits, M // 32 or 1))
        ext.conv_wgrad(x.data_ptr(), dout.data_ptr(), dw.data_ptr(), *d,
                       n_splits, _stream())
    else:
        M = d.N * d.Ho * d.Wo
        if d.C == 3 and d.K % 64 == 0 and d.R <= 8 and d.S <= 8 \
                and M >= 100_000:
            # padded-stem wgrad: pad x to C'=4 / 8x8 taps, run the regular
            # implicit-GEMM wgrad on rsc'=256, unpad-accumulate into dw
            xp, Hp, Wp = _stem_pad_x(ext, x, d)
            dwp = torch.zeros(d.K * 256, dtype=torch.float32, device=x.device)
            dp = ConvDims(d.N, Hp, Wp, 4, d.K, 8, 8, d.Ho, d.Wo, d.stride, 0)
            tiles = (d.K // 64) * 4
            ns = max(1, min(1024 // tiles, 128, M // 32 or 1))
            forced = os.environ.get("FLASHY_WGRAD_SPLITS")
            if forced:
                ns = int(forced)
            ext.conv_wgrad(xp.data_ptr(), dout.data_ptr(), dwp.data_ptr(),
                           *dp, ns, _stream())
            ext.stem_unpad_dw(dwp.data_ptr(), dw.data_ptr(), d.K, d.R, d.S,
                              _stream())
            return
        assert rsc <= 160, d  # small-C stem kernels stage taps/weights in LDS
        ext.conv_stem_wgrad(x.data_ptr(), dout.data_ptr(), dw.data_ptr(), *d,
                            _stream())


# ---------------------------------------------------------------------------
# batchnorm kernels (NHWC training BN; see flashy_amd/nn.py)
# ---------------------------------------------------------------------------

def bn_msplit(M: int, C: int) -> int:
    """Blocks along M for the BN reductions: ~256 blocks saturate the chip
    while keeping the partial-combine kernels cheap."""
    cols = max(1, C // 64)
    msplit = max(1, min(512 // cols, 512))
    msplit = max(1, min(msplit, (M + 31) // 32))
    if msplit >= 4:
        msplit &= ~3  # multiple of 4: per-channel partial rows stay 16B-aligned
    return msplit


def _bn_width(name: str, C: int, mult: int) -> None:
    """The reductions walk 64-channel groups (grid C/64) and the combine and
    elementwise kernels 8-channel octets (grid C/8, 16-byte lanes): any other
    width would leave channels unwritten, so it is refused before a launch."""
    if C < mult or C % mult:
        raise ValueError(f"{name}: C = {C} must be a positive multiple of "
                         f"{mult}")


def bn_stats(x: torch.Tensor, partials: torch.Tensor, M: int, C: int,
             msplit: int) -> None:
    _bn_width("bn_stats", C, 64)
    require().bn_stats(x.data_ptr(), partials.data_ptr(), M, C, msplit, _stream())


def bn_finalize(partials, msplit: int, gamma, beta, rmean, rvar, work,
                M: int, C: int, eps: float, momentum: float,
                update_running: bool) -> None:
    _bn_width("bn_finalize", C, 8)
    require().bn_finalize(partials.data_ptr(), msplit, gamma.data_ptr(),
                          beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(),
                          work.data_ptr(), M, C, eps, momentum,
                          update_running, _stream())


def bn_apply(x, res, y, work, M: int, C: int, relu: bool,
             slope: float = 0.0) -> None:
    _bn_width("bn_apply", C, 8)
    require().bn_apply(x.data_ptr(), res.data_ptr() if res is not None else 0,
                       y.data_ptr(), work.data_ptr(), M, C, relu, slope,
                       _stream())


def bn_bwd_reduce(dy, y, x, work, dz_out, partials, M: int, C: int,
                  msplit: int, relu: bool, slope: float = 0.0) -> None:
    _bn_width("bn_bwd_reduce", C, 64)
    require().bn_bwd_reduce(dy.data_ptr(), y.data_ptr(), x.data_ptr(),
                            work.data_ptr(), dz_out.data_ptr(),
                            partials.data_ptr(), M, C, msplit, relu, slope,
                            _stream())


def bn_bwd_grads(partials, msplit: int, bsums, dgamma, dbeta, C: int) -> None:
    _bn_width("bn_bwd_grads", C, 8)
    require().bn_bwd_grads(partials.data_ptr(), msplit, bsums.data_ptr(),
                           dgamma.data_ptr(), dbeta.data_ptr(), C, _stream())


def bn_bwd_apply(dz, x, work, bsums, dx, M: int, C: int) -> None:
    _bn_width("bn_bwd_apply", C, 8)
    require().bn_bwd_apply(dz.data_ptr(), x.data_ptr(), work.data_ptr(),
                           bsums.data_ptr(), dx.data_ptr(), M, C, _stream())


BN_BWD_SMALL_FORMS = {"chain": 0, "regs8": 1}


def bn_small_plan(M: int, C: int) -> tp.Tuple[str, str]:
    """(forward form, backward form) the plan picks for a training BatchNorm
    over ``[M, C]``: forward "small" (finalize + apply in one kernel) or
    "chain"; backward one of :data:`BN_BWD_SMALL_FORMS` (reduce + grads +
    apply in one kernel, 8 channels per block, its rows kept in registers) or
    "chain" (the separate kernels).  ``C % 64 != 0`` is always ("chain",
    "chain"), whose reductions then raise: no kernel produces such
    statistics."""
    fwd, bwd = require().bn_small_plan(M, C)
    names = {v: k for k, v in BN_BWD_SMALL_FORMS.items()}
    return ("small" if fwd else "chain"), names[bwd]


def bn_fwd_small(partials, msplit: int, gamma, beta, rmean, rvar, work, x,
                 res, y, M: int, C: int, eps: float, momentum: float,
                 update_running: bool, relu: bool, slope: float = 0.0) -> None:
    """:func:`bn_finalize` + :func:`bn_apply` in one launch, whatever the plan
    says (tests and scripts/bn_small_sweep.py); bitwise the chain's ``y``,
    ``work`` and running statistics.  Raises where it cannot run the shape."""
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == M * C
    assert res is None or res.is_contiguous()
    require().bn_fwd_small(
        partials.data_ptr(), msplit, gamma.data_ptr(), beta.data_ptr(),
        rmean.data_ptr(), rvar.data_ptr(), work.data_ptr(), x.data_ptr(),
        res.data_ptr() if res is not None else 0, y.data_ptr(), M, C, eps,
        momentum, update_running, relu, slope, 1, _stream())


def bn_bwd_small(dy, y, x, work, dz, dgamma, dbeta, dx, M: int, C: int,
                 relu: bool, slope: float = 0.0, write_dz: bool = True,
                 form: str = "regs8") -> None:
    """:func:`bn_bwd_reduce` + :func:`bn_bwd_grads` + :func:`bn_bwd_apply` in
    one launch through the named form, whatever the plan says.  ``dgamma`` /
    ``dbeta`` are accumulated (+=); ``dz`` is written only with ``write_dz``
    (and may be None without it).
    Raises where the form cannot run the shape."""
    assert all(t.is_contiguous() for t in (dy, y, x, dx))
    assert x.numel() == M * C
    assert dz.is_contiguous() if write_dz else True
    if form == "chain":
        raise ValueError("bn_bwd_small: 'chain' is not a single-kernel form")
    require().bn_bwd_small(
        dy.data_ptr(), y.data_ptr(), x.data_ptr(), work.data_ptr(),
        dz.data_ptr() if dz is not None else 0, dgamma.data_ptr(),
        dbeta.data_ptr(), dx.data_ptr(),
        M, C, relu, slope, write_dz, BN_BWD_SMALL_FORMS[form], _stream())


# ---------------------------------------------------------------------------
# loss kernels (fused forward+input-grad; see flashy_amd/functional.py)
# ---------------------------------------------------------------------------

def _check_loss_out(x: torch.Tensor, dx: torch.Tensor,
                    loss_sum: torch.Tensor) -> None:
    """The kernels write ``dx`` row-major through its pointer and add into
    ``loss_sum[0]``: ``dx`` is a contiguous twin of ``x``, ``loss_sum`` an
    fp32 tensor on the same device."""
    assert x.is_cuda and x.is_contiguous()
    assert dx.is_contiguous() and dx.shape == x.shape
    assert dx.dtype == x.dtype and dx.device == x.device
    assert loss_sum.dtype == torch.float32 and loss_sum.numel() >= 1
    assert loss_sum.device == x.device


def _check_targets(logits: torch.Tensor, *targets) -> None:
    B = logits.shape[0]
    for t in targets:
        if t is not None:
            assert t.dtype == torch.int64 and tuple(t.shape) == (B,)
            assert t.is_contiguous() and t.device == logits.device


def cross_entropy_fwd_bwd(logits: torch.Tensor, target: torch.Tensor,
                          dlogits: torch.Tensor, loss_sum: torch.Tensor,
                          loss_scale: float, grad_scale: float) -> None:
    """dlogits = (softmax - onehot) * grad_scale, loss_sum[0] += the rows'
    loss * loss_scale.  A target outside [0, C) marks no class (its row's
    loss is lse); nothing on the host checks the range."""
    ext = require()
    B, C = logits.shape
    _check_loss_out(logits, dlogits, loss_sum)
    _check_targets(logits, target)
    ext.cross_entropy(logits.data_ptr(), target.data_ptr(), dlogits.data_ptr(),
                      loss_sum.data_ptr(), B, C, loss_scale, grad_scale,
                      _is_bf16(logits), _stream())


def cross_entropy_mix_fwd_bwd(logits: torch.Tensor, target: torch.Tensor,
                              target_b: tp.Optional[torch.Tensor],
                              lam: tp.Optional[torch.Tensor],
                              dlogits: torch.Tensor, loss_sum: torch.Tensor,
                              label_smoothing: float, loss_scale: float,
                              grad_scale: float) -> None:
    """Cross-entropy against the mixed, smoothed target ``(1-eps) *
    (lam*onehot(target) + (1-lam)*onehot(target_b)) + eps/C``.  ``target_b``
    None means ``target``; ``lam`` is a one-element fp32 device tensor the
    kernel reads (None: 1), so a captured launch follows its value."""
    ext = require()
    B, C = logits.shape
    _check_loss_out(logits, dlogits, loss_sum)
    _check_targets(logits, target, target_b)
    if lam is not None:
        assert lam.dtype == torch.float32 and lam.numel() == 1
        assert lam.device == logits.device
    assert 0.0 <= label_smoothing <= 1.0, label_smoothing
    ext.cross_entropy_mix(logits.data_ptr(), target.data_ptr(),
                          target_b.data_ptr() if target_b is not None else 0,
                          lam.data_ptr() if lam is not None else 0,
                          dlogits.data_ptr(), loss_sum.data_ptr(), B, C,
                          float(label_smoothing), loss_scale, grad_scale,
                          _is_bf16(logits), _stream())


def bce_logits_fwd_bwd(x: torch.Tensor, dx: torch.Tensor,
                       loss_sum: torch.Tensor, target: float,
                       loss_scale: float, grad_scale: float) -> None:
    ext = require()
    _check_loss_out(x, dx, loss_sum)
    ext.bce_logits(x.data_ptr(), dx.data_ptr(), loss_sum.data_ptr(), x.numel(),
                   target, loss_scale, grad_scale, _is_bf16(x), _stream())


def mse_fwd_bwd(x: torch.Tensor, t: torch.Tensor, dx: torch.Tensor,
                loss_sum: torch.Tensor, loss_scale: float,
                grad_scale: float) -> None:
    ext = require()
    _check_loss_out(x, dx, loss_sum)
    assert t.is_contiguous() and t.dtype == x.dtype and t.shape == x.shape
    assert t.device == x.device
    ext.mse(x.data_ptr(), t.data_ptr(), dx.data_ptr(), loss_sum.data_ptr(),
            x.numel(), loss_scale, grad_scale, _is_bf16(x), _stream())


def accuracy_count(logits: torch.Tensor, target: torch.Tensor,
                   out: torch.Tensor) -> None:
    """out[0] += number of rows whose argmax == target (caller zeroes out)."""
    ext = require()
    B, C = logits.shape
    assert logits.is_cuda and logits.is_contiguous()
    _check_targets(logits, target)
    assert out.dtype == torch.float32 and out.device == logits.device
    ext.accuracy(logits.data_ptr(), target.data_ptr(), out.data_ptr(), B, C,
                 _is_bf16(logits), _stream())


# ---------------------------------------------------------------------------
# linear (fc) kernels — fp32, small shapes (see csrc/linear.hip)
# ---------------------------------------------------------------------------

def linear_fwd(x: torch.Tensor, w: torch.Tensor,
               b: tp.Optional[torch.Tensor], y: torch.Tensor) -> None:
    ext = require()
    B, I = x.shape
    O = w.shape[0]
    assert x.dtype == torch.float32 and w.shape == (O, I)
    ext.linear_fwd(x.data_ptr(), w.data_ptr(),
                   b.data_ptr() if b is not None else 0,
                   y.data_ptr(), B, I, O, _stream())


def linear_dx(dy: torch.Tensor, w: torch.Tensor, dx: torch.Tensor) -> None:
    ext = require()
    B, O = dy.shape
    I = w.shape[1]
    ext.linear_dx(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), B, I, O,
                  _stream())


def linear_dw(x: torch.Tensor, dy: torch.Tensor, dw: torch.Tensor,
              db: tp.Optional[torch.Tensor]) -> None:
    """Accumulates (+=) into dw / db (autograd accumulate semantics)."""
    ext = require()
    B, I = x.shape
    O = dy.shape[1]
    ext.linear_dw(x.data_ptr(), dy.data_ptr(), dw.data_ptr(),
                  db.data_ptr() if db is not None else 0, B, I, O, _stream())


# ---------------------------------------------------------------------------
# classifier head: global average pool (+ small fc) — see csrc/head.hip
# ---------------------------------------------------------------------------

def pool_linear_fwd(x: torch.Tensor, w: tp.Optional[torch.Tensor],
                    b: tp.Optional[torch.Tensor], pooled: torch.Tensor,
                    y: tp.Optional[torch.Tensor]) -> None:
    """pooled[N,C] = mean over HW of NHWC bf16 ``x``; with ``w`` [O,C] also
    y[N,O] = pooled @ w^T + b in the same kernel (``w=None``: pool only)."""
    ext = require()
    N, H, W, C = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and C % 8 == 0
    assert pooled.dtype == torch.float32 and pooled.shape == (N, C)
    assert C * max(1, 2048 // C) * 4 <= 65536, f"C={C} exceeds the LDS row"
    O = 0
    if w is not None:
        O = w.shape[0]
        assert w.dtype == torch.float32 and w.shape == (O, C) \
            and w.is_contiguous() and y is not None and y.shape == (N, O)
    ext.pool_fc_fwd(x.data_ptr(), w.data_ptr() if w is not None else 0,
                    b.data_ptr() if b is not None else 0, pooled.data_ptr(),
                    y.data_ptr() if y is not None else 0, N, H * W, C, O,
                    _stream())


def head_dw(pooled: torch.Tensor, dy: torch.Tensor,
            dw: tp.Optional[torch.Tensor],
            db: tp.Optional[torch.Tensor]) -> None:
    """Accumulates (+=) dw[O,C] / db[O] from dy[B,O] and the saved pooled
    [B,C]; either target may be None (frozen).  Deterministic."""
    B, C = pooled.shape
    O = dy.shape[1]
    assert dy.dtype == torch.float32 and dy.is_contiguous()
    require().head_dw(pooled.data_ptr(), dy.data_ptr(),
                      dw.data_ptr() if dw is not None else 0,
                      db.data_ptr() if db is not None else 0, B, C, O,
                      _stream())


def head_dx(dy: torch.Tensor, w: tp.Optional[torch.Tensor],
            dx: torch.Tensor) -> None:
    """dx[N,H,W,C] (bf16) = (dy @ w) / HW broadcast over HW; with ``w=None``
    ``dy`` is the fp32 [N,C] pooled gradient (plain pool backward)."""
    N, H, W, C = dx.shape
    assert dx.dtype == torch.bfloat16 and dx.is_contiguous() and C % 8 == 0
    assert dy.dtype == torch.float32 and dy.is_contiguous()
    O = 0
    if w is not None:
        O = w.shape[0]
        assert w.shape == (O, C) and w.is_contiguous() and dy.shape == (N, O)
    else:
        assert dy.shape == (N, C)
    require().head_dx(dy.data_ptr(), w.data_ptr() if w is not None else 0,
                      dx.data_ptr(), N, H * W, C, O, _stream())
