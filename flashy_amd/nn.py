# Copyright (c) Flashy-AMD authors.
"""Native NHWC modules backed by the gfx950 kernels.

Layout convention: activations are logical-NHWC tensors ``[N, H, W, C]``
(plain contiguous — the same bytes as torch channels_last), conv weights are
``[K, R, S, C]``.  These modules are GPU-only (bf16 activations, fp32 master
params) and pair with :class:`flashy_amd.optim.FlatOptimizer`:

* weight gradients are fp32 and written (accumulated) directly into
  ``param.grad`` when it exists — with a flat optimizer that is the flat
  gradient buffer, so conv/BN backward needs no extra accumulate kernels;
* when the optimizer keeps a bf16 mirror of the flat params
  (``bf16_mirror=True``), forward reads the mirror view stashed on the
  parameter (``param._bf16_mirror``) — zero weight-cast kernels per step.

Replaces the ResNet conv+bn+relu torch chains of the reference workload
 with MFMA implicit-GEMM conv and fused NHWC BatchNorm
(+residual +ReLU) kernels.
"""
from __future__ import annotations

import math
import os
import typing as tp

import torch
from torch import nn

from . import ops


def _weight_bf16(w: torch.Tensor) -> torch.Tensor:
    mirror = getattr(w, "_bf16_mirror", None)
    if mirror is not None:
        return mirror
    return w.detach().to(torch.bfloat16)


def _grad_target(p: torch.Tensor) -> tp.Tuple[torch.Tensor, bool]:
    """(fp32 accumulation buffer, direct) — direct=True writes into
    ``p.grad`` in place (flat-optimizer fast path), else a temp returned to
    autograd for accumulation."""
    if p.grad is not None and p.grad.is_contiguous():
        return p.grad, True
    return torch.zeros_like(p, memory_format=torch.contiguous_format), False


# FLASHY_BN_GRAD_SOURCES=0 (read once, at import) restores the unfused
# backward chain in the same build: autograd's add kernel for an activation
# two layers read, and a split-K dgrad's own combine kernel (A/B traces; the
# tests flip the variable itself).
_FUSE_GRAD_SOURCES = os.environ.get("FLASHY_BN_GRAD_SOURCES", "1") != "0"
# The single-kernel backward walks all M rows of its 8 channels on one CU, so
# fp32 slices cost it M * zn rows of 32 bytes: at (M, C) = (1024, 512), zn = 5
# it took 14.9 us against 7.3 + 4.4 us for the plain form plus the combine
# kernel (profiles/README.md, r07a).  The added time is taken as linear in
# M * zn (7.6 us at 5120); it stays under 3 us, below a combine launch, up to
# 2048 rows.  Larger workspaces keep their combine kernel.
_SMALL_FORM_WS_ROWS = 2048


class _GradLink:
    """Side channel from the one conv that reads a BatchNorm's output to that
    BatchNorm's backward, for a split-K dgrad that leaves its fp32 slices
    un-combined (``ops.conv_dgrad(defer_combine=True)``).  The conv claims
    the link in forward and posts ``(dx, ws, zn)`` in backward; ``dx`` is the
    unwritten tensor it returns to autograd.  The BatchNorm backward takes
    the post and reads the slices, but only if that very tensor object
    arrives, unmodified, as one of its gradients: if autograd summed it with
    another gradient (in place or not), or a hook replaced it, its content
    is lost and the backward raises instead of computing from it.  The link
    keeps ``dx`` and ``ws`` alive until they are taken.

    What stays unprotected is a reader of the conv's input gradient other
    than the BatchNorm backward (a tensor hook or ``retain_grad`` on the
    BatchNorm output, ``torch.autograd.grad`` with respect to it): it sees
    unwritten memory.  ``Conv2d.dgrad_to_bn`` / ``sole_reader`` are set by a
    model for whose tensors that cannot happen, never by default."""
    __slots__ = ("claimed", "post", "max_ws_rows")

    def __init__(self, max_ws_rows: tp.Optional[int] = None):
        self.claimed = False
        self.post = None
        # the reader takes slices only while M * zn stays within this
        self.max_ws_rows = max_ws_rows

    def take(self, grads: tp.Sequence[tp.Optional[torch.Tensor]]
             ) -> tp.Optional[tp.Tuple[int, torch.Tensor, int]]:
        """(index of the deferred gradient in ``grads``, ws, zn) or None."""
        post, self.post = self.post, None
        if post is None:
            return None
        dx, version, ws, zn = post
        for i, g in enumerate(grads):
            if g is dx and g._version == version:
                return i, ws, zn
        raise RuntimeError(
            "a split-K dgrad deferred its combine to this BatchNorm's "
            "backward, but its gradient did not arrive as it was returned "
            "(summed with another gradient, or replaced by a hook): clear "
            "Conv2d.dgrad_to_bn / sole_reader for the conv that reads this "
            "BatchNorm")


class _ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, stride: int, pad: int,
                input_grad: bool, wt_cached: tp.Optional[torch.Tensor],
                want_stats: bool = False,
                link: tp.Optional[_GradLink] = None):
        w16 = _weight_bf16(w)
        d = ops.ConvDims.infer(x, w16, stride, pad)
        y = x.new_empty((d.N, d.Ho, d.Wo, d.K))
        stats = ops.conv_fwd(x, w16, y, d, want_stats=want_stats)
        if stats is not None:
            # consumed by the following BatchNorm2d (skips its stats pass)
            y._bn_stats = stats
        ctx.save_for_backward(x, w16)
        ctx.dims = d
        ctx.input_grad = input_grad
        ctx.w_ref = w
        ctx.wt_cached = wt_cached
        ctx.link = link
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w16 = ctx.saved_tensors
        d: ops.ConvDims = ctx.dims
        dy = dy.contiguous()
        dw_buf = None
        direct = True
        if ctx.needs_input_grad[1]:  # skip wgrad entirely for frozen weights
            dw_buf, direct = _grad_target(ctx.w_ref)
            ops.conv_wgrad(x, dy, dw_buf, d)
        dx = None
        if ctx.input_grad:
            dx = x.new_empty(x.shape)
            if d.C % 64 == 0:
                wt = ctx.wt_cached  # RSCK copy refreshed per step (WtCache)
                if wt is None:
                    wt = w16.new_empty((d.R, d.S, d.C, d.K))
                    ops.weight_transpose(w16, wt)
                link = ctx.link
                deferred = ops.conv_dgrad(
                    dy, wt, dx, d, defer_combine=link is not None,
                    defer_max_rows=link.max_ws_rows if link else None)
                if deferred is not None:
                    # dx stays unwritten: the BatchNorm backward that
                    # produced x sums the slices itself (_GradLink)
                    link.post = (dx, dx._version, *deferred)
            else:  # small-C edge conv (e.g. a discriminator RGB stem)
                ops.conv_stem_dgrad(dy, w16, dx, d)
        return (dx, dw_buf if dw_buf is not None and not direct else None,
                None, None, None, None, None, None)


def _gconv_dims(x_shape, K: int, stride: int, pad: int) -> ops.ConvDims:
    N, H, W, C = x_shape
    return ops.ConvDims(N, H, W, C, K, 3, 3, (H + 2 * pad - 3) // stride + 1,
                        (W + 2 * pad - 3) // stride + 1, stride, pad)


class _GroupedConvFn(torch.autograd.Function):
    """Grouped 3x3 conv (csrc/conv_group.hip).  Emits no BatchNorm partials:
    a following BatchNorm2d runs its own statistics pass."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, stride: int, pad: int,
                groups: int, input_grad: bool):
        w16 = _weight_bf16(w).contiguous()
        x = x.contiguous()
        d = _gconv_dims(x.shape, w.shape[0], stride, pad)
        y = x.new_empty((d.N, d.Ho, d.Wo, d.K))
        ops.gconv_fwd(x, w16, y, d, groups)
        ctx.save_for_backward(x, w16)
        ctx.dims = d
        ctx.groups = groups
        ctx.input_grad = input_grad
        ctx.w_ref = w
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w16 = ctx.saved_tensors
        d: ops.ConvDims = ctx.dims
        dy = dy.contiguous()
        dw_buf = None
        direct = True
        if ctx.needs_input_grad[1]:  # skip wgrad entirely for frozen weights
            dw_buf, direct = _grad_target(ctx.w_ref)
            ops.gconv_wgrad(x, dy, dw_buf, d, ctx.groups)
        dx = None
        if ctx.input_grad:
            dx = x.new_empty(x.shape)
            ops.gconv_dgrad(dy, w16, dx, d, ctx.groups)
        return (dx, dw_buf if dw_buf is not None and not direct else None,
                None, None, None, None)


class _DepthwiseConvFn(torch.autograd.Function):
    """Depthwise k x k conv (csrc/conv_depthwise.hip), weight [C, k, k, 1].
    Emits no BatchNorm partials, as the grouped path."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, stride: int, pad: int,
                input_grad: bool):
        w16 = _weight_bf16(w).contiguous()
        x = x.contiguous()
        N, H, W, C = x.shape
        k = w.shape[1]
        d = ops.ConvDims(N, H, W, C, C, k, k, (H + 2 * pad - k) // stride + 1,
                         (W + 2 * pad - k) // stride + 1, stride, pad)
        y = x.new_empty((d.N, d.Ho, d.Wo, d.K))
        ops.dwconv_fwd(x, w16, y, d)
        ctx.save_for_backward(x, w16)
        ctx.dims = d
        ctx.input_grad = input_grad
        ctx.w_ref = w
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w16 = ctx.saved_tensors
        d: ops.ConvDims = ctx.dims
        dy = dy.contiguous()
        dw_buf = None
        direct = True
        if ctx.needs_input_grad[1]:  # skip wgrad entirely for frozen weights
            dw_buf, direct = _grad_target(ctx.w_ref)
            ops.dwconv_wgrad(x, dy, dw_buf, d)
        dx = None
        if ctx.input_grad:
            dx = x.new_empty(x.shape)
            ops.dwconv_dgrad(dy, w16, dx, d)
        return (dx, dw_buf if dw_buf is not None and not direct else None,
                None, None, None)


class _PatchConvFn(torch.autograd.Function):
    """Patch conv, kernel == stride, pad 0, 3 or 4 input channels
    (csrc/conv_patch.hip), weight [K, p, p, C]; backward-data reads the same
    KRSC weight.  Emits no BatchNorm partials, as the grouped path."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, stride: int,
                input_grad: bool):
        w16 = _weight_bf16(w).contiguous()
        x = x.contiguous()
        d = ops.ConvDims.infer(x, w16, stride, 0)
        y = x.new_empty((d.N, d.Ho, d.Wo, d.K))
        ops.patchconv_fwd(x, w16, y, d)
        ctx.save_for_backward(x, w16)
        ctx.dims = d
        ctx.input_grad = input_grad
        ctx.w_ref = w
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w16 = ctx.saved_tensors
        d: ops.ConvDims = ctx.dims
        dy = dy.contiguous()
        dw_buf = None
        direct = True
        if ctx.needs_input_grad[1]:  # skip wgrad entirely for frozen weights
            dw_buf, direct = _grad_target(ctx.w_ref)
            ops.patchconv_wgrad(x, dy, dw_buf, d)
        dx = None
        if ctx.input_grad:
            dx = x.new_empty(x.shape)
            ops.patchconv_dgrad(dy, w16, dx, d)
        return (dx, dw_buf if dw_buf is not None and not direct else None,
                None, None)


class _PointwiseConvFn(torch.autograd.Function):
    """Dense conv with kernel == stride in {1, 2}, pad 0 and a width off the
    64 grid (csrc/conv_point.hip), weight [K, p, p, C]; backward-data reads
    the same KRSC weight.  Emits no BatchNorm partials, as the grouped path."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, stride: int,
                input_grad: bool):
        w16 = _weight_bf16(w).contiguous()
        x = x.contiguous()
        d = ops.ConvDims.infer(x, w16, stride, 0)
        y = x.new_empty((d.N, d.Ho, d.Wo, d.K))
        ops.pwconv_fwd(x, w16, y, d)
        ctx.save_for_backward(x, w16)
        ctx.dims = d
        ctx.input_grad = input_grad
        ctx.w_ref = w
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w16 = ctx.saved_tensors
        d: ops.ConvDims = ctx.dims
        dy = dy.contiguous()
        dw_buf = None
        direct = True
        if ctx.needs_input_grad[1]:  # skip wgrad entirely for frozen weights
            dw_buf, direct = _grad_target(ctx.w_ref)
            ops.pwconv_wgrad(x, dy, dw_buf, d)
        dx = None
        if ctx.input_grad:
            dx = x.new_empty(x.shape)
            ops.pwconv_dgrad(dy, w16, dx, d)
        return (dx, dw_buf if dw_buf is not None and not direct else None,
                None, None)


class Conv2d(nn.Module):
    """NHWC bf16 conv (no bias, as in ResNet).  Weight: [K, R, S, C] fp32;
    a patch conv (kernel == stride, no padding, 3 or 4 input channels:
    :func:`flashy_amd.ops.patchconv_supported`) runs the patch kernels; a
    dense conv with kernel == stride in {1, 2}, no padding and a width off
    the 64 grid (:func:`flashy_amd.ops.pwconv_supported`) runs the pointwise
    kernels and sets ``pointwise``;
    with ``groups > 1`` a grouped 3x3 conv with weight [K, 3, 3, C // groups]
    (the shapes :func:`flashy_amd.ops.gconv_supported` accepts), or, with
    ``groups == in_channels == out_channels``, a depthwise k x k conv with
    weight [C, k, k, 1] (:func:`flashy_amd.ops.dwconv_supported`); anything
    else raises ``ValueError`` here."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int,
                 stride: int = 1, padding: int = 0, input_grad: bool = True,
                 feeds_bn: bool = False, groups: int = 1):
        super().__init__()
        self.stride = stride
        self.padding = padding
        self.input_grad = input_grad
        self.groups = groups
        # when the conv output goes straight into a training BatchNorm2d,
        # the conv epilogue emits the BN sum/sumsq partials for free
        self.feeds_bn = feeds_bn
        # set by a model (or said per call, forward's ``sole_reader``) when
        # a BatchNorm output reaches this conv directly and nobody else reads
        # that tensor or its gradient: a split-K dgrad then leaves its
        # combine to that BatchNorm's backward (_GradLink)
        self.dgrad_to_bn = False
        self._wt_view: tp.Optional[torch.Tensor] = None
        k = kernel_size
        self.depthwise = groups != 1 and groups == in_channels == out_channels
        # the plans are dims-only and ignore the image size: probe 8x8
        probe = ops.ConvDims(1, 8, 8, in_channels, out_channels, k, k,
                             (8 + 2 * padding - k) // stride + 1
                             if stride > 0 else 0,
                             (8 + 2 * padding - k) // stride + 1
                             if stride > 0 else 0, stride, padding)
        # the cheap part of the rule first: most convs never ask the plan
        self.patch = groups == 1 and k == stride and padding == 0 \
            and in_channels <= 4 and ops.patchconv_supported(probe)
        self.pointwise = groups == 1 and not self.patch and k == stride \
            and k in (1, 2) and padding == 0 \
            and (in_channels % 64 != 0 or out_channels % 64 != 0) \
            and ops.pwconv_supported(probe)
        if groups != 1:
            if self.depthwise:
                if not ops.dwconv_supported(probe):
                    raise ValueError(
                        f"{ops.DWCONV_RULE}; got in={in_channels} "
                        f"out={out_channels} kernel={k} stride={stride} "
                        f"padding={padding} groups={groups}")
            elif groups < 1 or in_channels % groups \
                    or not ops.gconv_supported(probe, groups):
                raise ValueError(
                    f"{ops.GCONV_RULE}; got in={in_channels} "
                    f"out={out_channels} kernel={k} stride={stride} "
                    f"padding={padding} groups={groups}")
        self.weight = nn.Parameter(
            torch.empty(out_channels, k, k, in_channels // groups))
        fan_out = out_channels * k * k
        nn.init.normal_(self.weight, std=math.sqrt(2.0 / fan_out))

    def forward(self, x: torch.Tensor,
                sole_reader: tp.Optional[bool] = None) -> torch.Tensor:
        """``sole_reader`` overrides ``dgrad_to_bn`` for this call."""
        if self.depthwise:
            return _DepthwiseConvFn.apply(x, self.weight, self.stride,
                                          self.padding,
                                          self.input_grad and x.requires_grad)
        if self.groups != 1:
            return _GroupedConvFn.apply(x, self.weight, self.stride,
                                        self.padding, self.groups,
                                        self.input_grad and x.requires_grad)
        if self.patch:
            return _PatchConvFn.apply(x, self.weight, self.stride,
                                      self.input_grad and x.requires_grad)
        if self.pointwise:
            return _PointwiseConvFn.apply(x, self.weight, self.stride,
                                          self.input_grad and x.requires_grad)
        input_grad = self.input_grad and x.requires_grad
        link = None
        if sole_reader is None:
            sole_reader = self.dgrad_to_bn
        if sole_reader and _FUSE_GRAD_SOURCES and input_grad \
                and torch.is_grad_enabled():
            link = getattr(x, "_grad_link", None)
            if link is not None and link.claimed:
                link = None     # one deferred dgrad per BatchNorm
            elif link is not None:
                link.claimed = True
        return _ConvFn.apply(x, self.weight, self.stride, self.padding,
                             input_grad, self._wt_view,
                             self.feeds_bn and self.training, link)


class WtCache:
    """One arena + ONE batched kernel refreshing every conv's RSCK weight
    copy per step (replaces a transpose launch per conv per backward).

    Requires the flat optimizer's bf16 mirror (``bf16_mirror=True``): the
    kernel reads each weight's mirror view straight out of the flat buffer.
    Call :meth:`refresh` once per step before backward — NativeResNet does it
    at the top of ``forward``.
    """

    def __init__(self, model: nn.Module):
        convs = [m for m in model.modules()
                 if isinstance(m, Conv2d) and m.input_grad
                 and m.groups == 1   # grouped convs build their own operand
                 and not m.pointwise  # reads the KRSC weight as it is
                 and m.weight.shape[-1] % 64 == 0]
        metas, total = [], 0
        mirrors = [getattr(c.weight, "_bf16_mirror", None) for c in convs]
        if not convs or any(m is None for m in mirrors):
            self.meta = None
            return
        base = mirrors[0]
        for c, mir in zip(convs, mirrors):
            assert mir.untyped_storage().data_ptr() == \
                base.untyped_storage().data_ptr(), \
                "all conv weights must share one flat bf16 mirror"
            src_off = (mir.data_ptr() - base.data_ptr()) // 2
            assert src_off >= 0
            K, R, S, C = c.weight.shape
            metas.append((src_off, total, K, R * S * C))
            total += K * R * S * C
        dev = convs[0].weight.device
        self.src = mirrors[0]
        self.arena = torch.empty(total, dtype=torch.bfloat16, device=dev)
        self.meta = torch.tensor([list(m) for m in metas],
                                 dtype=torch.int32, device=dev).flatten()
        self.max_elems = max(m[2] * m[3] for m in metas)
        self.n = len(convs)
        for c, m in zip(convs, metas):
            K, R, S, C = c.weight.shape
            c._wt_view = self.arena[m[1]:m[1] + K * R * S * C].view(R, S, C, K)

    @property
    def active(self) -> bool:
        return self.meta is not None

    def refresh(self) -> None:
        if self.meta is not None:
            ops.weight_transpose_batched(self.src, self.arena, self.meta,
                                         self.n, self.max_elems)


class _BnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                res: tp.Optional[torch.Tensor], relu: bool, slope: float,
                module, split: bool = False):
        N, H, W, C = x.shape
        M = N * H * W
        y = torch.empty_like(x)
        # small-M layers: one kernel forward, one backward (the plan lives
        # in batchnorm.hip); eval mode always keeps the separate kernels
        fwd_form, bwd_form = ops.bn_small_plan(M, C) if module.training \
            else ("chain", "chain")
        if module.training:
            fused = getattr(x, "_bn_stats", None)
            if fused is not None:   # producing conv already emitted partials
                partials, msplit = fused
            else:
                msplit = ops.bn_msplit(M, C)
                partials = torch.empty(msplit * 2 * C, dtype=torch.float32,
                                       device=x.device)
                ops.bn_stats(x, partials, M, C, msplit)
            work = torch.empty(4 * C, dtype=torch.float32, device=x.device)
            if fwd_form == "small":
                ops.bn_fwd_small(partials, msplit, gamma, beta,
                                 module.running_mean, module.running_var, work,
                                 x, res, y, M, C, module.eps, module.momentum,
                                 True, relu, slope)
            else:
                ops.bn_finalize(partials, msplit, gamma, beta,
                                module.running_mean, module.running_var, work,
                                M, C, module.eps, module.momentum,
                                update_running=True)
        else:
            invstd = torch.rsqrt(module.running_var + module.eps)
            scale = gamma.detach() * invstd
            shift = beta.detach() - module.running_mean * scale
            work = torch.cat([module.running_mean, invstd, scale, shift])
        if fwd_form != "small":
            ops.bn_apply(x, res, y, work, M, C, relu, slope)
        ctx.save_for_backward(x, y, work)
        ctx.relu = relu
        ctx.slope = slope
        ctx.bwd_form = bwd_form   # "chain" in eval mode
        # with running statistics mean and invstd are constants of x
        ctx.frozen_stats = not module.training
        ctx.has_res = res is not None
        ctx.refs = (gamma, beta)
        # backward takes its gradients as they come: None where an output
        # went unused, never a zero-filled stand-in
        ctx.set_materialize_grads(False)
        ctx.split = split
        ctx.link = None
        if _FUSE_GRAD_SOURCES:
            ctx.link = y._grad_link = _GradLink(
                None if bwd_form == "chain" else _SMALL_FORM_WS_ROWS)
        if not split:
            return y
        # the same storage on a second autograd edge: two readers of this
        # activation (a conv and a shortcut) each return their gradient to
        # an edge of their own, and backward forms the sum where it reads it
        y2 = y.detach()
        if ctx.link is not None:
            y2._grad_link = ctx.link
        return y, y2

    @staticmethod
    def backward(ctx, *grads: tp.Optional[torch.Tensor]):
        x, y, work = ctx.saved_tensors
        gamma, beta = ctx.refs
        N, H, W, C = x.shape
        M = N * H * W
        # dy = A [+ B]: A is a bf16 gradient or the fp32 slices a split-K
        # dgrad left un-combined (zn > 0), B the second edge's gradient
        taken = ctx.link.take(grads) if ctx.link is not None else None
        zn = 0
        if taken is not None:
            i, dy, zn = taken
            rest = [g for j, g in enumerate(grads) if j != i and g is not None]
        else:
            rest = [g for g in grads if g is not None]
            if not rest:
                return (None,) * 8
            dy = rest.pop(0).contiguous()
        dy_b = rest[0].contiguous() if rest else None
        # the sums are needed for dx, so the grads step always runs; frozen
        # gamma/beta just accumulate into a discarded temp instead of
        # param.grad (never pollute frozen params' grads).
        need_g, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dgamma, g_direct = _grad_target(gamma) if need_g \
            else (torch.empty_like(gamma), True)
        dbeta, b_direct = _grad_target(beta) if need_b \
            else (torch.empty_like(beta), True)
        dx = torch.empty_like(x)
        if ctx.bwd_form != "chain":
            # dz is the residual branch's gradient: written only if one reads it
            dz = torch.empty_like(x) if ctx.has_res else None
            ops.bn_bwd_small(dy, y, x, work, dz, dgamma, dbeta, dx, M, C,
                             ctx.relu, ctx.slope, write_dz=ctx.has_res,
                             form=ctx.bwd_form, dy_b=dy_b, zn=zn)
        else:
            msplit = ops.bn_msplit(M, C)
            partials = torch.empty(msplit * 2 * C, dtype=torch.float32,
                                   device=x.device)
            bsums = torch.empty(2 * C, dtype=torch.float32, device=x.device)
            dz = torch.empty_like(x)
            ops.bn_bwd_reduce(dy, y, x, work, dz, partials, M, C, msplit,
                              ctx.relu, ctx.slope, dy_b=dy_b, zn=zn)
            ops.bn_bwd_grads(partials, msplit, bsums, dgamma, dbeta, C)
            if ctx.frozen_stats:
                # eval mode: the batch terms of dx vanish, dx = scale * dz.
                # Zeroed sums make b0 = b1 = 0 in the apply kernel, which
                # leaves exactly that one fp32 product (dgamma/dbeta above
                # are the same in both modes).
                bsums.zero_()
            ops.bn_bwd_apply(dz, x, work, bsums, dx, M, C)
        return (dx,
                dgamma if need_g and not g_direct else None,
                dbeta if need_b and not b_direct else None,
                dz if ctx.has_res else None,
                None, None, None, None)


class _ConvTransposeFn(torch.autograd.Function):
    """Transposed conv via the equivalent regular conv C (weight [K=C_in]
    [R][S][C=C_out]):  fwd = C's dgrad,  dx = C's fwd,  dw = C's wgrad with
    the operand roles swapped (dL/dw = wgrad(x=dy, dout=x))."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, stride: int, pad: int,
                input_grad: bool):
        w16 = _weight_bf16(w)
        N, Hi, Wi, Cin = x.shape
        K, R, S, Cout = w16.shape
        assert K == Cin, (x.shape, w16.shape)
        Ho = (Hi - 1) * stride - 2 * pad + R
        Wo = (Wi - 1) * stride - 2 * pad + S
        # equivalent-conv dims: "input" = our OUTPUT, "output" = our input
        d = ops.ConvDims(N, Ho, Wo, Cout, Cin, R, S, Hi, Wi, stride, pad)
        y = x.new_empty((N, Ho, Wo, Cout))
        if Cout % 64 == 0:
            wt = w16.new_empty((R, S, Cout, Cin))
            ops.weight_transpose(w16, wt)
            ops.conv_dgrad(x, wt, y, d)
        else:  # RGB head: small-C direct kernel, KRSC weights as stored
            ops.conv_stem_dgrad(x, w16, y, d)
        ctx.save_for_backward(x, w16)
        ctx.dims = d
        ctx.input_grad = input_grad
        ctx.w_ref = w
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w16 = ctx.saved_tensors
        d: ops.ConvDims = ctx.dims
        dy = dy.contiguous()
        dw_buf = None
        direct = True
        if ctx.needs_input_grad[1]:  # skip wgrad entirely for frozen weights
            dw_buf, direct = _grad_target(ctx.w_ref)
            ops.conv_wgrad(dy, x, dw_buf, d)   # roles swapped vs regular conv
        dx = None
        if ctx.input_grad:
            dx = x.new_empty(x.shape)
            ops.conv_fwd(dy, w16, dx, d)
        return (dx, dw_buf if dw_buf is not None and not direct else None,
                None, None, None)


class ConvTranspose2d(nn.Module):
    """NHWC bf16 transposed conv.  Weight [C_in, R, S, C_out] fp32
    (= the equivalent regular conv's [K][R][S][C]).
    Trunk layers need C_in % 64 == 0 and C_out % 64 == 0; a small-C output
    head (e.g. RGB, C_out <= 8 with C_in == 64) uses the direct edge
    kernels."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int,
                 stride: int = 1, padding: int = 0, input_grad: bool = True,
                 feeds_bn: bool = False):
        super().__init__()
        self.stride = stride
        self.padding = padding
        self.input_grad = input_grad
        # when the conv output goes straight into a training BatchNorm2d,
        # the conv epilogue emits the BN sum/sumsq partials for free
        self.feeds_bn = feeds_bn
        k = kernel_size
        self.weight = nn.Parameter(
            torch.empty(in_channels, k, k, out_channels))
        fan_out = out_channels * k * k
        nn.init.normal_(self.weight, std=math.sqrt(2.0 / fan_out))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _ConvTransposeFn.apply(x, self.weight, self.stride,
                                      self.padding,
                                      self.input_grad and x.requires_grad)


# Above this many FLOPs per product the fc goes to rocBLAS (the guide's
# rule for PLAIN library GEMMs — no fusion opportunity here); below it the
# one-kernel-per-product native path wins on launch overhead.  The ResNet-50
# head (64x2048 -> 1000, 262 MFLOP) sits far above; the example MLPs far
# below.  Measured: the naive fc kernels cost 435 us/step on the R50 head
# vs ~15 us through rocBLAS (profiles/r02h).
_LINEAR_GEMM_CUTOFF = int(os.environ.get("FLASHY_LINEAR_CUTOFF", 1 << 23))


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor,
                b: tp.Optional[torch.Tensor]):
        B, I = x.shape
        O = w.shape[0]
        big = 2 * B * I * O >= _LINEAR_GEMM_CUTOFF and x.dtype == torch.float32
        if big:
            x = x.contiguous()
            y = torch.addmm(b, x, w.t()) if b is not None else x.mm(w.t())
        else:
            y = x.new_empty((B, O))
            ops.linear_fwd(x.contiguous(), w, b, y)
        ctx.save_for_backward(x)
        ctx.refs = (w, b)
        ctx.big = big
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        (x,) = ctx.saved_tensors
        w, b = ctx.refs
        dy = dy.contiguous()
        dw = db = None
        need_w = ctx.needs_input_grad[1]
        need_b = b is not None and ctx.needs_input_grad[2]
        if ctx.big:
            if need_w:
                dw, w_direct = _grad_target(w)
                dw.addmm_(dy.t(), x)  # += dy^T @ x (rocBLAS, fp32)
                dw = None if w_direct else dw
            if need_b:
                db, b_direct = _grad_target(b)
                db.add_(dy.sum(0))
                db = None if b_direct else db
        elif need_w or need_b:
            # one kernel produces both; frozen side goes to a discarded temp
            dw, w_direct = _grad_target(w) if need_w \
                else (torch.empty_like(w), True)
            db, b_direct = (_grad_target(b) if need_b else (None, True))
            ops.linear_dw(x, dy, dw, db)
            dw = dw if need_w and not w_direct else None
            db = db if need_b and not b_direct else None
        dx = None
        if ctx.needs_input_grad[0]:
            if ctx.big:
                dx = dy.mm(w)
            else:
                dx = x.new_empty(x.shape)
                ops.linear_dx(dy, w, dx)
        return dx, dw, db


class Linear(nn.Module):
    """fp32 fully-connected layer.  Tiny (launch-bound) shapes run the
    native fc kernels, one kernel per product; large heads (e.g. ResNet-50's
    2048->1000) go through rocBLAS — a plain dense GEMM with no fusion
    opportunity belongs on the library path (guide rule; 435 us -> ~15 us
    per step measured).  Weight [O, I], bias [O]; CPU falls back to
    torch.nn.functional.linear."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        bound = 1.0 / math.sqrt(in_features)
        nn.init.uniform_(self.weight, -bound, bound)
        self.bias: tp.Optional[nn.Parameter] = None
        if bias:
            self.bias = nn.Parameter(torch.empty(out_features))
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.device.type != "cuda":
            return torch.nn.functional.linear(x, self.weight, self.bias)
        return _LinearFn.apply(x, self.weight, self.bias)


class _PoolLinearFn(torch.autograd.Function):
    """Global average pool + small fc as ONE forward kernel and two
    deterministic backward kernels (csrc/head.hip).  x: NHWC bf16 trunk
    output, w [O, C] / b [O] fp32; returns fp32 logits [N, O]."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor,
                b: tp.Optional[torch.Tensor]):
        x = x.contiguous()
        N, H, W, C = x.shape
        pooled = torch.empty((N, C), dtype=torch.float32, device=x.device)
        y = torch.empty((N, w.shape[0]), dtype=torch.float32, device=x.device)
        ops.pool_linear_fwd(x, w, b, pooled, y)
        ctx.save_for_backward(pooled)
        ctx.refs = (w, b)
        ctx.x_shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        (pooled,) = ctx.saved_tensors
        w, b = ctx.refs
        dy = dy.contiguous()
        dw = db = None
        need_w = ctx.needs_input_grad[1]
        need_b = b is not None and ctx.needs_input_grad[2]
        if need_w or need_b:
            # one kernel produces both; a frozen side is simply not written
            dw, w_direct = _grad_target(w) if need_w else (None, True)
            db, b_direct = _grad_target(b) if need_b else (None, True)
            ops.head_dw(pooled, dy, dw, db)
            dw = None if w_direct else dw
            db = None if b_direct else db
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(ctx.x_shape, dtype=torch.bfloat16,
                             device=dy.device)
            ops.head_dx(dy, w, dx)
        return dx, dw, db


class _PoolFn(torch.autograd.Function):
    """Global average pool, NHWC bf16 -> fp32 [N, C] (the pooling half of
    the fused head, in front of a large rocBLAS fc)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor):
        x = x.contiguous()
        N, H, W, C = x.shape
        pooled = torch.empty((N, C), dtype=torch.float32, device=x.device)
        ops.pool_linear_fwd(x, None, None, pooled, None)
        ctx.x_shape = x.shape
        return pooled

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        dx = torch.empty(ctx.x_shape, dtype=torch.bfloat16, device=g.device)
        ops.head_dx(g.contiguous(), None, dx)
        return dx


def pool_linear(x: torch.Tensor, weight: torch.Tensor,
                bias: tp.Optional[torch.Tensor]) -> torch.Tensor:
    """Classifier head ``linear(mean_hw(x))`` on an NHWC trunk output
    ``[N, H, W, C]``; fp32 logits ``[N, O]``.  Heads below the rocBLAS
    cutoff of :class:`Linear` run the fused pool+fc kernels; larger ones
    the native pool kernels followed by the rocBLAS fc.  CPU falls back to
    torch."""
    if x.device.type != "cuda":
        return torch.nn.functional.linear(x.float().mean(dim=(1, 2)),
                                          weight, bias)
    N, C = x.shape[0], x.shape[3]
    if 2 * N * C * weight.shape[0] < _LINEAR_GEMM_CUTOFF:
        return _PoolLinearFn.apply(x, weight, bias)
    return _LinearFn.apply(_PoolFn.apply(x), weight, bias)


class PoolLinearHead(nn.Module):
    """Global average pool + :class:`Linear` over an NHWC bf16 input, run
    through :func:`pool_linear`.  Parameters live in ``fc`` so state-dict
    keys stay ``fc.weight`` / ``fc.bias``."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True):
        super().__init__()
        self.fc = Linear(in_features, out_features, bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return pool_linear(x, self.fc.weight, self.fc.bias)


class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, kernel: int, stride: int, pad: int):
        N, H, W, C = x.shape
        Ho = (H + 2 * pad - kernel) // stride + 1
        Wo = (W + 2 * pad - kernel) // stride + 1
        d = ops.ConvDims(N, H, W, C, C, kernel, kernel, Ho, Wo, stride, pad)
        y = x.new_empty((N, Ho, Wo, C))
        argmax = torch.empty(N * Ho * Wo * C, dtype=torch.uint8, device=x.device)
        ops.maxpool_fwd(x, y, argmax, d)
        ctx.save_for_backward(argmax)
        ctx.dims = d
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        (argmax,) = ctx.saved_tensors
        d: ops.ConvDims = ctx.dims
        dx = dy.new_empty((d.N, d.H, d.W, d.C))
        ops.maxpool_bwd(dy.contiguous(), argmax, dx, d)
        return dx, None, None, None


class MaxPool2d(nn.Module):
    """NHWC bf16 max pool with deterministic gather-based backward."""

    def __init__(self, kernel_size: int, stride: int, padding: int = 0):
        super().__init__()
        self.kernel_size = kernel_size
        self.stride = stride
        self.padding = padding

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _MaxPoolFn.apply(x, self.kernel_size, self.stride, self.padding)


class BatchNorm2d(nn.Module):
    """NHWC training BatchNorm with optional fused residual-add + ReLU.

    Training mode and every backward need ``num_features % 64 == 0`` (the
    reduction kernels walk 64-channel groups; other widths raise
    ``ValueError``); the eval-mode forward needs ``% 8``.  In eval mode the
    running statistics are constants, so the input gradient is ``scale * dz``.
    """

    def __init__(self, num_features: int, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def forward(self, x: torch.Tensor,
                res: tp.Optional[torch.Tensor] = None,
                relu: bool = False, slope: float = 0.0, split: bool = False
                ) -> tp.Union[torch.Tensor, tp.Tuple[torch.Tensor, torch.Tensor]]:
        """``relu=True, slope=s`` applies LeakyReLU(s) (s=0: plain ReLU).

        ``split=True`` returns the output twice, ``(y, y2)``: one value, one
        storage, two autograd edges.  A model that reads the output in two
        places (a conv and a shortcut) gives each reader its own copy; the
        two gradients then reach backward un-summed and the backward kernel
        adds them as it reads them, instead of autograd launching an add.
        The result is bitwise that of the summed gradient.  Treat the pair
        as read-only."""
        if not split:
            return _BnFn.apply(x, self.weight, self.bias, res, relu, slope,
                               self)
        if not (_FUSE_GRAD_SOURCES and torch.is_grad_enabled()):
            y = _BnFn.apply(x, self.weight, self.bias, res, relu, slope, self)
            return y, y
        return _BnFn.apply(x, self.weight, self.bias, res, relu, slope, self,
                           True)


def _param_grads(ctx, params: tp.Sequence[tp.Optional[torch.Tensor]],
                 first: int):
    """(kernel targets, autograd returns) for the fp32 parameters at inputs
    ``first``, ...: a frozen or absent one gets no target and no gradient, a
    live one accumulates straight into ``p.grad`` where that exists."""
    targets, returns = [], []
    for i, p in enumerate(params):
        if p is None or not ctx.needs_input_grad[first + i]:
            targets.append(None)
            returns.append(None)
            continue
        buf, direct = _grad_target(p)
        targets.append(buf)
        returns.append(None if direct else buf)
    return targets, returns


class _LayerNormFn(torch.autograd.Function):
    """LayerNorm over the channels of an NHWC tensor (csrc/layernorm.hip);
    saves the input and each row's (mean, rstd), not the output."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                in_bias: tp.Optional[torch.Tensor], eps: float):
        x = x.contiguous()
        y = torch.empty_like(x)
        stats = torch.empty(x.numel() // x.shape[-1], 2, dtype=torch.float32,
                            device=x.device)
        ops.ln_fwd(x, gamma, beta, y, stats, eps, in_bias)
        ctx.save_for_backward(x, stats)
        ctx.refs = (gamma, beta, in_bias)
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, stats = ctx.saved_tensors
        gamma, beta, in_bias = ctx.refs
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        (dgamma, dbeta, db_in), grads = _param_grads(
            ctx, (gamma, beta, in_bias), 1)
        ops.ln_bwd(dy.contiguous(), x, stats, gamma, dx, dgamma, dbeta,
                   in_bias, db_in)
        return (dx, *grads, None)


class LayerNorm2d(nn.Module):
    """LayerNorm over the channels of an NHWC bf16 tensor, NHWC out, fp32
    ``weight`` / ``bias``; ``num_channels % 8 == 0``, at most 1024
    (:data:`flashy_amd.ops.LN_RULE`).  ``forward(x, in_bias)`` normalizes
    ``x + in_bias``: the bias of the conv that produced ``x`` folded in, so
    it costs no pass of its own."""

    def __init__(self, num_channels: int, eps: float = 1e-6):
        super().__init__()
        if num_channels < 8 or num_channels % 8 or num_channels > 1024:
            raise ValueError(f"{ops.LN_RULE}; got {num_channels} channels")
        self.num_channels = num_channels
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))

    def forward(self, x: torch.Tensor,
                in_bias: tp.Optional[torch.Tensor] = None) -> torch.Tensor:
        return _LayerNormFn.apply(x, self.weight, self.bias, in_bias, self.eps)


class _BiasGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h: torch.Tensor, bias: torch.Tensor):
        h = h.contiguous()
        g = torch.empty_like(h)
        ops.bias_gelu_fwd(h, bias, g)
        ctx.save_for_backward(h)
        ctx.refs = (bias,)
        return g

    @staticmethod
    def backward(ctx, dg: torch.Tensor):
        (h,) = ctx.saved_tensors
        (bias,) = ctx.refs
        dh = torch.empty_like(h)
        (db,), grads = _param_grads(ctx, (bias,), 1)
        ops.bias_gelu_bwd(dg.contiguous(), h, bias, dh, db)
        return (dh, *grads)


def bias_gelu(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``gelu(x + bias)`` (erf form) over NHWC bf16 ``x`` with an fp32
    per-channel ``bias``, one launch; backward recomputes from ``x``."""
    return _BiasGeluFn.apply(x, bias)


class _BiasAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z: torch.Tensor, bias: torch.Tensor):
        ops.bias_add(z, bias)
        ctx.mark_dirty(z)
        ctx.refs = (bias,)
        return z

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        (bias,) = ctx.refs
        (db,), grads = _param_grads(ctx, (bias,), 1)
        if db is not None:
            ops.bias_add_bwd(dout.contiguous(), db)
        return (dout, *grads)


def bias_add(z: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``z + bias`` over contiguous NHWC bf16 ``z`` with an fp32 per-channel
    ``bias``, one launch, IN PLACE on ``z`` (the conv that produced it does
    not save its output); the input gradient is the output's, unchanged."""
    return _BiasAddFn.apply(z, bias)


def global_avg_pool(x: torch.Tensor) -> torch.Tensor:
    """Mean over H and W of an NHWC bf16 tensor: fp32 ``[N, C]`` (the
    pooling kernels of the classifier head, csrc/head.hip)."""
    return _PoolFn.apply(x)


class _ScaleResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z: torch.Tensor, bias: torch.Tensor, scale: torch.Tensor,
                res: torch.Tensor):
        z = z.contiguous()
        out = torch.empty_like(z)
        ops.scale_residual_fwd(z, bias, scale, res.contiguous(), out)
        ctx.save_for_backward(z)
        ctx.refs = (bias, scale)
        return out

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        (z,) = ctx.saved_tensors
        bias, scale = ctx.refs
        dout = dout.contiguous()
        dz = torch.empty_like(z)
        (db, ds), grads = _param_grads(ctx, (bias, scale), 1)
        ops.scale_residual_bwd(dout, z, bias, scale, dz, ds, db)
        # the residual branch's gradient is dout itself, not a copy
        return (dz, *grads, dout if ctx.needs_input_grad[3] else None)


def scale_residual(z: torch.Tensor, bias: torch.Tensor, scale: torch.Tensor,
                   res: torch.Tensor) -> torch.Tensor:
    """``res + scale * (z + bias)`` over NHWC bf16 ``z`` / ``res`` with fp32
    per-channel ``bias`` and layer ``scale``, one launch."""
    return _ScaleResidualFn.apply(z, bias, scale, res)


def _grn_coefs(x: torch.Tensor):
    n, c = x.shape[0], x.shape[-1]
    return (torch.empty(n, c, dtype=torch.float32, device=x.device),
            torch.empty(n, c, dtype=torch.float32, device=x.device),
            torch.empty(n, dtype=torch.float32, device=x.device))


class _GrnFn(torch.autograd.Function):
    """Global response normalization of an NHWC tensor (csrc/grn.hip); saves
    the input, Nx, a = 1 + gamma * Nx and each image's 1 / (mu + eps), not
    the output."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                eps: float):
        x = x.contiguous()
        out = torch.empty_like(x)
        nx, a, rden = _grn_coefs(x)
        ops.grn_fwd(x, gamma, beta, out, nx, a, rden, eps)
        ctx.save_for_backward(x, nx, a, rden)
        ctx.refs = (gamma, beta)
        return out

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        x, nx, a, rden = ctx.saved_tensors
        gamma, beta = ctx.refs
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        (dgamma, dbeta), grads = _param_grads(ctx, (gamma, beta), 1)
        ops.grn_bwd(dout.contiguous(), x, nx, a, rden, gamma, dx, dgamma,
                    dbeta)
        return (dx, *grads, None)


class GRN(nn.Module):
    """Global response normalization (ConvNeXt V2) of an NHWC bf16 tensor,
    NHWC out: ``weight * (x * Nx) + bias + x`` with ``Nx`` each (image,
    channel) plane's L2 norm over the mean of the image's norms plus ``eps``.
    fp32 ``weight`` / ``bias``, zero at the start as in the paper;
    ``num_channels % 8 == 0``, at most 4096 (:data:`flashy_amd.ops.GRN_RULE`).
    """

    def __init__(self, num_channels: int, eps: float = 1e-6):
        super().__init__()
        if num_channels < 8 or num_channels % 8 or num_channels > 4096:
            raise ValueError(f"{ops.GRN_RULE}; got {num_channels} channels")
        self.num_channels = num_channels
        self.eps = eps
        self.weight = nn.Parameter(torch.zeros(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _GrnFn.apply(x, self.weight, self.bias, self.eps)


class _BiasGeluGrnFn(torch.autograd.Function):
    """grn(gelu(h + bias)): the GELU walk gathers GRN's sums of squares, so
    ``g`` is not read again for them.  ``g`` is kept, not recomputed: GRN's
    backward reads it."""

    @staticmethod
    def forward(ctx, h: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor,
                beta: torch.Tensor, eps: float):
        h = h.contiguous()
        g, out = torch.empty_like(h), torch.empty_like(h)
        nx, a, rden = _grn_coefs(h)
        plan = ops.grn_plan(h.shape[0], h.numel() // (h.shape[0] * h.shape[-1]),
                            h.shape[-1])
        sq = torch.empty(h.shape[0], plan.slices, h.shape[-1],
                         dtype=torch.float32, device=h.device)
        ops.bias_gelu_sqsum(h, bias, g, sq)
        ops.grn_fwd(g, gamma, beta, out, nx, a, rden, eps, sq)
        ctx.save_for_backward(h, g, nx, a, rden)
        ctx.refs = (bias, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        h, g, nx, a, rden = ctx.saved_tensors
        bias, gamma, beta = ctx.refs
        (db, dgamma, dbeta), grads = _param_grads(ctx, (bias, gamma, beta), 1)
        dg, dh = torch.empty_like(g), torch.empty_like(h)
        ops.grn_bwd(dout.contiguous(), g, nx, a, rden, gamma, dg, dgamma,
                    dbeta)
        ops.bias_gelu_bwd(dg, h, bias, dh, db)
        return (dh, *grads, None)


def bias_gelu_grn(h: torch.Tensor, bias: torch.Tensor,
                  grn: GRN) -> torch.Tensor:
    """``grn(gelu(h + bias))`` over NHWC bf16 ``h`` with an fp32 per-channel
    ``bias``: the fused GELU + sum-of-squares forward, then GRN's coefficient
    and apply kernels.  Backward is GRN's followed by that of
    :func:`bias_gelu`."""
    return _BiasGeluGrnFn.apply(h, bias, grn.weight, grn.bias, grn.eps)
