# Copyright (c) Flashy-AMD authors.
"""Autograd-integrated functional ops backed by the gfx950 kernels.

Each loss computes its input gradient during the forward pass (training
always runs backward, so fusing saves a full re-read of the logits), wrapped
in ``torch.autograd.Function`` so ``loss.backward()`` works as usual.
On CPU they fall back to the torch implementations (tests/CI); on CUDA the
native extension is required.
"""
from __future__ import annotations

import typing as tp

import torch

from . import ops
from .data import MixedTarget


def _grad_buffer(x: torch.Tensor) -> torch.Tensor:
    """The kernels write the gradient row-major: a contiguous buffer, never
    ``empty_like``, which keeps the strides of a dense permuted input."""
    return torch.empty(x.shape, dtype=x.dtype, device=x.device)


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        B, C = logits.shape
        dlogits = _grad_buffer(logits)
        loss = torch.zeros((), dtype=torch.float32, device=logits.device)
        ops.cross_entropy_fwd_bwd(logits.contiguous(), target.contiguous(),
                                  dlogits, loss,
                                  loss_scale=1.0 / B, grad_scale=1.0 / B)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (dlogits,) = ctx.saved_tensors
        return dlogits * grad_out, None


class _CrossEntropyMix(torch.autograd.Function):
    """Mixed / smoothed target: ``target_b`` and ``lam`` may be None."""

    @staticmethod
    def forward(ctx, logits, target, target_b, lam, eps: float):
        B, C = logits.shape
        dlogits = _grad_buffer(logits)
        loss = torch.zeros((), dtype=torch.float32, device=logits.device)
        ops.cross_entropy_mix_fwd_bwd(
            logits.contiguous(), target.contiguous(),
            target_b.contiguous() if target_b is not None else None, lam,
            dlogits, loss, eps, loss_scale=1.0 / B, grad_scale=1.0 / B)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (dlogits,) = ctx.saved_tensors
        return dlogits * grad_out, None, None, None, None


def cross_entropy(logits: torch.Tensor,
                  target: tp.Union[torch.Tensor, MixedTarget],
                  label_smoothing: float = 0.0) -> torch.Tensor:
    """Mean cross-entropy over [B, C] logits (fp32 or bf16) and int64 targets.

    ``target`` may also be the :class:`flashy_amd.data.MixedTarget` of a
    :class:`flashy_amd.data.DeviceMix`; the loss is then ``lam * CE(logits,
    target_a) + (1 - lam) * CE(logits, target_b)``, with ``lam`` read on the
    device (so a captured loss follows each replay's draw) and no gradient
    into ``lam``.  ``label_smoothing`` is torch's: the target distribution
    becomes ``(1 - eps) * target + eps / C``.

    GPU: one fused kernel producing loss + dlogits (``k_cross_entropy`` for
    a plain target without smoothing, else ``k_cross_entropy_mix``).  CPU:
    torch fallback.
    """
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError(
            f"label_smoothing must lie in [0, 1], got {label_smoothing}")
    mixed = isinstance(target, MixedTarget)
    if logits.device.type != "cuda":
        ce = torch.nn.functional.cross_entropy
        if not mixed:
            return ce(logits, target, label_smoothing=label_smoothing)
        lam = target.lam.detach().reshape(())
        return (lam * ce(logits, target.target_a,
                         label_smoothing=label_smoothing)
                + (1 - lam) * ce(logits, target.target_b,
                                 label_smoothing=label_smoothing))
    if mixed:
        return _CrossEntropyMix.apply(logits, target.target_a,
                                      target.target_b, target.lam,
                                      float(label_smoothing))
    if label_smoothing == 0.0:
        return _CrossEntropy.apply(logits, target)
    return _CrossEntropyMix.apply(logits, target, None, None,
                                  float(label_smoothing))


class _BCEWithLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, target_value: float) -> torch.Tensor:
        n = x.numel()
        dx = _grad_buffer(x)
        loss = torch.zeros((), dtype=torch.float32, device=x.device)
        ops.bce_logits_fwd_bwd(x.contiguous(), dx, loss, target_value,
                               loss_scale=1.0 / n, grad_scale=1.0 / n)
        ctx.save_for_backward(dx)
        return loss

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (dx,) = ctx.saved_tensors
        return dx * grad_out, None


def bce_with_logits_const(x: torch.Tensor, target_value: float) -> torch.Tensor:
    """Mean BCE-with-logits against a constant target (GAN labels)."""
    if x.device.type != "cuda":
        target = torch.full_like(x, target_value)
        return torch.nn.functional.binary_cross_entropy_with_logits(x, target)
    return _BCEWithLogits.apply(x, target_value)


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        n = x.numel()
        dx = _grad_buffer(x)
        loss = torch.zeros((), dtype=torch.float32, device=x.device)
        ops.mse_fwd_bwd(x.contiguous(), t.contiguous(), dx, loss,
                        loss_scale=1.0 / n, grad_scale=1.0 / n)
        ctx.save_for_backward(dx)
        return loss

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (dx,) = ctx.saved_tensors
        return dx * grad_out, None


def mse_loss(x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Mean squared error (fused fwd+grad kernel on GPU; torch on CPU).

    Replaces F.mse_loss of the teacher-student workload
    (/root/reference/tests/dummy/train.py:93)."""
    if x.shape != target.shape:
        raise ValueError(f"mse_loss: target of shape {tuple(target.shape)} "
                         f"against input of shape {tuple(x.shape)} (no "
                         "broadcasting)")
    if x.device.type != "cuda":
        return torch.nn.functional.mse_loss(x, target)
    return _MSE.apply(x, target.detach())


def accuracy(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean(argmax(logits, 1) == target) as a device scalar — one kernel on
    GPU (vs the argmax+eq+mean 3-launch chain), torch ops on CPU."""
    if logits.device.type != "cuda":
        return (logits.argmax(1) == target).float().mean()
    B = logits.shape[0]
    out = torch.zeros((), dtype=torch.float32, device=logits.device)
    ops.accuracy_count(logits.detach().contiguous(), target.contiguous(),
                       out)
    return out / B
