# Copyright (c) Flashy-AMD authors.
"""CIFAR-10-shaped ResNet-18 solver: train/valid stages, DP via the bucketed
``sync_model`` path, accuracy formatting, image logging.

Parity: reference examples/cifar/solver.py + train.py (torchvision download
replaced by a deterministic synthetic dataset — this environment has no
network; shapes and the training loop structure are the same).
"""
from __future__ import annotations

import math

import torch
from torch.nn import functional as F

from flashy_amd import BaseSolver, Formatter, distrib
from flashy_amd.data import DeviceAugment, DeviceMix, DeviceResizedCrop
from flashy_amd.functional import accuracy, cross_entropy
from flashy_amd.graph import CapturedStep
from flashy_amd.models.resnet_native import NativeResNet
from flashy_amd.utils import averager


class SyntheticCIFAR:
    """Deterministic CIFAR-10-shaped dataset: sample i is seeded noise with a
    class-dependent mean, so accuracy is learnable above chance.

    ``uint8=True`` yields the same seeded image as a decoder would hand it
    over: uint8 HWC ``[32, 32, 3]``, quantized as ``round(img * 64 + 128)``
    clamped to 0..255 (the input of :class:`flashy_amd.data.DeviceAugment`)."""

    def __init__(self, size: int, num_classes: int = 10, train: bool = True,
                 uint8: bool = False):
        self.size = size
        self.num_classes = num_classes
        self.offset = 0 if train else 1 << 24
        self.uint8 = uint8

    def __len__(self):
        return self.size

    def __getitem__(self, index: int):
        g = torch.Generator().manual_seed(index + self.offset)
        label = int(torch.randint(self.num_classes, (1,), generator=g))
        img = torch.randn(3, 32, 32, generator=g) * 0.5 + label * 0.1
        if self.uint8:
            img = (img * 64 + 128).round().clamp(0, 255).to(torch.uint8)
            img = img.permute(1, 2, 0).contiguous()
        return img, label


def make_augment(section, seed: int, device):
    """The on-device ingest the ``augment`` config section asks for, or
    None when it is off: :class:`DeviceAugment` (crop with padding), or
    :class:`DeviceResizedCrop` when ``augment.resized_crop`` is set — to
    ``true`` for the defaults, or to a section with ``scale`` / ``ratio``."""
    if not section.get("enabled", False):
        return None
    common = dict(flip=section.get("flip", 0.5),
                  mean=tuple(section.get("mean", (0., 0., 0.))),
                  std=tuple(section.get("std", (1., 1., 1.))),
                  seed=seed, device=device)
    resized = section.get("resized_crop", False)
    if not resized:
        return DeviceAugment(32, pad=section.get("pad", 4), **common)
    opts = resized if isinstance(resized, dict) else {}
    return DeviceResizedCrop(32, scale=tuple(opts.get("scale", (0.08, 1.0))),
                             ratio=tuple(opts.get("ratio", (3 / 4, 4 / 3))),
                             **common)


def make_mix(section, seed: int, device):
    """The :class:`DeviceMix` the ``mix`` config section asks for, or None
    when both alphas are 0 (the default)."""
    mixup = float(section.get("mixup_alpha", 0.0))
    cutmix = float(section.get("cutmix_alpha", 0.0))
    if mixup == 0.0 and cutmix == 0.0:
        return None
    return DeviceMix(mixup_alpha=mixup, cutmix_alpha=cutmix,
                     prob=section.get("prob", 1.0),
                     switch_prob=section.get("switch_prob", 0.5),
                     seed=seed, device=device)


class Solver(BaseSolver):
    def __init__(self, cfg, model, loaders, optim):
        super().__init__()
        self.cfg = cfg
        self.async_checkpoint = bool(cfg.get('async_checkpoint', False))
        self.model = model
        self.loaders = loaders
        self.optim = optim
        self.device = next(model.parameters()).device
        self.native = isinstance(model, NativeResNet)
        self.autocast = (self.device.type == "cuda" and cfg.dtype == "bf16"
                         and not self.native)
        # HIP-graph whole-step capture: native path, single process only
        self.use_graph = (cfg.get("use_graph", True) and self.native
                          and not distrib.is_distributed())
        self._graph = None
        self.register_stateful("model", "optim")
        # optional on-device ingest: uint8 NHWC batches -> crop / flip /
        # normalize -> bf16 NHWC.  Its step counter lives on the device and
        # is checkpointed, so a resumed run continues the augmentation stream.
        self.augment = make_augment(cfg.get("augment") or {}, cfg.seed,
                                    self.device)
        if self.augment is not None:
            self.register_stateful("augment")
            if isinstance(self.augment, DeviceResizedCrop):
                # the run's log names the recipe that was actually selected
                self.logger.info("on-device ingest: %r", self.augment)
        # optional label smoothing and Mixup / CutMix of the ingested batch
        # (train only); the mixer's counter is checkpointed like the augment's
        self.label_smoothing = float(cfg.get("label_smoothing", 0.0))
        self.mix = make_mix(cfg.get("mix") or {}, cfg.seed, self.device)
        if self.mix is not None:
            if self.augment is None or (self.device.type == "cuda"
                                        and not self.native):
                raise ValueError(
                    "mix.mixup_alpha / mix.cutmix_alpha need "
                    "augment.enabled=true and, on a GPU, native=true: the "
                    "mixer works on the bf16 NHWC batch the on-device ingest "
                    "produces")
            self.register_stateful("mix")
            self.logger.info("batch mixing: %r", self.mix)

    def get_formatter(self, stage_name):
        return Formatter({"acc": ".1%", "loss": ".5f", "lr": ".2e",
                          "grad_norm": ".3f"})

    def _ingest(self, img, train: bool):
        """uint8 NHWC device batch -> model input.  The native model takes
        the bf16 NHWC output as is; the torch model (CPU runs, native=false)
        gets it as fp32 NCHW."""
        x = self.augment(img, train=train)
        if not self.native:
            x = x.permute(0, 3, 1, 2).float()
        return x

    def _mix(self, x, label):
        """Mix the ingested batch in place (train only); returns what the
        loss takes as target.  The torch model's fp32 NCHW input is mixed
        through its NHWC view."""
        if self.mix is None:
            return label
        return self.mix(x if self.native else x.permute(0, 2, 3, 1), label)

    def _capture(self, shape):
        self._static_img = torch.zeros(
            shape, device=self.device,
            dtype=torch.uint8 if self.augment is not None else None)
        self._static_label = torch.zeros(shape[0], dtype=torch.long,
                                         device=self.device)

        def step():
            self.optim.zero_grad(set_to_none=False)
            x = self._static_img
            if self.augment is not None:
                # ingest + counter bump are part of the graph: every replay
                # reads the advanced counter and crops differently
                x = self._ingest(x, True)
            # the mixer draws on the device too; lam reaches the loss
            # through device memory, so every replay mixes differently
            target = self._mix(x, self._static_label)
            est = self.model(x)
            loss = cross_entropy(est, target,
                                 label_smoothing=self.label_smoothing)
            loss.backward()
            self.optim.step()
            return loss, est

        drawers = [d for d in (self.augment, self.mix) if d is not None]
        drawn = [d.state_dict() for d in drawers]
        self._graph = CapturedStep(step, warmup=3).capture()
        for drawer, state in zip(drawers, drawn):
            # the warmup steps ran on the zero buffer: give their draws back
            drawer.load_state_dict(state)

    def _graphed_step(self, img, label):
        """One training step as a single hipGraph replay (static buffers)."""
        if self._graph is None:
            self._capture(img.shape)
        self._static_img.copy_(img, non_blocking=True)
        self._static_label.copy_(label, non_blocking=True)
        loss, est = self._graph()
        acc = accuracy(est, self._static_label)
        return loss, acc

    def _step(self, img, label, train: bool):
        if (train and self.use_graph and self.device.type == "cuda"
                and img.shape[0] == self.cfg.batch_size):
            return self._graphed_step(img, label)
        img = img.to(self.device, non_blocking=True)
        label = label.to(self.device, non_blocking=True)
        if self.augment is not None:
            img = self._ingest(img, train)
        target = self._mix(img, label) if train else label
        with torch.autocast("cuda", torch.bfloat16, enabled=self.autocast):
            est = self.model(img)
        if self.native and train:
            # fused fwd+grad kernel
            loss = cross_entropy(est, target,
                                 label_smoothing=self.label_smoothing)
        elif train and self.mix is not None:
            loss = cross_entropy(est, target,        # CPU: the torch formula
                                 label_smoothing=self.label_smoothing)
        elif train:
            loss = F.cross_entropy(est, label,
                                   label_smoothing=self.label_smoothing)
        else:
            loss = F.cross_entropy(est, label)       # valid: plain CE
        acc = accuracy(est, label)
        if train:
            self.optim.zero_grad()
            loss.backward()
            if hasattr(self.optim, "grad_buffers"):
                distrib.sync_flat_gradients(self.optim)
            else:
                distrib.sync_model(self.model)
            self.optim.step()
        return loss, acc

    def _optim_metrics(self):
        """End-of-stage read-outs of the on-device schedule / clipping (one
        host read each, here only): the lr the next step will use and the
        last step's pre-clip gradient norm."""
        out = {}
        if getattr(self.optim, "schedule", None) is not None:
            out["lr"] = self.optim.current_lr()
        norm = getattr(self.optim, "last_grad_norm", None)
        if norm is not None:
            out["grad_norm"] = norm.item()
        return out

    def do_train_valid(self, train: bool):
        stage = "train" if train else "valid"
        loader = self.loaders[stage]
        self.model.train(train)
        avg = averager()
        lp = self.log_progress(stage, loader, updates=5)
        with torch.set_grad_enabled(train):
            for img, label in lp:
                loss, acc = self._step(img, label, train)
                metrics = avg({"loss": loss.item(), "acc": acc.item()})
                lp.update(**metrics)
        if train:
            metrics.update(self._optim_metrics())
        if not math.isfinite(metrics["loss"]):
            # a NaN must halt the run loudly, not be silently averaged —
            # especially with graph capture in the loop
            raise RuntimeError(
                f"non-finite {stage} loss at epoch {self.epoch}: {metrics}")
        return distrib.average_metrics(metrics, len(loader))

    def run(self):
        if self.restore() and hasattr(self.optim, "refresh_bf16"):
            # restored fp32 params -> re-sync the bf16 weight mirrors
            self.optim.refresh_bf16()
        self.log_hyperparams(self.cfg)
        for epoch in range(self.epoch, self.cfg.epochs + 1):
            self.run_stage("train", self.do_train_valid, True)
            self.run_stage("valid", self.do_train_valid, False)
            self.commit()
        self.finalize_checkpoint()   # join an in-flight async write, if any
