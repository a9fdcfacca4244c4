# Copyright (c) Flashy-AMD authors.
"""CIFAR example entry point (parity: reference examples/cifar/train.py)."""
from __future__ import annotations

from pathlib import Path

import torch

import flashy_amd
from flashy_amd import distrib
from flashy_amd.models import native_resnet18, resnet18
from flashy_amd.optim import (LARS, FusedSGD, MultiStep, WarmupCosine,
                              WarmupLinear, no_decay_1d)
from flashy_amd import xp as fxp

from .solver import Solver, SyntheticCIFAR

main = fxp.entry_point("examples.cifar", Path(__file__).parent / "conf")


def get_schedule(cfg, steps_per_epoch: int):
    """The optional ``schedule:`` section -> an LRSchedule (None = off).
    All lengths are in optimizer steps; ``total_steps`` defaults to the
    whole run."""
    section = cfg.get("schedule") or {}
    kind = section.get("kind")
    if kind is None:
        return None
    warmup = dict(warmup_steps=section.get("warmup_steps", 0),
                  start_factor=section.get("start_factor", 0.0))
    if kind == "multistep":
        return MultiStep(section.get("milestones") or [],
                         gamma=section.get("gamma", 0.1), **warmup)
    klass = {"cosine": WarmupCosine, "linear": WarmupLinear}.get(kind)
    if klass is None:
        raise ValueError(f"schedule.kind must be cosine, linear or multistep, "
                         f"got {kind!r}")
    total = section.get("total_steps") or cfg.epochs * steps_per_epoch
    return klass(total_steps=total, min_ratio=section.get("min_ratio", 0.0),
                 **warmup)


def get_tensor_options(cfg):
    """``no_decay_1d`` and the ``lars:`` section -> the ``param_options`` /
    ``lars`` keywords of FusedSGD (both None = off)."""
    section = cfg.get("lars") or {}
    lars = None
    if section.get("enabled", False):
        lars = LARS(eta=section.get("eta", 1e-3), eps=section.get("eps", 1e-8))
    return dict(
        param_options=no_decay_1d if cfg.get("no_decay_1d", False) else None,
        lars=lars)


def get_solver(cfg):
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu") \
        if cfg.device == "auto" else torch.device(cfg.device)
    native = device.type == "cuda" and cfg.get("native", True)
    if native:  # the gfx950 NHWC kernel path + flat fused optimizer
        model = native_resnet18(cfg.num_classes).to(device)
        distrib.broadcast_model(model)
        loaders = _loaders(cfg)
        # schedule and clipping run on the device inside optim.step(), so
        # the captured step follows them under graph replay
        optim = FusedSGD(model.parameters(), lr=cfg.lr, momentum=cfg.momentum,
                         weight_decay=cfg.weight_decay, bf16_mirror=True,
                         schedule=get_schedule(cfg, len(loaders["train"])),
                         max_grad_norm=cfg.get("max_grad_norm"),
                         **get_tensor_options(cfg))
        model.enable_wt_cache()
        return Solver(cfg, model, loaders, optim)
    if (cfg.get("schedule") or {}).get("kind") or cfg.get("max_grad_norm"):
        raise ValueError("schedule / max_grad_norm need the native path "
                         "(FusedSGD); this run uses torch.optim.SGD")
    if any(v is not None for v in get_tensor_options(cfg).values()):
        raise ValueError("no_decay_1d / lars need the native path (FusedSGD); "
                         "this run uses torch.optim.SGD")
    model = resnet18(num_classes=cfg.num_classes, small_input=True).to(device)
    distrib.broadcast_model(model)
    optim = torch.optim.SGD(model.parameters(), lr=cfg.lr,
                            momentum=cfg.momentum, weight_decay=cfg.weight_decay)
    return Solver(cfg, model, _loaders(cfg), optim)


def _loaders(cfg):
    # augment.enabled: samples travel as uint8 HWC and the solver's
    # DeviceAugment turns them into the model's input on the device
    uint8 = bool((cfg.get("augment") or {}).get("enabled", False))
    return {
        "train": distrib.loader(SyntheticCIFAR(cfg.dataset_size, cfg.num_classes,
                                               uint8=uint8),
                                batch_size=cfg.batch_size, shuffle=True),
        "valid": distrib.loader(SyntheticCIFAR(cfg.valid_size, cfg.num_classes,
                                               train=False, uint8=uint8),
                                batch_size=cfg.batch_size, shuffle=False),
    }


def get_solver_from_sig(sig: str):
    """Notebook workflow: rebuild + restore the solver of an existing run."""
    xp = main.get_xp_from_sig(sig)
    xp.enter()
    solver = get_solver(xp.cfg)
    solver.restore()
    return solver


@main.bind
def run(cfg):
    flashy_amd.setup_logging()
    distrib.init()
    torch.manual_seed(cfg.seed)
    get_solver(cfg).run()


if __name__ == "__main__":
    main()
