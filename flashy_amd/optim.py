# Copyright (c) Flashy-AMD authors.
"""Flat-buffer fused optimizers for MI355X.

Design: at construction ALL trainable parameters of one (device, dtype)
group are packed into a single contiguous fp32 buffer; each ``param.data``
is re-pointed to a view of that buffer, and ``param.grad`` to a view of a
matching flat gradient buffer.  Consequences:

* ``step()`` is ONE HIP kernel over the flat buffers (float4-vectorized,
  grid-strided — flashy_amd/ops/csrc/fused_optim.hip) instead of torch's
  per-parameter loop: the whole ResNet update is a single launch.
* ``zero_grad()`` is one memset.
* Data-parallel gradient sync is ONE RCCL all-reduce of the flat gradient
  buffer — the maximal bucket for the xGMI ring (see
  :func:`flashy_amd.distrib.sync_flat_gradients`).

Replaces the reference's use of torch.optim.SGD/Adam in its workloads
(SURVEY.md §2.10 "SGD step / Adam step (fused over all params)").

On CUDA devices the native extension is REQUIRED (loud failure otherwise);
on CPU the same classes run a torch fallback with identical numerics, so
every test runs in CI.

Learning-rate schedules and global-norm gradient clipping are part of
``step()`` (``schedule=`` / ``max_grad_norm=``): the effective ``lr`` and the
clip coefficient are computed ON THE DEVICE each step from a device step
counter and the gradient arena, and the update kernels read them from
memory.  A step captured into a HIP graph therefore follows the schedule and
clips, with no re-capture and no host sync.  :class:`LRSchedule` objects are
the host mirror of the same closed forms.

Per-tensor hyperparameters (``param_options=`` / torch-style param groups) and
LARS trust ratios (``FusedSGD(..., lars=LARS())``) ride on a chunk table that
tells the kernels where each tensor lies in the flat buffer; the layout of
the buffer itself never changes, and an optimizer built without them launches
exactly the unsegmented kernels.  The trust ratios are computed on the device
from the hyper block, so they too are correct under graph replay.
"""
from __future__ import annotations

import dataclasses
import math
import typing as tp

import torch

from . import ops

ParamsT = tp.Union[tp.Iterable[torch.nn.Parameter],
                   tp.Iterable[tp.Mapping[str, tp.Any]]]
ParamOptionsT = tp.Union[
    tp.Callable[[torch.nn.Parameter], tp.Optional[tp.Mapping[str, tp.Any]]],
    tp.Mapping[torch.nn.Parameter, tp.Mapping[str, tp.Any]]]

MAX_MILESTONES = 8


# ---------------------------------------------------------------------------
# LR schedules: closed forms of the step index (0 for the first step() call).
# The device evaluates the same expressions in k_optim_prepare
# (ops/csrc/fused_optim.hip); `kernel_args` is the POD that travels there.
# ---------------------------------------------------------------------------

class LRSchedule:
    """Immutable description of a learning-rate schedule.

    ``lr_at(step, base_lr)`` is the learning rate used by the ``step``-th
    update counted from 0 — torch's convention of calling
    ``scheduler.step()`` after ``optimizer.step()``.  Plain Python floats:
    this is the CPU path, the host mirror for logging, and what the tests
    compare the device against."""

    KIND = 0

    def factor(self, step: int) -> float:
        del step
        return 1.0

    def lr_at(self, step: int, base_lr: float) -> float:
        return base_lr * self.factor(max(int(step), 0))

    def _warm(self, step: int) -> float:
        if step >= self.warmup_steps:
            return 1.0
        return self.start_factor + (1.0 - self.start_factor) * (
            step / self.warmup_steps)

    def _check_warmup(self) -> None:
        if self.warmup_steps < 0:
            raise ValueError(f"warmup_steps must be >= 0: {self.warmup_steps}")
        if self.start_factor < 0:
            raise ValueError(f"start_factor must be >= 0: {self.start_factor}")

    def kernel_args(self) -> tp.Tuple[tp.Any, ...]:
        """(kind, warmup_steps, start_factor, total_steps, min_ratio,
        milestones, gamma) as plain ints / floats."""
        def get(name: str, default: tp.Any) -> tp.Any:
            return getattr(self, name, default)

        return (self.KIND, int(get("warmup_steps", 0)),
                float(get("start_factor", 0.0)), int(get("total_steps", 1)),
                float(get("min_ratio", 0.0)),
                tuple(int(m) for m in get("milestones", ())),
                float(get("gamma", 1.0)))


@dataclasses.dataclass(frozen=True)
class Constant(LRSchedule):
    """``lr`` stays at the base value."""
    KIND = 0


@dataclasses.dataclass(frozen=True)
class _WarmupDecay(LRSchedule):
    warmup_steps: int
    total_steps: int
    min_ratio: float = 0.0
    start_factor: float = 0.0

    def __post_init__(self):
        self._check_warmup()
        if self.total_steps <= self.warmup_steps:
            raise ValueError(
                f"total_steps ({self.total_steps}) must exceed warmup_steps "
                f"({self.warmup_steps})")

    def _decay(self, x: float) -> float:
        raise NotImplementedError

    def factor(self, step: int) -> float:
        if step < self.warmup_steps:
            return self._warm(step)
        t = min(step, self.total_steps) - self.warmup_steps
        x = t / (self.total_steps - self.warmup_steps)
        return self.min_ratio + (1.0 - self.min_ratio) * self._decay(x)


@dataclasses.dataclass(frozen=True)
class WarmupCosine(_WarmupDecay):
    """Linear warmup from ``start_factor`` to 1 over ``warmup_steps``, then a
    half cosine down to ``min_ratio`` at ``total_steps``; the floor holds
    afterwards."""
    KIND = 1

    def _decay(self, x: float) -> float:
        return 0.5 * (1.0 + math.cos(math.pi * x))


@dataclasses.dataclass(frozen=True)
class WarmupLinear(_WarmupDecay):
    """Linear warmup, then a straight line down to ``min_ratio`` at
    ``total_steps``; the floor holds afterwards."""
    KIND = 2

    def _decay(self, x: float) -> float:
        return 1.0 - x


@dataclasses.dataclass(frozen=True)
class MultiStep(LRSchedule):
    """``lr`` is multiplied by ``gamma`` at each milestone (at most 8), on top
    of an optional linear warmup."""
    KIND = 3
    milestones: tp.Sequence[int]
    gamma: float = 0.1
    warmup_steps: int = 0
    start_factor: float = 0.0

    def __post_init__(self):
        object.__setattr__(self, "milestones",
                           tuple(int(m) for m in self.milestones))
        if len(self.milestones) > MAX_MILESTONES:
            raise ValueError(
                f"at most {MAX_MILESTONES} milestones, got "
                f"{len(self.milestones)}")
        if any(m < 0 for m in self.milestones):
            raise ValueError(f"milestones must be >= 0: {self.milestones}")
        self._check_warmup()

    def factor(self, step: int) -> float:
        passed = sum(1 for m in self.milestones if m <= step)
        return self._warm(step) * math.pow(self.gamma, float(passed))


# ---------------------------------------------------------------------------
# Per-tensor options and LARS
# ---------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class LARS:
    """Layer-wise adaptive rate scaling (timm's ``Lars``, ``trust_clip`` off):
    a tensor's update is multiplied by
    ``eta * |p| / (|g| + weight_decay * |p| + eps)``, or by 1 where either
    norm is 0."""
    eta: float = 1e-3
    eps: float = 1e-8

    def __post_init__(self):
        if not self.eta > 0:
            raise ValueError(f"eta must be > 0: {self.eta}")
        if self.eps < 0:
            raise ValueError(f"eps must be >= 0: {self.eps}")


OPTION_KEYS = ("weight_decay", "lr_scale", "lars")
_GROUP_KEYS = ("params", "weight_decay", "lr", "lars")


def no_decay_1d(p: torch.nn.Parameter) -> tp.Dict[str, tp.Any]:
    """``param_options`` callable for the usual BatchNorm / bias exemption:
    no weight decay and no LARS on tensors with ``ndim <= 1``."""
    if p.ndim <= 1:
        return {"weight_decay": 0.0, "lars": False}
    return {}


def _checked_options(raw: tp.Optional[tp.Mapping[str, tp.Any]]
                     ) -> tp.Dict[str, tp.Any]:
    """One tensor's options; ``None`` for weight_decay / lars means "use the
    optimizer's value"."""
    raw = raw or {}
    unknown = sorted(set(raw) - set(OPTION_KEYS))
    if unknown:
        raise ValueError(f"unknown param option(s) {unknown}; "
                         f"known: {list(OPTION_KEYS)}")
    wd = raw.get("weight_decay")
    lars = raw.get("lars")
    return {"weight_decay": None if wd is None else float(wd),
            "lr_scale": float(raw.get("lr_scale", 1.0)),
            "lars": None if lars is None else bool(lars)}


def _unpack_param_groups(groups: tp.Sequence[tp.Mapping[str, tp.Any]],
                         default_lr: float):
    """torch-style param groups -> (parameters in order of appearance,
    {id(param): options})."""
    params: tp.List[torch.nn.Parameter] = []
    options: tp.Dict[int, tp.Dict[str, tp.Any]] = {}
    for group in groups:
        if not isinstance(group, tp.Mapping) or "params" not in group:
            raise ValueError("a param group is a dict with a 'params' entry")
        unknown = sorted(set(group) - set(_GROUP_KEYS))
        if unknown:
            raise ValueError(f"unknown param group key(s) {unknown}; "
                             f"known: {list(_GROUP_KEYS)}")
        opts = {k: group[k] for k in ("weight_decay", "lars") if k in group}
        if "lr" in group:
            if default_lr == 0:
                raise ValueError("a group lr needs a non-zero default lr")
            opts["lr_scale"] = group["lr"] / default_lr
        members = group["params"]
        if isinstance(members, torch.Tensor):
            members = [members]
        for p in members:
            if id(p) in options:
                raise ValueError(
                    "some parameters appear in more than one parameter group")
            options[id(p)] = opts
            params.append(p)
    return params, options


class _Group:
    """One (device, dtype) flat group."""

    def __init__(self, params: tp.List[torch.nn.Parameter],
                 bf16_mirror: bool = False):
        self.params = params
        self.device = params[0].device
        self.dtype = params[0].dtype
        total = sum(p.numel() for p in params)
        self.flat_p = torch.empty(total, device=self.device, dtype=self.dtype)
        offset = 0
        views = []
        for p in params:
            n = p.numel()
            view = self.flat_p[offset:offset + n].view_as(p)
            view.copy_(p.data)
            views.append(view)
            offset += n
        # re-point after all copies (a param could alias another's storage)
        for p, view in zip(params, views):
            p.data = view
        self.flat_g = torch.zeros_like(self.flat_p)
        offset = 0
        for p in params:
            n = p.numel()
            p.grad = self.flat_g[offset:offset + n].view_as(p)
            offset += n
        # optional bf16 mirror of the packed params, refreshed by the fused
        # optimizer kernel in the same pass as the update; modules read the
        # per-param view via `param._bf16_mirror` (flashy_amd/nn.py) so the
        # step needs zero weight-cast kernels.
        # per-tensor options (one dict per param, see _checked_options), and
        # when they make the step segmented: the device chunk table, the
        # per-chunk (sum p^2, sum g^2) workspace and the trust ratios
        self.options: tp.List[tp.Dict[str, tp.Any]] = []
        self.seg: tp.Optional[ops.SegTable] = None
        self.seg_partials: tp.Optional[torch.Tensor] = None
        self.ratio: tp.Optional[torch.Tensor] = None
        self.flat_p16: tp.Optional[torch.Tensor] = None
        if bf16_mirror:
            self.flat_p16 = self.flat_p.to(torch.bfloat16)
            offset = 0
            for p in params:
                n = p.numel()
                p._bf16_mirror = self.flat_p16[offset:offset + n].view_as(p)
                offset += n

    def refresh_bf16(self) -> None:
        if self.flat_p16 is not None:
            self.flat_p16.copy_(self.flat_p)

    def buffers_like(self) -> torch.Tensor:
        return torch.zeros_like(self.flat_p)


class FlatOptimizer:
    """Base: flat parameter/grad packing + state dict plumbing.

    ``params`` is an iterable of parameters or a list of torch-style param
    groups (``{"params": [...], "weight_decay": ..., "lr": ..., "lars":
    ...}``, packed in order of appearance; a group ``lr`` becomes
    ``lr_scale = lr / default lr``).  Prefer ``param_options``: a callable
    ``(param) -> options or None`` or a mapping ``param -> options`` with the
    keys ``weight_decay``, ``lr_scale`` and ``lars``, which keeps the
    parameters packed in the model's own order (e.g.
    ``param_options=no_decay_1d``)."""

    _SUPPORTS_LARS = False

    def __init__(self, params: ParamsT, defaults: tp.Dict[str, tp.Any],
                 bf16_mirror: bool = False,
                 schedule: tp.Optional[LRSchedule] = None,
                 max_grad_norm: tp.Optional[float] = None,
                 param_options: tp.Optional[ParamOptionsT] = None,
                 lars: tp.Optional[LARS] = None):
        if schedule is not None and not isinstance(schedule, LRSchedule):
            raise TypeError(f"schedule must be an LRSchedule, got {schedule!r}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(
                f"max_grad_norm must be > 0 or None, got {max_grad_norm}")
        if lars is not None and not isinstance(lars, LARS):
            raise TypeError(f"lars must be a LARS, got {lars!r}")
        if lars is not None and not self._SUPPORTS_LARS:
            raise NotImplementedError(
                f"{type(self).__name__} has no LARS (LAMB needs the norm of "
                f"the update); use FusedSGD(..., lars=LARS())")
        params = list(params)
        group_options: tp.Dict[int, tp.Dict[str, tp.Any]] = {}
        if params and isinstance(params[0], tp.Mapping):
            if param_options is not None:
                raise ValueError(
                    "give either param groups or param_options, not both")
            params, group_options = _unpack_param_groups(
                params, defaults["lr"])
        params =[p for p in params if p.requires_grad]
        if not params:
            raise ValueError("no trainable parameters")
        for p in params:
            if p.dtype != torch.float32:
                raise TypeError(
                    f"FlatOptimizer packs fp32 master params, got {p.dtype}")
        by_key: tp.Dict[tp.Any, tp.List[torch.nn.Parameter]] = {}
        for p in params:
            by_key.setdefault((p.device, p.dtype), []).append(p)
        self.groups = [_Group(ps, bf16_mirror) for ps in by_key.values()]
        self.defaults = dict(defaults)
        self.lars = lars

        def options_of(p: torch.nn.Parameter) -> tp.Dict[str, tp.Any]:
            if id(p) in group_options:
                raw = group_options[id(p)]
            elif param_options is None:
                raw = None
            elif isinstance(param_options, tp.Mapping):
                raw = param_options.get(p)
            else:
                raw = param_options(p)
            return _checked_options(raw)

        for g in self.groups:
            g.options = [options_of(p) for p in g.params]
        self._segmented = False
        self.step_count = 0
        self._use_hip = any(g.device.type == "cuda" for g in self.groups)
        if self._use_hip:
            ops.require()  # fail loudly now, not at the first step
        # device step counters (one int64 per CUDA device), created by the
        # subclasses that need one; each holds the 1-based number of the
        # NEXT step, and is authoritative under HIP-graph replay
        self._step_dev: tp.Dict[torch.device, torch.Tensor] = {}
        self.schedule = schedule
        self.max_grad_norm = max_grad_norm
        # "managed" step: lr / clip coefficient come from a per-device hyper
        # block (CUDA) or from _host_hyper (CPU) instead of defaults["lr"]
        self._managed = schedule is not None or max_grad_norm is not None
        self._sched = schedule if schedule is not None else Constant()
        self._hyper: tp.Dict[torch.device, torch.Tensor] = {}
        self._partials: tp.Dict[torch.device, torch.Tensor] = {}
        self._partial_slices: tp.Dict[int, torch.Tensor] = {}
        self._host_hyper: tp.Tuple[float, tp.Optional[float]] = (0.0, None)
        self._host_norm: tp.Optional[torch.Tensor] = None
        if self._managed:
            self._init_managed()
        self._configure_segments()

    # -- per-tensor options --------------------------------------------------
    def _resolved(self, group: _Group
                  ) -> tp.List[tp.Tuple[float, float, bool]]:
        """(weight_decay, lr_scale, lars) per tensor of ``group``."""
        wd = self.defaults["weight_decay"]
        return [(wd if o["weight_decay"] is None else o["weight_decay"],
                 o["lr_scale"],
                 self.lars is not None if o["lars"] is None else o["lars"])
                for o in group.options]

    def _configure_segments(self) -> None:
        """Decide whether the step is segmented (some tensor's options differ
        from the defaults, or LARS is on for some tensor) and build or
        refresh the chunk tables.  Values are rewritten in place, so a
        captured step sees restored options."""
        resolved = [self._resolved(g) for g in self.groups]
        wd = self.defaults["weight_decay"]
        uses_lars = any(r[2] for rs in resolved for r in rs)
        if uses_lars and not self._SUPPORTS_LARS:
            raise NotImplementedError(
                f"'lars': True on {type(self).__name__}: LARS is implemented "
                f"for FusedSGD only")
        if uses_lars and self.lars is None:
            raise ValueError("'lars': True needs lars=LARS(...) on the "
                             "optimizer")
        self._segmented = uses_lars or any(
            r[0] != wd or r[1] != 1.0 for rs in resolved for r in rs)
        if not self._segmented:
            return
        for g, rs in zip(self.groups, resolved):
            cols = list(zip(*rs))
            if g.device.type == "cuda":
                if g.seg is None:
                    g.seg = ops.SegTable([p.numel() for p in g.params],
                                         *cols, device=g.device)
                else:
                    g.seg.set_options(*cols)
            if uses_lars and g.ratio is None:
                g.ratio = torch.ones(len(g.params), dtype=torch.float32,
                                     device=g.device)
                if g.seg is not None:
                    g.seg_partials = torch.empty(
                        g.seg.n_chunks, 2, dtype=torch.float32,
                        device=g.device)

    @property
    def last_trust_ratios(self) -> tp.Optional[tp.List[torch.Tensor]]:
        """LARS trust ratios of the last step: one fp32 tensor per flat group
        (see ``param_buffers``), on that group's device, one entry per
        parameter in packing order (1 where LARS is off or a norm is 0).  No
        sync.  ``None`` without LARS."""
        if not any(g.ratio is not None for g in self.groups):
            return None
        return [g.ratio for g in self.groups]

    def _init_managed(self) -> None:
        devices = []
        for g in self.groups:
            if g.device not in devices:
                devices.append(g.device)
        clip = self.max_grad_norm is not None
        if clip and len(devices) > 1:
            raise NotImplementedError(
                "max_grad_norm with parameters on more than one device: a "
                "cross-device gradient norm is not implemented")
        for dev in devices:
            if dev.type != "cuda":
                if clip:
                    self._host_norm = torch.zeros((), dtype=torch.float32)
                continue
            hyper = torch.zeros(ops.HYPER_SIZE, dtype=torch.float32, device=dev)
            hyper[ops.HYPER_LR] = self.defaults["lr"]
            hyper[ops.HYPER_COEF] = 1.0
            self._hyper[dev] = hyper
            if not clip:
                continue
            mine = [g for g in self.groups if g.device == dev]
            counts = [ops.grad_sqsum_blocks(g.flat_g.numel()) for g in mine]
            ws = torch.zeros(sum(counts), dtype=torch.float32, device=dev)
            self._partials[dev] = ws
            offset = 0
            for g, n in zip(mine, counts):
                self._partial_slices[id(g)] = ws[offset:offset + n]
                offset += n

    def _make_step_counters(self) -> None:
        for g in self.groups:
            if g.device.type == "cuda" and g.device not in self._step_dev:
                self._step_dev[g.device] = torch.ones(
                    1, dtype=torch.int64, device=g.device)

    def _steps_done(self) -> int:
        """Number of completed steps; the device counter is authoritative
        (under graph replay the host count freezes).  Reads the device."""
        if self._step_dev:
            return max(int(s.item()) for s in self._step_dev.values()) - 1
        return self.step_count

    def current_lr(self) -> float:
        """Learning rate the next ``step()`` will use (host mirror of the
        schedule at the authoritative step count) — what
        ``scheduler.get_last_lr()`` reports in a torch loop."""
        return self._sched.lr_at(self._steps_done(), self.defaults["lr"])

    @property
    def last_grad_norm(self) -> tp.Optional[torch.Tensor]:
        """Pre-clip global gradient norm of the last step as a 0-dim tensor
        on the parameters' device (no sync; call ``.item()`` when logging).
        ``None`` unless ``max_grad_norm`` is set."""
        if self.max_grad_norm is None:
            return None
        for hyper in self._hyper.values():
            return hyper[ops.HYPER_NORM]
        return self._host_norm

    def _prepare(self) -> None:
        """Norm pass (only when clipping) + the 1-block prepare kernel per
        device; on CPU the same math in Python floats.  Stream-ordered, no
        host reads of device memory: capturable."""
        clip = self.max_grad_norm is not None
        base_lr = self.defaults["lr"]
        for dev, hyper in self._hyper.items():
            if clip:
                for g in self.groups:
                    if g.device == dev:
                        ops.grad_sqsum(g.flat_g, self._partial_slices[id(g)])
            ops.optim_prepare(hyper, self._sched, base_lr,
                              step_dev=self._step_dev.get(dev),
                              partials=self._partials.get(dev),
                              max_norm=self.max_grad_norm if clip else 0.0)
        if len(self._hyper) == len({g.device for g in self.groups}):
            return
        coef = None
        if clip:
            sq = sum(float(g.flat_g.double().pow(2).sum())
                     for g in self.groups if g.device.type != "cuda")
            norm = math.sqrt(sq)
            c = self.max_grad_norm / (norm + 1e-6)
            coef = 1.0 if c > 1.0 else c  # a NaN norm stays NaN, as in torch
            self._host_norm.fill_(norm)
        self._host_hyper = (
            self._sched.lr_at(self.step_count - 1, base_lr), coef)

    def _lr_coef(self) -> tp.Tuple[float, tp.Optional[float]]:
        """(lr, clip coefficient or None) for the CPU fallback."""
        if self._managed:
            return self._host_hyper
        return self.defaults["lr"], None

    # -- torch-optimizer-compatible surface ---------------------------------
    def zero_grad(self, set_to_none: bool = False) -> None:
        # grads are views into the flat buffer: never set to None
        del set_to_none
        for g in self.groups:
            g.flat_g.zero_()

    @property
    def grad_buffers(self) -> tp.List[torch.Tensor]:
        """Flat gradient buffers (one per group) — the DP sync payload."""
        return [g.flat_g for g in self.groups]

    @property
    def param_buffers(self) -> tp.List[torch.Tensor]:
        return [g.flat_p for g in self.groups]

    def refresh_bf16(self) -> None:
        """Re-sync the bf16 mirrors after any out-of-band param mutation
        (checkpoint restore, broadcast_model)."""
        for g in self.groups:
            g.refresh_bf16()

    def step(self, closure: tp.Optional[tp.Callable] = None) -> None:
        loss = closure() if closure is not None else None
        self.step_count += 1
        if self._managed:
            self._prepare()
        for g in self.groups:
            self._step_group(g)
        for dev_step in self._step_dev.values():
            ops.adam_step_inc(dev_step)
        return loss

    def _step_group(self, group: _Group) -> None:
        raise NotImplementedError

    # -- checkpointing -------------------------------------------------------
    def _extra_state(self) -> tp.Dict[str, tp.Any]:
        return {}

    def _load_extra_state(self, state: tp.Dict[str, tp.Any]) -> None:
        del state

    def state_dict(self) -> tp.Dict[str, tp.Any]:
        # The device counter is authoritative: under HIP-graph capture
        # step() runs only at capture time, so the host count freezes
        # while the device counter advances per replay.
        self.step_count = self._steps_done()
        return {
            "defaults": dict(self.defaults),
            "step_count": self.step_count,
            "extra": self._extra_state(),
            # per flat group, per tensor in packing order; weight_decay None
            # = the optimizer's value
            "param_options": [
                [{"numel": p.numel(), "weight_decay": o["weight_decay"],
                  "lr_scale": o["lr_scale"], "lars": r[2]}
                 for p, o, r in zip(g.params, g.options, self._resolved(g))]
                for g in self.groups],
        }

    def load_state_dict(self, state: tp.Mapping[str, tp.Any]) -> None:
        saved = state.get("param_options")  # absent in older checkpoints
        if saved is not None:
            if [[o["numel"] for o in opts] for opts in saved] != \
                    [[p.numel() for p in g.params] for g in self.groups]:
                raise ValueError(
                    "saved param_options do not match this optimizer's "
                    "tensors (count or sizes differ)")
        self.defaults.update(state.get("defaults", {}))
        if saved is not None:
            for g, opts in zip(self.groups, saved):
                g.options = [_checked_options(
                    {k: o[k] for k in OPTION_KEYS}) for o in opts]
            self._configure_segments()
        self.step_count = state.get("step_count", 0)
        self._load_extra_state(state.get("extra", {}))
        for dev_step in self._step_dev.values():
            dev_step.fill_(self.step_count + 1)
        # model params are usually restored in the same breath
        # (StateManager restores the model first); re-sync the bf16 mirrors
        self.refresh_bf16()


class FusedSGD(FlatOptimizer):
    """torch.optim.SGD semantics (momentum / weight decay / nesterov) as one
    fused HIP kernel over the flat buffers.

    ``param_options`` / param groups: see :class:`FlatOptimizer`.  With
    ``lars=LARS(eta, eps)`` every tensor whose ``lars`` option is not False
    is updated as, with ``g' = clip_coef * g``::

        ratio = eta * |p| / (|g'| + wd_t * |p| + eps)  if |p| > 0 and |g'| > 0
                1                                       otherwise
        d = ratio * (g' + wd_t * p)
        m = mu * m + d ; d = nesterov ? d + mu * m : m       (if momentum)
        p -= lr * lr_scale_t * d

    and the others (``ratio = 1``) by the plain SGD formula.  The norms are
    taken on the device each step (``last_trust_ratios``)."""

    _SUPPORTS_LARS = True

    def __init__(self, params: ParamsT, lr: float, momentum: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False,
                 bf16_mirror: bool = False,
                 schedule: tp.Optional[LRSchedule] = None,
                 max_grad_norm: tp.Optional[float] = None,
                 param_options: tp.Optional[ParamOptionsT] = None,
                 lars: tp.Optional[LARS] = None):
        super().__init__(params, dict(lr=lr, momentum=momentum,
                                      weight_decay=weight_decay,
                                      nesterov=nesterov), bf16_mirror,
                         schedule, max_grad_norm, param_options, lars)
        self._momentum_buffers = [
            g.buffers_like() if momentum != 0 else None for g in self.groups]
        if schedule is not None:
            # the schedule is evaluated on the device from this counter, so
            # a captured step keeps following it under replay
            self._make_step_counters()

    def _step_group(self, group: _Group) -> None:
        d = self.defaults
        m = self._momentum_buffers[self.groups.index(group)]
        if self._segmented:
            self._step_group_segmented(group, m)
            return
        if group.device.type == "cuda":
            ops.fused_sgd(group.flat_p, group.flat_g, m, d["lr"],
                          d["momentum"], d["weight_decay"],
                          nesterov=d["nesterov"], p_bf16=group.flat_p16,
                          hyper=self._hyper.get(group.device))
            return
        # CPU fallback, identical math
        lr, coef = self._lr_coef()
        with torch.no_grad():
            g = group.flat_g
            if coef is not None:
                g = g * coef
            if d["weight_decay"] != 0:
                g = g.add(group.flat_p, alpha=d["weight_decay"])
            if d["momentum"] != 0:
                m.mul_(d["momentum"]).add_(g)
                g = g.add(m, alpha=d["momentum"]) if d["nesterov"] else m
            group.flat_p.add_(g, alpha=-lr)
            group.refresh_bf16()

    def _step_group_segmented(self, group: _Group,
                              m: tp.Optional[torch.Tensor]) -> None:
        d = self.defaults
        if group.device.type == "cuda":
            hyper = self._hyper.get(group.device)
            if group.ratio is not None:
                ops.seg_sqsum(group.flat_p, group.flat_g, group.seg,
                              group.seg_partials)
                ops.lars_prepare(group.seg_partials, group.seg, group.ratio,
                                 self.lars.eta, self.lars.eps, hyper=hyper)
            ops.fused_sgd_seg(group.flat_p, group.flat_g, m, d["lr"],
                              d["momentum"], group.seg,
                              nesterov=d["nesterov"], p_bf16=group.flat_p16,
                              hyper=hyper, ratio=group.ratio)
            return
        # CPU fallback: the same math, tensor by tensor
        lr, coef = self._lr_coef()
        with torch.no_grad():
            offset = 0
            for t, (p, (wd, lr_scale, lars_on)) in enumerate(
                    zip(group.params, self._resolved(group))):
                n = p.numel()
                w = group.flat_p[offset:offset + n]
                g = group.flat_g[offset:offset + n]
                if coef is not None:
                    g = g * coef
                ratio = 1.0
                if lars_on:
                    wn = float(w.double().norm())
                    gn = float(g.double().norm())
                    if wn > 0 and gn > 0:
                        ratio = self.lars.eta * wn / (
                            gn + wd * wn + self.lars.eps)
                if group.ratio is not None:
                    group.ratio[t] = ratio
                if wd != 0:
                    g = g.add(w, alpha=wd)
                if ratio != 1.0:
                    g = g * ratio
                if d["momentum"] != 0:
                    mt = m[offset:offset + n]
                    mt.mul_(d["momentum"]).add_(g)
                    g = g.add(mt, alpha=d["momentum"]) if d["nesterov"] else mt
                w.add_(g, alpha=-lr * lr_scale)
                offset += n
            group.refresh_bf16()

    def _extra_state(self):
        return {"momentum_buffers": self._momentum_buffers}

    def _load_extra_state(self, state):
        saved = state.get("momentum_buffers")
        if saved:
            for mine, got in zip(self._momentum_buffers, saved):
                if mine is not None and got is not None:
                    mine.copy_(got.to(mine.device))


class FusedAdam(FlatOptimizer):
    """torch.optim.Adam/AdamW semantics as one fused HIP kernel per group.

    ``param_options`` / param groups: see :class:`FlatOptimizer`
    (``weight_decay`` and ``lr_scale`` per tensor).  LARS is not implemented
    here: ``lars=`` and ``'lars': True`` raise ``NotImplementedError``."""

    def __init__(self, params: ParamsT, lr: float = 1e-3,
                 betas: tp.Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0,
                 adamw: bool = False, bf16_mirror: bool = False,
                 schedule: tp.Optional[LRSchedule] = None,
                 max_grad_norm: tp.Optional[float] = None,
                 param_options: tp.Optional[ParamOptionsT] = None,
                 lars: tp.Optional[LARS] = None):
        super().__init__(params, dict(lr=lr, beta1=betas[0], beta2=betas[1],
                                      eps=eps, weight_decay=weight_decay,
                                      adamw=adamw), bf16_mirror,
                         schedule, max_grad_norm, param_options, lars)
        self._exp_avg = [g.buffers_like() for g in self.groups]
        self._exp_avg_sq = [g.buffers_like() for g in self.groups]
        # device-side step counter: the kernel reads it for bias correction,
        # so the whole step is HIP-graph-replay-safe (a captured host step
        # count would freeze).  Starts at 1 = the value used by step #1.
        # A schedule reads the same counter (at index count - 1).
        self._make_step_counters()

    def _step_group(self, group: _Group) -> None:
        d = self.defaults
        i = self.groups.index(group)
        m, v = self._exp_avg[i], self._exp_avg_sq[i]
        if self._segmented and group.device.type == "cuda":
            ops.fused_adam_seg(group.flat_p, group.flat_g, m, v, d["lr"],
                               d["beta1"], d["beta2"], d["eps"],
                               self.step_count, group.seg, adamw=d["adamw"],
                               p_bf16=group.flat_p16,
                               step_dev=self._step_dev[group.device],
                               hyper=self._hyper.get(group.device))
            return
        if group.device.type == "cuda":
            ops.fused_adam(group.flat_p, group.flat_g, m, v, d["lr"],
                           d["beta1"], d["beta2"], d["eps"],
                           d["weight_decay"], self.step_count,
                           adamw=d["adamw"], p_bf16=group.flat_p16,
                           step_dev=self._step_dev[group.device],
                           hyper=self._hyper.get(group.device))
            return
        lr, coef = self._lr_coef()
        if self._segmented:
            self._step_group_segmented_cpu(group, m, v, lr, coef)
            return
        with torch.no_grad():
            g = group.flat_g
            p = group.flat_p
            if coef is not None:
                g = g * coef
            if d["adamw"]:
                p.mul_(1 - lr * d["weight_decay"])
            elif d["weight_decay"] != 0:
                g = g.add(p, alpha=d["weight_decay"])
            m.mul_(d["beta1"]).add_(g, alpha=1 - d["beta1"])
            v.mul_(d["beta2"]).addcmul_(g, g, value=1 - d["beta2"])
            bc1 = 1 - d["beta1"] ** self.step_count
            bc2 = 1 - d["beta2"] ** self.step_count
            denom = (v / bc2).sqrt_().add_(d["eps"])
            p.addcdiv_(m / bc1, denom, value=-lr)
            group.refresh_bf16()

    def _step_group_segmented_cpu(self, group, m, v, lr, coef) -> None:
        """The same math as above, tensor by tensor."""
        d = self.defaults
        bc1 = 1 - d["beta1"] ** self.step_count
        bc2 = 1 - d["beta2"] ** self.step_count
        with torch.no_grad():
            offset = 0
            for param, (wd, lr_scale, _) in zip(group.params,
                                                self._resolved(group)):
                sl = slice(offset, offset + param.numel())
                offset = sl.stop
                p, g, mt, vt = group.flat_p[sl], group.flat_g[sl], m[sl], v[sl]
                lr_t = lr * lr_scale
                if coef is not None:
                    g = g * coef
                if d["adamw"]:
                    p.mul_(1 - lr_t * wd)
                elif wd != 0:
                    g = g.add(p, alpha=wd)
                mt.mul_(d["beta1"]).add_(g, alpha=1 - d["beta1"])
                vt.mul_(d["beta2"]).addcmul_(g, g, value=1 - d["beta2"])
                denom = (vt / bc2).sqrt_().add_(d["eps"])
                p.addcdiv_(mt / bc1, denom, value=-lr_t)
            group.refresh_bf16()

    def _extra_state(self):
        return {"exp_avg": self._exp_avg, "exp_avg_sq": self._exp_avg_sq}

    def _load_extra_state(self, state):
        for mine, got in zip(self._exp_avg, state.get("exp_avg", [])):
            mine.copy_(got.to(mine.device))
        for mine, got in zip(self._exp_avg_sq, state.get("exp_avg_sq", [])):
            mine.copy_(got.to(mine.device))
