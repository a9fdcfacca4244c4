# Copyright (c) Flashy-AMD authors.
"""LR schedules and global-norm gradient clipping of the flat optimizers, CPU
path.  The oracle is torch itself: torch.optim + clip_grad_norm_ +
torch.optim.lr_scheduler, run eagerly on a deep copy of the model.  The GPU
kernels are held to the same oracle in test_optim_sched_gpu.py."""
import copy
import math

import pytest
import torch
from torch import nn
from torch.optim import lr_scheduler as tls

from flashy_amd.optim import (Constant, FusedAdam, FusedSGD, MultiStep,
                              WarmupCosine, WarmupLinear)

BASE_LR = 0.05


# -- an independent statement of the closed forms (the LambdaLR oracle) ------

def _warm(k, warmup, start):
    return start + (1 - start) * k / warmup if k < warmup else 1.0


def _ref_factor(sched, k):
    if isinstance(sched, Constant):
        return 1.0
    if isinstance(sched, MultiStep):
        n = len([m for m in sched.milestones if k >= m])
        return _warm(k, sched.warmup_steps, sched.start_factor) * sched.gamma ** n
    if k < sched.warmup_steps:
        return _warm(k, sched.warmup_steps, sched.start_factor)
    span = sched.total_steps - sched.warmup_steps
    x = (min(k, sched.total_steps) - sched.warmup_steps) / span
    if isinstance(sched, WarmupCosine):
        shape = (1 + math.cos(math.pi * x)) / 2
    else:
        shape = 1 - x
    return sched.min_ratio + (1 - sched.min_ratio) * shape


def _torch_lrs(make_scheduler, n, base_lr=BASE_LR):
    """get_last_lr() before step 0, 1, ..., n-1 of a torch scheduler."""
    opt = torch.optim.SGD([nn.Parameter(torch.zeros(1))], lr=base_lr)
    sched = make_scheduler(opt)
    out = []
    for _ in range(n):
        out.append(sched.get_last_lr()[0])
        opt.step()
        sched.step()
    return out


def _close(a, b, base_lr=BASE_LR):
    # 1e-12 relative.  Both sides are base_lr * (a few O(1) double terms), so
    # where the schedule touches a floor of 0 the error is absolute,
    # ~1e-16 * base_lr, and "relative to the value" means nothing there:
    # that is the only thing the absolute term lets through.
    return math.isclose(a, b, rel_tol=1e-12, abs_tol=1e-14 * base_lr)


SCHEDULES = [
    Constant(),
    WarmupCosine(3, 10),
    WarmupCosine(0, 10, min_ratio=0.1),
    WarmupCosine(4, 12, min_ratio=0.01, start_factor=0.25),
    WarmupLinear(3, 10),
    WarmupLinear(0, 8, min_ratio=0.2),
    WarmupLinear(5, 9, min_ratio=0.05, start_factor=0.1),
    MultiStep([2, 5]),
    MultiStep([3, 6, 9], gamma=0.5, warmup_steps=4, start_factor=0.2),
    MultiStep([1, 2, 3, 4, 5, 6, 7, 8], gamma=0.7),
]


def _horizon(sched):
    total = getattr(sched, "total_steps", None)
    if total is None:
        total = max(getattr(sched, "milestones", (0,)) or (0,)) + 1
    return total + 6   # steps 0 .. total + 5


@pytest.mark.parametrize("sched", SCHEDULES, ids=repr)
def test_schedule_matches_lambda_lr(sched):
    n = _horizon(sched)
    ref = _torch_lrs(
        lambda opt: tls.LambdaLR(opt, lambda k: _ref_factor(sched, k)), n)
    for k in range(n):
        assert _close(sched.lr_at(k, BASE_LR), ref[k]), (k, ref[k])
    # steps past total_steps hold the floor
    if hasattr(sched, "total_steps"):
        floor = sched.lr_at(sched.total_steps, BASE_LR)
        assert _close(floor, BASE_LR * sched.min_ratio)
        for k in range(sched.total_steps, n):
            assert sched.lr_at(k, BASE_LR) == floor


def test_schedule_matches_torch_builtin_schedulers():
    """Where torch has the same schedule built in, compare with that too."""
    # MultiStepLR, and a milestone at the last warmup step (3 of 0..3) with
    # the warmup chained on top
    sched = MultiStep([2, 5], gamma=0.1)
    ref = _torch_lrs(lambda o: tls.MultiStepLR(o, [2, 5], gamma=0.1), 11)
    for k in range(11):
        assert _close(sched.lr_at(k, BASE_LR), ref[k]), k
    sched = MultiStep([3, 7], gamma=0.5, warmup_steps=4, start_factor=0.2)
    ref = _torch_lrs(lambda o: tls.ChainedScheduler([
        tls.LinearLR(o, start_factor=0.2, end_factor=1.0, total_iters=4),
        tls.MultiStepLR(o, [3, 7], gamma=0.5)]), 13)
    for k in range(13):
        assert _close(sched.lr_at(k, BASE_LR), ref[k]), k
    # CosineAnnealingLR coincides without warmup, up to total_steps (it is
    # periodic afterwards; ours holds the floor)
    sched = WarmupCosine(0, 10, min_ratio=0.1)
    ref = _torch_lrs(lambda o: tls.CosineAnnealingLR(
        o, T_max=10, eta_min=0.1 * BASE_LR), 11)
    for k in range(11):
        assert _close(sched.lr_at(k, BASE_LR), ref[k]), k
    # LinearLR is the linear decay without warmup, and holds its end value
    sched = WarmupLinear(0, 8, min_ratio=0.2)
    ref = _torch_lrs(lambda o: tls.LinearLR(
        o, start_factor=1.0, end_factor=0.2, total_iters=8), 14)
    for k in range(14):
        assert _close(sched.lr_at(k, BASE_LR), ref[k]), k


def test_argument_errors():
    with pytest.raises(ValueError):
        MultiStep(list(range(1, 10)))          # 9 milestones
    MultiStep(list(range(1, 9)))               # 8 are fine
    with pytest.raises(ValueError):
        WarmupCosine(10, 10)
    model = nn.Linear(4, 4)
    for bad in (0, 0.0, -1.0):
        with pytest.raises(ValueError):
            FusedSGD(model.parameters(), lr=0.1, max_grad_norm=bad)
        with pytest.raises(ValueError):
            FusedAdam(model.parameters(), lr=0.1, max_grad_norm=bad)


# -- optimizer parity ---------------------------------------------------------

MAX_NORM = 0.05
# (m(x) ** 2).mean() on this MLP has gradient norms of 0.13-0.37 under SGD and
# AdamW for all 12 steps: every step would clip.  The loss of step 9 is
# scaled down so that this step stays under MAX_NORM for every optimizer;
# the parity test asserts that the reference takes both branches.
SMALL_STEP, SMALL_SCALE = 9, 0.1


def _mlp():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(64, 128), nn.ReLU(), nn.Linear(128, 10))


def _batches(steps, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(16, 64, generator=g) for _ in range(steps)]


def _loss(model, x, k):
    return (model(x) ** 2).mean() * (SMALL_SCALE if k == SMALL_STEP else 1.0)


def _run_ours(model, opt, batches):
    norms = []
    for k, x in enumerate(batches):
        opt.zero_grad()
        _loss(model, x, k).backward()
        opt.step()
        if opt.last_grad_norm is not None:
            norms.append(opt.last_grad_norm.item())
    return norms


def _run_ref(model, opt, batches, sched=None, max_norm=None):
    """Eager torch loop: clip, step, then scheduler.step()."""
    scheduler = None
    if sched is not None:
        scheduler = tls.LambdaLR(opt, lambda k: _ref_factor(sched, k))
    norms = []
    for k, x in enumerate(batches):
        opt.zero_grad()
        _loss(model, x, k).backward()
        if max_norm is not None:
            norms.append(nn.utils.clip_grad_norm_(
                model.parameters(), max_norm).item())
        opt.step()
        if scheduler is not None:
            scheduler.step()
    return norms


def _assert_params_close(a, b, atol):
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.allclose(p, q, atol=atol), (p - q).abs().max().item()


def _assert_params_equal(a, b):
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q), (p - q).abs().max().item()


def _make(kind, params, schedule=None, max_grad_norm=None, **kw):
    if kind == "sgd":
        return FusedSGD(params, lr=BASE_LR, momentum=0.9, weight_decay=5e-4,
                        nesterov=True, schedule=schedule,
                        max_grad_norm=max_grad_norm, **kw)
    return FusedAdam(params, lr=1e-2, weight_decay=1e-2,
                     adamw=(kind == "adamw"), schedule=schedule,
                     max_grad_norm=max_grad_norm, **kw)


def _make_ref(kind, params):
    if kind == "sgd":
        return torch.optim.SGD(params, lr=BASE_LR, momentum=0.9,
                               weight_decay=5e-4, nesterov=True)
    klass = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    return klass(params, lr=1e-2, weight_decay=1e-2)


@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
@pytest.mark.parametrize("sched", [
    WarmupCosine(3, 10, start_factor=0.1), MultiStep([2, 5], gamma=0.5)],
    ids=["cosine", "multistep"])
def test_torch_parity_schedule_and_clipping(kind, sched):
    ours = _mlp()
    ref = copy.deepcopy(ours)
    batches = _batches(12)
    opt = _make(kind, ours.parameters(), sched, MAX_NORM)
    norms = _run_ours(ours, opt, batches)
    ref_norms = _run_ref(ref, _make_ref(kind, ref.parameters()), batches,
                         sched, MAX_NORM)
    # the reference must really take both branches of the clip
    clipped = sum(n > MAX_NORM for n in ref_norms)
    assert 7 <= clipped < 12 and ref_norms[SMALL_STEP] < MAX_NORM, ref_norms
    _assert_params_close(ours, ref, atol=1e-5)
    assert norms == pytest.approx(ref_norms, rel=1e-4)
    assert opt.current_lr() == sched.lr_at(12, opt.defaults["lr"])


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_noop_clipping_is_bitwise(kind):
    a = _mlp()
    b = copy.deepcopy(a)
    batches = _batches(5)
    opt_a = _make(kind, a.parameters(), max_grad_norm=1e9)
    opt_b = _make(kind, b.parameters())
    norms = _run_ours(a, opt_a, batches)
    _run_ours(b, opt_b, batches)
    assert all(n > 0 for n in norms)
    assert opt_a._lr_coef()[1] == 1.0      # clamped to exactly 1
    _assert_params_equal(a, b)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_zero_gradient(kind):
    model = _mlp()
    before = [p.detach().clone() for p in model.parameters()]
    opt = _make(kind, model.parameters(), WarmupCosine(0, 10), MAX_NORM)
    opt.zero_grad()
    opt.step()
    assert opt.last_grad_norm.item() == 0.0
    assert opt._lr_coef()[1] == 1.0
    for p, q in zip(model.parameters(), before):
        assert torch.isfinite(p).all()
        # only weight decay moves them: lr * wd * p for SGD, at most one
        # normalised Adam step of lr = 1e-2
        assert torch.allclose(p, q, atol=1.1e-2, rtol=0)


def test_inactive_feature_is_bitwise():
    """schedule=None, max_grad_norm=None: the plain formula, bit for bit."""
    model = _mlp()
    plain = copy.deepcopy(model)
    batches = _batches(5)
    opt = FusedSGD(model.parameters(), lr=BASE_LR, momentum=0.9,
                   weight_decay=5e-4, nesterov=True)
    assert not opt._managed and not opt._step_dev and opt.last_grad_norm is None
    _run_ours(model, opt, batches)
    # the parent commit's CPU step, spelled out on a flat copy
    flat_p = torch.cat([p.detach().reshape(-1) for p in plain.parameters()])
    mom = torch.zeros_like(flat_p)
    for k, x in enumerate(batches):
        offset = 0
        for p in plain.parameters():
            p.data.copy_(flat_p[offset:offset + p.numel()].view_as(p))
            offset += p.numel()
        plain.zero_grad()
        _loss(plain, x, k).backward()
        g = torch.cat([p.grad.reshape(-1) for p in plain.parameters()])
        g = g.add(flat_p, alpha=5e-4)
        mom.mul_(0.9).add_(g)
        g = g.add(mom, alpha=0.9)
        flat_p.add_(g, alpha=-BASE_LR)
    assert torch.equal(opt.param_buffers[0], flat_p)
    assert opt.current_lr() == BASE_LR


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_state_roundtrip_continues_schedule(kind):
    sched = WarmupCosine(3, 10, min_ratio=0.05, start_factor=0.1)
    batches = _batches(8)
    model = _mlp()
    opt = _make(kind, model.parameters(), sched, MAX_NORM)
    _run_ours(model, opt, batches[:7])
    saved = copy.deepcopy(opt.state_dict())
    assert saved["step_count"] == 7
    model2 = _mlp()
    model2.load_state_dict(copy.deepcopy(model.state_dict()))
    opt2 = _make(kind, model2.parameters(), sched, MAX_NORM)
    opt2.load_state_dict(saved)
    assert opt2.current_lr() == opt.current_lr() == sched.lr_at(
        7, opt.defaults["lr"])
    _run_ours(model, opt, batches[7:])
    _run_ours(model2, opt2, batches[7:])
    _assert_params_equal(model, model2)
    assert opt2.current_lr() == opt.current_lr() == sched.lr_at(
        8, opt.defaults["lr"])


def test_cifar_example_schedule_config():
    """The example's `schedule:` section maps onto the schedule classes, and
    is off when absent or when kind is null."""
    from flashy_amd.config import Config
    from examples.cifar.train import get_schedule
    assert get_schedule(Config.wrap({"epochs": 2}), 100) is None
    assert get_schedule(
        Config.wrap({"epochs": 2, "schedule": {"kind": None}}), 100) is None
    cfg = Config.wrap({"epochs": 2, "schedule": {
        "kind": "cosine", "warmup_steps": 5, "min_ratio": 0.01}})
    assert get_schedule(cfg, 100) == WarmupCosine(5, 200, min_ratio=0.01)
    cfg = Config.wrap({"epochs": 2, "schedule": {
        "kind": "linear", "total_steps": 50, "start_factor": 0.1}})
    assert get_schedule(cfg, 100) == WarmupLinear(0, 50, start_factor=0.1)
    cfg = Config.wrap({"epochs": 2, "schedule": {
        "kind": "multistep", "milestones": [30, 60], "gamma": 0.2}})
    assert get_schedule(cfg, 100) == MultiStep([30, 60], gamma=0.2)
    with pytest.raises(ValueError):
        get_schedule(Config.wrap({"epochs": 2, "schedule": {"kind": "exp"}}), 1)
