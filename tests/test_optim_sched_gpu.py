# Copyright (c) Flashy-AMD authors.
"""GPU tests: on-device LR schedule and global-norm clipping of the flat
optimizers — the norm kernels against an fp64 norm, and the optimizers, eager
and captured into a HIP graph, against eager torch.optim + clip_grad_norm_ +
LambdaLR on a deep copy of the model."""
import copy
import math

import pytest
import torch
from torch import nn
from torch.optim import lr_scheduler as tls

from flashy_amd.optim import (Constant, FusedAdam, FusedSGD, MultiStep,
                              WarmupCosine, WarmupLinear)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

MAX_NORM = 0.05


def _mlp():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(64, 128), nn.ReLU(),
                         nn.Linear(128, 10)).cuda()


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(16, 64, generator=g).cuda()


def _loss(model, x):
    return (model(x) ** 2).mean()


def _ref_factor(sched, k):
    """The schedules' closed forms, stated independently for LambdaLR."""
    warmup = getattr(sched, "warmup_steps", 0)
    warm = 1.0
    if k < warmup:
        warm = sched.start_factor + (1 - sched.start_factor) * k / warmup
    if isinstance(sched, Constant):
        return 1.0
    if isinstance(sched, MultiStep):
        return warm * sched.gamma ** len(
            [m for m in sched.milestones if k >= m])
    if k < warmup:
        return warm
    x = (min(k, sched.total_steps) - warmup) / (sched.total_steps - warmup)
    shape = (1 + math.cos(math.pi * x)) / 2 \
        if isinstance(sched, WarmupCosine) else 1 - x
    return sched.min_ratio + (1 - sched.min_ratio) * shape


def _run_ref(model, opt, batches, sched, max_norm):
    """Eager torch: clip, step, scheduler.step(); returns the pre-clip norms."""
    scheduler = tls.LambdaLR(opt, lambda k: _ref_factor(sched, k))
    norms = []
    for x in batches:
        opt.zero_grad()
        _loss(model, x).backward()
        norms.append(nn.utils.clip_grad_norm_(model.parameters(), max_norm))
        opt.step()
        scheduler.step()
    return [n.item() for n in norms]


def _run_eager(model, opt, batches):
    for x in batches:
        opt.zero_grad()
        _loss(model, x).backward()
        opt.step()


def _max_diff(a, b):
    return max((p - q).abs().max().item()
               for p, q in zip(a.parameters(), b.parameters()))


def _capture(model, opt, x):
    from flashy_amd.graph import CapturedStep

    # warmup=0 keeps the optimizer untouched before capture, so the BLAS
    # library must be initialised by hand: it refuses to create its handle
    # while a stream is capturing.  A throwaway copy takes the same GEMMs.
    _loss(copy.deepcopy(model), x).backward()
    torch.cuda.synchronize()

    def step():
        opt.zero_grad()
        loss = _loss(model, x)
        loss.backward()
        opt.step()
        return loss

    return CapturedStep(step, warmup=0).capture()


# -- the norm kernels ---------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4_194_307])
def test_grad_sqsum_and_prepare_vs_fp64_norm(n):
    """rtol 1e-5: a sum of non-negative fp32 terms is off by at most
    (terms per running sum) * 2^-24 relative; each thread keeps four running
    sums of at most 3 terms at these sizes, the lane, wave and block steps
    add 10 more, and from the block partials on everything is fp64."""
    from flashy_amd import ops
    torch.manual_seed(n)
    g = torch.randn(n, device="cuda")
    blocks = ops.grad_sqsum_blocks(n)
    assert blocks == min(2048, (n // 4 + 1 + 255) // 256)
    want = g.double().norm().item()
    out = []
    for _ in range(2):
        # no pre-zeroing needed: every partial is overwritten
        partials = torch.full((blocks,), float("nan"), device="cuda")
        hyper = torch.full((ops.HYPER_SIZE,), float("nan"), device="cuda")
        assert ops.grad_sqsum(g, partials) == blocks
        ops.optim_prepare(hyper, Constant(), 0.1, partials=partials,
                          max_norm=0.5 * want)
        out.append((partials, hyper))
    norm = out[0][1][ops.HYPER_NORM].item()
    assert norm == pytest.approx(want, rel=1e-5)
    assert out[0][1][ops.HYPER_COEF].item() == pytest.approx(
        0.5 * want / (want + 1e-6), rel=1e-5)
    assert out[0][1][ops.HYPER_LR].item() == pytest.approx(0.1, rel=1e-7)
    # deterministic: bitwise identical on a second call
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1][:3], out[1][1][:3])


# -- captured steps -----------------------------------------------------------

@requires_gpu
def test_captured_sgd_follows_schedule_and_clips():
    """A captured step must follow the schedule: with lr passed by value it
    would train all 10 replays at the lr it was captured with."""
    sched = WarmupCosine(3, 10)
    model = _mlp()
    ref = copy.deepcopy(model)
    frozen = copy.deepcopy(model)
    x = _batch()
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, schedule=sched,
                   max_grad_norm=MAX_NORM)
    graphed = _capture(model, opt, x)
    for _ in range(10):
        graphed()
    torch.cuda.synchronize()
    ref_norms = _run_ref(
        ref, torch.optim.SGD(ref.parameters(), lr=0.05, momentum=0.9),
        [x] * 10, sched, MAX_NORM)
    assert sum(n > MAX_NORM for n in ref_norms) >= 1, ref_norms
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.allclose(p, q, atol=1e-5), (p - q).abs().max().item()
    assert opt.current_lr() == sched.lr_at(10, 0.05)
    assert opt.last_grad_norm.is_cuda
    assert opt.last_grad_norm.item() == pytest.approx(ref_norms[-1], rel=1e-4)
    # a frozen lr cannot pass: same run without the schedule lands elsewhere
    _run_eager(frozen, FusedSGD(frozen.parameters(), lr=0.05, momentum=0.9,
                                max_grad_norm=MAX_NORM), [x] * 10)
    assert _max_diff(model, frozen) > 100 * 1e-5


@requires_gpu
def test_captured_adamw_follows_multistep_and_clips():
    sched = MultiStep([2, 5])
    model = _mlp()
    ref = copy.deepcopy(model)
    frozen = copy.deepcopy(model)
    x = _batch()
    opt = FusedAdam(model.parameters(), lr=1e-2, weight_decay=1e-2,
                    adamw=True, schedule=sched, max_grad_norm=MAX_NORM)
    graphed = _capture(model, opt, x)
    for _ in range(10):
        graphed()
    torch.cuda.synchronize()
    ref_norms = _run_ref(
        ref, torch.optim.AdamW(ref.parameters(), lr=1e-2, weight_decay=1e-2),
        [x] * 10, sched, MAX_NORM)
    assert sum(n > MAX_NORM for n in ref_norms) >= 1, ref_norms
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.allclose(p, q, atol=1e-4), (p - q).abs().max().item()
    assert opt.current_lr() == sched.lr_at(10, 1e-2)
    assert opt.last_grad_norm.item() == pytest.approx(ref_norms[-1], rel=1e-4)
    _run_eager(frozen, FusedAdam(frozen.parameters(), lr=1e-2,
                                 weight_decay=1e-2, adamw=True,
                                 max_grad_norm=MAX_NORM), [x] * 10)
    assert _max_diff(model, frozen) > 100 * 1e-4


@requires_gpu
def test_state_roundtrip_under_capture():
    sched = WarmupCosine(3, 10, min_ratio=0.05)
    model = _mlp()
    x = _batch()
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, schedule=sched,
                   max_grad_norm=MAX_NORM)
    graphed = _capture(model, opt, x)
    for _ in range(4):
        graphed()
    torch.cuda.synchronize()
    saved = opt.state_dict()
    assert saved["step_count"] == 4      # the host count froze at capture
    fresh = _mlp()
    fresh.load_state_dict(copy.deepcopy(model.state_dict()))
    opt2 = FusedSGD(fresh.parameters(), lr=0.05, momentum=0.9, schedule=sched,
                    max_grad_norm=MAX_NORM)
    opt2.load_state_dict(copy.deepcopy(saved))
    assert opt2.current_lr() == opt.current_lr() == sched.lr_at(4, 0.05)
    graphed()
    _run_eager(fresh, opt2, [x])
    torch.cuda.synchronize()
    for p, q in zip(model.parameters(), fresh.parameters()):
        assert torch.allclose(p, q, atol=1e-5), (p - q).abs().max().item()
    assert opt.state_dict()["step_count"] == 5
    assert opt2.state_dict()["step_count"] == 5


# -- eager --------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_eager_parity_with_bf16_mirror(kind):
    sched = WarmupLinear(2, 6, min_ratio=0.1, start_factor=0.2)
    model = _mlp()
    ref = copy.deepcopy(model)
    batches = [_batch(seed) for seed in range(5)]
    if kind == "sgd":
        opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9,
                       weight_decay=5e-4, nesterov=True, bf16_mirror=True,
                       schedule=sched, max_grad_norm=MAX_NORM)
        opt_ref = torch.optim.SGD(ref.parameters(), lr=0.05, momentum=0.9,
                                  weight_decay=5e-4, nesterov=True)
    else:
        opt = FusedAdam(model.parameters(), lr=1e-2, weight_decay=1e-2,
                        bf16_mirror=True, schedule=sched,
                        max_grad_norm=MAX_NORM)
        opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-2,
                                   weight_decay=1e-2)
    _run_eager(model, opt, batches)
    ref_norms = _run_ref(ref, opt_ref, batches, sched, MAX_NORM)
    assert sum(n > MAX_NORM for n in ref_norms) >= 1, ref_norms
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.allclose(p, q, atol=1e-5), (p - q).abs().max().item()
        assert torch.equal(p._bf16_mirror, p.detach().to(torch.bfloat16))
    assert opt.last_grad_norm.item() == pytest.approx(ref_norms[-1], rel=1e-4)


@requires_gpu
@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("sched", [
    Constant(),
    WarmupCosine(3, 10),
    WarmupCosine(0, 7, min_ratio=0.1),
    WarmupLinear(4, 9, min_ratio=0.05, start_factor=0.25),
    MultiStep([2, 5]),
    MultiStep([3, 6, 7], gamma=0.5, warmup_steps=4, start_factor=0.1),
], ids=repr)
def test_device_lr_matches_host_mirror(kind, sched):
    """atol 1e-6 * base_lr: the device evaluates the closed form once per
    step and stores an fp32 — a few ulp of 6e-8 relative to a value that is
    never above base_lr."""
    from flashy_amd import ops
    base_lr = 0.3
    p = nn.Parameter(torch.ones(4, device="cuda"))
    klass = FusedSGD if kind == "sgd" else FusedAdam
    opt = klass([p], lr=base_lr, schedule=sched)
    hyper = opt._hyper[p.device]
    total = getattr(sched, "total_steps", 8)
    seen = []
    for _ in range(total + 2):
        opt.step()
        seen.append(hyper[ops.HYPER_LR].item())
    for k, lr in enumerate(seen):
        assert abs(lr - sched.lr_at(k, base_lr)) <= 1e-6 * base_lr, (k, lr)
    assert hyper[ops.HYPER_COEF].item() == 1.0      # no clipping configured
    assert opt.current_lr() == sched.lr_at(total + 2, base_lr)


@requires_gpu
def test_inactive_feature_is_bitwise():
    """schedule=None, max_grad_norm=None: the step is the plain kernel call
    with the arguments the optimizer has always passed."""
    from flashy_amd import ops
    model = _mlp()
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9,
                   weight_decay=5e-4, nesterov=True, bf16_mirror=True)
    assert not opt._hyper and not opt._step_dev and opt.last_grad_norm is None
    group = opt.groups[0]
    p = group.flat_p.clone()
    m = torch.zeros_like(p)
    p16 = group.flat_p16.clone()
    for seed in range(3):
        opt.zero_grad()
        _loss(model, _batch(seed)).backward()
        opt.step()
        ops.fused_sgd(p, group.flat_g.clone(), m, 0.05, 0.9, 5e-4,
                      nesterov=True, p_bf16=p16)
    assert torch.equal(group.flat_p, p)
    assert torch.equal(opt._momentum_buffers[0], m)
    assert torch.equal(group.flat_p16, p16)


@requires_gpu
def test_noop_clipping_is_bitwise_gpu():
    a = _mlp()
    b = copy.deepcopy(a)
    batches = [_batch(seed) for seed in range(3)]
    opt_a = FusedSGD(a.parameters(), lr=0.05, momentum=0.9, max_grad_norm=1e9)
    opt_b = FusedSGD(b.parameters(), lr=0.05, momentum=0.9)
    _run_eager(a, opt_a, batches)
    _run_eager(b, opt_b, batches)
    from flashy_amd import ops
    assert opt_a._hyper[opt_a.groups[0].device][ops.HYPER_COEF].item() == 1.0
    assert opt_a.last_grad_norm.item() > 0
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
