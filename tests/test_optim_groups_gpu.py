# Copyright (c) Flashy-AMD authors.
"""GPU tests: the segmented optimizer kernels (per-tensor weight decay / lr
scale, LARS trust ratios) — the norm kernels against fp64, the update kernels
against the unsegmented ones on the same buffers (SGD bitwise, Adam to 1e-7),
and the optimizers, eager and captured
into a HIP graph, against torch param groups and the LARS composite of
test_optim_groups.py."""
import copy
import math

import pytest
import torch
from torch import nn

from flashy_amd.optim import LARS, FusedAdam, FusedSGD, WarmupCosine, \
    no_decay_1d
from tests.test_optim_groups import (EDGE_SHAPES, ZERO_GRAD, ZERO_WEIGHT,
                                     LarsComposite, edge_grads, edge_options,
                                     edge_params, make_ours,
                                     resolved_edge_options, run_torch_groups,
                                     set_grads, _mlp_options)
from tests.test_optim_sched_gpu import (MAX_NORM, _batch, _capture, _loss,
                                        _max_diff, _mlp)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

EDGE_SIZES = [math.prod(s) for s in EDGE_SHAPES]
# one tensor over more chunks than the grid has blocks (2048), so the chunk
# loop strides, plus an unaligned neighbour on each side
BIG_SIZES = [5, 2100 * 4096 + 3, 9]


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).contiguous()


def _edge_flat():
    return (_flat(edge_params("cuda")), _flat(edge_grads(0, "cuda")))


def _big_flat():
    g = torch.Generator(device="cuda").manual_seed(3)
    n = sum(BIG_SIZES)
    return (torch.randn(n, device="cuda", generator=g) * 0.1,
            torch.randn(n, device="cuda", generator=g) * 0.01)


def _table(sizes, wd=5e-4, lr_scale=1.0, lars=False):
    from flashy_amd import ops
    t = len(sizes)
    return ops.SegTable(sizes, [wd] * t, [lr_scale] * t, [lars] * t, "cuda")


# -- 1. the norm kernels ------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("case", ["edge", "big"])
def test_seg_sqsum_and_lars_prepare_vs_fp64(case):
    """rtol 1e-5: a sum of non-negative fp32 terms is off by at most
    (terms per running sum) * 2^-24 relative.  With CHUNK = 4096 and 256
    threads a thread's running sum sees at most 6 terms (one head element,
    four float4 lanes, one tail element); folding the four lanes adds 2
    steps, the wave 6 and the block 2: 16 * 2^-24 = 9.5e-7.  From the chunk
    partials on everything is fp64, and the ratio is rounded to fp32 once."""
    from flashy_amd import ops
    sizes = EDGE_SIZES if case == "edge" else BIG_SIZES
    p, g = _edge_flat() if case == "edge" else _big_flat()
    wds = [1e-3 * (i % 3) for i in range(len(sizes))]
    lars_on = [i != 1 for i in range(len(sizes))]
    table = ops.SegTable(sizes, wds, [1.0] * len(sizes), lars_on, "cuda")
    assert table.n_chunks <= -(-sum(sizes) // ops.SEG_CHUNK) + len(sizes) - 1
    if case == "big":
        assert table.n_chunks > 2048
    hyper = torch.zeros(ops.HYPER_SIZE, device="cuda")
    hyper[ops.HYPER_COEF] = 0.25
    eta, eps, grad_scale = 1e-2, 1e-8, 0.5
    out = []
    for _ in range(2):
        # no pre-zeroing needed: every slot is overwritten
        partials = torch.full((table.n_chunks, 2), float("nan"),
                              device="cuda")
        ratio = torch.full((len(sizes),), float("nan"), device="cuda")
        ops.seg_sqsum(p, g, table, partials)
        ops.lars_prepare(partials, table, ratio, eta, eps,
                         grad_scale=grad_scale, hyper=hyper)
        out.append((partials, ratio))
    partials, ratio = out[0]
    assert torch.isfinite(partials).all() and torch.isfinite(ratio).all()
    first = table.tensor_chunk.tolist()
    offset = 0
    for t, n in enumerate(sizes):
        sl = slice(offset, offset + n)
        offset += n
        want_p = p[sl].double().pow(2).sum().item()
        want_g = g[sl].double().pow(2).sum().item()
        got = partials[first[t]:first[t + 1]].double().sum(0).tolist()
        assert got == pytest.approx([want_p, want_g], rel=1e-5), t
        wn = math.sqrt(want_p)
        gn = grad_scale * 0.25 * math.sqrt(want_g)
        want = 1.0
        if lars_on[t] and wn > 0 and gn > 0:
            want = eta * wn / (gn + wds[t] * wn + eps)
        assert ratio[t].item() == pytest.approx(want, rel=1e-5), t
    if case == "edge":
        assert ratio[ZERO_WEIGHT].item() == 1.0
        assert ratio[ZERO_GRAD].item() == 1.0
    assert ratio[1].item() == 1.0          # LARS off for this tensor
    assert (ratio != 1.0).sum().item() >= 2
    # deterministic: bitwise identical on a second call
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    # without a hyper block the coefficient is 1
    ops.lars_prepare(partials, table, ratio, eta, eps)
    wn = p[:sizes[0]].double().norm().item()
    gn = g[:sizes[0]].double().norm().item()
    assert ratio[0].item() == pytest.approx(
        eta * wn / (gn + wds[0] * wn + eps), rel=1e-5)


# -- 2. the segmented update kernels, uniform options -------------------------

@requires_gpu
@pytest.mark.parametrize("case", ["edge", "big"])
@pytest.mark.parametrize("momentum", [True, False])
def test_fused_sgd_seg_uniform_is_bitwise(case, momentum):
    """Uniform options through the segmented kernel: sgd_one is shared with
    k_fused_sgd and every factor the chunk walk adds is exactly 1, so the
    results are expected to be bitwise equal."""
    from flashy_amd import ops
    sizes = EDGE_SIZES if case == "edge" else BIG_SIZES
    p, g = _edge_flat() if case == "edge" else _big_flat()
    table = _table(sizes)
    q = p.clone()
    m = torch.zeros_like(p) if momentum else None
    mq = torch.zeros_like(p) if momentum else None
    p16 = p.to(torch.bfloat16) if momentum else None
    q16 = q.to(torch.bfloat16) if momentum else None
    mu = 0.9 if momentum else 0.0
    for step in range(3):
        ops.fused_sgd(p, g, m, 0.05, mu, 5e-4, nesterov=momentum, p_bf16=p16)
        ops.fused_sgd_seg(q, g, mq, 0.05, mu, table, nesterov=momentum,
                          p_bf16=q16)
        g = g * 0.5 + 0.001
    assert torch.equal(p, q)
    if momentum:
        assert torch.equal(m, mq)
        assert torch.equal(p16, q16)
        assert torch.equal(q16, q.to(torch.bfloat16))


@requires_gpu
@pytest.mark.parametrize("case", ["edge", "big"])
@pytest.mark.parametrize("adamw", [True, False])
def test_fused_adam_seg_uniform_matches_unsegmented(case, adamw):
    """adam_one is shared with k_fused_adam and the per-tensor factors are
    exactly 1, but the compiler contracts the inlined body differently in the
    two kernels (measured on gfx950: not bitwise equal), so this asserts
    atol 1e-7 on p and m.  v is ~1e-8 here, where an absolute bound says
    nothing: it gets rtol 1e-6, a few fp32 ulps (6e-8 each) for the handful
    of differently fused operations over three steps, plus the absolute
    bound."""
    from flashy_amd import ops
    sizes = EDGE_SIZES if case == "edge" else BIG_SIZES
    p, g = _edge_flat() if case == "edge" else _big_flat()
    table = _table(sizes, wd=1e-2)
    q = p.clone()
    m, v, mq, vq = (torch.zeros_like(p) for _ in range(4))
    p16 = p.to(torch.bfloat16) if adamw else None
    q16 = q.to(torch.bfloat16) if adamw else None
    step_dev = torch.ones(1, dtype=torch.int64, device="cuda")
    for step in range(1, 4):
        ops.fused_adam(p, g, m, v, 1e-2, 0.9, 0.999, 1e-8, 1e-2, step,
                       adamw=adamw, p_bf16=p16, step_dev=step_dev)
        ops.fused_adam_seg(q, g, mq, vq, 1e-2, 0.9, 0.999, 1e-8, step, table,
                           adamw=adamw, p_bf16=q16, step_dev=step_dev)
        ops.adam_step_inc(step_dev)
        g = g * 0.5 + 0.001
    print("max |dp|, |dm|, rel |dv|:", (p - q).abs().max().item(),
          (m - mq).abs().max().item(),
          ((v - vq).abs() / v.abs().clamp_min(1e-30)).max().item())
    assert torch.allclose(p, q, atol=1e-7, rtol=0)
    assert torch.allclose(m, mq, atol=1e-7, rtol=0)
    assert torch.allclose(v, vq, atol=1e-7, rtol=1e-6)
    if adamw:
        # each mirror is the bf16 rounding of its own fp32 master
        assert torch.equal(p16, p.to(torch.bfloat16))
        assert torch.equal(q16, q.to(torch.bfloat16))


# -- 3. eager parity ----------------------------------------------------------

def _loss_k(model, x, k):
    del k
    return _loss(model, x)


@requires_gpu
@pytest.mark.parametrize("managed", [False, True], ids=["plain", "sched+clip"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_eager_per_tensor_options_match_torch_param_groups(kind, managed):
    model = _mlp()
    ref = copy.deepcopy(model)
    batches = [_batch(seed) for seed in range(5)]
    kw = {}
    if managed:
        kw = dict(schedule=WarmupCosine(2, 5), max_grad_norm=MAX_NORM)
    opt = make_ours(kind, model.parameters(), bf16_mirror=True,
                    param_options=_mlp_options(model), **kw)
    assert opt.groups[0].seg is not None
    for x in batches:
        opt.zero_grad()
        _loss(model, x).backward()
        opt.step()
    run_torch_groups(ref, kind, batches, kw.get("schedule"),
                     kw.get("max_grad_norm"), loss=_loss_k)
    atol = 1e-5 if kind == "sgd" else 1e-4
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.allclose(p, q, atol=atol), (p - q).abs().max().item()
        assert torch.equal(p._bf16_mirror, p.detach().to(torch.bfloat16))


@requires_gpu
@pytest.mark.parametrize("clip", [None, MAX_NORM], ids=["noclip", "clip"])
@pytest.mark.parametrize("momentum,nesterov",
                         [(0.0, False), (0.9, False), (0.9, True)])
def test_eager_lars_matches_composite(momentum, nesterov, clip):
    params = edge_params("cuda")
    ref = LarsComposite(params, resolved_edge_options(5e-4, True), lr=0.5,
                        momentum=momentum, nesterov=nesterov, eta=1e-2,
                        max_norm=clip)
    opt = FusedSGD(params, lr=0.5, momentum=momentum, weight_decay=5e-4,
                   nesterov=nesterov, max_grad_norm=clip, bf16_mirror=True,
                   param_options=edge_options, lars=LARS(eta=1e-2))
    for step in range(4):
        grads = edge_grads(step, "cuda")
        set_grads(params, grads)
        opt.step()
        ref.step(grads)
        (ratios,) = opt.last_trust_ratios
        assert ratios.is_cuda
        assert ratios.tolist() == pytest.approx(ref.ratios, rel=1e-4)
        if step == 0:
            assert ratios[ZERO_WEIGHT].item() == 1.0
        assert ratios[ZERO_GRAD].item() == 1.0
    for p, q in zip(params, ref.p):
        assert torch.allclose(p, q, atol=1e-5), (p - q).abs().max().item()
        assert torch.equal(p._bf16_mirror, p.detach().to(torch.bfloat16))


# -- 4. captured --------------------------------------------------------------

LARS_LR, LARS_ETA = 0.1, 0.02


def _composite_on(model, **kw):
    """A LarsComposite that updates `model`'s parameters in place."""
    comp = LarsComposite(
        list(model.parameters()),
        [(0.0, 1.0, False) if p.ndim <= 1 else (5e-4, 1.0, True)
         for p in model.parameters()], **kw)
    for p, q in zip(model.parameters(), comp.p):
        p.data = q
    return comp


@requires_gpu
def test_captured_lars_follows_ratios_schedule_and_clip():
    """The trust ratios are recomputed on the device at every replay: with a
    ratio frozen at capture, or ignored, the run lands elsewhere."""
    sched = WarmupCosine(3, 10)
    model = _mlp()
    ref = copy.deepcopy(model)
    no_lars = copy.deepcopy(model)
    x = _batch()
    opt = FusedSGD(model.parameters(), lr=LARS_LR, momentum=0.9,
                   weight_decay=5e-4, schedule=sched, max_grad_norm=MAX_NORM,
                   param_options=no_decay_1d, lars=LARS(eta=LARS_ETA))
    graphed = _capture(model, opt, x)
    for _ in range(10):
        graphed()
    torch.cuda.synchronize()
    comp = _composite_on(ref, lr=LARS_LR, momentum=0.9, eta=LARS_ETA,
                         max_norm=MAX_NORM, schedule=sched)
    first = None
    for _ in range(10):
        ref.zero_grad()
        _loss(ref, x).backward()
        comp.step([p.grad for p in ref.parameters()])
        first = first or list(comp.ratios)
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.allclose(p, q, atol=1e-5), (p - q).abs().max().item()
    (ratios,) = opt.last_trust_ratios
    assert ratios.is_cuda
    assert ratios.tolist() == pytest.approx(comp.ratios, rel=1e-4)
    # the ratios really moved between the first and the last replay
    assert max(abs(a - b) / a for a, b in zip(first, comp.ratios)) > 1e-2
    assert opt.current_lr() == sched.lr_at(10, LARS_LR)
    # same run with LARS off lands elsewhere
    opt2 = FusedSGD(no_lars.parameters(), lr=LARS_LR, momentum=0.9,
                    weight_decay=5e-4, schedule=sched, max_grad_norm=MAX_NORM,
                    param_options=no_decay_1d)
    for _ in range(10):
        opt2.zero_grad()
        _loss(no_lars, x).backward()
        opt2.step()
    assert _max_diff(model, no_lars) > 100 * 1e-5


# -- 5. defaults --------------------------------------------------------------

@requires_gpu
def test_defaults_allocate_no_chunk_table_and_are_bitwise():
    """No new keyword: no chunk table, and the step is the plain kernel call
    with the arguments the optimizer has always passed."""
    from flashy_amd import ops
    model = _mlp()
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9,
                   weight_decay=5e-4, nesterov=True, bf16_mirror=True)
    group = opt.groups[0]
    assert not opt._segmented and opt.last_trust_ratios is None
    assert group.seg is None and group.seg_partials is None
    assert group.ratio is None
    adam = FusedAdam(_mlp().parameters(), lr=1e-3)
    assert not adam._segmented and adam.groups[0].seg is None
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
