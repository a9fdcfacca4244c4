# Copyright (c) Flashy-AMD authors.
"""GPU tests: the LAMB kernel chain and FusedLAMB, eager and captured into a
HIP graph, against the float64 composite of test_optim_lamb.py."""
import copy

import pytest
import torch

from flashy_amd.optim import FusedLAMB, WarmupCosine, no_decay_1d
from tests.test_optim_groups import ZERO_WEIGHT
from tests.test_optim_groups_gpu import (BIG_SIZES, EDGE_SIZES, _big_flat,
                                         _edge_flat)
from tests.test_optim_lamb import EPS, LR, WD, LambComposite, check_edge
from tests.test_optim_sched_gpu import MAX_NORM, _batch, _capture, _loss, _mlp

no_gpu = not torch.cuda.is_available()
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(no_gpu, reason="no GPU")]

# the kernels take fp32 betas; the composite is handed the same two numbers
BETAS = torch.tensor([0.9, 0.999], dtype=torch.float32).tolist()
STEP, COEF, GRAD_SCALE = 7, 0.25, 0.5


def _within(name, got, want, tol):
    # an exact zero (a zero-gradient tensor's m of g's sign) has tolerance 0
    worst = ((got.double() - want).abs() / tol.clamp_min(1e-300)).max().item()
    print(f"{name}: worst error / tolerance = {worst:.3g}")
    assert worst <= 1.0, name


@pytest.mark.parametrize("m_sign", ["of_g", "random"])
@pytest.mark.parametrize("case", ["edge", "big"])
def test_lamb_kernel_chain_vs_fp64(case, m_sign):
    """One step from random state at step 7 (bc1 = 0.52, bc2 = 0.007).
    m, v: 1e-6, a handful of fp32 roundings, of b1 |m| + (1 - b1) |g'|: with
    m of g's sign the two terms do not cancel and that is rtol 1e-6 on the
    new m; with a random sign it is the same bound where they do.
    Sums of the partials: rtol 1e-5, k_seg_sqsum's tree (16 * 2^-24, see
    test_seg_sqsum_and_lars_prepare_vs_fp64) plus the error of u^2.  ratio:
    rtol 1e-5.  p: 2^-23 |p_ref| for the final rounding plus 2e-5 of the
    un-cancelled step lr * s * r * (|a| + wd |p|)."""
    from flashy_amd import ops
    sizes = EDGE_SIZES if case == "edge" else BIG_SIZES
    p, g = _edge_flat() if case == "edge" else _big_flat()
    gen = torch.Generator(device="cuda").manual_seed(5)
    m = torch.randn(p.shape, device="cuda", generator=gen) * 0.01
    m = m.abs() * g.sign() if m_sign == "of_g" else m
    v = (torch.rand(p.shape, device="cuda", generator=gen) + 0.1) * 1e-4
    options = [(1e-2 * (i % 3), (1.0, 0.5, 2.0)[i % 3], i != 1)
               for i in range(len(sizes))]      # trust off on tensor 1
    table = ops.SegTable(sizes, *zip(*options), "cuda")
    assert case == "edge" or table.n_chunks > 2048   # the chunk loop strides
    hyper = torch.tensor([LR, COEF, 0.0, 0.0], device="cuda")   # lr, coef
    step_dev = torch.full((1,), STEP, dtype=torch.int64, device="cuda")
    ref = LambComposite(p.split(sizes), options, LR, betas=BETAS, k=STEP - 1)
    ref.m, ref.v = ([t.double() for t in s.split(sizes)] for s in (m, v))
    old_p = [t.clone() for t in ref.p]
    ref.step(g.split(sizes), coef=COEF * GRAD_SCALE)
    out = []
    for _ in range(2):
        partials = torch.full((table.n_chunks, 2), float("nan"),
                              device="cuda")
        ratio = torch.full((len(sizes),), float("nan"), device="cuda")
        q, g1, m1, v1 = p.clone(), g.clone(), m.clone(), v.clone()
        q16 = torch.zeros_like(q, dtype=torch.bfloat16)
        ops.lamb_moments(q, g1, m1, v1, *BETAS, EPS, 0, table, partials,
                         grad_scale=GRAD_SCALE, step_dev=step_dev,
                         hyper=hyper)
        ops.lamb_ratio(partials, table, ratio)
        assert torch.equal(q, p)                # pass 1 only reads p
        ops.lamb_apply(q, m1, v1, 0.0, *BETAS, EPS, 0, table, ratio,
                       p_bf16=q16, step_dev=step_dev, hyper=hyper)
        assert torch.equal(g1, g)               # nobody writes g
        out.append((partials, ratio, q))
    for a, b in zip(*out):                      # bitwise repeatable
        assert torch.equal(a, b)
    assert torch.equal(q16, q.to(torch.bfloat16))
    want_m, want_v = torch.cat(ref.m), torch.cat(ref.v)
    _within("m", m1, want_m, 1e-6 * (BETAS[0] * m.double().abs() + (
        1 - BETAS[0]) * COEF * GRAD_SCALE * g.double().abs()))
    _within("v", v1, want_v, 1e-6 * want_v.abs())
    first = table.tensor_chunk.tolist()
    sums = torch.stack([partials[first[t]:first[t + 1]].double().sum(0)
                        for t in range(len(sizes))])
    want = torch.stack([torch.stack([w.pow(2).sum(), (a + wd * w).pow(2).sum()])
                        for w, a, (wd, _, _) in zip(old_p, ref.adam, options)])
    _within("partial sums", sums, want, 1e-5 * want)
    want = torch.tensor(ref.ratios, device="cuda", dtype=torch.float64)
    _within("ratio", ratio, want, 1e-5 * want)
    assert ratio[1].item() == 1.0 and (ratio != 1.0).sum().item() >= 2
    assert case == "big" or ratio[ZERO_WEIGHT].item() == 1.0
    assert (q != p).sum().item() > 0.99 * p.numel()
    want_p = torch.cat(ref.p)
    tol = torch.cat([2e-5 * s * (a.abs() + wd * w.abs()) for s, a, w, (wd, _, _)
                     in zip(ref.steps, ref.adam, old_p, options)])
    _within("p", q, want_p, 2.0 ** -23 * want_p.abs() + tol)


@pytest.mark.parametrize("clip", [None, MAX_NORM], ids=["noclip", "clip"])
@pytest.mark.parametrize("trust_clip", [False, True])
def test_eager_lamb_matches_composite(trust_clip, clip):
    """The tolerances of test_eager_lars_matches_composite (ratios 1e-4, p
    1e-5).  HAS_BF16: the mirror must be the rounding of p, bitwise."""
    for p in check_edge("cuda", trust_clip, clip, False, None, 1e-4, 1e-5):
        assert torch.equal(p._bf16_mirror, p.detach().to(torch.bfloat16))


def test_captured_lamb_follows_ratios_schedule_and_clip():
    """Captured once, replayed on fresh batches: LR, bias corrections and
    trust ratios are read on the device at every replay.  The reference is
    the composite updating a float64 copy of the model in place."""
    sched = WarmupCosine(2, 6)
    model = _mlp()
    ref = copy.deepcopy(model).double()
    x = _batch(0)
    opt = FusedLAMB(model.parameters(), lr=LR, weight_decay=WD,
                    schedule=sched, max_grad_norm=MAX_NORM,
                    param_options=no_decay_1d)
    graphed = _capture(model, opt, x)
    comp = LambComposite(
        list(ref.parameters()),
        [(0.0, 1.0, False) if p.ndim <= 1 else (WD, 1.0, True)
         for p in ref.parameters()], LR, max_norm=MAX_NORM, schedule=sched)
    seen = []
    for seed in range(1, 5):
        x.copy_(_batch(seed))
        graphed()
        ref.zero_grad()
        _loss(ref, x.double()).backward()
        comp.step([p.grad for p in ref.parameters()])
        seen.append(opt.last_trust_ratios[0].tolist())
        assert seen[-1] == pytest.approx(comp.ratios, rel=1e-4)
        assert seen[-1][1] == 1.0 and seen[-1][0] != 1.0
    assert all(a != b for a, b in zip(seen, seen[1:]))
    worst = max((p.double() - q).abs().max().item()
                for p, q in zip(model.parameters(), ref.parameters()))
    print("max |p - p_ref|:", worst)
    assert worst <= 1e-5
    assert opt.current_lr() == sched.lr_at(4, LR)
