# Copyright (c) Flashy-AMD authors.
"""FusedLAMB, CPU path, against a float64 composite of the documented formula
(test_optim_lamb_gpu.py holds the kernels to the same composite)."""
import copy

import pytest
import torch

from flashy_amd.optim import FusedAdam, FusedLAMB, WarmupCosine, no_decay_1d
from tests.test_optim_groups import (EDGE_SHAPES, ZERO_GRAD, ZERO_WEIGHT,
                                     edge_grads, edge_params, set_grads)
from tests.test_optim_sched import MAX_NORM, _ref_factor

LR, WD, EPS = 0.02, 0.05, 1e-6


class LambComposite:
    """The formula of FusedLAMB's docstring in float64, tensor by tensor;
    `options` holds (wd, lr_scale, trust) per tensor.  After a step: `ratios`,
    `steps` (lr * lr_scale * ratio) and `adam` (the Adam term of u).  float64
    parameters are updated in place, others copied."""

    def __init__(self, params, options, lr, betas=(0.9, 0.999), eps=EPS,
                 trust_clip=False, max_norm=None, schedule=None, k=0):
        self.p = [p.detach().double() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.options, self.lr, self.betas, self.eps = options, lr, betas, eps
        self.trust_clip, self.max_norm = trust_clip, max_norm
        self.schedule, self.k = schedule, k

    def step(self, grads, coef=1.0):
        grads = [g.double() for g in grads]
        if self.max_norm is not None:
            total = sum(g.pow(2).sum().item() for g in grads) ** 0.5
            coef = min(1.0, self.max_norm / (total + 1e-6))
        lr = self.lr * (_ref_factor(self.schedule, self.k)
                        if self.schedule is not None else 1.0)
        self.k += 1
        (b1, b2), k = self.betas, self.k
        self.ratios, self.steps, self.adam = [], [], []
        for p, m, v, g, (wd, lr_scale, trust) in zip(
                self.p, self.m, self.v, grads, self.options):
            m.mul_(b1).add_((1 - b1) * coef * g)
            v.mul_(b2).add_((1 - b2) * (coef * g) ** 2)
            a = (m / (1 - b1 ** k)) / ((v / (1 - b2 ** k)).sqrt() + self.eps)
            u = a + wd * p
            wn, un = p.norm().item(), u.norm().item()
            r = wn / un if trust and wn > 0 and un > 0 else 1.0
            r = min(r, 1.0) if self.trust_clip else r
            self.ratios.append(r)
            self.steps.append(lr * lr_scale * r)
            self.adam.append(a)
            p.sub_(lr * lr_scale * r * u)


CASES = [(t, c, d, None) for t in (False, True) for c in (None, MAX_NORM)
         for d in (False, True)] + [(False, MAX_NORM, True, WarmupCosine(2, 6))]


def check_edge(device, trust_clip, clip, decay_1d, sched, rel, atol):
    """FusedLAMB against the composite on the edge tensors, and a state
    round-trip after 2 steps: the next step must be identical."""
    kw = dict(lr=LR, weight_decay=WD, eps=EPS, trust_clip=trust_clip,
              max_grad_norm=clip, schedule=sched, bf16_mirror=device != "cpu")
    params, steps = edge_params(device), 3 if sched is None else 5
    options = [(0.0, 1.0, False) if decay_1d and len(s) == 1
               else (WD, 1.0, True) for s in EDGE_SHAPES]
    ref = LambComposite(params, options, LR, trust_clip=trust_clip,
                        max_norm=clip, schedule=sched)
    opt = FusedLAMB(params, param_options=no_decay_1d if decay_1d else None,
                    **kw)
    for step in range(steps):
        grads = edge_grads(step, device)
        if step == 2:   # built WITHOUT the options: the state restores them
            fresh = [torch.nn.Parameter(p.detach().clone()) for p in params]
            opt2 = FusedLAMB(fresh, **kw)
            opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
            set_grads(fresh, grads)
            opt2.step()
        set_grads(params, grads)
        opt.step()
        ref.step(grads)
        if step == 2:
            assert all(torch.equal(p, q) for p, q in zip(params, fresh))
            assert torch.equal(opt.last_trust_ratios[0],
                               opt2.last_trust_ratios[0])
        (ratios,) = opt.last_trust_ratios
        assert ratios.device.type == device
        assert ratios.tolist() == pytest.approx(ref.ratios, rel=rel)
        assert all(trust or r == 1.0 for r, (_, _, trust)
                   in zip(ratios.tolist(), ref.options))
        # the zero gradient leaves m = 0, so u = wd * p
        want = 1.0 if decay_1d else min(1 / WD, 1.0) if trust_clip else 1 / WD
        assert ratios[ZERO_GRAD].item() == pytest.approx(want, rel=1e-5)
        assert step > 0 or ratios[ZERO_WEIGHT].item() == 1.0  # then it moves
        assert min(ref.ratios) < 1.0
    worst = max((p.double() - q).abs().max().item()
                for p, q in zip(params, ref.p))
    print("max |p - p_ref|:", worst)
    assert worst <= atol
    assert opt.current_lr() == opt._sched.lr_at(steps, LR)
    return params


@pytest.mark.parametrize("trust_clip,clip,decay_1d,sched", CASES)
def test_lamb_matches_composite(trust_clip, clip, decay_1d, sched):
    """atol 1e-6: p is ~0.1 and takes up to five fp32 steps of ~lr * r * |u|,
    each a dozen roundings at 2^-24 relative."""
    check_edge("cpu", trust_clip, clip, decay_1d, sched, 1e-5, 1e-6)


def test_lamb_without_trust_is_adam():
    """Trust off everywhere and no weight decay: u is Adam's update.  The two
    CPU paths round it in a different order: at most an ulp of p (3e-8 below
    0.5) in each of three steps."""
    ours, adam = edge_params(), edge_params()
    opt = FusedLAMB(ours, lr=LR, eps=1e-8,
                    param_options=lambda p: {"lars": False})
    ref = FusedAdam(adam, lr=LR, eps=1e-8)
    for step in range(3):
        for o, ps in ((opt, ours), (ref, adam)):
            set_grads(ps, edge_grads(step))
            o.step()
    assert (opt.last_trust_ratios[0] == 1.0).all()
    assert sorted(opt.state_dict()["extra"]) == ["exp_avg", "exp_avg_sq"]
    for p, q in zip(ours, adam):
        assert torch.allclose(p, q, atol=1e-7, rtol=0)
