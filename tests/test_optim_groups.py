# Copyright (c) Flashy-AMD authors.
"""Per-tensor weight decay / lr scale and LARS on the flat optimizers, CPU
path.  Oracles: torch.optim with the equivalent param groups, and for LARS an
independent per-tensor composite of the documented formula with fp64 norms.
The GPU kernels are held to the same oracles in test_optim_groups_gpu.py,
which imports the shared pieces from here."""
import copy
import math

import pytest
import torch
from torch import nn
from torch.optim import lr_scheduler as tls

from flashy_amd import ops
from flashy_amd.optim import (LARS, FusedAdam, FusedSGD, WarmupCosine,
                              no_decay_1d)
from tests.test_optim_sched import (BASE_LR, MAX_NORM, _assert_params_close,
                                    _assert_params_equal, _batches, _loss,
                                    _mlp, _ref_factor, _run_ours)

# -- the shared tiny parameter set -------------------------------------------
# Every chunk edge case in 20582 elements (CHUNK = 4096): unaligned offsets
# and tensors smaller than a float4; (4096,) at offset 39 crosses one window
# edge; (3, 4099) at offset 8228 spans four windows; (10,) leaves the running
# total off a multiple of 4, and so does the grand total (20582 = 2 mod 4).
EDGE_SHAPES = [(1,), (3,), (5, 7), (4096,), (4093,), (3, 4099), (10,),
               (6, 5), (17,)]
ZERO_WEIGHT, ZERO_GRAD = 7, 8     # indices into EDGE_SHAPES
EDGE_TOTAL = 20582


def edge_params(device="cpu"):
    g = torch.Generator().manual_seed(11)
    params = []
    for i, shape in enumerate(EDGE_SHAPES):
        t = torch.randn(shape, generator=g) * 0.1
        if i == ZERO_WEIGHT:
            t.zero_()
        params.append(nn.Parameter(t.to(device)))
    return params


def edge_grads(step, device="cpu"):
    """One gradient per edge tensor for `step`; ZERO_GRAD's is all zero.
    Their global norm is ~1.4, so MAX_NORM = 0.05 really clips."""
    g = torch.Generator().manual_seed(100 + step)
    grads = [torch.randn(shape, generator=g) * 0.01 for shape in EDGE_SHAPES]
    grads[ZERO_GRAD].zero_()
    return [t.to(device) for t in grads]


def edge_options(p):
    """no_decay_1d, plus a per-tensor lr_scale and weight decay on two of the
    2-d tensors, so every option takes more than one value."""
    if tuple(p.shape) == (5, 7):
        return {"lr_scale": 0.5}
    if tuple(p.shape) == (3, 4099):
        return {"weight_decay": 1e-3, "lr_scale": 2.0}
    return no_decay_1d(p)


def resolved_edge_options(weight_decay, lars):
    """(weight_decay, lr_scale, lars) per edge tensor, spelled out by hand."""
    out = []
    for shape in EDGE_SHAPES:
        if len(shape) == 1:
            out.append((0.0, 1.0, False))
        elif shape == (5, 7):
            out.append((weight_decay, 0.5, lars))
        elif shape == (3, 4099):
            out.append((1e-3, 2.0, lars))
        else:
            out.append((weight_decay, 1.0, lars))
    return out


class LarsComposite:
    """The documented formula, tensor by tensor, with fp64 norms:

        g' = clip_coef * g
        ratio = eta * |p| / (|g'| + wd * |p| + eps) if |p| > 0 and |g'| > 0
                else 1
        d = ratio * (g' + wd * p)
        m = mu * m + d ; d = nesterov ? d + mu * m : m
        p -= lr * lr_scale * d
    """

    def __init__(self, params, options, lr, momentum=0.0, nesterov=False,
                 eta=1e-3, eps=1e-8, max_norm=None, schedule=None):
        self.p = [p.detach().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.options = options
        self.lr, self.mu, self.nesterov = lr, momentum, nesterov
        self.eta, self.eps, self.max_norm = eta, eps, max_norm
        self.schedule = schedule
        self.k = 0
        self.ratios = []

    def step(self, grads):
        coef = 1.0
        if self.max_norm is not None:
            total = math.sqrt(sum(g.double().pow(2).sum().item()
                                  for g in grads))
            coef = min(1.0, self.max_norm / (total + 1e-6))
        lr = self.lr
        if self.schedule is not None:
            lr = self.lr * _ref_factor(self.schedule, self.k)
        self.ratios = []
        for p, m, g, (wd, lr_scale, lars) in zip(self.p, self.m, grads,
                                                 self.options):
            g = g * coef
            ratio = 1.0
            if lars:
                wn = p.double().norm().item()
                gn = g.double().norm().item()
                if wn > 0 and gn > 0:
                    ratio = self.eta * wn / (gn + wd * wn + self.eps)
            self.ratios.append(ratio)
            d = ratio * (g + wd * p)
            if self.mu != 0:
                m.mul_(self.mu).add_(d)
                d = d + self.mu * m if self.nesterov else m
            p.sub_(lr * lr_scale * d)
        self.k += 1


def set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad.copy_(g)     # a view into the flat gradient buffer


# -- 1. per-tensor weight decay / lr against torch param groups ---------------

def _mlp_options(model):
    """no_decay_1d, and half the lr on the last layer."""
    last = {id(p) for p in model[2].parameters()}

    def options(p):
        out = dict(no_decay_1d(p))
        if id(p) in last:
            out["lr_scale"] = 0.5
        return out
    return options


def _torch_groups(model, lr, weight_decay):
    return [
        {"params": [model[0].weight], "weight_decay": weight_decay, "lr": lr},
        {"params": [model[0].bias], "weight_decay": 0.0, "lr": lr},
        {"params": [model[2].weight], "weight_decay": weight_decay,
         "lr": 0.5 * lr},
        {"params": [model[2].bias], "weight_decay": 0.0, "lr": 0.5 * lr},
    ]


def run_torch_groups(ref, kind, batches, sched=None, max_norm=None,
                     loss=_loss):
    if kind == "sgd":
        opt = torch.optim.SGD(_torch_groups(ref, BASE_LR, 5e-4), lr=BASE_LR,
                              momentum=0.9, nesterov=True)
    else:
        opt = torch.optim.AdamW(_torch_groups(ref, 1e-2, 1e-2), lr=1e-2)
    scheduler = None
    if sched is not None:
        scheduler = tls.LambdaLR(opt, lambda k: _ref_factor(sched, k))
    for k, x in enumerate(batches):
        opt.zero_grad()
        loss(ref, x, k).backward()
        if max_norm is not None:
            nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
        opt.step()
        if scheduler is not None:
            scheduler.step()


def make_ours(kind, params, **kw):
    if kind == "sgd":
        return FusedSGD(params, lr=BASE_LR, momentum=0.9, weight_decay=5e-4,
                        nesterov=True, **kw)
    return FusedAdam(params, lr=1e-2, weight_decay=1e-2, adamw=True, **kw)


@pytest.mark.parametrize("managed", [False, True], ids=["plain", "sched+clip"])
@pytest.mark.parametrize("form", ["param_options", "groups"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_per_tensor_options_match_torch_param_groups(kind, form, managed):
    ours = _mlp()
    ref = copy.deepcopy(ours)
    batches = _batches(5)
    kw = {}
    if managed:
        kw = dict(schedule=WarmupCosine(2, 5), max_grad_norm=MAX_NORM)
    if form == "param_options":
        opt = make_ours(kind, ours.parameters(),
                        param_options=_mlp_options(ours), **kw)
    else:
        lr, wd = (BASE_LR, 5e-4) if kind == "sgd" else (1e-2, 1e-2)
        opt = make_ours(kind, _torch_groups(ours, lr, wd), **kw)
    assert opt._segmented
    _run_ours(ours, opt, batches)
    run_torch_groups(ref, kind, batches, kw.get("schedule"),
                     kw.get("max_grad_norm"))
    _assert_params_close(ours, ref, atol=1e-5 if kind == "sgd" else 1e-4)
    # the exemption must matter at this tolerance, or the test shows nothing
    uniform = _mlp()
    _run_ours(uniform, make_ours(kind, uniform.parameters(), **kw), batches)
    diff = max((p - q).abs().max().item()
               for p, q in zip(ours.parameters(), uniform.parameters()))
    assert diff > 1e-3


# -- 2. LARS against the composite --------------------------------------------

@pytest.mark.parametrize("clip", [None, MAX_NORM], ids=["noclip", "clip"])
@pytest.mark.parametrize("momentum,nesterov",
                         [(0.0, False), (0.9, False), (0.9, True)])
def test_lars_matches_composite(momentum, nesterov, clip):
    params = edge_params()
    ref = LarsComposite(params, resolved_edge_options(5e-4, True), lr=0.5,
                        momentum=momentum, nesterov=nesterov, eta=1e-2,
                        max_norm=clip)
    opt = FusedSGD(params, lr=0.5, momentum=momentum, weight_decay=5e-4,
                   nesterov=nesterov, max_grad_norm=clip,
                   param_options=edge_options, lars=LARS(eta=1e-2))
    seen = []
    for step in range(4):
        grads = edge_grads(step)
        set_grads(params, grads)
        opt.step()
        ref.step(grads)
        seen.append(ref.ratios)
        (ratios,) = opt.last_trust_ratios
        assert ratios.tolist() == pytest.approx(ref.ratios, rel=1e-5)
    for p, q in zip(params, ref.p):
        assert torch.allclose(p, q, atol=1e-5), (p - q).abs().max().item()
    # zero weight (first step only: it moves afterwards), zero gradient and
    # the 1-d tensors have ratio exactly 1; the others do not
    assert seen[0][ZERO_WEIGHT] == 1.0 and seen[1][ZERO_WEIGHT] != 1.0
    for ratios in seen:
        assert ratios[ZERO_GRAD] == 1.0
        assert all(r == 1.0 for r, s in zip(ratios, EDGE_SHAPES)
                   if len(s) == 1)
        assert ratios[2] != 1.0 and ratios[5] != 1.0
    # LARS must matter at this tolerance
    plain = edge_params()
    opt2 = FusedSGD(plain, lr=0.5, momentum=momentum, weight_decay=5e-4,
                    nesterov=nesterov, max_grad_norm=clip,
                    param_options=edge_options)
    assert opt2.last_trust_ratios is None
    for step in range(4):
        set_grads(plain, edge_grads(step))
        opt2.step()
    assert max((p - q).abs().max().item()
               for p, q in zip(params, plain)) > 100 * 1e-5


def test_lars_with_schedule_matches_composite():
    sched = WarmupCosine(2, 6)
    params = edge_params()
    ref = LarsComposite(params, resolved_edge_options(5e-4, True), lr=0.5,
                        momentum=0.9, eta=1e-2, max_norm=MAX_NORM,
                        schedule=sched)
    opt = FusedSGD(params, lr=0.5, momentum=0.9, weight_decay=5e-4,
                   schedule=sched, max_grad_norm=MAX_NORM,
                   param_options=edge_options, lars=LARS(eta=1e-2))
    for step in range(5):
        grads = edge_grads(step)
        set_grads(params, grads)
        opt.step()
        ref.step(grads)
    for p, q in zip(params, ref.p):
        assert torch.allclose(p, q, atol=1e-5), (p - q).abs().max().item()


# -- 3. layout ----------------------------------------------------------------

def test_chunk_table_rule():
    sizes = [math.prod(s) for s in EDGE_SHAPES]
    chunks = ops.seg_chunks(sizes)
    assert sum(sizes) == EDGE_TOTAL and EDGE_TOTAL % 4 == 2
    assert len(chunks) <= -(-EDGE_TOTAL // ops.SEG_CHUNK) + len(sizes) - 1
    offsets = [sum(sizes[:t]) for t in range(len(sizes) + 1)]
    pos = 0
    for start, length, tensor in chunks:
        assert start == pos and 0 < length <= ops.SEG_CHUNK
        # inside one tensor and inside one window
        assert offsets[tensor] <= start
        assert start + length <= offsets[tensor + 1]
        assert start // ops.SEG_CHUNK == (start + length - 1) // ops.SEG_CHUNK
        # an edge inside a tensor is a multiple of 4
        if start != offsets[tensor]:
            assert start % 4 == 0
        pos += length
    assert pos == EDGE_TOTAL
    windows = {}
    for start, _, tensor in chunks:
        windows.setdefault(tensor, set()).add(start // ops.SEG_CHUNK)
    assert len(windows[3]) == 2 and len(windows[5]) == 4
    assert ops.seg_chunks([0, 5, 0]) == [(0, 5, 1)]


def test_layout_is_unchanged_by_options():
    a, b = _mlp(), _mlp()
    opt_a = FusedSGD(a.parameters(), lr=BASE_LR, momentum=0.9)
    opt_b = FusedSGD(b.parameters(), lr=BASE_LR, momentum=0.9,
                     param_options=no_decay_1d, lars=LARS())
    assert not opt_a._segmented and opt_b._segmented
    assert torch.equal(opt_a.param_buffers[0], opt_b.param_buffers[0])
    for p, q in zip(a.parameters(), b.parameters()):
        assert p.data_ptr() - opt_a.param_buffers[0].data_ptr() == \
            q.data_ptr() - opt_b.param_buffers[0].data_ptr()
        assert p.grad.data_ptr() - opt_a.grad_buffers[0].data_ptr() == \
            q.grad.data_ptr() - opt_b.grad_buffers[0].data_ptr()
    # momentum saved without options loads into an optimizer with options
    _run_ours(a, opt_a, _batches(2))
    state = copy.deepcopy(opt_a.state_dict())
    opt_b.load_state_dict(state)
    assert torch.equal(opt_b._momentum_buffers[0], opt_a._momentum_buffers[0])
    assert opt_b.step_count == 2


def test_param_groups_pack_in_order_of_appearance():
    model = _mlp()
    w0, b0, w1, b1 = model.parameters()
    want = torch.cat([t.detach().reshape(-1) for t in (b0, b1, w1, w0)])
    opt = FusedSGD([{"params": [b0, b1], "weight_decay": 0.0},
                    {"params": w1, "lr": 0.5 * BASE_LR},
                    {"params": [w0]}], lr=BASE_LR, weight_decay=5e-4)
    assert torch.equal(opt.param_buffers[0], want)
    assert opt._resolved(opt.groups[0]) == [
        (0.0, 1.0, False), (0.0, 1.0, False), (5e-4, 0.5, False),
        (5e-4, 1.0, False)]
    assert b1.data_ptr() == opt.param_buffers[0].data_ptr() + 4 * b0.numel()


def test_uniform_options_stay_on_the_unsegmented_path():
    model = _mlp()
    opt = FusedSGD(model.parameters(), lr=BASE_LR, weight_decay=5e-4,
                   param_options=lambda p: {"weight_decay": 5e-4,
                                            "lr_scale": 1.0})
    assert not opt._segmented and opt.groups[0].seg is None
    assert opt.last_trust_ratios is None
    # a mapping works like the callable
    model = _mlp()
    opt = FusedSGD(model.parameters(), lr=BASE_LR, weight_decay=5e-4,
                   param_options={model[0].bias: {"weight_decay": 0.0}})
    assert opt._segmented
    assert [r[0] for r in opt._resolved(opt.groups[0])] == [
        5e-4, 0.0, 5e-4, 5e-4]


# -- 4. errors ----------------------------------------------------------------

def test_validation_errors():
    model = _mlp()
    with pytest.raises(ValueError, match="unknown param option"):
        FusedSGD(model.parameters(), lr=0.1,
                 param_options=lambda p: {"weight_decoy": 0.0})
    with pytest.raises(ValueError, match="unknown param group key"):
        FusedSGD([{"params": list(model.parameters()), "momentum": 0.5}],
                 lr=0.1)
    with pytest.raises(ValueError, match="more than one parameter group"):
        FusedSGD([{"params": list(model.parameters())},
                  {"params": [model[0].bias]}], lr=0.1)
    with pytest.raises(ValueError, match="not both"):
        FusedSGD([{"params": list(model.parameters())}], lr=0.1,
                 param_options=no_decay_1d)
    with pytest.raises(ValueError, match="needs lars=LARS"):
        FusedSGD(model.parameters(), lr=0.1,
                 param_options=lambda p: {"lars": True})
    with pytest.raises(TypeError):
        FusedSGD(model.parameters(), lr=0.1, lars=True)
    with pytest.raises(ValueError):
        LARS(eta=0.0)
    with pytest.raises(NotImplementedError):
        FusedAdam(model.parameters(), lr=0.1, lars=LARS())
    with pytest.raises(NotImplementedError):
        FusedAdam(model.parameters(), lr=0.1,
                  param_options=lambda p: {"lars": True})
    with pytest.raises(NotImplementedError):
        FusedAdam([{"params": list(model.parameters()), "lars": True}], lr=0.1)
    assert no_decay_1d(model[0].bias) == {"weight_decay": 0.0, "lars": False}
    assert no_decay_1d(model[0].weight) == {}


# -- 5. state -----------------------------------------------------------------

def _lars_opt(model, **kw):
    return FusedSGD(model.parameters(), lr=BASE_LR, momentum=0.9,
                    weight_decay=5e-4, schedule=WarmupCosine(2, 8),
                    max_grad_norm=MAX_NORM, lars=LARS(eta=1e-2), **kw)


@pytest.mark.parametrize("kind", ["lars", "adamw"])
def test_state_roundtrip_continues_identically(kind):
    def make(model, options):
        if kind == "lars":
            return _lars_opt(model, param_options=options)
        return make_ours("adamw", model.parameters(), param_options=options)

    batches = _batches(6)
    model = _mlp()
    opt = make(model, _mlp_options(model))
    _run_ours(model, opt, batches[:4])
    saved = copy.deepcopy(opt.state_dict())
    assert [o["weight_decay"] for o in saved["param_options"][0]] == [
        None, 0.0, None, 0.0]
    assert [o["lr_scale"] for o in saved["param_options"][0]] == [
        1.0, 1.0, 0.5, 0.5]
    assert [o["lars"] for o in saved["param_options"][0]] == [
        kind == "lars", False, kind == "lars", False]
    model2 = _mlp()
    model2.load_state_dict(copy.deepcopy(model.state_dict()))
    # built WITHOUT the per-tensor options: the state restores them
    opt2 = make(model2, None)
    opt2.load_state_dict(saved)
    _run_ours(model, opt, batches[4:])
    _run_ours(model2, opt2, batches[4:])
    _assert_params_equal(model, model2)
    # tensor count or sizes differ: refuse
    other = nn.Linear(64, 128)
    with pytest.raises(ValueError, match="do not match"):
        FusedSGD(other.parameters(), lr=0.1, momentum=0.9).load_state_dict(
            saved)


def test_parent_format_state_loads():
    batches = _batches(4)
    a, b = _mlp(), _mlp()
    opt_a = FusedSGD(a.parameters(), lr=BASE_LR, momentum=0.9,
                     weight_decay=5e-4, param_options=no_decay_1d)
    opt_b = FusedSGD(b.parameters(), lr=BASE_LR, momentum=0.9,
                     weight_decay=5e-4, param_options=no_decay_1d)
    _run_ours(a, opt_a, batches[:2])
    _run_ours(b, opt_b, batches[:2])
    old = copy.deepcopy(opt_a.state_dict())
    del old["param_options"]          # what the parent commit wrote
    assert sorted(old) == ["defaults", "extra", "step_count"]
    opt_b.load_state_dict(old)
    assert opt_b._segmented           # its own options stay
    _run_ours(a, opt_a, batches[2:])
    _run_ours(b, opt_b, batches[2:])
    _assert_params_equal(a, b)


# -- 6. the example's config keys ---------------------------------------------

def test_cifar_example_tensor_option_config():
    from flashy_amd.config import Config
    from examples.cifar.train import get_tensor_options
    assert get_tensor_options(Config.wrap({"epochs": 2})) == dict(
        param_options=None, lars=None)
    cfg = Config.wrap({"no_decay_1d": False, "lars": {
        "enabled": False, "eta": 1e-3, "eps": 1e-8}})
    assert get_tensor_options(cfg) == dict(param_options=None, lars=None)
    cfg = Config.wrap({"no_decay_1d": True, "lars": {
        "enabled": True, "eta": 2e-3, "eps": 1e-9}})
    assert get_tensor_options(cfg) == dict(
        param_options=no_decay_1d, lars=LARS(eta=2e-3, eps=1e-9))
    cfg = Config.wrap({"lars": {"enabled": True}})
    assert get_tensor_options(cfg) == dict(param_options=None, lars=LARS())
    # the shipped defaults keep the example's optimizer as it was
    import yaml
    from pathlib import Path
    import examples.cifar.train as train
    shipped = yaml.safe_load(
        (Path(train.__file__).parent / "conf" / "config.yaml").read_text())
    assert shipped["no_decay_1d"] is False
    assert shipped["lars"] == {"enabled": False, "eta": 1e-3, "eps": 1e-8}
    assert get_tensor_options(Config.wrap(shipped)) == dict(
        param_options=None, lars=None)
