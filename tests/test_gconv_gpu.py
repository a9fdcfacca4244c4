# Copyright (c) Flashy-AMD authors.
"""Grouped 3x3 convolution (csrc/conv_group.hip) against a float64 CPU
reference built from the bf16-rounded inputs, F.conv2d(groups=G) in double.

Forward / backward-data: max |got - ref| / max |ref| < 2^-8, the bound of
tests/test_dgrad_s2_gpu.py: half a bf16 ulp at the largest element, doubled
for the fp32 accumulation (at most 288 terms here).  Weight gradient,
elementwise: |got - (pre + ref)| <= 4 M 2^-24 S + 2^-23 |pre + ref| with
S = sum |dy| |x| and M = N Ho Wo, the summation-order bound of
tests/bn_reference.py (bf16 products are exact in fp32).  Outputs are
NaN-filled before every launch, so an unwritten element shows.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -8

# (N, H, W, C, stride); the last two are wider than one 32-column tile, at
# stride 2 also in every backward-data parity class
SHAPES = [(2, 8, 8, 64, 1), (3, 7, 5, 128, 1), (2, 9, 9, 128, 2),
          (2, 8, 8, 64, 2), (5, 16, 16, 64, 1), (1, 3, 40, 64, 1),
          (1, 5, 133, 64, 2)]
CASES = [pytest.param(i, cg, id=f"{'x'.join(map(str, s))}-cg{cg}")
         for i, s in enumerate(SHAPES) for cg in (4, 8, 16, 32)]
CGS = [4, 8, 16, 32]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _case(i, cg):
    """Inputs (bf16, on the device) and float64 references of one case."""
    from flashy_amd import ops
    N, H, W, C, stride = SHAPES[i]
    G = C // cg
    g = torch.Generator().manual_seed(7 + i)
    x = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(C, 3, 3, cg, generator=g) * 0.2).to(torch.bfloat16)
    d = ops.ConvDims(N, H, W, C, C, 3, 3, (H - 1) // stride + 1,
                     (W - 1) // stride + 1, stride, 1)
    dy = torch.randn(N, d.Ho, d.Wo, C, generator=g).to(torch.bfloat16)
    pre = torch.randn(C, 3, 3, cg, generator=g)

    def conv(xx, ww):
        return F.conv2d(xx.permute(0, 3, 1, 2), ww.permute(0, 3, 1, 2),
                        stride=stride, padding=1, groups=G)

    xd = x.double().requires_grad_()
    wd = w.double().requires_grad_()
    y = conv(xd, wd)
    gy = dy.double().permute(0, 3, 1, 2)
    dx, dw = torch.autograd.grad(y, (xd, wd), gy)
    wa = w.double().abs().requires_grad_()
    (S,) = torch.autograd.grad(conv(x.double().abs(), wa), wa, gy.abs())
    return dict(d=d, G=G, x=x.cuda(), w=w.cuda(), dy=dy.cuda(), pre=pre,
                y=_nhwc(y.detach()), dx=dx, dw=dw, S=S)


def _rel(got, ref):
    assert not torch.isnan(got).any(), "an element was not written"
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _nan(shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


@pytest.mark.parametrize("i,cg", CASES)
def test_fwd_and_dgrad(i, cg):
    from flashy_amd import ops
    c = _case(i, cg)
    d = c["d"]
    y = _nan((d.N, d.Ho, d.Wo, d.K))
    ops.gconv_fwd(c["x"], c["w"], y, d, c["G"])
    dx = _nan((d.N, d.H, d.W, d.C))
    ops.gconv_dgrad(c["dy"], c["w"], dx, d, c["G"])
    ey, ex = _rel(y, c["y"]), _rel(dx, c["dx"])
    print(f"fwd {ey:.3e} dgrad {ex:.3e} bound {BOUND:.3e}")
    assert ey < BOUND and ex < BOUND, (ey, ex)


@pytest.mark.parametrize("i,cg", CASES)
def test_wgrad_accumulates(i, cg):
    from flashy_amd import ops
    c = _case(i, cg)
    d = c["d"]
    runs = []
    for _ in range(2):
        dw = c["pre"].cuda()
        ops.gconv_wgrad(c["x"], c["dy"], dw, d, c["G"])
        runs.append(dw)
    want = c["pre"].double() + c["dw"]
    M = d.N * d.Ho * d.Wo
    tol = 4 * M * 2.0 ** -24 * c["S"] + 2.0 ** -23 * want.abs()
    err = (runs[0].double().cpu() - want).abs()
    print(f"wgrad worst err/tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), (err / tol).max().item()
    assert torch.equal(runs[0], runs[1]), "wgrad is not bitwise repeatable"


@pytest.mark.parametrize("cg", CGS)
def test_group_isolation(cg):
    from flashy_amd import ops
    c = _case(1, cg)     # (3, 7, 5, 128, 1): two slabs
    d = c["d"]
    # the first group of the second slab: it has neighbours on both sides
    lo = c["G"] // 2 * cg
    hi = lo + cg
    x = torch.zeros_like(c["x"])
    x[..., lo:hi] = c["x"][..., lo:hi]
    y = _nan((d.N, d.Ho, d.Wo, d.K))
    ops.gconv_fwd(x, c["w"], y, d, c["G"])
    dy = torch.zeros_like(c["dy"])
    dy[..., lo:hi] = c["dy"][..., lo:hi]
    dx = _nan((d.N, d.H, d.W, d.C))
    ops.gconv_dgrad(dy, c["w"], dx, d, c["G"])
    for out in (y, dx):
        assert (out[..., :lo] == 0).all() and (out[..., hi:] == 0).all()
        assert out[..., lo:hi].abs().sum() > 0


@pytest.mark.parametrize("i,cg", [(1, 8), (2, 32)])
def test_module_autograd(i, cg):
    from flashy_amd import nn as fnn
    c = _case(i, cg)
    d = c["d"]
    conv = fnn.Conv2d(d.C, d.K, 3, d.stride, 1, groups=c["G"]).cuda()
    with torch.no_grad():
        conv.weight.copy_(c["w"].float())
    x = c["x"].clone().requires_grad_()
    y = conv(x)
    y.backward(c["dy"])
    assert _rel(y, c["y"]) < BOUND
    assert _rel(x.grad, c["dx"]) < BOUND
    M = d.N * d.Ho * d.Wo
    tol = 4 * M * 2.0 ** -24 * c["S"] + 2.0 ** -23 * c["dw"].abs()
    assert ((conv.weight.grad.double().cpu() - c["dw"]).abs() <= tol).all()


@pytest.mark.parametrize("cin,k,groups", [(128, 3, 2), (128, 1, 32), (96, 3, 12)])
def test_module_rejects_unsupported(cin, k, groups):
    from flashy_amd import nn as fnn
    with pytest.raises(ValueError, match="grouped conv needs"):
        fnn.Conv2d(cin, cin, k, 1, k // 2, groups=groups)


def test_reduced_resnext_matches_torch():
    from flashy_amd.models import NativeResNet, ResNet
    from flashy_amd.models.resnet import Bottleneck
    from flashy_amd.models.resnet_native import NativeBottleneck
    torch.manual_seed(5)
    twin = ResNet(Bottleneck, [1, 1, 1, 1], 10, small_input=True, groups=32,
                  base_width=4).cuda().train()
    model = NativeResNet(NativeBottleneck, [1, 1, 1, 1], groups=32,
                         base_width=4).cuda().train().from_torch(twin)
    x = torch.randn(8, 3, 32, 32, device="cuda")
    y = torch.randint(10, (8,), device="cuda")
    logits_n = model(x)
    loss_n = F.cross_entropy(logits_n, y)
    loss_n.backward()
    logits_t = twin(x)
    loss_t = F.cross_entropy(logits_t, y)
    diff = (logits_n - logits_t).abs().max().item()
    spread = logits_t.std().item() + 1e-6
    assert diff / spread < 0.35, (diff, spread)
    assert abs(loss_n.item() - loss_t.item()) < 0.25
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert p.grad.abs().sum() > 0, name
