# Copyright (c) Flashy-AMD authors.
"""Depthwise k x k convolution (csrc/conv_depthwise.hip) against a float64
CPU reference built from the bf16-rounded inputs, F.conv2d(groups=C) in
double.

Forward / backward-data: max |got - ref| / max |ref| < 2^-8, the bound of
tests/test_gconv_gpu.py (at most 49 terms here).  Weight gradient,
elementwise: |got - (pre + ref)| <= 4 M 2^-24 S + 2^-23 |pre + ref| with
S = sum |dy| |x| and M = N Ho Wo.  Outputs are NaN-filled before every
launch, so an unwritten element shows.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -8

# (N, H, W, C, stride): plain; odd sizes under the 7x7 window with a full and
# a one-octet slab; odd at stride 2 (unequal parity classes), one octet; even
# at stride 2, three slabs; all halo; two wider than one 16-column tile
SHAPES = [(2, 8, 8, 64, 1), (3, 7, 5, 72, 1), (2, 9, 9, 8, 2),
          (2, 8, 8, 136, 2), (1, 1, 1, 64, 1), (1, 3, 40, 64, 1),
          (1, 5, 133, 24, 2)]
KS = (3, 5, 7)
CASES = [pytest.param(k, i, id=f"k{k}-{'x'.join(map(str, s))}")
         for k in KS for i, s in enumerate(SHAPES)]


@functools.lru_cache(maxsize=None)
def _case(k, i):
    """Inputs (bf16, on the device) and float64 references of one case."""
    from flashy_amd import ops
    N, H, W, C, stride = SHAPES[i]
    g = torch.Generator().manual_seed(11 * k + i)
    x = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(C, k, k, 1, generator=g) * 0.2).to(torch.bfloat16)
    d = ops.ConvDims(N, H, W, C, C, k, k, (H - 1) // stride + 1,
                     (W - 1) // stride + 1, stride, k // 2)
    dy = torch.randn(N, d.Ho, d.Wo, C, generator=g).to(torch.bfloat16)
    pre = torch.randn(C, k, k, 1, generator=g)

    def conv(xx, ww):
        return F.conv2d(xx.permute(0, 3, 1, 2), ww.permute(0, 3, 1, 2),
                        stride=stride, padding=k // 2, groups=C)

    xd = x.double().requires_grad_()
    wd = w.double().requires_grad_()
    y = conv(xd, wd)
    gy = dy.double().permute(0, 3, 1, 2)
    dx, dw = torch.autograd.grad(y, (xd, wd), gy)
    wa = w.double().abs().requires_grad_()
    (S,) = torch.autograd.grad(conv(x.double().abs(), wa), wa, gy.abs())
    return dict(d=d, x=x.cuda(), w=w.cuda(), dy=dy.cuda(), pre=pre,
                y=y.detach().permute(0, 2, 3, 1).contiguous(), dx=dx, dw=dw,
                S=S)


def _rel(got, ref):
    assert not torch.isnan(got).any(), "an element was not written"
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _nan(shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


@pytest.mark.parametrize("k,i", CASES)
def test_fwd_and_dgrad(k, i):
    from flashy_amd import ops
    c = _case(k, i)
    d = c["d"]
    y = _nan((d.N, d.Ho, d.Wo, d.K))
    ops.dwconv_fwd(c["x"], c["w"], y, d)
    dx = _nan((d.N, d.H, d.W, d.C))
    ops.dwconv_dgrad(c["dy"], c["w"], dx, d)
    ey, ex = _rel(y, c["y"]), _rel(dx, c["dx"])
    print(f"fwd {ey:.3e} dgrad {ex:.3e} bound {BOUND:.3e}")
    assert ey < BOUND and ex < BOUND, (ey, ex)


@pytest.mark.parametrize("k,i", CASES)
def test_wgrad_accumulates(k, i):
    from flashy_amd import ops
    c = _case(k, i)
    d = c["d"]
    runs = []
    for _ in range(2):
        dw = c["pre"].cuda()
        ops.dwconv_wgrad(c["x"], c["dy"], dw, d)
        runs.append(dw)
    want = c["pre"].double() + c["dw"]
    M = d.N * d.Ho * d.Wo
    tol = 4 * M * 2.0 ** -24 * c["S"] + 2.0 ** -23 * want.abs()
    err = (runs[0].double().cpu() - want).abs()
    print(f"wgrad worst err/tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), (err / tol).max().item()
    assert torch.equal(runs[0], runs[1]), "wgrad is not bitwise repeatable"


@pytest.mark.parametrize("k", KS)
def test_channel_isolation(k):
    from flashy_amd import ops
    c = _case(k, 1)     # (3, 7, 5, 72, 1): a full slab and a one-octet slab
    d = c["d"]
    ch = 67             # in the second slab, neighbours on both sides
    x = torch.zeros_like(c["x"])
    x[..., ch] = c["x"][..., ch]
    y = _nan((d.N, d.Ho, d.Wo, d.K))
    ops.dwconv_fwd(x, c["w"], y, d)
    dy = torch.zeros_like(c["dy"])
    dy[..., ch] = c["dy"][..., ch]
    dx = _nan((d.N, d.H, d.W, d.C))
    ops.dwconv_dgrad(dy, c["w"], dx, d)
    for out in (y, dx):
        assert (out[..., :ch] == 0).all() and (out[..., ch + 1:] == 0).all()
        assert out[..., ch].abs().sum() > 0


@pytest.mark.parametrize("k,i", [(5, 1), (7, 2)])
def test_module_autograd(k, i):
    from flashy_amd import nn as fnn
    c = _case(k, i)
    d = c["d"]
    conv = fnn.Conv2d(d.C, d.C, k, d.stride, k // 2, groups=d.C).cuda()
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
    frozen = fnn.Conv2d(d.C, d.C, k, d.stride, k // 2, groups=d.C).cuda()
    frozen.weight.requires_grad_(False)
    x2 = c["x"].clone().requires_grad_()
    frozen(x2).backward(c["dy"])
    assert frozen.weight.grad is None and x2.grad is not None


@pytest.mark.parametrize("cin,k,stride,pad", [
    (12, 3, 1, 1), (64, 4, 1, 2), (64, 9, 1, 4), (64, 3, 1, 0), (64, 3, 3, 1)])
def test_module_rejects_unsupported(cin, k, stride, pad):
    from flashy_amd import nn as fnn
    with pytest.raises(ValueError, match="depthwise conv needs"):
        fnn.Conv2d(cin, cin, k, stride, pad, groups=cin)
    with pytest.raises(ValueError, match="grouped conv needs"):
        fnn.Conv2d(128, 128, 3, 1, 1, groups=2)
