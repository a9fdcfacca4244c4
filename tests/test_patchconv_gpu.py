# Copyright (c) Flashy-AMD authors.
"""Patch convolution (csrc/conv_patch.hip), the dense 2x2 stride-2 conv, the
per-channel bias add and the whole native ConvNeXt, against float64 CPU
references built from the bf16-rounded inputs (F.conv2d in double).

Forward / backward-data: max |got - ref| / max |ref| < 2^-8, the bound of
tests/test_gconv_gpu.py.  Weight gradient, elementwise: |got - (pre + ref)|
<= 4 M 2^-24 S + 2^-23 |pre + ref| with S = sum |dy| |x| and M = N Ho Wo.
Outputs are NaN-filled before every launch, so an unwritten element shows.
"""
import copy
import functools
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -8

# (N, H, W, C, p, K): plain; one output pixel, K off the 32 / 64 grid; Wo = 5,
# tiles that end mid-row and cross rows and images; H, W no multiples of p;
# C = 4, a row wider than one tile, K above 256; p = 2 with 4-byte-aligned
# rows; the minimum; M = 65 536 = 1024 tiles of 64 pixels: the forward grid
# of 512 blocks wraps and the weight gradient sums 256 partials of 4 tiles
PATCH = [(2, 8, 8, 3, 4, 64), (1, 4, 4, 3, 4, 48), (3, 12, 20, 3, 4, 128),
         (2, 10, 14, 3, 4, 64), (1, 8, 264, 4, 4, 320), (2, 6, 10, 3, 2, 96),
         (1, 2, 2, 4, 2, 16), (16, 256, 256, 3, 4, 64)]
# (N, H, W, C, p, K) of the dense 2x2 stride-2 downsample convs
DENSE = [(2, 8, 8, 64, 2, 128), (1, 6, 10, 128, 2, 256)]
BIAS = [(1, 8), (37, 96), (130, 128), (9, 24)]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (bf16, on the device) and float64 references of one conv."""
    from flashy_amd import ops
    N, H, W, C, p, K = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(K, p, p, C, generator=g) * 0.2).to(torch.bfloat16)
    d = ops.ConvDims(N, H, W, C, K, p, p, H // p, W // p, p, 0)
    dy = torch.randn(N, d.Ho, d.Wo, K, generator=g).to(torch.bfloat16)
    pre = torch.randn(K, p, p, C, generator=g)

    def conv(xx, ww):
        return F.conv2d(xx.permute(0, 3, 1, 2), ww.permute(0, 3, 1, 2),
                        stride=p)

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


@pytest.mark.parametrize("shape", PATCH, ids=lambda s: "x".join(map(str, s)))
def test_fwd_and_dgrad(shape):
    from flashy_amd import ops
    c = _case(shape)
    d = c["d"]
    y = _nan((d.N, d.Ho, d.Wo, d.K))
    ops.patchconv_fwd(c["x"], c["w"], y, d)
    dx = _nan((d.N, d.H, d.W, d.C))
    ops.patchconv_dgrad(c["dy"], c["w"], dx, d)
    ey, ex = _rel(y, c["y"]), _rel(dx, c["dx"])
    print(f"fwd {ey:.3e} dgrad {ex:.3e} bound {BOUND:.3e}")
    assert ey < BOUND and ex < BOUND, (ey, ex)
    # what no patch covers (H % p rows, W % p columns) is exactly zero
    assert (dx[:, d.Ho * d.R:] == 0).all() and (dx[:, :, d.Wo * d.R:] == 0).all()


@pytest.mark.parametrize("shape", PATCH, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_accumulates(shape):
    from flashy_amd import ops
    c = _case(shape)
    d = c["d"]
    runs = []
    for _ in range(2):
        dw = c["pre"].cuda()
        ops.patchconv_wgrad(c["x"], c["dy"], dw, d)
        runs.append(dw)
    want = c["pre"].double() + c["dw"]
    M = d.N * d.Ho * d.Wo
    tol = 4 * M * 2.0 ** -24 * c["S"] + 2.0 ** -23 * want.abs()
    err = (runs[0].double().cpu() - want).abs()
    print(f"wgrad worst err/tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), (err / tol).max().item()
    assert torch.equal(runs[0], runs[1]), "wgrad is not bitwise repeatable"


@pytest.mark.parametrize("shape", [(2, 32, 32, 3, 4, 128)] + DENSE,
                         ids=lambda s: "x".join(map(str, s)))
def test_module_autograd(shape):
    """fnn.Conv2d on the patch path (C = 3) and on the dense path (2x2
    stride 2, where repeatability is not asked: that path uses atomics)."""
    from flashy_amd import nn as fnn
    c = _case(shape)
    d = c["d"]
    conv = fnn.Conv2d(d.C, d.K, d.R, d.stride, 0).cuda()
    assert conv.patch == (d.C == 3)
    with torch.no_grad():
        conv.weight.copy_(c["w"].float())
    x = c["x"].clone().requires_grad_()
    y = conv(x)
    y.backward(c["dy"])
    ey, ex = _rel(y, c["y"]), _rel(x.grad, c["dx"])
    print(f"fwd {ey:.3e} dgrad {ex:.3e} bound {BOUND:.3e}")
    assert ey < BOUND and ex < BOUND, (ey, ex)
    M = d.N * d.Ho * d.Wo
    tol = 4 * M * 2.0 ** -24 * c["S"] + 2.0 ** -23 * c["dw"].abs()
    err = (conv.weight.grad.double().cpu() - c["dw"]).abs()
    print(f"wgrad worst err/tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), (err / tol).max().item()
    frozen = fnn.Conv2d(d.C, d.K, d.R, d.stride, 0).cuda()
    frozen.weight.requires_grad_(False)
    x2 = c["x"].clone().requires_grad_()
    frozen(x2).backward(c["dy"])
    assert frozen.weight.grad is None and x2.grad is not None


@pytest.mark.parametrize("k,stride,pad", [(7, 2, 3), (3, 1, 1)])
def test_other_stems_keep_their_route(k, stride, pad):
    from flashy_amd import ops
    ho = (32 + 2 * pad - k) // stride + 1
    assert not ops.patchconv_supported(
        ops.ConvDims(2, 32, 32, 3, 64, k, k, ho, ho, stride, pad))


@pytest.mark.parametrize("M,C", BIAS)
def test_bias_add(M, C):
    from flashy_amd import nn as fnn
    g = torch.Generator().manual_seed(1000 * C + M)
    z, dout = (torch.randn(M, C, generator=g).to(torch.bfloat16)
               for _ in range(2))
    b, pre = torch.randn(C, generator=g), torch.randn(C, generator=g)
    runs = []
    for _ in range(2):
        bias = b.cuda().requires_grad_()
        bias.grad = pre.cuda()
        zin = z.cuda().requires_grad_()
        out = fnn.bias_add(zin.clone(), bias)
        out.backward(dout.cuda())
        assert torch.equal(zin.grad, dout.cuda())
        runs.append(bias.grad)
    e = _rel(out.detach(), z.double() + b.double())
    print(f"out {e:.3e} bound {BOUND:.3e}")
    assert e < BOUND, e
    want = pre.double() + dout.double().sum(0)
    tol = 4 * M * 2.0 ** -24 * dout.double().abs().sum(0) + 2.0 ** -23 * want.abs()
    err = (runs[0].double().cpu() - want).abs()
    print(f"db worst err/tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), (err / tol).max().item()
    assert torch.equal(runs[0], runs[1]), "db is not bitwise repeatable"


@pytest.mark.parametrize("patch", [4, 2])
def test_convnext(patch):
    """Native network against the float64 twin; the permitted error of each
    quantity is twice that of the same twin run on the CPU in bf16.  A
    quantity the bf16 twin gets exactly is compared for equality."""
    from flashy_amd.models import ConvNeXt, NativeConvNeXt
    torch.manual_seed(patch)
    twin = ConvNeXt((1, 1, 1, 1), (64, 128, 192, 256), 10, patch=patch)
    with torch.no_grad():
        for name, p in twin.named_parameters():
            if "norm" in name and name.endswith("weight"):
                p.add_(0.5 * torch.randn_like(p))
            elif "norm" in name or name.endswith("gamma"):
                p.copy_(torch.randn_like(p) * (0.5 if "norm" in name else 1))
    x = torch.randn(2, 64, 64, 3).to(torch.bfloat16)
    dy = torch.randn(2, 10)

    def run_twin(dtype):
        m = copy.deepcopy(twin).to(dtype)
        out = m(x.to(dtype).permute(0, 3, 1, 2))
        out.backward(dy.to(dtype))
        q = {"out": out.detach()}
        q.update({k: p.grad for k, p in m.named_parameters()})
        return q

    ref, low = run_twin(torch.float64), run_twin(torch.bfloat16)
    with pytest.raises(ValueError):
        NativeConvNeXt((1, 1, 1, 1), (64, 96, 192, 256), 10)
    net = NativeConvNeXt.from_torch(twin).cuda()
    out = net(x.cuda())
    out.backward(dy.cuda())
    ours = dict(net.named_parameters())
    for k in ref:
        if k == "out":
            got = out.detach()
        else:
            name = re.sub(r"down_convs\.(\d)\.bias", r"down_biases.\1", k)
            got = ours[name if name in ours
                       else name.replace(".bias", "_bias")].grad
            if got.dim() == 4 and ref[k].dim() == 4:    # KRSC -> KCRS
                got = got.permute(0, 3, 1, 2)
        e_native = _rel(got.reshape(ref[k].shape), ref[k])
        e_bf16 = _rel(low[k], ref[k])
        print(f"{k}: native {e_native:.3e} bf16 twin {e_bf16:.3e}")
        assert e_native <= 2 * e_bf16, (k, e_native, e_bf16)
