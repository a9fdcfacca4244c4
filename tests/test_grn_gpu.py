# Copyright (c) Flashy-AMD authors.
"""Global response normalization (csrc/grn.hip), the fused bias+GELU that
gathers its sums of squares, and the native ConvNeXt V2, against float64 CPU
references built from the bf16-rounded inputs with plain torch (torch.norm,
a mean, arithmetic) under torch.autograd.grad.

Elementwise outputs (out, dx): max |got - ref| / max |ref| < 2^-8, the bound
of tests/test_layernorm_gpu.py.  Parameter gradients, elementwise, from a
random ``pre`` in the buffer, two runs bitwise equal:

  dbeta:  |got - (pre + ref)| <= 4 M 2^-24 S + 2^-23 |pre + ref|, M = N * HW
          terms, S the column sum of |dout|.
  dgamma: the same with S = sum_n |Nx| * sum_hw |dout * x|, and M + HW + C + 2
          in the place of M.  The extra terms are the fp32 error of Nx itself,
          from the rule that a fixed order of k fp32 adds stays within
          4 k 2^-24 of the sum of the absolute values: S[n,c] adds HW
          non-negative terms, so it is within 4 HW 2^-24 of itself; the square
          root halves that and rounds once (2 HW + 1); mu adds C non-negative
          Gx and divides by C (another 4 C + 1); mu + eps, the reciprocal and
          Gx times it round three times; Nx * P once more.  Together
          (4 HW + 4 C + 7) 2^-24 < 4 (HW + C + 2) 2^-24, relative to
          |Nx * P| <= |Nx| * sum_hw |dout * x|.

Outputs are NaN-filled before every launch, so an unwritten element shows.

Measured on an MI355X, worst error / bound over the shapes below: dgamma 0.242
and dbeta 0.102, both at one image of one pixel; from 5 pixels up at most
0.006 and 0.059.  out and dx: 1.5e-3 to 3.2e-3 against 2^-8 = 3.9e-3
(docs/kernels.md, "Global response normalization").
"""
import copy
import functools
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -8
EPS = 1e-6

# (N, HW, C, zeros).  One image of one pixel, one lane per row; a 4-lane group
# with an idle lane, three images inside what one block's 64 rows would hold;
# 16-lane groups, four slices per image, the last one a single row, with a
# zero channel and a zero image; the same without zeros; a 64-lane group with
# idle lanes and a ragged last row slot; a ragged second column chunk; eight
# chunks and all 16 channels of a coefficient thread; 196 slices per image
SHAPES = [(1, 1, 8, False), (3, 5, 24, False), (3, 49, 96, True),
          (3, 49, 96, False), (2, 37, 384, False), (2, 5, 520, False),
          (2, 3, 4096, False), (3, 3136, 96, False)]


def _grn(x, gamma, beta):
    gx = torch.norm(x, p=2, dim=1, keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + EPS)
    return gamma * (x * nx) + beta + x, nx.squeeze(1)


@functools.lru_cache(maxsize=None)
def _case(N, HW, C, zeros=False):
    g = torch.Generator().manual_seed(100000 * N + 10 * C + HW)
    x = torch.randn(N, HW, C, generator=g).to(torch.bfloat16)
    if zeros:
        x[0, :, 5] = 0      # one channel of one image
        x[N - 1] = 0        # a whole image
    dout = torch.randn(N, HW, C, generator=g).to(torch.bfloat16)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    c = {"x": x.cuda(), "dout": dout.cuda(), "gamma": gamma.cuda(),
         "beta": beta.cuda(), "pre": torch.randn(2, C, generator=g)}
    xd, gd, bd = (t.double().requires_grad_() for t in (x, gamma, beta))
    out, nx = _grn(xd, gd, bd)
    dx, dgamma, dbeta = torch.autograd.grad(out, (xd, gd, bd), dout.double())
    c.update(out=out.detach(), dx=dx, sums=(dgamma, dbeta),
             S=((nx.detach().abs() * (dout.double() * xd.detach()).abs().sum(1)
                 ).sum(0), dout.double().abs().sum((0, 1))))
    return c


def _rel(got, ref):
    assert torch.isfinite(got).all(), "an element is unwritten or not finite"
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _nan(like):
    return torch.full_like(like, float("nan"))


def _fwd(c, x=None):
    from flashy_amd import ops
    x = c["x"] if x is None else x
    N, _, C = x.shape
    out = _nan(x)
    coefs = [_nan(torch.empty(N, C, device="cuda")) for _ in range(2)]
    coefs.append(_nan(torch.empty(N, device="cuda")))
    ops.grn_fwd(x, c["gamma"], c["beta"], out, *coefs, EPS)
    return out, coefs


@pytest.mark.parametrize("N,HW,C,zeros", SHAPES)
def test_grn(N, HW, C, zeros):
    from flashy_amd import ops
    c = _case(N, HW, C, zeros)
    out, coefs = _fwd(c)
    assert all(torch.isfinite(t).all() for t in coefs)
    runs = []
    for _ in range(2):
        dx, sums = _nan(c["x"]), [p.cuda() for p in c["pre"]]
        ops.grn_bwd(c["dout"], c["x"], *coefs, c["gamma"], dx, *sums)
        runs.append(sums)
    eo, ex = _rel(out, c["out"]), _rel(dx, c["dx"])
    print(f"out {eo:.3e} dx {ex:.3e} bound {BOUND:.3e}")
    assert eo < BOUND and ex < BOUND, (eo, ex)
    if zeros:       # dx = dout and out = x + beta where Nx == 0, not a NaN
        for got, ref in ((out, c["out"]), (dx, c["dx"])):
            for at in ((0, slice(None), 5), (N - 1,)):
                assert _rel(got[at], ref[at]) < BOUND
    terms = (N * HW + HW + C + 2, N * HW)
    for j, (got, again) in enumerate(zip(*runs)):
        want = c["pre"][j].double() + c["sums"][j]
        tol = 4 * terms[j] * 2.0 ** -24 * c["S"][j] + 2.0 ** -23 * want.abs()
        err = (got.double().cpu() - want).abs()
        print(f"{('dgamma', 'dbeta')[j]} worst err/tol "
              f"{(err / tol).max().item():.3f}")
        assert (err <= tol).all(), (j, (err / tol).max().item())
        assert torch.equal(got, again), "sums are not bitwise repeatable"
    # absent targets: dx alone, and the parameter gradients alone
    dx2, sums = _nan(c["x"]), [p.cuda() for p in c["pre"]]
    ops.grn_bwd(c["dout"], c["x"], *coefs, c["gamma"], dx2, None, None)
    ops.grn_bwd(c["dout"], c["x"], *coefs, c["gamma"], None, *sums)
    assert torch.equal(dx2, dx) and torch.equal(sums[0], runs[0][0])


@pytest.mark.parametrize("N,HW,C", [(3, 49, 96), (2, 5, 520)])
def test_fused_gelu_is_bitwise(N, HW, C):
    from flashy_amd import ops
    c = _case(N, HW, C)
    slices = ops.grn_plan(N, HW, C).slices
    g, g2 = _nan(c["x"]), _nan(c["x"])
    sq, sq2 = (_nan(torch.empty(N, slices, C, device="cuda")) for _ in "ab")
    ops.bias_gelu_fwd(c["x"], c["beta"], g)
    ops.grn_sqsum(g, sq)
    ops.bias_gelu_sqsum(c["x"], c["beta"], g2, sq2)
    assert torch.isfinite(sq).all() and sq.sum() > 0
    assert torch.equal(g, g2) and torch.equal(sq, sq2)


def test_image_isolation():
    from flashy_amd import ops
    c = _case(3, 49, 96)
    x2 = c["x"].clone()
    x2[1] = c["x"][2]
    got = []
    for x in (c["x"], x2):
        out, coefs = _fwd(c, x)
        dx = _nan(x)
        ops.grn_bwd(c["dout"], x, *coefs, c["gamma"], dx, None, None)
        got.append((out, dx))
    for a, b in zip(*got):
        assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


@pytest.mark.parametrize("whole", [False, True], ids=["block", "network"])
def test_convnextv2(whole):
    """Native V2 block (dim 96) and network against the float64 twin; the
    permitted error of each quantity is twice that of the same twin run on
    the CPU in bf16 (tests/test_pwconv_gpu.py::test_convnext_off_grid)."""
    from flashy_amd.models import (ConvNeXt, ConvNeXtV2Block, NativeConvNeXt,
                                   NativeConvNeXtV2Block)
    torch.manual_seed(196 + whole)
    twin = ConvNeXt((1, 1, 1, 1), (48, 96, 192, 384), 10,
                    block=ConvNeXtV2Block) if whole else ConvNeXtV2Block(96)
    with torch.no_grad():
        for name, p in twin.named_parameters():
            if "norm" in name and name.endswith("weight"):
                p.add_(0.5 * torch.randn_like(p))
            elif "norm" in name or "grn" in name:   # GRN starts at zero
                p.copy_(0.5 * torch.randn_like(p))
    x = torch.randn((2, 64, 64, 3) if whole else (2, 8, 8, 96))
    x = x.to(torch.bfloat16).requires_grad_(not whole)
    dy = torch.randn(2, 10) if whole else \
        torch.randn(2, 8, 8, 96).to(torch.bfloat16)

    def run_twin(dtype):
        m = copy.deepcopy(twin).to(dtype)
        xin = x.detach().to(dtype).requires_grad_(not whole)
        out = m(xin.permute(0, 3, 1, 2))
        out = out if whole else out.permute(0, 2, 3, 1)
        out.backward(dy.to(dtype))
        q = {"out": out.detach()}
        if not whole:
            q["x"] = xin.grad
        q.update({k: p.grad for k, p in m.named_parameters()})
        return q

    ref, low = run_twin(torch.float64), run_twin(torch.bfloat16)
    net = (NativeConvNeXt if whole else NativeConvNeXtV2Block).from_torch(
        twin).cuda()
    xg = x.detach().cuda().requires_grad_(not whole)
    out = net(xg)
    out.backward(dy.cuda())
    ours = dict(net.named_parameters())
    for k in ref:
        if k in ("out", "x"):
            got = out.detach() if k == "out" else xg.grad
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
