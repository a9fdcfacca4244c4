# Copyright (c) Flashy-AMD authors.
"""Channel LayerNorm, bias+GELU and layer scale + residual
(csrc/layernorm.hip) and the native ConvNeXt block, against float64 CPU
references built from the bf16-rounded inputs (F.layer_norm, F.gelu and plain
arithmetic under torch.autograd.grad).

Elementwise outputs: max |got - ref| / max |ref| < 2^-8 (one bf16 rounding is
2^-9 of the element; the bound of tests/test_dwconv_gpu.py).  Column sums,
elementwise: |got - (pre + ref)| <= 4 M 2^-24 S + 2^-23 |pre + ref| with S the
column sum of the absolute values of the terms, from a random ``pre`` in the
buffer, and two runs bitwise equal.  Outputs are NaN-filled before every
launch, so an unwritten element shows.

Measured on an MI355X, worst column-sum error / bound: 0.79 at one row, 0.37
at 5 rows, under 0.15 from 9 rows up.  The one-row LayerNorm case is what the
compensated deviation of k_ln_bwd is for: a plain fp32 x + b - mean missed
dgamma[6] there by 3.09 times (docs/kernels.md, "LayerNorm, bias+GELU, layer
scale").
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -8
EPS = 1e-6

# one row, one lane per row; 16-lane groups with idle lanes and ragged rows
# per wave; a plain power-of-two group; a ragged last block; a second, ragged
# octet per lane; the maximum width; several blocks and column-sum slices
LN_SHAPES = [(1, 8), (37, 96), (64, 64), (130, 128), (5, 520), (33, 1024),
             (3001, 96)]
# eight column chunks; a 4-lane group with an idle lane
EW_SHAPES = LN_SHAPES + [(37, 4096), (9, 24)]


@functools.lru_cache(maxsize=None)
def _case(M, C):
    """Inputs (activations bf16 on the device, parameters fp32) and the
    float64 references of all three families at one shape."""
    g = torch.Generator().manual_seed(1000 * C + M)
    act = {k: torch.randn(M, C, generator=g).to(torch.bfloat16)
           for k in ("x", "dy", "res")}
    par = {k: torch.randn(C, generator=g) for k in ("gamma", "beta", "b", "s")}
    c = {k: v.cuda() for k, v in {**act, **par}.items()}
    c["pre"] = torch.randn(3, C, generator=g)
    x, b, gamma, beta, s = (t.double().requires_grad_() for t in
                            (act["x"], par["b"], par["gamma"], par["beta"],
                             par["s"]))
    dy, res = act["dy"].double(), act["res"].double()
    if C <= 1024:
        y = F.layer_norm(x + b, (C,), gamma, beta, EPS)
        dx, dgamma, dbeta, db = torch.autograd.grad(y, (x, gamma, beta, b), dy)
        xhat = F.layer_norm((x + b).detach(), (C,), eps=EPS)
        c["ln"] = dict(y=y.detach(), dx=dx, sums=(dgamma, dbeta, db),
                       S=((dy * xhat).abs().sum(0), dy.abs().sum(0),
                          dx.abs().sum(0)))
    out = F.gelu(x + b)
    dh, db = torch.autograd.grad(out, (x, b), dy)
    c["gelu"] = dict(g=out.detach(), dh=dh, sums=(db,), S=(dh.abs().sum(0),))
    out = res + s * (x + b)
    dz, ds, db = torch.autograd.grad(out, (x, s, b), dy)
    c["sr"] = dict(out=out.detach(), dz=dz, sums=(ds, db),
                   S=((dy * (x + b)).abs().sum(0).detach(),
                      (s * dy).abs().sum(0).detach()))
    return c


def _rel(got, ref):
    assert not torch.isnan(got).any(), "an element was not written"
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _nan(like):
    return torch.full_like(like, float("nan"))


def _sums_ok(runs, c, ref, M):
    """runs: two lists of accumulated buffers, each started from c['pre']."""
    for j, (got, again) in enumerate(zip(*runs)):
        want = c["pre"][j].double() + ref["sums"][j]
        tol = 4 * M * 2.0 ** -24 * ref["S"][j] + 2.0 ** -23 * want.abs()
        err = (got.double().cpu() - want).abs()
        print(f"sum {j} worst err/tol {(err / tol).max().item():.3f}")
        assert (err <= tol).all(), (j, (err / tol).max().item())
        assert torch.equal(got, again), "column sums are not bitwise repeatable"


@pytest.mark.parametrize("M,C", LN_SHAPES)
def test_layernorm(M, C):
    from flashy_amd import ops
    c, ref = _case(M, C), _case(M, C)["ln"]
    y, stats = _nan(c["x"]), _nan(torch.empty(M, 2, device="cuda"))
    ops.ln_fwd(c["x"], c["gamma"], c["beta"], y, stats, EPS, c["b"])
    assert not torch.isnan(stats).any()
    runs = []
    for _ in range(2):
        dx = _nan(c["x"])
        sums = [p.cuda() for p in c["pre"]]
        ops.ln_bwd(c["dy"], c["x"], stats, c["gamma"], dx, *sums[:2],
                   b_in=c["b"], db_in=sums[2])
        runs.append(sums)
    ey, ex = _rel(y, ref["y"]), _rel(dx, ref["dx"])
    print(f"y {ey:.3e} dx {ex:.3e} bound {BOUND:.3e}")
    assert ey < BOUND and ex < BOUND, (ey, ex)
    _sums_ok(runs, c, ref, M)


@pytest.mark.parametrize("M,C", EW_SHAPES)
def test_bias_gelu(M, C):
    from flashy_amd import ops
    c, ref = _case(M, C), _case(M, C)["gelu"]
    g = _nan(c["x"])
    ops.bias_gelu_fwd(c["x"], c["b"], g)
    runs = []
    for _ in range(2):
        dh, db = _nan(c["x"]), c["pre"][0].cuda()
        ops.bias_gelu_bwd(c["dy"], c["x"], c["b"], dh, db)
        runs.append([db])
    eg, eh = _rel(g, ref["g"]), _rel(dh, ref["dh"])
    print(f"g {eg:.3e} dh {eh:.3e} bound {BOUND:.3e}")
    assert eg < BOUND and eh < BOUND, (eg, eh)
    _sums_ok(runs, c, ref, M)


@pytest.mark.parametrize("M,C", EW_SHAPES)
def test_scale_residual(M, C):
    from flashy_amd import ops
    c, ref = _case(M, C), _case(M, C)["sr"]
    out = _nan(c["x"])
    ops.scale_residual_fwd(c["x"], c["b"], c["s"], c["res"], out)
    runs = []
    for _ in range(2):
        dz, sums = _nan(c["x"]), [p.cuda() for p in c["pre"][:2]]
        ops.scale_residual_bwd(c["dy"], c["x"], c["b"], c["s"], dz, *sums)
        runs.append(sums)
    eo, ez = _rel(out, ref["out"]), _rel(dz, ref["dz"])
    print(f"out {eo:.3e} dz {ez:.3e} bound {BOUND:.3e}")
    assert eo < BOUND and ez < BOUND, (eo, ez)
    _sums_ok(runs, c, ref, M)


def test_plan_slices():
    from flashy_amd import ops
    assert ops.ln_plan(3001, 96).slices >= 3
    assert ops.ln_supported(33, 1024) and not ops.ln_supported(33, 1032)


def test_rstd_is_two_pass():
    """x = 64 + randn: E[x^2] / var ~ 4000.  Two-pass statistics err by about
    |mean| 2^-24 / sigma ~ 2^-18 per deviation, E[x^2] - mean^2 loses about
    4000 * 2^-24 ~ 2^-12; the bound, 2^-16, sits between."""
    from flashy_amd import ops
    M, C = 64, 128
    g = torch.Generator().manual_seed(5)
    x = (64 + torch.randn(M, C, generator=g)).to(torch.bfloat16)
    ones = torch.ones(C, device="cuda")
    stats = _nan(torch.empty(M, 2, device="cuda"))
    ops.ln_fwd(x.cuda(), ones, ones, _nan(x.cuda()), stats, EPS)
    want = (x.double().var(1, unbiased=False) + EPS).rsqrt()
    err = ((stats[:, 1].double().cpu() - want).abs() / want).max().item()
    print(f"rstd relative error {err:.3e} bound {2.0 ** -16:.3e}")
    assert err < 2.0 ** -16, err


def test_row_isolation():
    from flashy_amd import ops
    M, C, row = 37, 96, 21      # a row in the middle of a wave's four groups
    c = _case(M, C)
    x, dy = torch.zeros_like(c["x"]), torch.zeros_like(c["dy"])
    x[row], dy[row] = c["x"][row], c["dy"][row]
    y, dx = _nan(x), _nan(x)
    stats = torch.empty(M, 2, device="cuda")
    ops.ln_fwd(x, c["gamma"], c["beta"], y, stats, EPS)
    ops.ln_bwd(dy, x, stats, c["gamma"], dx, None, None)
    others = torch.arange(M) != row
    assert (dx[others] == 0).all() and dx[row].abs().sum() > 0
    assert (y[others] == c["beta"].to(torch.bfloat16)).all()


@pytest.mark.parametrize("dim", [64, 128])
def test_convnext_block(dim):
    """Native block against the float64 twin; the permitted error of each
    quantity is twice that of the same twin run on the CPU in bf16."""
    from flashy_amd.models import ConvNeXtBlock, NativeConvNeXtBlock
    torch.manual_seed(dim)
    twin = ConvNeXtBlock(dim)
    with torch.no_grad():
        twin.norm.weight.add_(0.5 * torch.randn(dim))
        twin.norm.bias.copy_(0.5 * torch.randn(dim))
        twin.gamma.copy_(torch.randn(dim))
    x = torch.randn(2, 8, 8, dim).to(torch.bfloat16)
    dy = torch.randn(2, 8, 8, dim).to(torch.bfloat16)

    def run_twin(dtype):
        m = copy.deepcopy(twin).to(dtype)
        xin = x.to(dtype).permute(0, 3, 1, 2).requires_grad_()
        out = m(xin)
        out.backward(dy.to(dtype).permute(0, 3, 1, 2))
        q = {"out": out.detach().permute(0, 2, 3, 1),
             "x.grad": xin.grad.permute(0, 2, 3, 1)}
        q.update({k: p.grad.flatten() for k, p in m.named_parameters()})
        return q

    ref, low = run_twin(torch.float64), run_twin(torch.bfloat16)
    block = NativeConvNeXtBlock.from_torch(twin).cuda()
    xin = x.cuda().requires_grad_()
    out = block(xin)
    out.backward(dy.cuda())
    ours = dict(block.named_parameters())
    got = {"out": out.detach(), "x.grad": xin.grad}
    for k in ref:
        if k not in got:    # the conv biases are block.<conv>_bias here
            got[k] = ours[k if k in ours else k.replace(".bias", "_bias")].grad
    got["dwconv.weight"] = got["dwconv.weight"].permute(0, 3, 1, 2)
    for k in ref:
        e_native = _rel(got[k].reshape(ref[k].shape), ref[k])
        e_bf16 = _rel(low[k], ref[k])
        print(f"{k}: native {e_native:.3e} bf16 twin {e_bf16:.3e}")
        assert e_native <= 2 * e_bf16, (k, e_native, e_bf16)

    for p in (block.norm.weight, block.norm.bias, block.gamma):
        p.requires_grad_(False)
        p.grad = None
    x2 = x.cuda().requires_grad_()
    block(x2).backward(dy.cuda())
    assert block.norm.weight.grad is None and block.gamma.grad is None
    assert x2.grad is not None and not torch.isnan(x2.grad).any()
