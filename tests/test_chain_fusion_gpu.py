# Copyright (c) Flashy-AMD authors.
"""GPU tests for the launch-chain fusions: BatchNorm partials emitted by the
split-K combine, and the fused global-average-pool + fc classifier head."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")


def _mk(N, H, W, C, K, R, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(N, H, W, C, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(K, R, R, C, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    return x, w


def _fwd_zn(d):
    """The split count ops.conv_fwd picks for these dims (0 = single pass)."""
    from flashy_amd import ops
    ext = ops.require()
    M = d.N * d.Ho * d.Wo
    stages = (d.R * d.S * d.C + 63) // 64
    if ext.conv8_eligible(*d, False):
        return 0
    zn = ops._splitk_plan(M, d.K // 64, stages)
    if zn == 0 and stages >= 16:
        mt8 = (M + 255) // 256
        bn8 = 128 if d.K % 128 == 0 else 64
        tiles8 = mt8 * (d.K // bn8)
        if tiles8 and tiles8 < 160:
            zn = min(max(2, -(-160 // tiles8)), 8, stages // 8)
            zn = 0 if zn < 2 else zn
    return zn


def _check_partials(stats, y, K):
    """Partials summed over msplit vs sums of the stored y, under the
    tolerance formula of test_conv_fused_bn_stats
    (~ sqrt(M) * bf16_eps * max|y|)."""
    partials, msplit = stats
    assert partials.numel() == 2 * K * msplit
    s = partials[:K * msplit].view(K, msplit).sum(1)
    s2 = partials[K * msplit:].view(K, msplit).sum(1)
    yf = y.float().reshape(-1, K)
    M = yf.shape[0]
    d1 = (s - yf.sum(0)).abs().max().item()
    tol = 0.02 * M ** 0.5 * yf.abs().max().item()
    d2 = (s2 - (yf * yf).sum(0)).abs().max().item()
    tol2 = 0.02 * M ** 0.5 * (yf * yf).max().item()
    print(f"M={M} K={K} msplit={msplit} dsum={d1:.4g}/{tol:.4g} "
          f"dsumsq={d2:.4g}/{tol2:.4g}")
    assert d1 < tol, (d1, tol)
    assert d2 < tol2, (d2, tol2)


SPLITK_SHAPES = [
    # (N, H, W, C, K)   all 3x3 stride 1 pad 1
    (2, 8, 8, 128, 128),   # M=128, 18 stages
    (3, 5, 5, 64, 64),     # M=75: ragged last m-block, msplit=3 (scalar
                           # combine_partials8 path)
    (2, 4, 4, 256, 192),   # three channel groups, M=32
]


@requires_gpu
@pytest.mark.parametrize("shape", SPLITK_SHAPES)
def test_splitk_combine_stats(shape):
    from flashy_amd import ops
    N, H, W, C, K = shape
    x, w = _mk(N, H, W, C, K, 3, seed=11)
    d = ops.ConvDims.infer(x, w, 1, 1)
    assert _fwd_zn(d) >= 2, "shape must take the split-K path"
    y = x.new_empty((d.N, d.Ho, d.Wo, d.K))
    stats = ops.conv_fwd(x, w, y, d, want_stats=True)
    assert stats is not None
    assert stats[1] == ops.bn_msplit(d.N * d.Ho * d.Wo, K)
    y_plain = torch.empty_like(y)
    assert ops.conv_fwd(x, w, y_plain, d, want_stats=False) is None
    torch.cuda.synchronize()
    # same conv kernel, same fp32 slice sum in the same z order
    assert torch.equal(y.view(torch.int16), y_plain.view(torch.int16))
    _check_partials(stats, y, K)
    # statistics of the rounded values in bn_stats' own order: bitwise the
    # pass this fusion removes, so training results cannot move
    M = d.N * d.Ho * d.Wo
    ref = torch.empty_like(stats[0])
    ops.bn_stats(y, ref, M, K, stats[1])
    torch.cuda.synchronize()
    assert torch.equal(stats[0], ref)


def test_splitk_msplit_scalar_path_shape():
    """The M=75 case must really leave msplit off the float4 path."""
    from flashy_amd import ops
    assert ops.bn_msplit(75, 64) % 4 != 0
    assert ops.bn_msplit(128, 128) % 4 == 0


@requires_gpu
def test_splitk_conv_bn_module_matches_unfused():
    """Conv2d(feeds_bn=True) -> BatchNorm2d with the combine's partials vs
    the same pair with the partials stripped (bn_stats runs)."""
    from flashy_amd import nn as fnn
    from flashy_amd import ops
    N, H, W, C, K = SPLITK_SHAPES[0]
    torch.manual_seed(7)
    conv = fnn.Conv2d(C, K, 3, 1, 1, feeds_bn=True).cuda().train()
    x16 = torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16)
    assert _fwd_zn(ops.ConvDims.infer(x16, conv.weight, 1, 1)) >= 2
    dy = torch.randn(N, H, W, K, device="cuda").to(torch.bfloat16)

    def run(strip):
        bn = fnn.BatchNorm2d(K).cuda().train()
        with torch.no_grad():
            bn.weight.mul_(1.5)
            bn.bias.add_(0.3)
        conv.weight.grad = None
        x = x16.detach().requires_grad_(True)
        y = conv(x)
        assert getattr(y, "_bn_stats", None) is not None
        if strip:
            del y._bn_stats
        y.retain_grad()   # the BatchNorm's dx, as in test_bn_fwd_bwd
        # no ReLU: a mask flip at out ~ 0 would turn a last-bit statistics
        # difference into an O(|dy|) gradient difference
        out = bn(y)
        out.backward(dy)
        torch.cuda.synchronize()
        return (out.detach().float(), bn.running_mean.clone(),
                bn.running_var.clone(), bn.weight.grad.clone(),
                bn.bias.grad.clone(), y.grad.float(), x.grad.float())

    out_f, rm_f, rv_f, dg_f, db_f, dx_f, dxc_f = run(strip=False)
    out_u, rm_u, rv_u, dg_u, db_u, dx_u, dxc_u = run(strip=True)
    tol = 5e-2   # tolerances of test_bn_fwd_bwd
    print("out", (out_f - out_u).abs().max().item(),
          "bn dx", (dx_f - dx_u).abs().max().item(),
          "conv dx", (dxc_f - dxc_u).abs().max().item(),
          "of max", dxc_u.abs().max().item())
    assert (out_f - out_u).abs().max().item() < tol
    assert (dx_f - dx_u).abs().max().item() < tol
    # the conv's own dx sums 9*K of those through dgrad and rounds to bf16
    # at a larger magnitude: same tolerance, relative to its range
    assert (dxc_f - dxc_u).abs().max().item() < \
        tol * max(1.0, dxc_u.abs().max().item())
    assert torch.allclose(rm_f, rm_u, atol=tol, rtol=2e-2)
    assert torch.allclose(rv_f, rv_u, atol=tol, rtol=2e-2)
    assert torch.allclose(dg_f, dg_u, atol=1.0, rtol=2e-2)
    assert torch.allclose(db_f, db_u, atol=1.0, rtol=2e-2)


# ---------------------------------------------------------------------------
# fused pool + fc head
# ---------------------------------------------------------------------------

HEAD_SHAPES = [
    # (B, H, W, C, O)
    (3, 2, 2, 64, 10),     # smallest; odd B
    (64, 4, 4, 512, 10),   # the flagship head
    (2, 1, 1, 128, 1),     # HW=1 and O=1
]

U32 = 2.0 ** -24   # fp32 unit roundoff
U16 = 2.0 ** -8    # one bf16 ulp, relative


def _head_inputs(B, H, W, C, O, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, H, W, C, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(O, C, device="cuda", generator=g) * C ** -0.5
    b = torch.randn(O, device="cuda", generator=g)
    dy = torch.randn(B, O, device="cuda", generator=g)
    return x, w, b, dy


def _within(name, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3g}, "
          f"max bound {bound.max().item():.3g}")
    assert worst <= 0, (name, err.max().item(), bound.max().item())


@requires_gpu
@pytest.mark.parametrize("shape", HEAD_SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_pool_linear_head(shape, bias):
    """Against x.float().mean((1,2)) -> F.linear in fp64 from the same bf16
    input.  Differences are fp32 summation order only: |err| <=
    2 * n * 2^-24 * sum|terms| with n the reduction length, plus one bf16
    ulp on the bf16-rounded dx."""
    from flashy_amd import nn as fnn
    B, H, W, C, O = shape
    HW = H * W
    x16, w32, b32, dy = _head_inputs(B, H, W, C, O)
    x = x16.detach().requires_grad_(True)
    w = w32.detach().requires_grad_(True)
    b = b32.detach().requires_grad_(True) if bias else None
    y = fnn.pool_linear(x, w, b)
    assert y.dtype == torch.float32 and y.shape == (B, O)
    y.backward(dy)
    torch.cuda.synchronize()

    x64, w64, dy64 = x16.double(), w32.double(), dy.double()
    pooled = x64.mean((1, 2))
    pooled_abs = x64.abs().mean((1, 2))
    ref_y = pooled @ w64.t()
    terms_y = pooled_abs @ w64.abs().t()
    if bias:
        ref_y = ref_y + b32.double()
        terms_y = terms_y + b32.double().abs()
    _within("logits", y, ref_y, 2 * (HW * C) * U32 * terms_y)

    ref_dw = dy64.t() @ pooled
    _within("dw", w.grad, ref_dw,
            2 * (B * HW) * U32 * (dy64.abs().t() @ pooled_abs))
    if bias:
        _within("db", b.grad, dy64.sum(0), 2 * B * U32 * dy64.abs().sum(0))

    ref_g = (dy64 @ w64) / HW                     # [B, C]
    terms_g = (dy64.abs() @ w64.abs()) / HW
    bound_g = 2 * O * U32 * terms_g + U16 * ref_g.abs()
    assert x.grad.dtype == torch.bfloat16 and x.grad.shape == x16.shape
    _within("dx", x.grad, ref_g[:, None, None, :].expand(B, H, W, C),
            bound_g[:, None, None, :].expand(B, H, W, C))


@requires_gpu
def test_pool_linear_head_grad_semantics(monkeypatch):
    from flashy_amd import nn as fnn
    from flashy_amd import ops
    B, H, W, C, O = HEAD_SHAPES[0]
    x16, w32, b32, dy = _head_inputs(B, H, W, C, O, seed=5)

    # two backward calls accumulate into .grad (second one in place)
    w = w32.detach().requires_grad_(True)
    b = b32.detach().requires_grad_(True)
    fnn.pool_linear(x16, w, b).backward(dy)
    g1w, g1b = w.grad.clone(), b.grad.clone()
    fnn.pool_linear(x16, w, b).backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(w.grad, 2 * g1w) and torch.equal(b.grad, 2 * g1b)

    # frozen weight / frozen bias: that .grad stays untouched
    sentinel_w = torch.full_like(w32, 7.0)
    wf = w32.detach().requires_grad_(False)
    wf.grad = sentinel_w.clone()
    b2 = b32.detach().requires_grad_(True)
    fnn.pool_linear(x16, wf, b2).backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(wf.grad, sentinel_w)
    assert torch.equal(b2.grad, g1b)

    sentinel_b = torch.full_like(b32, -3.0)
    bf = b32.detach().requires_grad_(False)
    bf.grad = sentinel_b.clone()
    w2 = w32.detach().requires_grad_(True)
    fnn.pool_linear(x16, w2, bf).backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(bf.grad, sentinel_b)
    assert torch.equal(w2.grad, g1w)

    # a trunk output without requires_grad: no dx kernel, no gradient
    calls = []
    real_dx = ops.head_dx
    monkeypatch.setattr(ops, "head_dx",
                        lambda *a, **k: (calls.append(1), real_dx(*a, **k)))
    w3 = w32.detach().requires_grad_(True)
    x_nograd = x16.detach()
    fnn.pool_linear(x_nograd, w3, None).backward(dy)
    torch.cuda.synchronize()
    assert not calls and x_nograd.grad is None
    xg = x16.detach().requires_grad_(True)
    fnn.pool_linear(xg, w3, None).backward(dy)
    torch.cuda.synchronize()
    assert len(calls) == 1 and xg.grad is not None


@requires_gpu
def test_pool_pair_large_head():
    """Above the rocBLAS cutoff the head is pool kernels + library fc."""
    from flashy_amd import nn as fnn
    B, H, W, C, O = 16, 3, 3, 1024, 512
    assert 2 * B * C * O >= fnn._LINEAR_GEMM_CUTOFF
    x16, w32, b32, dy = _head_inputs(B, H, W, C, O, seed=9)
    HW = H * W
    x = x16.detach().requires_grad_(True)
    pooled = fnn._PoolFn.apply(x)
    g = torch.randn(B, C, device="cuda")
    pooled.backward(g)
    torch.cuda.synchronize()
    x64 = x16.double()
    _within("pooled", pooled, x64.mean((1, 2)),
            2 * HW * U32 * x64.abs().mean((1, 2)))
    ref_dx = (g.double() / HW)[:, None, None, :].expand(B, H, W, C)
    _within("pool dx", x.grad, ref_dx, (2 * U32 + U16) * ref_dx.abs())
    # whole large head against torch (rocBLAS fc: library tolerance)
    y = fnn.pool_linear(x16, w32, b32)
    ref = F.linear(x16.float().mean((1, 2)), w32, b32)
    assert torch.allclose(y, ref, atol=1e-3, rtol=1e-3)


@requires_gpu
def test_native_resnet18_head_capture_safe():
    """forward/backward/step under CapturedStep: the head's saved pooled
    buffer and the partials allocations must survive graph replay."""
    from flashy_amd.functional import cross_entropy
    from flashy_amd.graph import CapturedStep
    from flashy_amd.models import native_resnet18
    from flashy_amd.optim import FusedSGD
    torch.manual_seed(6)
    model = native_resnet18(10).cuda().train()
    opt = FusedSGD(model.parameters(), lr=0.01, momentum=0.9,
                   bf16_mirror=True)
    model.enable_wt_cache()
    x = torch.randn(8, 3, 32, 32, device="cuda")
    y = torch.randint(10, (8,), device="cuda")

    def step():
        opt.zero_grad()
        loss = cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        return loss

    graphed = CapturedStep(step, warmup=1).capture()
    losses = []
    for _ in range(2):
        losses.append(graphed().item())
    torch.cuda.synchronize()
    assert all(torch.isfinite(torch.tensor(losses))), losses
