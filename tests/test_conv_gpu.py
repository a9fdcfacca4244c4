# Copyright (c) Flashy-AMD authors.
"""GPU numerics tests for the NHWC implicit-GEMM conv and fused BN kernels,
each against a plain torch fp32 reference of the same op (inputs are
bf16-rounded first so only kernel arithmetic differs)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

SHAPES = [
    # (N, H, W, C, K, R, stride, pad)
    (4, 8, 8, 64, 64, 3, 1, 1),
    (2, 16, 16, 64, 128, 3, 2, 1),
    (2, 8, 8, 128, 128, 3, 1, 1),
    (2, 16, 16, 64, 128, 1, 2, 0),
    (2, 4, 4, 256, 512, 3, 2, 1),
    (3, 7, 5, 64, 64, 3, 1, 1),       # non-pow2 spatial, odd M tail
    (2, 16, 16, 64, 128, 4, 2, 1),    # even kernel, stride 2 (GAN shapes)
    (2, 32, 32, 3, 64, 7, 2, 3),      # ImageNet-style stem (C=3, chunked taps)
    # large-M shapes that engage the 8-wave deep-pipeline kernels
    (64, 28, 28, 128, 128, 3, 1, 1),  # fwd8/dgrad8 BN=128 + wgrad8
    (64, 29, 28, 128, 128, 3, 1, 1),  # same with an M tail (odd rows)
    (16, 56, 56, 256, 512, 1, 2, 0),  # 1x1 stride-2: dgrad8 SCAT2 scatter
    (64, 112, 112, 3, 64, 7, 2, 3),   # 224-class stem: padded fwd8 + wgrad
    (64, 7, 7, 512, 512, 3, 1, 1),    # r4_3x3: 8-wave split-K fwd/dgrad
]


def _mk(N, H, W, C, K, R, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(N, H, W, C, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(K, R, R, C, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    return x, w


def _torch_conv(x16, w16, stride, pad):
    # fp32 reference on the same bf16-rounded values, NCHW
    x = x16.float().permute(0, 3, 1, 2)
    w = w16.float().permute(0, 3, 1, 2)
    return F.conv2d(x, w, stride=stride, padding=pad)


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_conv_fwd(shape):
    from flashy_amd import ops
    N, H, W, C, K, R, stride, pad = shape
    x, w = _mk(N, H, W, C, K, R)
    d = ops.ConvDims.infer(x, w, stride, pad)
    y = x.new_empty((d.N, d.Ho, d.Wo, d.K))
    ops.conv_fwd(x, w, y, d)
    torch.cuda.synchronize()
    ref = _torch_conv(x, w, stride, pad).permute(0, 2, 3, 1)
    err = (y.float() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err / scale < 2e-2, (err, scale)


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES[:5] + SHAPES[6:])
def test_conv_dgrad(shape):
    from flashy_amd import ops
    N, H, W, C, K, R, stride, pad = shape
    x, w = _mk(N, H, W, C, K, R)
    d = ops.ConvDims.infer(x, w, stride, pad)
    g = torch.Generator(device="cuda").manual_seed(1)
    dy = torch.randn(N, d.Ho, d.Wo, K, device="cuda", generator=g).to(torch.bfloat16)

    dx = x.new_empty(x.shape)
    if C < 8:   # small-C edge path takes KRSC weights (as flashy_amd/nn.py)
        ops.conv_stem_dgrad(dy, w, dx, d)
    else:
        wt = w.new_empty((d.R, d.S, d.C, d.K))
        ops.weight_transpose(w, wt)
        ops.conv_dgrad(dy, wt, dx, d)
    torch.cuda.synchronize()

    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    ref = F.conv2d(xr, w.float().permute(0, 3, 1, 2), stride=stride, padding=pad)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    ref_dx = xr.grad.permute(0, 2, 3, 1)
    err = (dx.float() - ref_dx).abs().max().item()
    scale = ref_dx.abs().max().item() + 1e-6
    assert err / scale < 2e-2, (err, scale)


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES[:5] + SHAPES[6:])
def test_conv_wgrad(shape):
    from flashy_amd import ops
    N, H, W, C, K, R, stride, pad = shape
    x, w = _mk(N, H, W, C, K, R)
    d = ops.ConvDims.infer(x, w, stride, pad)
    g = torch.Generator(device="cuda").manual_seed(2)
    dy = torch.randn(N, d.Ho, d.Wo, K, device="cuda", generator=g).to(torch.bfloat16)

    dw = torch.zeros(K, R, R, C, device="cuda", dtype=torch.float32)
    ops.conv_wgrad(x, dy, dw, d)
    torch.cuda.synchronize()

    wr = w.float().permute(0, 3, 1, 2).requires_grad_(True)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), wr, stride=stride, padding=pad)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    ref_dw = wr.grad.permute(0, 2, 3, 1)
    err = (dw - ref_dw).abs().max().item()
    scale = ref_dw.abs().max().item() + 1e-6
    assert err / scale < 2e-2, (err, scale)


@requires_gpu
def test_conv_stem():
    from flashy_amd import ops
    N, H, W, C, K, R = 4, 32, 32, 3, 64, 3
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(N, H, W, C, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(K, R, R, C, device="cuda", generator=g) * 0.2).to(torch.bfloat16)
    d = ops.ConvDims.infer(x, w, 1, 1)
    y = x.new_empty((N, d.Ho, d.Wo, K))
    ops.conv_fwd(x, w, y, d)  # routes to the stem kernel (C=3)
    ref = _torch_conv(x, w, 1, 1).permute(0, 2, 3, 1)
    err = (y.float() - ref).abs().max().item()
    assert err / (ref.abs().max().item() + 1e-6) < 2e-2

    dy = torch.randn_like(ref).to(torch.bfloat16)
    dw = torch.zeros(K, R, R, C, device="cuda", dtype=torch.float32)
    ops.conv_wgrad(x, dy, dw, d)
    torch.cuda.synchronize()
    wr = w.float().permute(0, 3, 1, 2).requires_grad_(True)
    out = F.conv2d(x.float().permute(0, 3, 1, 2), wr, stride=1, padding=1)
    out.backward(dy.float().permute(0, 3, 1, 2))
    ref_dw = wr.grad.permute(0, 2, 3, 1)
    err = (dw - ref_dw).abs().max().item()
    assert err / (ref_dw.abs().max().item() + 1e-6) < 2e-2


@requires_gpu
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
def test_bn_fwd_bwd(relu, res):
    from flashy_amd import nn as fnn
    torch.manual_seed(4)
    N, H, W, C = 4, 8, 8, 64
    M = N * H * W
    x16 = torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16)
    r16 = torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16) if res else None

    bn = fnn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.mul_(1.5)
        bn.bias.add_(0.3)
    x = x16.detach().requires_grad_(True)
    rr = r16.detach().requires_grad_(True) if res else None
    y = bn(x, res=rr, relu=relu)
    dy = torch.randn_like(y).to(torch.bfloat16)
    y.backward(dy)

    # fp32 reference
    xr = x16.float().requires_grad_(True)
    g = bn.weight.detach().float().clone().requires_grad_(True)
    b = bn.bias.detach().float().clone().requires_grad_(True)
    flat = xr.reshape(M, C)
    mean = flat.mean(0)
    var = flat.var(0, unbiased=False)
    ref = (flat - mean) * torch.rsqrt(var + bn.eps) * g + b
    if res:
        ref = ref + r16.float().reshape(M, C)
    if relu:
        ref = torch.relu(ref)
    ref = ref.reshape(N, H, W, C)
    ref.backward(dy.float())

    tol = 5e-2
    assert (y.float() - ref).abs().max().item() < tol
    assert (x.grad.float() - xr.grad).abs().max().item() < tol
    assert torch.allclose(bn.weight.grad, g.grad, atol=1.0, rtol=2e-2)
    assert torch.allclose(bn.bias.grad, b.grad, atol=1.0, rtol=2e-2)
    if res:
        ref_dres = dy.float() * (ref > 0).float() if relu else dy.float()
        assert (rr.grad.float() - ref_dres).abs().max().item() < tol


@requires_gpu
def test_native_resnet18_matches_torch():
    from flashy_amd.models import native_resnet18, resnet18
    torch.manual_seed(5)
    twin = resnet18(num_classes=10, small_input=True).cuda().train()
    model = native_resnet18(10).cuda().train().from_torch(twin)
    x = torch.randn(8, 3, 32, 32, device="cuda")
    y = torch.randint(10, (8,), device="cuda")

    logits_n = model(x)
    loss_n = F.cross_entropy(logits_n, y)
    loss_n.backward()

    logits_t = twin(x)
    loss_t = F.cross_entropy(logits_t, y)
    loss_t.backward()

    # bf16 stack vs fp32 twin over 18 layers: compare scale-aware
    diff = (logits_n - logits_t).abs().max().item()
    spread = logits_t.std().item() + 1e-6
    assert diff / spread < 0.35, (diff, spread)
    assert abs(loss_n.item() - loss_t.item()) < 0.25, \
        (loss_n.item(), loss_t.item())
    # Early-layer weight grads of a bf16 stack legitimately drift from the
    # fp32 twin (long backward chains + ReLU mask flips).  Calibrate the
    # tolerance against the same twin run under bf16 autocast: our kernels
    # must not be much noisier than torch's own bf16 path.
    twin2 = resnet18(num_classes=10, small_input=True).cuda().train()
    twin2.load_state_dict(twin.state_dict())
    twin2.zero_grad()
    with torch.autocast("cuda", torch.bfloat16):
        logits_a = twin2(x)
    F.cross_entropy(logits_a.float(), y).backward()

    def _rel_cos(a, b):
        a, b = a.flatten(), b.flatten()
        rel = (a - b).norm().item() / (b.norm().item() + 1e-8)
        cos = torch.nn.functional.cosine_similarity(a, b, dim=0).item()
        return rel, cos

    gn = model.layer1[0].conv1.weight.grad.permute(0, 3, 1, 2)
    gt = twin.layer1[0].conv1.weight.grad
    ga = twin2.layer1[0].conv1.weight.grad
    ours_rel, ours_cos = _rel_cos(gn, gt)
    floor_rel, floor_cos = _rel_cos(ga, gt)
    assert ours_rel < max(2.5 * floor_rel, 0.05), (ours_rel, floor_rel)
    assert ours_cos > 1 - 2.5 * (1 - floor_cos) - 1e-3, (ours_cos, floor_cos)


@requires_gpu
def test_native_resnet_trains():
    from flashy_amd.models import native_resnet18
    from flashy_amd.optim import FusedSGD
    from flashy_amd.functional import cross_entropy
    torch.manual_seed(6)
    model = native_resnet18(10).cuda().train()
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9)
    x = torch.randn(32, 3, 32, 32, device="cuda")
    y = torch.randint(10, (32,), device="cuda")
    losses = []
    for i in range(12):
        logits = model(x)
        loss = cross_entropy(logits, y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0] * 0.7, losses  # overfits a fixed batch


@requires_gpu
def test_conv_fused_bn_stats():
    """The conv epilogue's fused BN partials must reproduce the standalone
    bn_stats sums (finalize consumes either)."""
    from flashy_amd import ops
    # single-pass path, but 64 to 128 tiles is under the 160-block floor of
    # every 8-wave plan: this exercises the 4-wave tile's stats epilogue
    # (the 8-wave epilogues are covered in test_conv8_gpu.py)
    N, H, W, C, K = 64, 16, 16, 64, 128
    x, w = _mk(N, H, W, C, K, 3)
    d = ops.ConvDims.infer(x, w, 1, 1)
    y = x.new_empty((d.N, d.Ho, d.Wo, d.K))
    stats = ops.conv_fwd(x, w, y, d, want_stats=True)
    assert stats is not None
    partials, msplit = stats
    torch.cuda.synchronize()
    s = partials[:K * msplit].view(K, msplit).sum(1)
    s2 = partials[K * msplit:].view(K, msplit).sum(1)
    # the fused path sums the fp32 accumulators BEFORE the bf16 store, so
    # it differs from sums of the rounded y by accumulated rounding noise:
    # tolerance ~ sqrt(M) * bf16_eps * max|y|
    yf = y.float().reshape(-1, K)
    M = yf.shape[0]
    tol = 0.02 * M ** 0.5 * yf.abs().max().item()
    assert (s - yf.sum(0)).abs().max().item() < tol, \
        ((s - yf.sum(0)).abs().max(), tol)
    tol2 = 0.02 * M ** 0.5 * (yf * yf).max().item()
    assert (s2 - (yf * yf).sum(0)).abs().max().item() < tol2, \
        ((s2 - (yf * yf).sum(0)).abs().max(), tol2)


def _fuzz_shapes(n=24, seed=1234):
    """Deterministic random sample of the supported conv envelope
    (C,K multiples of 64, R in {1,3,5}, stride in {1,2}) — regression net
    for the dispatch chain (dedup / mloop / fwd8 / split-K under-fill
    forcing / SCAT2 / s2-parity / old-tile fallbacks)."""
    import random
    rng = random.Random(seed)
    shapes = []
    while len(shapes) < n:
        C = 64 * rng.choice([1, 1, 2, 3, 4])
        K = 64 * rng.choice([1, 1, 2, 3, 4])
        R = rng.choice([1, 1, 3, 3, 5])
        stride = rng.choice([1, 1, 2])
        pad = R // 2 if R > 1 else 0
        N = rng.choice([1, 2, 3, 8])
        H = rng.randint(4, 36)
        W = rng.randint(4, 36)
        Ho = (H + 2 * pad - R) // stride + 1
        Wo = (W + 2 * pad - R) // stride + 1
        if Ho < 1 or Wo < 1:
            continue
        shapes.append((N, H, W, C, K, R, stride, pad))
    # two large-M entries to engage the 8-wave family + under-fill split-K
    shapes.append((64, 14, 14, 256, 256, 3, 1, 1))
    shapes.append((64, 14, 14, 1024, 256, 1, 1, 0))
    return shapes


@requires_gpu
@pytest.mark.parametrize("shape", _fuzz_shapes())
def test_conv_fuzz(shape):
    from flashy_amd import ops
    N, H, W, C, K, R, stride, pad = shape
    x, w = _mk(N, H, W, C, K, R, seed=hash(shape) & 0xffff)
    d = ops.ConvDims.infer(x, w, stride, pad)
    g = torch.Generator(device="cuda").manual_seed(5)
    dy = torch.randn(N, d.Ho, d.Wo, K, device="cuda", generator=g).to(torch.bfloat16)

    y = x.new_empty((d.N, d.Ho, d.Wo, d.K))
    ops.conv_fwd(x, w, y, d)
    dx = x.new_empty(x.shape)
    wt = w.new_empty((d.R, d.S, d.C, d.K))
    ops.weight_transpose(w, wt)
    ops.conv_dgrad(dy, wt, dx, d)
    dw = torch.zeros(K, R, R, C, device="cuda", dtype=torch.float32)
    ops.conv_wgrad(x, dy, dw, d)
    torch.cuda.synchronize()

    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.float().permute(0, 3, 1, 2).requires_grad_(True)
    ref = F.conv2d(xr, wr, stride=stride, padding=pad)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    for got, want, tag in [
            (y.float(), ref.detach().permute(0, 2, 3, 1), "fwd"),
            (dx.float(), xr.grad.permute(0, 2, 3, 1), "dgrad"),
            (dw, wr.grad.permute(0, 2, 3, 1), "wgrad")]:
        err = (got - want).abs().max().item()
        scale = want.abs().max().item() + 1e-6
        assert err / scale < 2e-2, (tag, err, scale, shape)
