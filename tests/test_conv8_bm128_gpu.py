# Copyright (c) Flashy-AMD authors.
"""The 128-row tile of the 8-wave conv family (k_conv_fwd8 / k_conv_dgrad8
with BM = 128), forced by name through ops.conv8_form and the "par8m128"
stride-2 form, whatever the plan would pick.

Reference: float64 F.conv2d (and its autograd) on the bf16-rounded inputs;
bound as in test_conv8_gpu.py: max-abs error / max-abs reference < 2e-2, BN
partials within 0.02*sqrt(M)*max|y| (resp. max y^2) of the sums over the
stored y.  Every case checks the whole output (dx starts as NaN).

Shapes are (N, H, W, C, K, R, stride, pad), the smallest that reach each
edge: M = 144 (a full 128-row tile and a ragged one), M = 961 (8 tiles, the
XCD block order), both BN, 1 / 2 / 9 / 18 stages against the prefetch depth
of 2, odd 7x7 inputs for the parity classes.

The CPU half checks that the plan still gives 256-row tiles to every shape
that had them.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from flashy_amd import ops

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")
gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(x, w, wt, dy, dims, float64 y, float64 dx), computed once per shape."""
    N, H, W, C, K, R, stride, pad = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(K, R, R, C, generator=g) * 0.1).to(torch.bfloat16)
    d = ops.ConvDims.infer(x, w, stride, pad)
    dy = torch.randn(N, d.Ho, d.Wo, K, generator=g).to(torch.bfloat16)
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    y = F.conv2d(xr, w.double().permute(0, 3, 1, 2), stride=stride,
                 padding=pad)
    y.backward(dy.double().permute(0, 3, 1, 2))
    xg, wg, dyg = x.cuda(), w.cuda(), dy.cuda()
    wt = wg.new_empty((d.R, d.S, d.C, d.K))
    ops.weight_transpose(wg, wt)
    return (xg, wg, wt, dyg, d, y.detach().permute(0, 2, 3, 1).cuda(),
            xr.grad.permute(0, 2, 3, 1).cuda())


def _check(got, want):
    err = (got.double() - want).abs().max().item()
    scale = want.abs().max().item() + 1e-6
    print(f"err/scale = {err / scale:.3e}")
    assert err / scale < 2e-2, (err, scale)


def _check_partials(partials, msplit, y, K):
    s = partials[:K * msplit].view(K, msplit).sum(1)
    s2 = partials[K * msplit:].view(K, msplit).sum(1)
    yf = y.float().reshape(-1, K)
    M = yf.shape[0]
    e1 = (s - yf.sum(0)).abs().max().item()
    e2 = (s2 - (yf * yf).sum(0)).abs().max().item()
    tol = 0.02 * M ** 0.5 * yf.abs().max().item()
    tol2 = 0.02 * M ** 0.5 * (yf * yf).max().item()
    print(f"sum err {e1:.3e} (tol {tol:.3e}), sq err {e2:.3e} (tol {tol2:.3e})")
    assert e1 < tol, (e1, tol)
    assert e2 < tol2, (e2, tol2)


# (shape, BN)
FWD = [
    ((1, 12, 12, 64, 64, 3, 1, 1), 64),      # M=144, 9 stages
    ((1, 12, 12, 128, 128, 3, 1, 1), 128),   # 18 stages
    ((1, 12, 12, 128, 64, 1, 1, 0), 64),     # 1x1, 2 stages = the depth
    ((1, 12, 12, 64, 128, 1, 1, 0), 128),    # 1x1, 1 stage < the depth
    ((3, 17, 17, 64, 128, 3, 2, 1), 128),    # stride 2, M=243
    ((1, 31, 31, 64, 64, 1, 1, 0), 64),      # M=961: 8 tiles, XCD order
]


@gpu
@requires_gpu
@pytest.mark.parametrize("shape,bn", FWD)
def test_fwd_bm128(shape, bn):
    x, w, _, _, d, yref, _ = _case(shape)
    M = d.N * d.Ho * d.Wo
    mtiles = (M + 127) // 128
    y = torch.full((d.N, d.Ho, d.Wo, d.K), float("nan"), device="cuda",
                   dtype=torch.bfloat16)
    partials = torch.full((2 * d.K * mtiles,), float("nan"), device="cuda")
    msplit = ops.conv8_form(x, w, y, d, False, 128, bn, bn_ws=partials)
    torch.cuda.synchronize()
    assert msplit == mtiles   # one partial per 128-row tile
    _check(y, yref)
    _check_partials(partials, msplit, y, d.K)


DGRAD = [
    ((1, 12, 12, 64, 64, 3, 1, 1), 64),
    ((1, 12, 12, 128, 128, 3, 1, 1), 128),
    ((1, 12, 12, 64, 128, 1, 1, 0), 64),     # 1x1: 2 stages over K
    ((3, 17, 17, 128, 64, 3, 2, 1), 128),    # stride 2: per-tap division
    ((1, 31, 31, 64, 64, 1, 1, 0), 64),      # 8 tiles, XCD order
]


@gpu
@requires_gpu
@pytest.mark.parametrize("shape,bn", DGRAD)
def test_dgrad_bm128(shape, bn):
    x, _, wt, dy, d, _, dxref = _case(shape)
    dx = torch.full_like(x, float("nan"))
    ops.conv8_form(dy, wt, dx, d, True, 128, bn)
    torch.cuda.synchronize()
    _check(dx, dxref)


# 7x7 inputs: class extents 4x4 / 4x3 / 3x4 / 3x3 (x 9 images = 144 .. 81
# rows, so the second tile of the short classes exits at the extent guard);
# the 1x1 filter leaves three classes without a tap (zeros)
@gpu
@requires_gpu
@pytest.mark.parametrize("shape,bn", [
    ((9, 7, 7, 64, 128, 3, 2, 1), 64),
    ((9, 7, 7, 128, 64, 3, 2, 1), 128),
    ((9, 7, 7, 64, 64, 1, 2, 0), 64),
])
def test_par2_dgrad_bm128(shape, bn):
    x, _, wt, dy, d, _, dxref = _case(shape)
    dx = torch.full_like(x, float("nan"))
    ops.conv_dgrad_s2_form(dy, wt, dx, d, "par8m128", bn)
    torch.cuda.synchronize()
    _check(dx, dxref)


# split-K: (shape, BN, spz).  9 stages at spz 4 = slices of 4, 4 and 1 (a
# short last slice, below the prefetch depth: the peeled tail); 2 stages at
# spz 1 = every slice below the depth; 18 at spz 5 = 5, 5, 5, 3
SPLITK = [
    ((1, 12, 12, 64, 64, 3, 1, 1), 64, 4),
    ((1, 12, 12, 128, 128, 3, 1, 1), 128, 5),
    ((1, 12, 12, 128, 128, 1, 1, 0), 128, 1),
]


@gpu
@requires_gpu
@pytest.mark.parametrize("shape,bn,spz", SPLITK)
@pytest.mark.parametrize("dgrad", [False, True])
def test_splitk_bm128(shape, bn, spz, dgrad):
    x, w, wt, dy, d, yref, dxref = _case(shape)
    M = d.N * d.H * d.W if dgrad else d.N * d.Ho * d.Wo
    cols = d.C if dgrad else d.K
    stages = d.R * d.S * (d.K if dgrad else d.C) // 64
    zeff = (stages + spz - 1) // spz
    assert zeff >= 2
    ws = torch.full((zeff * M * cols,), float("nan"), device="cuda")
    out = torch.full((M, cols), float("nan"), device="cuda",
                     dtype=torch.bfloat16)
    if dgrad:
        ops.conv8_form(dy, wt, ws, d, True, 128, bn, spz=spz)
    else:
        ops.conv8_form(x, w, ws, d, False, 128, bn, spz=spz)
    ops.splitk_combine(ws, out, zeff)
    torch.cuda.synchronize()
    _check(out.view((dxref if dgrad else yref).shape), dxref if dgrad else yref)


@gpu
@requires_gpu
def test_splitk_bm128_combine_stats_bitwise():
    """Slices of the 128-row kernel through k_splitk_combine_stats: its
    partials are bitwise k_bn_stats on the y it wrote."""
    shape, bn, spz = SPLITK[0]
    x, w, _, _, d, yref, _ = _case(shape)
    M = d.N * d.Ho * d.Wo
    zeff = (d.R * d.S * d.C // 64 + spz - 1) // spz
    ws = torch.empty(zeff * M * d.K, device="cuda")
    ops.conv8_form(x, w, ws, d, False, 128, bn, spz=spz)
    msplit = ops.bn_msplit(M, d.K)
    y = torch.empty((d.N, d.Ho, d.Wo, d.K), device="cuda",
                    dtype=torch.bfloat16)
    partials = torch.empty(2 * d.K * msplit, device="cuda")
    ops.require().splitk_combine_stats(ws.data_ptr(), y.data_ptr(),
                                       partials.data_ptr(), M, d.K, zeff,
                                       msplit, ops._stream())
    ref = torch.empty_like(partials)
    ops.bn_stats(y, ref, M, d.K, msplit)
    torch.cuda.synchronize()
    _check(y, yref)
    assert torch.equal(partials, ref)


@gpu
@requires_gpu
def test_forms_refuse_what_they_cannot_run():
    x, w, wt, dy, d, _, _ = _case(FWD[0][0])       # C = K = 64
    y = torch.empty((d.N, d.Ho, d.Wo, d.K), device="cuda",
                    dtype=torch.bfloat16)
    for bm, bn in ((64, 64), (128, 32), (128, 128)):
        with pytest.raises(ValueError):
            ops.conv8_form(x, w, y, d, False, bm, bn)
    with pytest.raises(ValueError):   # stride 1 has no parity classes
        ops.conv_dgrad_s2_form(dy, wt, torch.empty_like(x), d, "par8m128", 64)


# --- CPU: the plan keeps 256-row tiles wherever it had them -------------------
def _old_plan(rows, channels, floor=160):
    """The single-pass rule before the 128-row tile: (bn, grid.x) or None."""
    mt = (rows + 255) // 256
    if channels % 128 == 0 and mt * (channels // 128) >= floor:
        return 128, mt
    if mt * (channels // 64) >= floor:
        return 64, mt
    return None


def test_plan_keeps_256_rows():
    ext = ops.require()
    seen = 0
    for N in (8, 64, 256):
        for hw in (4, 7, 8, 14, 16, 28, 32, 56):
            for C, K in ((64, 64), (64, 256), (128, 128), (192, 64),
                         (256, 256), (256, 1024), (512, 512), (512, 2048)):
                for R, stride in ((1, 1), (3, 1), (3, 2), (1, 2)):
                    pad = R // 2
                    Ho = (hw + 2 * pad - R) // stride + 1
                    d = ops.ConvDims(N, hw, hw, C, K, R, R, Ho, Ho, stride,
                                     pad)
                    for dgrad in (False, True):
                        rows = N * hw * hw if dgrad else N * Ho * Ho
                        old = _old_plan(rows, C if dgrad else K)
                        bm, bn, mt = ext.conv8_plan(*d, dgrad)
                        if old is not None:
                            assert (bm, bn, mt) == (256,) + old, (d, dgrad)
                            seen += 1
                        else:   # and no shape gained a single-pass route
                            assert (bm, bn, mt) == (0, 0, 0), (d, dgrad)
    assert seen > 100


def test_splitk_tile_large_m_is_256():
    ext = ops.require()
    # the shapes the 8-wave split-K already served: r50 layer4 at 224 px
    # (52 blocks of 256 x 128) and the 7x7x192 edge cases of test_conv8_gpu
    for rows, ch in ((3136, 512), (3136, 192), (12544, 256)):
        assert ext.conv8_splitk_tile(rows, ch)[:2] == \
            (256, 128 if ch % 128 == 0 else 64), (rows, ch)
    # under 33 blocks of 256 rows: the flagship's layer3 / layer4 3x3 convs
    assert ext.conv8_splitk_tile(4096, 256)[:2] == (128, 128)
    assert ext.conv8_splitk_tile(1024, 512)[:2] == (128, 128)
