# Copyright (c) Flashy-AMD authors.
"""Edge cases of the 8-wave deep-pipeline conv family (k_conv_fwd8,
k_conv1x1_mloop, k_conv_dedup, k_conv_dgrad8 with SCAT2 / split-K), run
through the public ops.conv_fwd / ops.conv_dgrad.

Every case first asserts that its shape really reaches the intended kernel,
so a dispatch change cannot quietly turn it into a test of the 4-wave
fallback.  Reference: fp32 F.conv2d (and its autograd) on the bf16-rounded
inputs; tolerance max-abs error / max-abs reference < 2e-2; BN partials
within 0.02*sqrt(M)*max|y| (resp. max y^2) of the sums over the stored y.

Shapes are (N, H, W, C, K, R, stride, pad), the smallest that reach each
pipeline edge (stage counts 1..5 at prefetch depth 2, 1..3 at depth 1,
m-tile tails, XCD-remap and no-remap grids).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")


@functools.lru_cache(maxsize=None)
def _fwd_case(shape):
    """(x, w, dims, fp32 reference y in NHWC) — computed once per shape."""
    from flashy_amd import ops
    N, H, W, C, K, R, stride, pad = shape
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(N, H, W, C, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(K, R, R, C, device="cuda", generator=g) * 0.1
         ).to(torch.bfloat16)
    d = ops.ConvDims.infer(x, w, stride, pad)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2),
                   stride=stride, padding=pad).permute(0, 2, 3, 1)
    return x, w, d, ref


def _check(got, want):
    err = (got.float() - want).abs().max().item()
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


def _run_fwd(shape, relu=False, stats=False, want_msplit=None):
    from flashy_amd import ops
    x, w, d, ref = _fwd_case(shape)
    y = x.new_empty((d.N, d.Ho, d.Wo, d.K))
    out = ops.conv_fwd(x, w, y, d, relu=relu, want_stats=stats)
    torch.cuda.synchronize()
    if stats:
        partials, msplit = out
        if want_msplit is not None:
            assert msplit == want_msplit, (msplit, want_msplit)
        _check_partials(partials, msplit, y, d.K)
    _check(y, torch.relu(ref) if relu else ref)


def _run_dgrad(shape):
    from flashy_amd import ops
    N, H, W, C, K, R, stride, pad = shape
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(N, H, W, C, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(K, R, R, C, device="cuda", generator=g) * 0.1
         ).to(torch.bfloat16)
    d = ops.ConvDims.infer(x, w, stride, pad)
    dy = torch.randn(N, d.Ho, d.Wo, K, device="cuda", generator=g
                     ).to(torch.bfloat16)
    dx = torch.full_like(x, float("nan"))   # every element must be written
    wt = w.new_empty((d.R, d.S, d.C, d.K))
    ops.weight_transpose(w, wt)
    ops.conv_dgrad(dy, wt, dx, d)
    torch.cuda.synchronize()
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    F.conv2d(xr, w.float().permute(0, 3, 1, 2), stride=stride,
             padding=pad).backward(dy.float().permute(0, 3, 1, 2))
    _check(dx, xr.grad.permute(0, 2, 3, 1))


def _dims(shape):
    from flashy_amd import ops
    N, H, W, C, K, R, stride, pad = shape
    Ho = (H + 2 * pad - R) // stride + 1
    Wo = (W + 2 * pad - R) // stride + 1
    return ops.ConvDims(N, H, W, C, K, R, R, Ho, Wo, stride, pad)


def _assert_conv8(shape, dgrad):
    from flashy_amd import ops
    assert ops.require().conv8_eligible(*_dims(shape), dgrad), shape


def _assert_splitk8(shape, dgrad, want_spz, want_last):
    """The shape is sliced over grid.z by ops.conv_fwd / ops.conv_dgrad and
    the slices fill the 8-wave split-K launcher's 120-block floor."""
    from flashy_amd import ops
    d = _dims(shape)
    assert not ops.require().conv8_eligible(*d, dgrad), shape
    M = d.N * d.H * d.W if dgrad else d.N * d.Ho * d.Wo
    cols = d.C if dgrad else d.K
    stages = d.R * d.S * (d.K if dgrad else d.C) // 64
    # zn as ops.conv_fwd / ops.conv_dgrad derive it, from the same helpers
    zn = ops._splitk_plan(M, cols // 64, stages)
    if zn == 0 and (d.stride == 1 or not dgrad):
        zn = ops._underfill_zn(M, cols, stages)
    assert zn >= 2, (shape, zn)
    spz = (stages + zn - 1) // zn
    zeff = (stages + spz - 1) // spz
    # launch_conv_{fwd,dgrad}_splitk take the 8-wave kernel from 120 blocks
    bn = 128 if cols % 128 == 0 else 64
    tiles8 = (M + 255) // 256 * (cols // bn)
    assert tiles8 * zeff >= 120, (shape, tiles8, zeff)
    assert (spz, stages - (zeff - 1) * spz) == (want_spz, want_last), \
        (shape, spz, stages, zeff)


# --- fwd8: 1x1 stride-2 convs never route to mloop or dedup -----------------
# BN=64 (prefetch depth 2): 56 m-tiles (32-row tail, XCD remap), 1/2/3/5 stages
FWD8_BN64 = [(8, 84, 84, C, 192, 1, 2, 0) for C in (64, 128, 192, 320)]
# BN=128 (depth 1): 82 m-tiles (72-row tail, no remap), 1/2/3 stages
FWD8_BN128 = [(8, 102, 102, C, 256, 1, 2, 0) for C in (64, 128, 192)]


@requires_gpu
@pytest.mark.parametrize("shape", FWD8_BN64 + FWD8_BN128)
def test_fwd8(shape):
    _assert_conv8(shape, False)
    _run_fwd(shape)


@requires_gpu
@pytest.mark.parametrize("shape", [FWD8_BN64[2], FWD8_BN128[1]])
def test_fwd8_relu(shape):
    _assert_conv8(shape, False)
    _run_fwd(shape, relu=True)


@requires_gpu
@pytest.mark.parametrize("shape", [FWD8_BN64[2], FWD8_BN128[1]])
def test_fwd8_stats(shape):
    _assert_conv8(shape, False)
    d = _dims(shape)
    _run_fwd(shape, stats=True,
             want_msplit=(d.N * d.Ho * d.Wo + 255) // 256)


# --- mloop: 131 tiles with a tail; ntl = 1, 1-2, 2-3 tiles per block --------
MLOOP = [(9, 61, 61, 64, K, 1, 1, 0) for K in (64, 192, 512)]
MLOOP_MSPLIT = 2 * ((9 * 61 * 61 + 255) // 256)


@requires_gpu
@pytest.mark.parametrize("shape", MLOOP)
def test_mloop(shape):
    # stats on every K: msplit == 2*mtiles is the proof the m-loop kernel ran
    _run_fwd(shape, stats=True, want_msplit=MLOOP_MSPLIT)


@requires_gpu
def test_mloop_relu():
    from flashy_amd import ops
    assert ops.require().conv_fwd_msplit(*_dims(MLOOP[1])) == MLOOP_MSPLIT
    _run_fwd(MLOOP[1], relu=True)


# --- dedup: per-image 256-pixel tiles, msplit == N * tiles-per-image --------
@requires_gpu
@pytest.mark.parametrize("shape", [
    pytest.param((32, 34, 34, 64, 64, 3, 1, 1), id="C64"),
    pytest.param((32, 34, 34, 128, 128, 3, 1, 1), id="C128"),  # 147 KiB LDS
])
def test_dedup(shape):
    N, H, W = shape[:3]
    _run_fwd(shape, stats=True, want_msplit=N * ((H * W + 255) // 256))


# --- dgrad8 ------------------------------------------------------------------
DGRAD8 = (
    # BN=64, 1/2/3 stages
    [(8, 42, 42, 192, K, 1, 1, 0) for K in (64, 128, 192)] +
    # BN=128, 1/2 stages (82 tiles < mloop's 128-tile floor at K=64)
    [(8, 51, 51, 256, K, 1, 1, 0) for K in (64, 128)] +
    # SCAT2 at BN=128.  No binding exposes conv_dgrad8_s2_plan, so by hand:
    # even H/W, Mq = 8*29*29 = 6728 -> 27 m-tiles x (512/128 = 4) = 108
    # blocks >= the plan's 104 floor (conv8_eligible below is the generic
    # dgrad8 plan, which launch_conv_dgrad consults only after the s2 plan)
    [(8, 58, 58, 512, 64, 1, 2, 0)] +
    # S1=false (per-tap exact-division check): 1x1 stride-2 with odd H/W,
    # which the SCAT2 plan (even sizes only) and the parity kernel (no 1x1)
    # both decline, so the generic plan takes them: 58 tiles x 3 = 174 at
    # BN=64 and 82 tiles x 2 = 164 at BN=128, both >= 160
    [(8, 43, 43, 192, 64, 1, 2, 0), (8, 51, 51, 256, 64, 1, 2, 0)]
)


@requires_gpu
@pytest.mark.parametrize("shape", DGRAD8)
def test_dgrad8(shape):
    _assert_conv8(shape, True)
    _run_dgrad(shape)


# --- 8-wave split-K ------------------------------------------------------------
@requires_gpu
def test_splitk8_fwd_bn64():
    shape = (64, 7, 7, 512, 192, 3, 1, 1)     # 72 stages: 4 x 15 + 12
    _assert_splitk8(shape, False, 15, 12)
    _run_fwd(shape)
    _run_fwd(shape, stats=True)               # combine-with-stats sibling


@requires_gpu
@pytest.mark.parametrize("shape,spz,last", [
    ((64, 7, 7, 512, 192, 3, 1, 1), 9, 9),    # BN=128 over C, forced zn=3
    ((64, 7, 7, 192, 512, 3, 1, 1), 15, 12),  # BN=64 over C, short last slice
    ((8, 16, 16, 192, 512, 3, 2, 1), 15, 12),  # stride 2: S1=false split-K
])
def test_splitk8_dgrad(shape, spz, last):
    _assert_splitk8(shape, True, spz, last)
    _run_dgrad(shape)
