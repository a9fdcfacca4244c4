# Copyright (c) Flashy-AMD authors.
"""Stride-2 backward-data forms (csrc/conv_dgrad8.hip PAR2 / SCAT2,
csrc/conv_dgrad.hip k_conv_dgrad_s2) against a float64 CPU reference built
from the bf16-rounded inputs.

Metric: max |dx - ref| / max |ref|.  dx is an fp32 sum rounded once to bf16,
so the bound is 2^-8: half a bf16 ulp at the largest element (2^-9), doubled
for the fp32 accumulation over at most 4608 terms.  Every form is forced
explicitly through ops.conv_dgrad_s2_form, dx is NaN-filled first so a pixel
no block writes shows up, and each form's error may exceed that of the
generic zero-filled kernel on the same inputs by at most a factor of 2.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

BOUND = 2.0 ** -8

# (N, H, W, C, K, R, stride, pad)
SHAPES = {
    "base": (2, 8, 8, 64, 64, 3, 2, 1),        # all four classes populated
    "odd": (3, 7, 5, 64, 128, 3, 2, 1),        # class sizes differ; row tails
    "m512": (2, 16, 16, 64, 128, 3, 2, 1),     # partial 256-row class tile
    "bn128": (2, 8, 8, 128, 64, 3, 2, 1),      # BN = 128
    "longk": (2, 8, 8, 256, 512, 3, 2, 1),     # 32-stage class, peeled tail
    "1x1": (2, 8, 8, 64, 128, 1, 2, 0),        # three empty classes -> zeros
    "1x1b": (2, 6, 10, 128, 256, 1, 2, 0),     # same, second size
    "pad": (1, 4, 4, 64, 64, 3, 2, 1),         # one tile, mostly padding
    # 320 rows per class: a full 256-row tile plus a partial one, and class
    # blocks past the first in grid.x
    "tiles2": (5, 16, 16, 64, 64, 3, 2, 1),
}


def _forms(shape):
    N, H, W, C, K, R, stride, pad = shape
    forms = [("par8", 64), ("par4", 32), ("par4", 64), ("par4", 128)]
    if C % 128 == 0:
        forms.append(("par8", 128))
    if R == 1:
        forms.append(("scat2", 64))
        if C % 128 == 0:
            forms.append(("scat2", 128))
    return forms


CASES = [pytest.param(name, form, tile, id=f"{name}-{form}{tile}")
         for name, shape in SHAPES.items() for form, tile in _forms(shape)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(dy, wt, dims, float64 reference, max |ref|, generic kernel's error)
    for one shape, computed once."""
    from flashy_amd import ops
    N, H, W, C, K, R, stride, pad = SHAPES[name]
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(K, R, R, C, generator=g) * 0.1).to(torch.bfloat16)
    Ho = (H + 2 * pad - R) // stride + 1
    Wo = (W + 2 * pad - R) // stride + 1
    dy = torch.randn(N, Ho, Wo, K, generator=g).to(torch.bfloat16)
    d = ops.ConvDims(N, H, W, C, K, R, R, Ho, Wo, stride, pad)
    oph = H - ((Ho - 1) * stride - 2 * pad + R)
    opw = W - ((Wo - 1) * stride - 2 * pad + R)
    ref = F.conv_transpose2d(
        dy.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2),
        stride=stride, padding=pad, output_padding=(oph, opw),
    ).permute(0, 2, 3, 1).contiguous()
    assert ref.shape == (N, H, W, C)
    dy, w = dy.cuda(), w.cuda()
    wt = w.new_empty((R, R, C, K))
    ops.weight_transpose(w, wt)
    scale = ref.abs().max().item()
    err_gen = _error(lambda dx: ops.conv_dgrad_s2_form(dy, wt, dx, d,
                                                       "generic", 0),
                     d, ref, scale)
    return dy, wt, d, ref, scale, err_gen


def _error(run, d, ref, scale):
    dx = torch.full((d.N, d.H, d.W, d.C), float("nan"),
                    dtype=torch.bfloat16, device="cuda")
    run(dx)
    torch.cuda.synchronize()
    got = dx.cpu().double()
    assert not torch.isnan(got).any(), \
        f"{int(torch.isnan(got).sum())} elements of dx were not written"
    return (got - ref).abs().max().item() / scale


def _check(name, label, err):
    err_gen = _case(name)[5]
    print(f"{name} {label}: err {err:.3e}  generic {err_gen:.3e}  "
          f"bound {BOUND:.3e}")
    assert err_gen < BOUND, (name, "generic", err_gen)
    assert err < BOUND, (name, label, err)
    assert err <= 2 * err_gen, (name, label, err, err_gen)


@requires_gpu
@pytest.mark.parametrize("name,form,tile", CASES)
def test_form(name, form, tile):
    from flashy_amd import ops
    dy, wt, d, ref, scale, _ = _case(name)
    err = _error(lambda dx: ops.conv_dgrad_s2_form(dy, wt, dx, d, form, tile),
                 d, ref, scale)
    _check(name, f"{form}{tile}", err)


@requires_gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_planned_dispatch(name):
    """ops.conv_dgrad itself (whatever the plan picks for the small shape)."""
    from flashy_amd import ops
    dy, wt, d, ref, scale, _ = _case(name)
    err = _error(lambda dx: ops.conv_dgrad(dy, wt, dx, d), d, ref, scale)
    _check(name, "plan:%s%d" % ops.conv_dgrad_s2_plan(d), err)


@requires_gpu
def test_forms_decline_what_they_cannot_run():
    from flashy_amd import ops
    dy, wt, d, *_ = _case("base")          # 3x3: no SCAT2; C = 64: no BN 128
    dx = torch.empty((d.N, d.H, d.W, d.C), dtype=torch.bfloat16,
                     device="cuda")
    for form, tile in (("scat2", 64), ("par8", 128), ("par8", 32),
                       ("par4", 256)):
        with pytest.raises(ValueError):
            ops.conv_dgrad_s2_form(dy, wt, dx, d, form, tile)


# The flagship's six stride-2 dgrad calls (ResNet-18, 32x32, batch 64) and the
# form docs/kernels.md documents for each (profiles/r05a_dgrad_s2_sweep.txt).
FLAGSHIP_PLAN = {
    (64, 32, 32, 64, 128, 3, 2, 1): ("par8", 64),
    (64, 16, 16, 128, 256, 3, 2, 1): ("par4", 32),
    (64, 8, 8, 256, 512, 3, 2, 1): ("par4", 32),
    (64, 32, 32, 64, 128, 1, 2, 0): ("none", 0),
    (64, 16, 16, 128, 256, 1, 2, 0): ("par4", 32),
    (64, 8, 8, 256, 512, 1, 2, 0): ("par4", 32),
}


@requires_gpu
@pytest.mark.parametrize("shape", list(FLAGSHIP_PLAN))
def test_flagship_plan(shape):
    from flashy_amd import ops
    N, H, W, C, K, R, stride, pad = shape
    Ho = (H + 2 * pad - R) // stride + 1
    Wo = (W + 2 * pad - R) // stride + 1
    d = ops.ConvDims(N, H, W, C, K, R, R, Ho, Wo, stride, pad)
    assert ops.conv_dgrad_s2_plan(d) == FLAGSHIP_PLAN[shape]
