# Copyright (c) Flashy-AMD authors.
"""GPU tests for the wave-group wgrad (csrc/conv_wgrad.hip): MG wave groups
per block each reduce their own m-range, the block sums the MG tiles in LDS
and adds full 256-byte rows to dw; a tile with one adder block does a plain
load-add-store.

Reference: torch conv2d backward in float64 on the same bf16-rounded inputs.
dw starts as non-zero random fp32 and every case calls the kernel twice, so
the expected result is ``init + 2 * grad`` (accumulate semantics).

Two bounds per case: the suite-wide ``2e-2 * max|ref|`` and a tight one, 4x
the relative error (max |dw - expected| / max|grad|) that the parent
commit's kernel (89a354a, one fp32 atomicAdd per accumulator element) gave
on the same inputs on an MI355X — a dropped 1-row tail hides under 2e-2 but
not under this.  The 4x covers the different fp32 summation order only.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

S_BODY = (4, 8, 8, 64, 64, 3, 1, 1)       # M=256
S_ODD = (3, 7, 5, 64, 64, 3, 1, 1)        # M=105: shorter than one range
S_1X1 = (2, 16, 16, 64, 128, 1, 2, 0)     # 1x1 stride 2, rsc = one tile
S_L4S2 = (2, 4, 4, 256, 512, 3, 2, 1)
S_L4 = (2, 4, 4, 512, 512, 3, 1, 1)       # k_conv_wgrad8 (tiles8 >= 100), M=32

# (shape, n_splits) -> relative error of the parent commit 89a354a, measured
# once on an MI355X with _rel_err below (same seeds, same two calls).
PARENT_ERR = {
    (S_BODY, 1): 3.6227e-07,
    (S_BODY, 2): 2.9089e-07,
    (S_BODY, 3): 2.9089e-07,
    (S_BODY, 4): 3.3289e-07,
    (S_BODY, 5): 2.2829e-07,
    (S_BODY, 8): 3.3289e-07,
    (S_ODD, 1): 2.6069e-07,
    (S_ODD, 2): 1.5586e-07,
    (S_ODD, 4): 1.5586e-07,
    (S_1X1, None): 3.0181e-07,
    (S_L4S2, None): 1.5092e-07,
    (S_L4, None): 2.3942e-07,
}
CASES = list(PARENT_ERR)

_cache = {}


def _inputs(shape):
    """x, dy (bf16), the non-zero start of dw (fp32), the float64 gradient;
    computed once per shape and shared (never modified) by all tests."""
    if shape not in _cache:
        from flashy_amd import ops
        N, H, W, C, K, R, stride, pad = shape
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn(N, H, W, C, device="cuda", generator=g).to(torch.bfloat16)
        w = (torch.randn(K, R, R, C, device="cuda", generator=g) * 0.1
             ).to(torch.bfloat16)
        d = ops.ConvDims.infer(x, w, stride, pad)
        g = torch.Generator(device="cuda").manual_seed(2)
        dy = torch.randn(N, d.Ho, d.Wo, K, device="cuda",
                         generator=g).to(torch.bfloat16)
        init = torch.randn(K, R, R, C, device="cuda", generator=g)
        wr = w.double().permute(0, 3, 1, 2).requires_grad_(True)
        out = F.conv2d(x.double().permute(0, 3, 1, 2), wr, stride=stride,
                       padding=pad)
        out.backward(dy.double().permute(0, 3, 1, 2))
        grad = wr.grad.permute(0, 2, 3, 1).contiguous()
        _cache[shape] = (x, dy, d, init, grad)
    return _cache[shape]


def _run(shape, n_splits, calls=2):
    from flashy_amd import ops
    x, dy, d, init, _ = _inputs(shape)
    dw = init.clone()
    for _ in range(calls):
        ops.conv_wgrad(x, dy, dw, d, n_splits=n_splits)
    torch.cuda.synchronize()
    return dw


def _rel_err(shape, n_splits):
    _, _, _, init, grad = _inputs(shape)
    dw = _run(shape, n_splits)
    err = (dw.double() - (init.double() + 2 * grad)).abs().max().item()
    return err / grad.abs().max().item()


def _check(shape, n_splits):
    rel = _rel_err(shape, n_splits)
    parent = PARENT_ERR[(shape, n_splits)]
    print(f"wgrad {shape} n_splits={n_splits}: rel err {rel:.3e} "
          f"(parent {parent:.3e})")
    assert rel < 2e-2, rel
    assert rel <= 4 * parent, (rel, parent)


@requires_gpu
@pytest.mark.parametrize("shape,n_splits", CASES)
def test_wgrad_accumulates(shape, n_splits):
    _check(shape, n_splits)


# FLASHY_WGRAD_MG pins the group count whatever the launcher would choose:
# MG=1 / MG=2 with four ranges keep several adder blocks per tile (the
# atomic epilogue), MG=4 with two ranges leaves two groups without a range,
# and on the odd shape the second range is a 41-row tail.
@requires_gpu
@pytest.mark.parametrize("shape,n_splits,mg", [
    (S_BODY, 4, 1), (S_BODY, 4, 2), (S_BODY, 2, 4), (S_BODY, 8, 2),
    (S_ODD, 2, 1), (S_ODD, 2, 4), (S_ODD, 1, 2),
])
def test_wgrad_forced_groups(shape, n_splits, mg, monkeypatch):
    monkeypatch.setenv("FLASHY_WGRAD_MG", str(mg))
    _check(shape, n_splits)


@requires_gpu
@pytest.mark.parametrize("shape", [S_BODY, S_L4])   # k_conv_wgrad, k_conv_wgrad8
def test_wgrad_single_range_bitwise(shape):
    a = _run(shape, 1)
    b = _run(shape, 1)
    assert torch.equal(a, b)


@requires_gpu
def test_wgrad_env_single_range_bitwise(monkeypatch):
    # FLASHY_WGRAD_SPLITS=1: one range per tile for every shape
    monkeypatch.setenv("FLASHY_WGRAD_SPLITS", "1")
    for shape in (S_ODD, S_L4S2):
        assert torch.equal(_run(shape, None), _run(shape, None))
