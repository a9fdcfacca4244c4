# Copyright (c) Flashy-AMD authors.
"""GPU tests for the DMA-staged 64x64 wgrad (k_conv_wgrad_dma,
csrc/conv_wgrad.hip): the decomposition, stage order and epilogue of
k_conv_wgrad<MG> with the operands staged global -> LDS by DMA through a
counted-wait multi-buffer pipeline.

* One adder block per tile: bitwise equal to k_conv_wgrad<MG> (pinned with
  FLASHY_WGRAD_DMA=0) at MG 1/2/4, from a non-zero dw, two calls.
* Several adders: the relative error ``max |dw - (init + 2 grad)| / max|grad|``
  against the float64 reference is at most twice the register-staged kernel's
  own error on the same case, measured in the same run.  Both kernels hand the
  same per-block sums to the same atomics, whose order moves a repeat between
  2.3e-7 and 3.3e-7 (profiles/README.md, r04a); the factor 2 covers that.
* The pin and the routing rule.

Shapes are (N, H, W, C, K, R, stride, pad).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

S_BODY = (4, 8, 8, 64, 64, 3, 1, 1)       # M=256: four 64-row stages
S_ODD = (3, 7, 5, 64, 64, 3, 1, 1)        # M=105: edge taps, last stage past me
S_1X1 = (2, 16, 16, 64, 128, 1, 2, 0)     # M=128: two stages
S_L4S2 = (2, 4, 4, 256, 512, 3, 2, 1)     # M=8
S_ONE = (1, 4, 4, 64, 64, 3, 1, 1)        # M=16: one stage
S_THREE = (3, 8, 8, 64, 64, 3, 1, 1)      # M=192: three stages
SHAPES = [S_BODY, S_ODD, S_1X1, S_L4S2, S_ONE, S_THREE]

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


def _rel_err(shape, dw):
    _, _, _, init, grad = _inputs(shape)
    err = (dw.double() - (init.double() + 2 * grad)).abs().max().item()
    return err / grad.abs().max().item()


def _form(shape, n_splits):
    from flashy_amd import ops
    return ops.conv_wgrad_form(_inputs(shape)[2], n_splits)


# n_splits <= MG: one block sums every range, plain load-add-store.  MG = 2 / 4
# with one range leaves groups without a range; S_ODD's second range is a
# 41-row tail; S_BODY at (2, 2) and (4, 4) gives two- and one-stage ranges.
SINGLE = [(s, 1, mg) for s in SHAPES for mg in (1, 2, 4)] + [
    (S_BODY, 2, 2), (S_BODY, 2, 4), (S_BODY, 4, 4), (S_BODY, 3, 4),
    (S_ODD, 2, 2), (S_ODD, 2, 4), (S_THREE, 3, 4), (S_1X1, 2, 2),
]


def _bitwise(shape, n_splits, mg, monkeypatch):
    monkeypatch.setenv("FLASHY_WGRAD_MG", str(mg))
    monkeypatch.setenv("FLASHY_WGRAD_DMA", "0")
    assert _form(shape, n_splits) == f"wgrad<{mg}>"
    old = _run(shape, n_splits)
    monkeypatch.setenv("FLASHY_WGRAD_DMA", "1")
    assert _form(shape, n_splits).startswith(f"wgrad_dma<{mg},")
    new = _run(shape, n_splits)
    assert torch.equal(old, new), (old - new).abs().max().item()
    assert _rel_err(shape, new) < 1e-5


@requires_gpu
@pytest.mark.parametrize("shape,n_splits,mg", SINGLE)
def test_dma_single_adder_bitwise(shape, n_splits, mg, monkeypatch):
    _bitwise(shape, n_splits, mg, monkeypatch)


# several adder blocks per tile: n_splits 2/3/4/5/8 on every shape whose M
# gives that many ranges, MG 1 and 2 (MG = 2 on 3 or 5 ranges has an empty
# group in the last block; S_ODD's and S_THREE's last ranges are short)
SEVERAL = [(s, ns, mg) for s in (S_BODY, S_THREE) for ns in (2, 3, 4, 5, 8)
           for mg in (1, 2)] + [
    (S_ODD, 2, 1), (S_ODD, 3, 1), (S_ODD, 3, 2), (S_1X1, 2, 1),
    (S_1X1, 3, 2), (S_BODY, 8, 4), (S_THREE, 5, 4),
]


@requires_gpu
@pytest.mark.parametrize("shape,n_splits,mg", SEVERAL)
def test_dma_several_adders(shape, n_splits, mg, monkeypatch):
    monkeypatch.setenv("FLASHY_WGRAD_MG", str(mg))
    monkeypatch.setenv("FLASHY_WGRAD_DMA", "0")
    old = _rel_err(shape, _run(shape, n_splits))
    monkeypatch.setenv("FLASHY_WGRAD_DMA", "1")
    assert _form(shape, n_splits).startswith("wgrad_dma<")
    new = _rel_err(shape, _run(shape, n_splits))
    print(f"wgrad_dma {shape} n_splits={n_splits} mg={mg}: "
          f"rel err {new:.3e} (register-staged {old:.3e})")
    assert new <= 2 * old, (new, old)


@requires_gpu
def test_pin_zero_is_the_old_kernel(monkeypatch):
    # FLASHY_WGRAD_DMA=0 against the launcher's own choice with the DMA
    # kernel switched off by the shape (unset pin, rule): both must be the
    # register-staged kernel's bits on a single-adder case
    monkeypatch.setenv("FLASHY_WGRAD_SPLITS", "1")
    monkeypatch.setenv("FLASHY_WGRAD_DMA", "0")
    a = _run(S_ODD, None)
    b = _run(S_ODD, None)
    assert _form(S_ODD, None) == "wgrad<1>"
    monkeypatch.setenv("FLASHY_WGRAD_DMA", "1")
    c = _run(S_ODD, None)
    assert _form(S_ODD, None).startswith("wgrad_dma<1,")
    assert torch.equal(a, b) and torch.equal(a, c)


# The flagship's ten wgrad shapes (batch 64) and what the rule chose for them
# in profiles/README.md, r09a.
FLAGSHIP = {
    (64, 32, 32, 64, 64, 3, 1, 1): "wgrad_dma<4,4>",
    (64, 32, 32, 64, 128, 3, 2, 1): "wgrad_dma<4,4>",
    (64, 16, 16, 128, 128, 3, 1, 1): "wgrad_dma<4,4>",
    (64, 16, 16, 128, 256, 3, 2, 1): "wgrad_dma<2,4>",
    (64, 8, 8, 256, 256, 3, 1, 1): "wgrad_dma<2,4>",
    (64, 8, 8, 256, 512, 3, 2, 1): "wgrad_dma<1,4>",
    (64, 4, 4, 512, 512, 3, 1, 1): "wgrad8",
    (64, 32, 32, 64, 128, 1, 2, 0): "wgrad_dma<2,4>",
    (64, 16, 16, 128, 256, 1, 2, 0): "wgrad<4>",
    (64, 8, 8, 256, 512, 1, 2, 0): "wgrad<4>",
}


@pytest.mark.parametrize("shape", list(FLAGSHIP))
def test_rule_on_flagship_shapes(shape, monkeypatch):
    from flashy_amd import ops
    for name in ("FLASHY_WGRAD_DMA", "FLASHY_WGRAD_MG", "FLASHY_WGRAD_SPLITS"):
        monkeypatch.delenv(name, raising=False)
    N, H, W, C, K, R, stride, pad = shape
    Ho = (H + 2 * pad - R) // stride + 1
    d = ops.ConvDims(N, H, W, C, K, R, R, Ho, Ho, stride, pad)
    assert ops.conv_wgrad_form(d) == FLAGSHIP[shape]
