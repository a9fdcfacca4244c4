# Copyright (c) Flashy-AMD authors.
"""The float64 BatchNorm oracle (tests/bn_reference.py) against torch's own
float64 batch_norm and autograd on the CPU: forward, every gradient and the
running statistics, in training and with ``training=False``, through ReLU,
LeakyReLU and a residual.  Agreement is held to 1e-12 of the largest
reference magnitude of each tensor (two float64 evaluations of the same
formula in different operation orders)."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_reference as R

EPS, MOM = 1e-5, 0.1
SHAPES = [(1, 8), (33, 64), (300, 96)]
FLAGS = [(False, False, 0.0), (True, False, 0.0), (False, True, 0.0),
         (True, True, 0.0), (True, True, 0.2)]    # (relu, res, slope)


def _close(name, got, want):
    err = (got - want).abs().max().item()
    tol = 1e-12 * max(want.abs().max().item(), 1e-300)
    assert torch.isfinite(got).all(), name
    assert err <= tol, (name, err, tol)


def _draw(M, C):
    g = torch.Generator().manual_seed(11 + M)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    # bf16-representable inputs, as the kernels see them
    x = (rnd(M, C) * 1.5 + 0.3).to(torch.bfloat16).double()
    res = rnd(M, C).to(torch.bfloat16).double()
    dy = rnd(M, C).to(torch.bfloat16).double()
    return (x, res, dy, 1.0 + 0.5 * rnd(C), 0.3 * rnd(C), 0.1 * rnd(C),
            1.0 + 0.1 * rnd(C).abs())


def _torch_bn(x, res, dy, gamma, beta, rmean, rvar, training, relu, slope):
    x = x.clone().requires_grad_(True)
    gamma = gamma.clone().requires_grad_(True)
    beta = beta.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if res is not None else None
    rm, rv = rmean.clone(), rvar.clone()
    # torch.batch_norm is F.batch_norm without its refusal of one value per
    # channel in training, which the kernels define (var = 0)
    z = torch.batch_norm(x, gamma, beta, rm, rv, training, MOM, EPS, False)
    if rr is not None:
        z = z + rr
    if relu:
        z = F.leaky_relu(z, slope) if slope else torch.relu(z)
    z.backward(dy)
    return (z.detach(), x.grad, gamma.grad, beta.grad,
            rr.grad if rr is not None else None, rm, rv)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("M,C", SHAPES)
def test_training_matches_torch_float64(M, C, flags):
    relu, has_res, slope = flags
    x, res, dy, gamma, beta, rmean, rvar = _draw(M, C)
    res = res if has_res else None
    y_t, dx_t, dg_t, db_t, dres_t, rm_t, rv_t = _torch_bn(
        x, res, dy, gamma, beta, rmean, rvar, True, relu, slope)
    st = R.stats64(x, gamma, beta, rmean, rvar, EPS, MOM)
    y = R.fwd64(x, res, st.scale, st.shift, relu, slope)
    bw = R.bwd_train64(x, dy, y, st.mean, st.invstd, st.scale, relu, slope)
    _close("mean", st.mean, x.mean(0))
    _close("var", st.var + EPS, x.var(0, unbiased=False) + EPS)
    _close("y", y, y_t)
    _close("dx", bw.dx, dx_t)
    _close("dgamma", bw.sx, dg_t)
    _close("dbeta", bw.s, db_t)
    if has_res:
        _close("dres", bw.dz, dres_t)
    _close("running_mean", st.running_mean, rm_t)
    if M > 1:
        _close("running_var", st.running_var, rv_t)
        _, save_mean, save_invstd = torch.native_batch_norm(
            x, gamma, beta, rmean.clone(), rvar.clone(), True, MOM, EPS)
        _close("save_mean", st.mean, save_mean)
        _close("save_invstd", st.invstd, save_invstd)
    else:
        # one row: torch's unbiased factor is 1/0; the kernels (and the
        # oracle) update with the biased variance, which is exactly 0
        assert torch.equal(st.var, torch.zeros_like(st.var))
        _close("running_var", st.running_var, rvar + MOM * (0.0 - rvar))
        _close("invstd", st.invstd, torch.full_like(st.invstd, EPS ** -0.5))
        assert torch.equal(bw.dx, torch.zeros_like(bw.dx))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("M,C", SHAPES)
def test_eval_matches_torch_float64(M, C, flags):
    relu, has_res, slope = flags
    x, res, dy, gamma, beta, rmean, rvar = _draw(M, C)
    res = res if has_res else None
    y_t, dx_t, dg_t, db_t, dres_t, rm_t, rv_t = _torch_bn(
        x, res, dy, gamma, beta, rmean, rvar, False, relu, slope)
    assert torch.equal(rm_t, rmean) and torch.equal(rv_t, rvar)
    invstd = 1.0 / torch.sqrt(rvar + EPS)
    scale = gamma * invstd
    shift = beta - rmean * scale
    y = R.fwd64(x, res, scale, shift, relu, slope)
    bw = R.bwd_eval64(x, dy, y, rmean, invstd, scale, relu, slope)
    _close("y", y, y_t)
    _close("dx", bw.dx, dx_t)
    _close("dgamma", bw.sx, dg_t)
    _close("dbeta", bw.s, db_t)
    if has_res:
        _close("dres", bw.dz, dres_t)
    # the training formula is a different function of the same inputs
    tr = R.bwd_train64(x, dy, y, rmean, invstd, scale, relu, slope)
    if M > 1:
        assert (tr.dx - bw.dx).abs().max() > 1e-3 * bw.dx.abs().max()


def test_bounds_hold_for_a_plain_fp32_evaluation():
    """The derived bounds against the simplest fp32 implementation (torch's
    fp32 reductions on the CPU): a sanity check that they are not vacuous in
    the wrong direction — an fp32 result must fit them — and that a result
    off by 2^-10 relative does not."""
    M, C = 300, 96
    x, _, _, gamma, beta, rmean, rvar = _draw(M, C)
    ref = R.stats64(x, gamma, beta, rmean, rvar, EPS, MOM)
    bnd = R.stats_bounds(x, gamma, beta, rmean, rvar, EPS, MOM)
    xf = x.float()
    mean = xf.sum(0) / M
    var = (xf * xf).sum(0) / M - mean * mean
    invstd = torch.rsqrt(var + EPS)
    scale = gamma.float() * invstd
    shift = beta.float() - mean * scale
    for name, got in (("mean", mean), ("var", var), ("invstd", invstd),
                      ("scale", scale), ("shift", shift)):
        err = (got.double() - getattr(ref, name)).abs()
        assert (err <= getattr(bnd, name)).all(), name
    off = ref.invstd * (1 + 2.0 ** -10)
    assert ((off - ref.invstd).abs() > bnd.invstd).all()
