# Copyright (c) Flashy-AMD authors.
"""The multi-kernel BatchNorm chain (k_bn_stats -> k_bn_finalize ->
k_bn_apply*, k_bn_bwd_reduce -> k_bn_bwd_grads -> k_bn_bwd_apply*) against
the float64 oracle of tests/bn_reference.py, with the bounds derived there.
The kernels are called through ``ops.bn_*`` so no plan can route around them;
the module tests then hold ``BatchNorm2d`` bitwise to that chain.

Shapes are the smallest that reach every path: one row, fewer rows than a
block's 32 m-lanes, ragged tails, C = 64 / 192 / 256 / 512 channel groups,
every branch of ``combine_partials8`` (scalar for msplit % 4 != 0, float4,
float4 with a second loop pass at msplit > 128, more splits than 32-row
groups so that trailing blocks own no rows), ``apply_mpb`` capped with a
ragged rows-per-block, and the generic (C % 64 != 0) elementwise kernels.
Every output buffer starts as NaN or a sentinel, so an unwritten element
fails.
"""
import functools

import pytest
import torch

from tests import bn_reference as R
from tests.test_bn_small_gpu import EPS, FLAGS, MOM, _dx_err

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

NAN = float("nan")
# (M, C, msplit); None = ops.bn_msplit
STAT_CASES = [(1, 64, None), (33, 64, None), (1000, 64, None),
              (3136, 256, None), (4100, 192, None)] + \
             [(1000, 64, ms) for ms in (1, 3, 4, 132, 512)] + \
             [(1056, 64, 132)]
# (1000, 64) puts 8 rows in each of 125 blocks at msplit = 132 and 2 rows in
# each of 500 at 512: the float4 combine's second pass (slots 128..131) reads
# only zero slots at 132 and data at 512.  (1056, 64, 132) fills all 132
# slots, so the second pass is a single float4 of data.
APPLY_C64 = [(1, 64), (33, 64), (1000, 192), (4100, 512), (32808, 64)]
APPLY_GENERIC = [(1, 8), (7, 40), (1000, 96)]
BWD_GENERIC = [(M, C) for C in (8, 40, 96) for M in (7, 1000)]


@functools.lru_cache(maxsize=None)
def _inputs(M, C, offset=False):
    """Drawn as in tests/test_bn_small_gpu.py::_inputs, over [M, C]; the
    offset set has E[x^2] / var ~ 65, where s2/M - mean^2 cancels."""
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    x = rnd(M, C)
    x = ((x * 0.5 + 4.0) if offset else (x * 1.5 + 0.3)).to(torch.bfloat16)
    res = rnd(M, C).to(torch.bfloat16)
    dy = rnd(M, C).to(torch.bfloat16)
    gamma = 1.0 + 0.5 * rnd(C)
    beta = 0.3 * rnd(C)
    rmean = 0.1 * rnd(C)
    rvar = 1.0 + 0.1 * rnd(C).abs()
    return x, res, dy, gamma, beta, rmean, rvar


def _nan(n):
    return torch.full((n,), NAN, dtype=torch.float32, device="cuda")


def _within(name, got, want, bound):
    """got (fp32) within ``bound`` of want (float64), elementwise; prints the
    worst error as a fraction of its bound."""
    assert torch.isfinite(got).all(), name
    err = (got.double() - want).abs()
    print(f"{name}: max err/bound "
          f"{(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all(), (name, err.max().item())


def _stats(x, M, C, msplit):
    from flashy_amd import ops
    partials = _nan(2 * C * msplit)
    ops.bn_stats(x, partials, M, C, msplit)
    return partials


def _finalize(partials, msplit, gamma, beta, rmean, rvar, M, C, update):
    from flashy_amd import ops
    work = _nan(4 * C)
    rm, rv = rmean.clone(), rvar.clone()
    ops.bn_finalize(partials, msplit, gamma, beta, rm, rv, work, M, C, EPS,
                    MOM, update_running=update)
    return work, rm, rv


# ---------------------------------------------------------------------------
# forward statistics
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("M,C,msplit", STAT_CASES)
def test_stats_finalize(M, C, msplit, offset):
    from flashy_amd import ops
    msplit = msplit or ops.bn_msplit(M, C)
    x, _, _, gamma, beta, rmean, rvar = _inputs(M, C, offset)
    partials = _stats(x, M, C, msplit)
    assert torch.isfinite(partials).all()
    # blocks past the last row own nothing and must still write their slot
    mpb = -(-M // msplit)
    used = -(-M // mpb)
    assert not partials.view(2, C, msplit)[:, :, used:].any()
    work, rm, rv = _finalize(partials, msplit, gamma, beta, rmean, rvar, M, C,
                             True)
    eps, mom = R.f32(EPS), R.f32(MOM)
    ref = R.stats64(x, gamma, beta, rmean, rvar, eps, mom)
    bnd = R.stats_bounds(x, gamma, beta, rmean, rvar, eps, mom)
    for i, name in enumerate(("mean", "invstd", "scale", "shift")):
        _within(name, work[i * C:(i + 1) * C], getattr(ref, name),
                getattr(bnd, name))
    _within("running_mean", rm, ref.running_mean, bnd.running_mean)
    _within("running_var", rv, ref.running_var, bnd.running_var)
    # without the update: same work, running statistics untouched
    work2, rm2, rv2 = _finalize(partials, msplit, gamma, beta, rmean, rvar, M,
                                C, False)
    assert torch.equal(work2, work)
    assert torch.equal(rm2, rmean) and torch.equal(rv2, rvar)
    if M == 1:
        # var = 0: invstd = eps^-1/2, and the running variance decays to 0
        assert not ref.var.any()
        want = torch.full((C,), eps ** -0.5, dtype=torch.float64,
                          device="cuda")
        _within("invstd (M = 1)", work[C:2 * C], want, 2.0 ** -22 * want)
        assert torch.isfinite(work).all() and torch.isfinite(rv).all()
        return
    if offset:
        # Cancellation in s2/M - mean^2: the observed error, next to what
        # torch's fp32 batch_norm gets on the same device (it uses Welford),
        # recorded in profiles/README.md ("BatchNorm numerics").  Below 2^-9
        # the error disappears in the bf16 rounding of y.
        e_chain = ((work[C:2 * C].double() - ref.invstd).abs()
                   / ref.invstd).max().item()
        _, _, t_invstd = torch.native_batch_norm(
            x.float(), gamma, beta, rmean.clone(), rvar.clone(), True, MOM,
            EPS)
        e_torch = ((t_invstd.double() - ref.invstd).abs()
                   / ref.invstd).max().item()
        print(f"offset invstd rel err (M={M}, C={C}, msplit={msplit}): "
              f"chain {e_chain:.3e} torch-fp32 {e_torch:.3e} "
              f"bound {(bnd.invstd / ref.invstd).max().item():.3e}")
        assert e_chain <= 2.0 ** -9


# ---------------------------------------------------------------------------
# forward apply
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hand_work(M, C):
    """A work buffer built on the host side of the kernels: the float64
    statistics of x rounded to fp32.  The oracle then starts from the same
    fp32 coefficients the kernel reads."""
    x, _, _, gamma, beta, rmean, rvar = _inputs(M, C)
    st = R.stats64(x, gamma, beta, rmean, rvar, EPS, MOM)
    return torch.cat([st.mean, st.invstd, st.scale, st.shift]).float()


def _check_apply(x, res, work, M, C, relu, slope):
    from flashy_amd import ops
    y = torch.full_like(x, NAN)
    ops.bn_apply(x, res, y, work, M, C, relu, slope)
    assert torch.isfinite(y).all()
    scale, shift = work[2 * C:3 * C], work[3 * C:]
    y64 = R.fwd64(x, res, scale, shift, relu, R.f32(slope))
    bound = R.fwd_bound(x, res, scale, shift, y64)
    err = (y.double() - y64).abs()
    print(f"y: max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all(), err.max().item()
    return y


@requires_gpu
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("M,C", APPLY_C64 + APPLY_GENERIC)
def test_apply(M, C, flags):
    relu, has_res, slope = flags
    x, res, _, _, _, _, _ = _inputs(M, C)
    _check_apply(x, res if has_res else None, _hand_work(M, C), M, C, relu,
                 slope)


# ---------------------------------------------------------------------------
# backward chain
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fwd_state(M, C, flags):
    """(y, work) of the chain's forward — the backward's inputs; computed
    once per case and left unchanged."""
    from flashy_amd import ops
    relu, has_res, slope = flags
    x, res, _, gamma, beta, rmean, rvar = _inputs(M, C)
    msplit = ops.bn_msplit(M, C)
    work, _, _ = _finalize(_stats(x, M, C, msplit), msplit, gamma, beta,
                           rmean, rvar, M, C, True)
    y = torch.full_like(x, NAN)
    ops.bn_apply(x, res if has_res else None, y, work, M, C, relu, slope)
    return y, work


def _dz_rounded(dy, y, relu, slope):
    """The kernels' dz: one fp32 product with the slope where y <= 0, one
    round-to-nearest-even to bf16."""
    g = dy.float()
    if relu:
        g = torch.where(y.float() > 0, g, g * slope)
    return g.to(torch.bfloat16)


def _check_dx(dx, ref, scale, dz16, sums_exact):
    assert torch.isfinite(dx).all()
    e = _dx_err(dx, ref.dx)
    print(f"dx rel err {e:.3e} (bound {2.0 ** -8:.3e})")
    assert e <= 2.0 ** -8
    bound = R.dx_bound(ref, scale, dz16, sums_exact)
    err = (dx.double() - ref.dx).abs()
    print(f"dx: max err/bound "
          f"{(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all(), err.max().item()


@requires_gpu
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("M,C,msplit", STAT_CASES)
def test_bwd_chain(M, C, msplit, flags):
    from flashy_amd import ops
    relu, _, slope = flags
    msplit = msplit or ops.bn_msplit(M, C)
    x, _, dy, gamma, beta, _, _ = _inputs(M, C)
    y, work = _fwd_state(M, C, flags)
    mean, invstd, scale = (work[i * C:(i + 1) * C] for i in range(3))
    dz = torch.full_like(dy, -7.0)
    dx = torch.full_like(x, NAN)
    bpart, bsums = _nan(2 * C * msplit), _nan(2 * C)
    dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(beta)
    ops.bn_bwd_reduce(dy, y, x, work, dz, bpart, M, C, msplit, relu, slope)
    ops.bn_bwd_grads(bpart, msplit, bsums, dgamma, dbeta, C)
    ops.bn_bwd_apply(dz, x, work, bsums, dx, M, C)

    dz16 = _dz_rounded(dy, y, relu, slope)
    assert torch.equal(dz, dz16)
    ref = R.bwd_train64(x, dy, y, mean, invstd, scale, relu, R.f32(slope),
                        dz_apply=dz16)
    _within("sum dz", bsums[:C], ref.s, ref.bound_s)
    _within("sum dz*xhat", bsums[C:], ref.sx, ref.bound_sx)
    _within("dbeta", dbeta, ref.s, ref.bound_s)
    _within("dgamma", dgamma, ref.sx, ref.bound_sx)
    # += : one fp32 add of the same sums onto what was there
    g0, b0 = gamma * 3.0 + 1.0, beta - 2.0
    dgamma1, dbeta1, bsums1 = g0.clone(), b0.clone(), _nan(2 * C)
    ops.bn_bwd_grads(bpart, msplit, bsums1, dgamma1, dbeta1, C)
    assert torch.equal(bsums1, bsums)
    assert torch.equal(dgamma1, g0 + dgamma)
    assert torch.equal(dbeta1, b0 + dbeta)
    _check_dx(dx, ref, scale, dz16, sums_exact=False)


@requires_gpu
@pytest.mark.parametrize("M,C", BWD_GENERIC)
def test_bwd_apply_generic(M, C):
    """k_bn_bwd_apply (C % 64 != 0), which the reduce kernel cannot feed:
    work and bsums are built by hand from the oracle and rounded to fp32."""
    from flashy_amd import ops
    x, _, dy, _, _, _, _ = _inputs(M, C)
    work = _hand_work(M, C)
    mean, invstd, scale = (work[i * C:(i + 1) * C] for i in range(3))
    sums = R.bwd_train64(x, dy, None, mean, invstd, scale, False, 0.0)
    bsums = torch.cat([sums.s, sums.sx]).float()
    # the oracle divides the same fp32 sums the kernel reads
    ref = sums._replace(s=bsums[:C].double(), sx=bsums[C:].double())
    ref = ref._replace(dx=scale.double() * (
        dy.double() - ref.s / M - ref.xhat * ref.sx / M))
    dx = torch.full_like(x, NAN)
    ops.bn_bwd_apply(dy, x, work, bsums, dx, M, C)
    _check_dx(dx, ref, scale, dy, sums_exact=True)


# ---------------------------------------------------------------------------
# module
# ---------------------------------------------------------------------------

def _module(C, gamma, beta, rmean, rvar):
    from flashy_amd import nn as fnn
    bn = fnn.BatchNorm2d(C, eps=EPS, momentum=MOM).cuda()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rmean)
        bn.running_var.copy_(rvar)
    return bn


@requires_gpu
def test_module_training_is_the_chain():
    """Two consecutive training steps of BatchNorm2d on a shape the small-M
    plan declines equal the ops-level chain called by hand, bit for bit."""
    from flashy_amd import ops
    N, H, W, C = 2, 40, 41, 128
    M = N * H * W
    relu, slope = True, 0.2
    assert ops.bn_small_plan(M, C) == ("chain", "chain")
    _, _, _, gamma, beta, rmean, rvar = _inputs(M, C)
    bn = _module(C, gamma, beta, rmean, rvar).train()
    rm, rv = rmean.clone(), rvar.clone()
    dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(beta)
    msplit = ops.bn_msplit(M, C)
    g = torch.Generator(device="cuda").manual_seed(21)
    for step in range(2):
        x16, r16, dy = ((torch.randn(N, H, W, C, device="cuda", generator=g)
                         * 1.5 + 0.3).to(torch.bfloat16) for _ in range(3))
        x = x16.detach().requires_grad_(True)
        rr = r16.detach().requires_grad_(True)
        y = bn(x, res=rr, relu=relu, slope=slope)
        y.backward(dy)
        # the chain by hand
        work = _nan(4 * C)
        ops.bn_finalize(_stats(x16, M, C, msplit), msplit, gamma, beta, rm,
                        rv, work, M, C, EPS, MOM, update_running=True)
        y_c = torch.full_like(x16, NAN)
        ops.bn_apply(x16, r16, y_c, work, M, C, relu, slope)
        dz, dx = torch.full_like(dy, NAN), torch.full_like(x16, NAN)
        bpart, bsums = _nan(2 * C * msplit), _nan(2 * C)
        ops.bn_bwd_reduce(dy, y_c, x16, work, dz, bpart, M, C, msplit, relu,
                          slope)
        ops.bn_bwd_grads(bpart, msplit, bsums, dgamma, dbeta, C)
        ops.bn_bwd_apply(dz, x16, work, bsums, dx, M, C)
        for name, u, v in (("y", y, y_c), ("dx", x.grad, dx),
                           ("dres", rr.grad, dz),
                           ("dgamma", bn.weight.grad, dgamma),
                           ("dbeta", bn.bias.grad, dbeta),
                           ("running_mean", bn.running_mean, rm),
                           ("running_var", bn.running_var, rv)):
            assert torch.equal(u, v), (step, name)
    assert not torch.equal(rm, rmean) and not torch.equal(rv, rvar)


@requires_gpu
@pytest.mark.parametrize("shape", [(4, 8, 8, 64), (4, 8, 8, 128),
                                   (2, 40, 41, 64), (2, 40, 41, 128)])
def test_module_eval(shape):
    """Eval mode: y from the running statistics, and their constant-statistics
    gradient dx = scale * dz — one fp32 product, one rounding."""
    from flashy_amd import ops
    N, H, W, C = shape
    M = N * H * W
    relu, slope = True, 0.2
    x2, r2, dy2, gamma, beta, rmean, rvar = _inputs(M, C)
    x16, r16, dy = (t.view(N, H, W, C) for t in (x2, r2, dy2))
    invstd = torch.rsqrt(rvar + EPS)
    scale = gamma * invstd
    work = torch.cat([rmean, invstd, scale, beta - rmean * scale])
    y_c = torch.full_like(x16, NAN)
    ops.bn_apply(x16, r16, y_c, work, M, C, relu, slope)
    dz16 = _dz_rounded(dy, y_c, relu, slope)
    want_dx = (scale * dz16.float()).to(torch.bfloat16)
    ref = R.bwd_eval64(x2, dy2, y_c.view(M, C), rmean, invstd, scale, relu,
                       R.f32(slope), dz_apply=dz16.view(M, C))

    grads = []
    for frozen in (False, True):
        bn = _module(C, gamma, beta, rmean, rvar).eval()
        if frozen:
            bn.weight.requires_grad_(False)
            bn.bias.requires_grad_(False)
        x = x16.detach().requires_grad_(True)
        rr = r16.detach().requires_grad_(True)
        y = bn(x, res=rr, relu=relu, slope=slope)
        y.backward(dy)
        assert torch.equal(bn.running_mean, rmean)
        assert torch.equal(bn.running_var, rvar)
        assert torch.equal(y, y_c)
        assert torch.equal(rr.grad, dz16)
        diff = (x.grad.float() - want_dx.float()).abs().max().item()
        print(f"frozen={frozen}: max |x.grad - bf16(scale*dz)| = {diff:.3e}, "
              f"max |scale*dz| = {want_dx.float().abs().max().item():.3e}")
        assert torch.equal(x.grad, want_dx), diff
        # and that product is the oracle's dx to one bf16 rounding
        assert _dx_err(x.grad, ref.dx) <= 2.0 ** -8
        if frozen:
            assert bn.weight.grad is None and bn.bias.grad is None
        else:
            _within("dgamma", bn.weight.grad, ref.sx, ref.bound_sx)
            _within("dbeta", bn.bias.grad, ref.s, ref.bound_s)
        grads.append(x.grad)
    assert torch.equal(grads[0], grads[1])


@requires_gpu
@pytest.mark.parametrize("C", [32, 96])
def test_unsupported_widths_raise(monkeypatch, C):
    """The reductions walk 64-channel groups: other widths are refused before
    anything is launched (they used to leave channels unwritten)."""
    from flashy_amd import ops
    assert ops.bn_small_plan(256, C) == ("chain", "chain")
    M = 256
    x2, _, _, gamma, beta, rmean, rvar = _inputs(M, C)
    launched = []
    ext = ops.require()

    class Spy:  # records every BatchNorm launcher the wrappers reach
        def __getattr__(self, name):
            if name.startswith("bn_") and name != "bn_small_plan":
                launched.append(name)
            return getattr(ext, name)

    monkeypatch.setattr(ops, "require", lambda: Spy())
    bn = _module(C, gamma, beta, rmean, rvar).train()
    x = x2.view(4, 8, 8, C).detach().requires_grad_(True)
    with pytest.raises(ValueError):
        bn(x, relu=True)
    assert launched == []
    assert torch.equal(bn.running_mean, rmean)
    f = torch.zeros(4 * C, device="cuda")
    with pytest.raises(ValueError):
        ops.bn_stats(x2, f, M, C, 1)
    with pytest.raises(ValueError):
        ops.bn_bwd_reduce(x2, x2, x2, f, x2.clone(), f.clone(), M, C, 1, False)
    x4 = torch.zeros(8, 4, device="cuda", dtype=torch.bfloat16)
    for call in (
            lambda: ops.bn_finalize(f, 1, f, f, f, f, f, 8, 4, EPS, MOM, False),
            lambda: ops.bn_bwd_grads(f, 1, f, f, f, 4),
            lambda: ops.bn_apply(x4, None, x4.clone(), f, 8, 4, False),
            lambda: ops.bn_bwd_apply(x4, x4, f, f, x4.clone(), 8, 4)):
        with pytest.raises(ValueError):
            call()
    assert launched == []


@requires_gpu
def test_eval_c32_forward_works_backward_raises():
    C, M = 32, 256
    x2, r2, dy2, gamma, beta, rmean, rvar = _inputs(M, C)
    bn = _module(C, gamma, beta, rmean, rvar).eval()
    x = x2.view(4, 8, 8, C).detach().requires_grad_(True)
    y = bn(x, res=r2.view(4, 8, 8, C), relu=True, slope=0.2)
    invstd = torch.rsqrt(rvar + EPS)
    scale = gamma * invstd
    work = torch.cat([rmean, invstd, scale, beta - rmean * scale])
    y_c = _check_apply(x2, r2, work, M, C, True, 0.2)
    assert torch.equal(y.view(M, C), y_c)
    with pytest.raises(ValueError):
        y.backward(dy2.view(4, 8, 8, C))
