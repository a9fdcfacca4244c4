# Copyright (c) Flashy-AMD authors.
"""Float64 oracle for BatchNorm over ``[M, C]`` and the error bounds the fp32
kernels are held to (tests/test_bn_reference.py checks the oracle itself
against torch's float64 batch_norm; tests/test_bn_chain_gpu.py uses it).

Every function takes tensors of any floating dtype and upcasts them exactly
(bf16 and fp32 are subsets of float64), on whatever device they live on.
Scalars (eps, momentum, slope) are used as given: a caller that compares with
an fp32 kernel passes ``f32(value)``, the value the kernel received.

Bounds.  u = 2^-24 is the fp32 unit roundoff.  Summing M fp32 terms in any
order (lanes, blocks, partials, a combine tree) does M - 1 additions, each
with relative error at most u, so the result is within (M - 1) u S (1 + O(Mu))
of the exact sum, S = sum of the terms' absolute values.  The convention
here, shared with tests/test_bn_small_gpu.py, is

    bound_sum = 4 M u S

whose factor 4 covers the rounding of the terms themselves (at most 3u each:
the fp32 xhat = (x - mean) * invstd and its product with dz), the O(Mu) tail,
the one division by M that follows, and the second-order terms below.

Forward statistics, with s = sum x, s2 = sum x^2, mean = s / M,
var = s2 / M - mean^2, as k_bn_finalize computes them:

    |d mean|   <= bound_s / M
    |d var|    <= bound_s2 / M + 2 |mean| |d mean| + 2^-22 (E[x^2] + mean^2)
    |d invstd| <= invstd (|d var| / (2 (var + eps)) + 2^-22)

d var: s2 / M carries bound_s2 / M and one rounding (u E[x^2]); mean^2
carries 2 |mean| |d mean| + (d mean)^2 and one rounding (u mean^2); the
subtraction rounds once more (u (E[x^2] + mean^2) at most), whether or not
the compiler contracts it into an fma.  That is 3u (E[x^2] + mean^2) <= 2^-22
(...); (d mean)^2 <= (4 M u)^2 E|x|^2 is below the slack 3 M u E[x^2] that the
factor 4 leaves in bound_s2 / M while M < 3 / (16 u) ~ 3e6 rows.  Clamping a
negative var to 0 only moves it towards the true value.
d invstd: d(v^-1/2) / v^-1/2 = -dv / (2 v) to first order; the next term,
3/8 (dv / v)^2, is again inside the factor 4.  fp32 eps (u), the addition
(u) and rsqrtf (1 ulp = 2u) add at most u/2 + u/2 + 2u <= 2^-22.

    |d scale| <= |gamma| |d invstd| + u |scale|
    |d shift| <= |mean| |d scale| + |scale| |d mean| + |d mean| |d scale|
                 + 2^-23 (|beta| + |mean scale|)
    running   <= momentum |d stat| + 2^-21 (|r| + momentum (|stat| + |r|))

for r += momentum * (stat - r) (at most 3 roundings plus fp32 momentum on
the increment, one on the result: 6u in all for the variance, whose unbiased
factor M / (M - 1) costs two more roundings; 2^-21 = 8u).

Forward apply, y = bf16(act(scale x + shift + res)) from fp32 scale/shift:

    |dy| <= 2^-8 |y| + 2^-22 (|scale x| + |shift| + |res|)

(one bf16 rounding, 8 significand bits, is at most 2^-8 of the exact value;
the fma, the addition and the slope product before it are fp32, 3u <= 2^-22
of the terms' magnitudes; where the fp32 and the exact pre-activation differ
in sign both are smaller than the second term, so the bound holds across the
ReLU kink too).
"""
import typing as tp

import torch

U32 = 2.0 ** -24


def f32(v: float) -> float:
    """``v`` rounded to fp32, as a kernel's float argument receives it."""
    return float(torch.tensor(v, dtype=torch.float32))


def sum_bound(terms: torch.Tensor) -> torch.Tensor:
    """Bound on |fp32 sum over dim 0 - exact sum| of the float64 ``terms``."""
    return 4.0 * terms.shape[0] * U32 * terms.abs().sum(0)


class Stats(tp.NamedTuple):
    mean: torch.Tensor
    var: torch.Tensor           # biased
    invstd: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    running_mean: torch.Tensor  # after the update
    running_var: torch.Tensor


def stats64(x, gamma, beta, rmean, rvar, eps: float,
            momentum: float) -> Stats:
    x = x.double()
    M = x.shape[0]
    gamma, beta, rmean, rvar = (t.double() for t in (gamma, beta, rmean, rvar))
    mean = x.sum(0) / M
    var = ((x - mean) ** 2).sum(0) / M
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    unbiased = var * M / (M - 1) if M > 1 else var
    return Stats(mean, var, invstd, scale, shift,
                 rmean + momentum * (mean - rmean),
                 rvar + momentum * (unbiased - rvar))


def stats_bounds(x, gamma, beta, rmean, rvar, eps: float,
                 momentum: float) -> Stats:
    """Per-channel bounds on an fp32 implementation's distance from
    :func:`stats64` (module docstring); ``var`` bounds the biased variance."""
    x = x.double()
    M = x.shape[0]
    gamma, beta, rmean, rvar = (t.double() for t in (gamma, beta, rmean, rvar))
    ref = stats64(x, gamma, beta, rmean, rvar, eps, momentum)
    ex2 = (x * x).sum(0) / M
    mean_sq = ref.mean ** 2
    d_mean = sum_bound(x) / M
    d_var = sum_bound(x * x) / M + 2 * ref.mean.abs() * d_mean \
        + 2.0 ** -22 * (ex2 + mean_sq)
    d_invstd = ref.invstd * (0.5 * d_var / (ref.var + eps) + 2.0 ** -22)
    d_scale = gamma.abs() * d_invstd + U32 * ref.scale.abs()
    d_shift = ref.mean.abs() * d_scale + ref.scale.abs() * d_mean \
        + d_mean * d_scale \
        + 2.0 ** -23 * (beta.abs() + (ref.mean * ref.scale).abs())
    k = M / (M - 1) if M > 1 else 1.0

    def running(d_stat, stat, r):
        return momentum * d_stat + 2.0 ** -21 * (
            r.abs() + momentum * (stat.abs() + r.abs()))

    return Stats(d_mean, d_var, d_invstd, d_scale, d_shift,
                 running(d_mean, ref.mean, rmean),
                 running(k * d_var, k * ref.var, rvar))


def fwd64(x, res, scale, shift, relu: bool, slope: float) -> torch.Tensor:
    """y = act(scale * x + shift [+ res]); act = LeakyReLU(slope) with
    ``relu`` (slope 0: plain ReLU), identity without."""
    y = x.double() * scale.double() + shift.double()
    if res is not None:
        y = y + res.double()
    if relu:
        y = torch.where(y > 0, y, slope * y)
    return y


def fwd_bound(x, res, scale, shift, y64) -> torch.Tensor:
    """Elementwise bound on |bf16 kernel output - fwd64| (module docstring)."""
    mag = (x.double() * scale.double()).abs() + shift.double().abs()
    if res is not None:
        mag = mag + res.double().abs()
    return 2.0 ** -8 * y64.abs() + 2.0 ** -22 * mag


class Bwd(tp.NamedTuple):
    dz: torch.Tensor      # dy through the activation, unrounded (float64)
    s: torch.Tensor       # sum dz           (= dbeta)
    sx: torch.Tensor      # sum dz * xhat    (= dgamma)
    dx: torch.Tensor
    xhat: torch.Tensor
    bound_s: torch.Tensor
    bound_sx: torch.Tensor


def _dz_sums(x, dy, y, mean, invstd, relu: bool, slope: float):
    dz = dy.double()
    if relu:  # the mask is taken from the forward output, as the kernels do
        dz = torch.where(y.double() > 0, dz, slope * dz)
    xhat = (x.double() - mean.double()) * invstd.double()
    return dz, xhat, dz.sum(0), (dz * xhat).sum(0)


def bwd_train64(x, dy, y, mean, invstd, scale, relu: bool, slope: float,
                dz_apply: tp.Optional[torch.Tensor] = None) -> Bwd:
    """Backward through batch statistics:
    dx = scale * (dz - sum(dz)/M - xhat * sum(dz*xhat)/M).  ``dz_apply`` is the
    dz that the dx expression reads when it is not the exact one — the
    kernels' second pass reads dz back rounded to bf16, the sums do not."""
    dz, xhat, s, sx = _dz_sums(x, dy, y, mean, invstd, relu, slope)
    M = dz.shape[0]
    g = dz if dz_apply is None else dz_apply.double()
    dx = scale.double() * (g - s / M - xhat * sx / M)
    return Bwd(dz, s, sx, dx, xhat, sum_bound(dz), sum_bound(dz * xhat))


def bwd_eval64(x, dy, y, mean, invstd, scale, relu: bool, slope: float,
               dz_apply: tp.Optional[torch.Tensor] = None) -> Bwd:
    """Backward through running statistics: mean and invstd do not depend on
    x, so dx = scale * dz; dz, dgamma = sx and dbeta = s are as in training
    (with xhat taken from the running statistics)."""
    dz, xhat, s, sx = _dz_sums(x, dy, y, mean, invstd, relu, slope)
    g = dz if dz_apply is None else dz_apply.double()
    return Bwd(dz, s, sx, scale.double() * g, xhat, sum_bound(dz),
               sum_bound(dz * xhat))


def dx_bound(ref: Bwd, scale, dz_apply, sums_exact: bool) -> torch.Tensor:
    """Elementwise bound on |bf16 training dx - ref.dx|: one bf16 rounding of
    the result (2^-8 of its value), 8u on each fp32 term of the expression
    (xhat 3u, 1/M and its products 3u, the subtractions and the scale product
    one each on the running value), and the error of the fp32 sums the kernel
    divides by M unless the caller handed it the reference's own sums."""
    M = ref.dz.shape[0]
    sc = scale.double().abs()
    t1, t2 = (ref.s / M).abs(), (ref.xhat * ref.sx / M).abs()
    b = 2.0 ** -8 * ref.dx.abs() \
        + 2.0 ** -21 * sc * (dz_apply.double().abs() + t1 + t2)
    if not sums_exact:
        b = b + sc * (ref.bound_s + ref.xhat.abs() * ref.bound_sx) / M
    return b
