# Copyright (c) Flashy-AMD authors.
"""Float64 oracle for the loss and accuracy kernels of csrc/losses.hip and the
error bounds they are held to (tests/test_loss_reference.py checks the oracle
against torch's float64 losses and shows that the bounds bite;
tests/test_loss_gpu.py holds the kernels to them).

Every function upcasts its tensors exactly (bf16 and fp32 are subsets of
float64), on whatever device they live on.  Scalars (eps, lam, the BCE target,
the two scales) are used as given: a caller that compares with a kernel passes
``f32(value)``, the value the kernel received; :func:`mean_scale` is the
``1 / B`` of the autograd wrappers as the kernel sees it.

Bounds.  u = 2^-24 is the fp32 unit roundoff; an error of K ulp is at most
2 K u relative.  K_EXP, K_LOG and K_LOG1P are the ulp errors of the device's
expf, logf and log1pf.  The build has no fast-math flag and the ROCm
installation carries no copy of HIP's math accuracy table, so they were
measured: ``test_math_function_ulps`` of tests/test_loss_gpu.py runs
torch.exp / log / log1p in fp32 against float64 over [-104, 0], [1, 4097] and
(0, 1] and asserts that the largest error, rounded up to a whole ulp, plus one
(the kernels call the device library directly, torch may not) does not exceed
the constant below.  Measured on an MI355X (MEASURED_ULPS): exp 0.9999 ulp,
log 1.8807 ulp, log1p 0.5698 ulp, hence K_EXP = 2, K_LOG = 3, K_LOG1P = 2.

Every gradient bound is elementwise and proportional to that element's own
terms.  The only absolute term is the underflow floor: a result below 2^-126
is rounded to a multiple of 2^-149 (bf16: 2^-133), which no relative bound
covers.

Softmax, as k_cross_entropy and k_cross_entropy_mix compute it, with
d_c = x_c - mx, e_c = exp(d_c), s = sum e_c, p_c = e_c / s:

    the maximum mx is exact (fmaxf selects);
    fl(d_c) = d_c (1 + delta) moves e_c by a relative u |d_c|;
    expf adds 2 K_EXP u, so e_c is within u (2 K_EXP + |d_c|) e_c;
    the lane and wave sum does at most C - 1 additions of positive terms
    (an idle lane adds an exact 0): C u s, plus the terms' own errors,
    u sum_c (2 K_EXP + |d_c|) e_c = u s (2 K_EXP + H), H = sum_c p_c |d_c|;
    so |ds| <= RS s with RS = u (C + 2 K_EXP + H);
    1 / s and the product round once each, and one more u covers the
    second-order terms (all of the above is below 2^-11 for C < 8192):

    |dp_c| <= p_c (u (3 + 2 K_EXP + |d_c| + C) + u (2 K_EXP + H))

This is the shape a + 2 K_EXP + |x_c - mx| + C with a = 3 (division, product,
second order), plus the part of the sum's error that comes from its terms,
which is a property of the row's sum and not of its maximum.

Gradient, g = (p - t) grad_scale with t = eps/C + wa [c == ta] + wb [c == tb],
wa = (1 - eps) lam, wb = (1 - eps)(1 - lam):

    |dg_c| <= (|dp_c| + 4 u t_c + u (p_c + t_c)) |grad_scale| + u |g_c| + FLOOR

4 u t: wa and wb take two roundings each, eps / C one, and the two additions
that build t one each on a value no larger than t (the plain kernel's t is an
exact 0 or 1 and stays inside).  The subtraction rounds once on |p - t| <=
p + t, the product once.  FLOOR = (K_EXP + 3) 2^-149: expf, the two products
and the division may each round in the subnormal range.

bf16 store: f32_to_bf16 rounds to nearest even, half a bf16 ulp of the value
it is given, at most 2^-8 of it (8 significand bits), or 2^-134 below the
normal range:

    |dg_c|_bf16 <= |dg_c| + 2^-8 (|g_c| + |dg_c|) + 2^-134

Loss.  lse = mx + log s: the error of s moves log s by RS, logf adds
2 K_LOG u |log s|, the addition u |lse|.  inner = wa x_ta + wb x_tb +
(eps/C) sum x: each product's factor carries at most 3 u and the products
and additions another 3 u of the terms' magnitudes, 7 u with the second
order; sum x is a sum of C terms, within sum_bound of bn_reference
(4 C u sum |x|).  The subtraction rounds on |lse| + |inner| at most, the
product with loss_scale on the row's value:

    |d row| <= RS + 2 K_LOG u |log s| + 2 u |lse| + 7 u (|wa x_ta| + |wb x_tb|
               + |eps/C sum x|) + eps/C 4 C u sum |x| + u |row|

The rows are added into ``loss_sum`` by one atomicAdd each, onto whatever the
caller left there (the += contract): a sum of B + 1 terms in an unknown order,
held to bn_reference's convention bound_sum = 4 M u S with M = B + 1 and S
the sum of the terms' magnitudes, the initial value included.

BCE-with-logits against a constant t, e = exp(-|v|), l = log1p(e),
loss_i = max(v, 0) - v t + l, sig = 1 / (1 + exp(-v)):

    |d loss_i| <= u (2 K_EXP e / (1 + e) + 2 K_LOG1P l
                     + 3 (max(v, 0) + |v t| + l))
    |d sig|    <= sig u (3 + 2 K_EXP (1 - sig))
    |dg_i|     <= (|d sig| + u (sig + |t|)) |grad_scale| + u |g_i| + FLOOR

(d log1p(e) / de = 1 / (1 + e); the product v t and the two additions round
on no more than the three terms' magnitudes; d sig / sig = (1 - sig) times
the relative error of the exponential, plus the addition, the division and
the second order; where exp(-v) overflows sig is an exact 0 and the true one
is below the floor.)

MSE, d = x - t, loss_i = d^2, g = 2 d grad_scale: the subtraction and the
product with grad_scale round once each (the 2 is exact), |dg_i| <= 2 u |g_i|
+ 2^-149; the loss is one fmaf per element, whose term error (2 u d^2) the
factor 4 of bound_sum covers.

The elementwise kernels sum in three stages: a thread's grid-stride terms, the
six steps of the wave sum, one atomicAdd per wave.  No term takes part in
more than :func:`ew_chain` additions, which is the M of their bound_sum.
"""
import math
import typing as tp

import torch

from .bn_reference import U32, f32, sum_bound

__all__ = ["U32", "f32", "sum_bound", "K_EXP", "K_LOG", "K_LOG1P"]

# largest error seen by test_math_function_ulps on an MI355X (gfx950), in ulp
MEASURED_ULPS = {"exp": 0.9999, "log": 1.8807, "log1p": 0.5698}
K_EXP = 2
K_LOG = 3
K_LOG1P = 2

ETA = 2.0 ** -149            # fp32 subnormal spacing
FLOOR = (K_EXP + 3) * ETA
BF16_HALF_ULP = 2.0 ** -8    # of the value; 8 significand bits, nearest even
BF16_FLOOR = 2.0 ** -134


def mean_scale(n: int) -> float:
    """The ``1.0 / n`` of the autograd wrappers, as the kernel receives it."""
    return f32(1.0 / n)


def store_bound(dtype: torch.dtype, value: torch.Tensor,
                bound: torch.Tensor) -> torch.Tensor:
    """``bound`` on an fp32 value, widened by the store into ``dtype``."""
    if dtype == torch.float32:
        return bound
    assert dtype == torch.bfloat16, dtype
    return bound + BF16_HALF_ULP * (value.abs() + bound) + BF16_FLOOR


def ew_chain(n: int) -> int:
    """Most additions any term of an elementwise kernel's loss takes part in:
    ew_grid(n, 256, 4) blocks of 256 threads, a grid-stride loop, the wave
    sum, one atomic per wave and the value already in ``loss_sum``."""
    blocks = min(2048, max(1, -(-n // 1024)))
    per_thread = -(-n // (blocks * 256))
    return min(n, per_thread + 6 + blocks * 4) + 1


class CE(tp.NamedTuple):
    loss: torch.Tensor        # scalar: init + sum of the scaled rows
    grad: torch.Tensor        # [B, C] float64
    loss_bound: torch.Tensor  # scalar, fp32 kernel
    grad_bound: torch.Tensor  # [B, C], before the store (see store_bound)
    rows: torch.Tensor        # [B] scaled row losses
    p: torch.Tensor           # softmax
    t: torch.Tensor           # target distribution


def _onehot(t: torch.Tensor, B: int, C: int, w) -> torch.Tensor:
    """w at [b, t_b]; a target outside [0, C) marks no class."""
    cols = torch.arange(C, device=t.device)
    return (cols[None, :] == t[:, None]).double() * w


def _pick(x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """x[b, t_b], 0 where t_b is outside [0, C)."""
    C = x.shape[1]
    ok = (t >= 0) & (t < C)
    v = x.gather(1, t.clamp(0, C - 1)[:, None])[:, 0]
    return torch.where(ok, v, torch.zeros_like(v))


def cross_entropy(x: torch.Tensor, ta: torch.Tensor,
                  tb: tp.Optional[torch.Tensor] = None, lam: float = 1.0,
                  eps: float = 0.0, *, loss_scale: float, grad_scale: float,
                  init: float = 0.0, drop_last_in_sum: bool = False) -> CE:
    """The formula above k_cross_entropy_mix; k_cross_entropy is tb = ta,
    lam = 1, eps = 0.  ``init`` is what ``loss_sum`` held before.
    ``drop_last_in_sum`` is a mutant for tests: s without column C - 1."""
    x = x.double()
    B, C = x.shape
    tb = ta if tb is None else tb
    wa, wb, uni = (1.0 - eps) * lam, (1.0 - eps) * (1.0 - lam), eps / C
    mx = x.max(1, keepdim=True).values
    d = x - mx
    e = torch.exp(d)
    s = (e[:, :-1] if drop_last_in_sum else e).sum(1, keepdim=True)
    p = e / s
    logs = torch.log(s)[:, 0]
    lse = mx[:, 0] + logs
    t = uni + _onehot(ta, B, C, wa) + _onehot(tb, B, C, wb)
    grad = (p - t) * grad_scale
    ia, ib = wa * _pick(x, ta), wb * _pick(x, tb)
    # eps = 0 reads no mean: a -inf logit outside the targets keeps the loss
    iu = uni * x.sum(1) if eps > 0 else torch.zeros_like(ia)
    rows = (lse - (ia + ib + iu)) * loss_scale

    absd = torch.where(torch.isfinite(d), d.abs(), torch.zeros_like(d))
    H = (p * absd).sum(1, keepdim=True)
    rs = U32 * (C + 2 * K_EXP + H)
    dp = p * (U32 * (3 + 2 * K_EXP + absd + C) + U32 * (2 * K_EXP + H))
    grad_bound = (dp + 4 * U32 * t + U32 * (p + t)) * abs(grad_scale) \
        + U32 * grad.abs() + FLOOR
    inner_mag = ia.abs() + ib.abs() + iu.abs()
    sx_bound = 4 * C * U32 * x.abs().sum(1) * uni if eps > 0 else 0.0
    d_row = rs[:, 0] + 2 * K_LOG * U32 * logs.abs() + 2 * U32 * lse.abs() \
        + 7 * U32 * inner_mag + sx_bound
    d_rows = d_row * abs(loss_scale) + U32 * rows.abs()
    terms = torch.cat([rows.new_tensor([init]), rows])
    return CE(terms.sum(), grad, d_rows.sum() + sum_bound(terms), grad_bound,
              rows, p, t)


class EW(tp.NamedTuple):
    loss: torch.Tensor
    grad: torch.Tensor
    loss_bound: torch.Tensor
    grad_bound: torch.Tensor


def _ew_loss(terms: torch.Tensor, d_terms: torch.Tensor, loss_scale: float,
             init: float):
    n = terms.numel()
    total = terms.sum() * loss_scale + init
    mag = terms.abs().sum() * abs(loss_scale) + abs(init)
    bound = d_terms.sum() * abs(loss_scale) + 4 * ew_chain(n) * U32 * mag
    return total, bound


def bce_logits(x: torch.Tensor, target: float, *, loss_scale: float,
               grad_scale: float, init: float = 0.0) -> EW:
    v = x.double()
    e = torch.exp(-v.abs())
    l1p = torch.log1p(e)
    relu = v.clamp_min(0)
    vt = v * target
    terms = relu - vt + l1p
    d_terms = U32 * (2 * K_EXP * e / (1 + e) + 2 * K_LOG1P * l1p
                     + 3 * (relu + vt.abs() + l1p))
    sig = torch.sigmoid(v)
    grad = (sig - target) * grad_scale
    d_sig = sig * U32 * (3 + 2 * K_EXP * (1 - sig))
    grad_bound = (d_sig + U32 * (sig + abs(target))) * abs(grad_scale) \
        + U32 * grad.abs() + FLOOR
    loss, loss_bound = _ew_loss(terms, d_terms, loss_scale, init)
    return EW(loss, grad, loss_bound, grad_bound)


def mse(x: torch.Tensor, t: torch.Tensor, *, loss_scale: float,
        grad_scale: float, init: float = 0.0) -> EW:
    assert x.shape == t.shape, (x.shape, t.shape)
    d = x.double() - t.double()
    grad = 2.0 * d * grad_scale
    loss, loss_bound = _ew_loss(d * d, torch.zeros_like(d), loss_scale, init)
    return EW(loss, grad, loss_bound, 2 * U32 * grad.abs() + ETA)


def accuracy_count(x: torch.Tensor, target: torch.Tensor) -> int:
    """Rows whose first maximal column is the target: ties go to the smallest
    index, spelled out so that no argmax convention is borrowed."""
    x = x.double()
    B, C = x.shape
    mx = x.max(1, keepdim=True).values
    cols = torch.arange(C, device=x.device).expand(B, C)
    first = torch.where(x == mx, cols, torch.full_like(cols, C)).min(1).values
    return int((first == target).sum())


# ---------------------------------------------------------------------------
# the cases, shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------

BATCHES = (1, 4, 5, 37)
CLASSES = (1, 2, 63, 64, 65, 1000, 4097)
DTYPES = (torch.float32, torch.bfloat16)
EPS = (0.0, 0.1, 1.0)
LAMS = (0.0, 0.37, 1.0)
EW_SIZES = (1, 63, 64, 65, 1025)
EW_LARGE = 4 * 256 * 2048 + 3     # a second, ragged grid-stride iteration
BCE_TARGETS = (0.0, 1.0, 0.9)


def regimes(dtype: torch.dtype) -> tp.Tuple[str, ...]:
    last = "shift1e4" if dtype == torch.float32 else "int256"
    return ("randn3", "wide", last)


def row_case(B: int, C: int, dtype: torch.dtype, regime: str,
             neg_inf: bool = True):
    """(logits, ta, tb) on the CPU.  Targets include columns 0, C-1, 63 and 64
    where they exist; row 0 has its maximum repeated at column C-1 (so that
    column matters to every row sum test and argmax meets a tie).  With four
    rows or more the ``randn3`` regime has a row of equal logits (row 1) and,
    with ``neg_inf``, a row with about half of its non-target entries -inf
    (row 2).  tb equals ta in the first two rows and differs elsewhere."""
    g = torch.Generator().manual_seed(1000 * B + C)
    x = torch.randn(B, C, generator=g)
    if regime == "randn3":
        x = x * 3
    elif regime == "wide":
        x = x * 25
    elif regime == "shift1e4":
        x = x * 3 + 1e4
    elif regime == "int256":
        x = torch.randint(-6, 7, (B, C), generator=g).float() + 256
    else:
        raise ValueError(regime)
    ta = torch.randint(C, (B,), generator=g)
    for i, col in enumerate(c for c in (63, 64, 0, C - 1) if c < C):
        ta[(i + 2) % B] = col
    tb = (ta + 1) % C
    if B > 1:
        tb[:2] = ta[:2]
    if B >= 4 and regime == "randn3":
        x[1] = 0.75
        if neg_inf and C >= 3:
            drop = torch.rand(C, generator=g) < 0.5
            drop[ta[2]] = drop[tb[2]] = False
            if not drop.any():
                drop[(int(ta[2]) + 1) % C] = int(tb[2]) != (int(ta[2]) + 1) % C
            x[2, drop] = -math.inf
    if C > 1:
        x[0, C - 1] = x[0].max()
        if B == 1:  # whichever column the only target is, the loss is large
            x[0, 0] = x[0, C - 1] - 1
    return x.to(dtype), ta, tb


def tie_case(dtype: torch.dtype):
    """Rows whose maximum sits at two columns, in different lanes (c, c + 5)
    and in the same lane (c, c + 64); the target is the first occurrence in
    the even rows (counts) and the later one in the odd rows (does not)."""
    C = 200
    g = torch.Generator().manual_seed(7)
    x = torch.randn(8, C, generator=g)
    target = torch.empty(8, dtype=torch.int64)
    for r in range(8):
        c = 3 + 7 * r
        other = c + (5 if r < 4 else 64)
        x[r, c] = x[r, other] = 9.0
        target[r] = c if r % 2 == 0 else other
    return x.to(dtype), target


BCE_PLANTED = (0.0, 2.0 ** -10, -2.0 ** -10, 20.0, -20.0, 88.0, -88.0, 104.0,
               -104.0)


def bce_case(n: int, dtype: torch.dtype) -> torch.Tensor:
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 2
    planted = BCE_PLANTED + ((1e4, -1e4) if dtype == torch.float32 else ())
    k = min(n, len(planted))
    # the last elements too, so the ragged tail of a large n sees them
    x[:k] = torch.tensor(planted[:k])
    x[n - k:] = torch.tensor(planted[:k])
    return x.to(dtype)


MSE_STRETCH_N = 320


def mse_case(n: int, dtype: torch.dtype, kind: str):
    """``random``; ``stretch``: x == t in the 256 consecutive elements from 64
    on.  At n = 320 that is one block whose waves 1 to 3 see only such
    elements, sum to zero and skip their atomic, while wave 0 has both kinds;
    ``equal``: x == t everywhere."""
    g = torch.Generator().manual_seed(n + 1)
    x = torch.randn(n, generator=g).to(dtype)
    t = torch.randn(n, generator=g).to(dtype)
    if kind == "stretch":
        assert n >= 320, n
        t[64:320] = x[64:320]
    elif kind == "equal":
        t = x.clone()
    else:
        assert kind == "random", kind
    return x, t


class RowJob(tp.NamedTuple):
    name: str
    x: torch.Tensor
    ta: torch.Tensor
    tb: tp.Optional[torch.Tensor]   # None: the kernel's null target_b
    lam: tp.Optional[float]         # None: the kernel's null lam pointer
    eps: float
    mix: bool                       # k_cross_entropy_mix, else k_cross_entropy


def row_jobs(dtype: torch.dtype) -> tp.Iterator[RowJob]:
    """Every cross-entropy case: the plain kernel over B x C x regime; the mix
    kernel over B x C x eps x lam on the ``randn3`` set (the -inf row only at
    eps = 0: with smoothing its loss is infinite by definition), once with
    null ``target_b`` and ``lam``, and once per other regime."""
    tag = "fp32" if dtype == torch.float32 else "bf16"
    for B in BATCHES:
        for C in CLASSES:
            for regime in regimes(dtype):
                x, ta, tb = row_case(B, C, dtype, regime)
                yield RowJob(f"ce {tag} {regime} B{B} C{C}", x, ta, None, None,
                             0.0, False)
            x_inf, ta, tb = row_case(B, C, dtype, "randn3")
            x_fin = row_case(B, C, dtype, "randn3", neg_inf=False)[0]
            for eps in EPS:
                for lam in LAMS:
                    yield RowJob(f"mix {tag} randn3 B{B} C{C} eps{eps} "
                                 f"lam{lam}", x_inf if eps == 0 else x_fin,
                                 ta, tb, lam, eps, True)
            yield RowJob(f"mix {tag} randn3 B{B} C{C} eps0.1 null", x_fin, ta,
                         None, None, 0.1, True)
            for regime, eps in zip(regimes(dtype)[1:], (0.1, 0.0)):
                x, ta, tb = row_case(B, C, dtype, regime)
                yield RowJob(f"mix {tag} {regime} B{B} C{C} eps{eps} lam0.37",
                             x, ta, tb, 0.37, eps, True)


def row_oracle(job: RowJob, x: torch.Tensor, ta: torch.Tensor,
               tb: tp.Optional[torch.Tensor], *, loss_scale: float,
               grad_scale: float, init: float = 0.0, **kw) -> CE:
    """:func:`cross_entropy` with the job's scalars as the kernel gets them."""
    return cross_entropy(x, ta, tb, 1.0 if job.lam is None else f32(job.lam),
                         f32(job.eps), loss_scale=loss_scale,
                         grad_scale=grad_scale, init=init, **kw)
