# Copyright (c) Flashy-AMD authors.
"""The loss and accuracy kernels of csrc/losses.hip against the float64
oracle of tests/loss_reference.py, with the bounds derived there: the cases
and what they must reach are listed in that module (``row_jobs`` and the
``*_case`` builders), shared with tests/test_loss_reference.py, which shows on
the CPU that the bounds reject wrong kernels.

Every gradient is written into a window in the middle of a larger buffer whose
guard elements must come back bitwise unchanged, and every loss is added onto
1.5 (the += contract of ``loss_sum``)."""
import math

import pytest
import torch

from tests import loss_reference as R

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")
DTYPES = [pytest.param(d, id=str(d).split(".")[1]) for d in R.DTYPES]
GUARD = 64
NAN_BITS = 0x7fc00000
BF16_BITS = 0x5aa5           # 2.3e16: far outside every bound if left behind
INIT = 1.5


def _window(shape, dtype):
    """(buffer, window): the window is a contiguous ``shape`` in the middle of
    the buffer, which is NaN (fp32) or a fixed bf16 pattern throughout."""
    n = math.prod(shape)
    if dtype == torch.float32:
        buf = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
        buf.view(torch.int32).fill_(NAN_BITS)
    else:
        buf = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
        buf.view(torch.int16).fill_(BF16_BITS)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(name, buf):
    if buf.dtype == torch.float32:
        bits, want = buf.view(torch.int32), NAN_BITS
    else:
        bits, want = buf.view(torch.int16), BF16_BITS
    assert bool((bits[:GUARD] == want).all()), (name, "guard before")
    assert bool((bits[-GUARD:] == want).all()), (name, "guard after")


class Worst:
    """The worst err/bound per kernel and quantity, printed once per test."""

    def __init__(self):
        self.worst = {}

    def within(self, key, name, got, want, bound):
        assert torch.isfinite(got).all(), name
        err = (got.double() - want).abs()
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        self.worst[key] = max(self.worst.get(key, 0.0), ratio)
        assert bool((err <= bound).all()), (name, key, err.max().item(), ratio)

    def report(self, tag):
        for key, ratio in sorted(self.worst.items()):
            print(f"{tag} {key}: max err/bound {ratio:.3e}")


def _loss_sum():
    return torch.full((1,), INIT, dtype=torch.float32, device="cuda")


# -- the device math functions behind K_EXP, K_LOG, K_LOG1P -------------------

def _ulps(got32, ref64):
    e = torch.floor(torch.log2(ref64.abs())) + 1    # |ref| in [2^(e-1), 2^e)
    ulp = torch.exp2((e - 24).clamp_min(-149))
    return ((got32.double() - ref64).abs() / ulp).max().item()


@requires_gpu
def test_math_function_ulps():
    """exp, log and log1p in fp32 against float64 over the ranges the cases
    use; each constant of loss_reference is at least the largest error,
    rounded up to a whole ulp, plus one."""
    g = torch.Generator(device="cuda").manual_seed(0)
    n = 1 << 21
    r = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    ranges = {
        "exp": (torch.exp, -104.0 * r, R.K_EXP),
        "log": (torch.log, 1.0 + 4096.0 * r, R.K_LOG),
        "log1p": (torch.log1p, 1.0 - r, R.K_LOG1P),      # (0, 1]
    }
    seen = {}
    for name, (fn, arg, k) in ranges.items():
        arg32 = arg.float()
        seen[name] = _ulps(fn(arg32), fn(arg32.double()))
        print(f"{name}: max error {seen[name]:.4f} ulp, constant {k}")
    for name, (_, _, k) in ranges.items():
        assert math.ceil(seen[name]) + 1 <= k, (name, seen[name], k)


# -- the row kernels ----------------------------------------------------------

def _launch_row(job, x, ta, tb, lam_dev, dl, loss, ls, gs):
    from flashy_amd import ops
    if not job.mix:
        ops.cross_entropy_fwd_bwd(x, ta, dl, loss, loss_scale=ls,
                                  grad_scale=gs)
        return
    if job.lam is not None:
        lam_dev.fill_(job.lam)                   # one device tensor throughout
    ops.cross_entropy_mix_fwd_bwd(
        x, ta, tb, lam_dev if job.lam is not None else None, dl, loss,
        job.eps, loss_scale=ls, grad_scale=gs)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_kernels_against_oracle(dtype):
    from flashy_amd import ops
    worst = Worst()
    lam_dev = torch.ones((), dtype=torch.float32, device="cuda")
    for job in R.row_jobs(dtype):
        B, C = job.x.shape
        ls, gs = R.mean_scale(B), R.f32(0.5 / B)
        x, ta = job.x.cuda(), job.ta.cuda()
        tb = None if job.tb is None else job.tb.cuda()
        buf, dl = _window((B, C), dtype)
        loss = _loss_sum()
        _launch_row(job, x, ta, tb, lam_dev, dl, loss, ls, gs)
        ref = R.row_oracle(job, x, ta, tb, loss_scale=ls, grad_scale=gs,
                           init=INIT)
        kernel = "k_cross_entropy_mix" if job.mix else "k_cross_entropy"
        worst.within(f"{kernel} dlogits", job.name, dl, ref.grad,
                     R.store_bound(dtype, ref.grad, ref.grad_bound))
        worst.within(f"{kernel} loss", job.name, loss[0], ref.loss,
                     ref.loss_bound)
        _guards_intact(job.name, buf)
        # where the probability underflows (or the logit is -inf) and no
        # target weight falls, the gradient is an exact zero
        d = x.double() - x.double().max(1, keepdim=True).values
        dead = (d < -110) & (ref.t == 0)
        assert bool((dl[dead] == 0).all()), job.name
        if not job.mix:
            out = torch.zeros((), dtype=torch.float32, device="cuda")
            ops.accuracy_count(x, ta, out)
            assert out.item() == R.accuracy_count(x, ta), job.name
    worst.report(str(dtype))


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_accuracy_ties_go_to_the_first_column(dtype):
    from flashy_amd import ops
    x, target = (t.cuda() for t in R.tie_case(dtype))
    out = torch.zeros((), dtype=torch.float32, device="cuda")
    ops.accuracy_count(x, target, out)
    assert out.item() == R.accuracy_count(x, target) == 4


# -- the elementwise kernels --------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_bce_kernel_against_oracle(dtype):
    from flashy_amd import ops
    worst = Worst()
    for n in R.EW_SIZES + (R.EW_LARGE,):
        x = R.bce_case(n, dtype).cuda()
        ls, gs = R.mean_scale(n), R.f32(0.5 / n)
        for target in R.BCE_TARGETS:
            name = f"bce n{n} t{target}"
            buf, dx = _window((n,), dtype)
            loss = _loss_sum()
            ops.bce_logits_fwd_bwd(x, dx, loss, target, loss_scale=ls,
                                   grad_scale=gs)
            ref = R.bce_logits(x, R.f32(target), loss_scale=ls, grad_scale=gs,
                               init=INIT)
            worst.within("k_bce_logits dx", name, dx, ref.grad,
                         R.store_bound(dtype, ref.grad, ref.grad_bound))
            worst.within("k_bce_logits loss", name, loss[0], ref.loss,
                         ref.loss_bound)
            _guards_intact(name, buf)
    worst.report(str(dtype))


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_mse_kernel_against_oracle(dtype):
    from flashy_amd import ops
    worst = Worst()
    sizes = [(n, "random") for n in R.EW_SIZES + (R.EW_LARGE,)] \
        + [(R.MSE_STRETCH_N, "stretch"), (65, "equal"), (1025, "equal")]
    for n, kind in sizes:
        name = f"mse n{n} {kind}"
        x, t = (v.cuda() for v in R.mse_case(n, dtype, kind))
        ls, gs = R.mean_scale(n), R.f32(0.5 / n)
        buf, dx = _window((n,), dtype)
        loss = _loss_sum()
        ops.mse_fwd_bwd(x, t, dx, loss, loss_scale=ls, grad_scale=gs)
        ref = R.mse(x, t, loss_scale=ls, grad_scale=gs, init=INIT)
        worst.within("k_mse dx", name, dx, ref.grad,
                     R.store_bound(dtype, ref.grad, ref.grad_bound))
        worst.within("k_mse loss", name, loss[0], ref.loss, ref.loss_bound)
        _guards_intact(name, buf)
        if kind == "equal":
            assert loss.item() == INIT and not bool(dx.any()), name
    worst.report(str(dtype))


# -- through flashy_amd.functional -------------------------------------------

def _half_ulp(dtype):
    return R.U32 if dtype == torch.float32 else R.BF16_HALF_ULP


def _routes(dtype, B=5, C=65):
    """(name, call(x) -> loss, oracle(x) -> (loss, grad, loss_bound,
    grad_bound)) for the four autograd functions on a [B, C] input."""
    import flashy_amd.functional as FF
    from flashy_amd.data import MixedTarget
    x0, ta, tb = R.row_case(B, C, dtype, "randn3", neg_inf=False)
    ta, tb = ta.cuda(), tb.cuda()
    lam = torch.full((), 0.37, dtype=torch.float32, device="cuda")
    g = torch.Generator().manual_seed(3)
    t_mse = torch.randn(C, B, generator=g).to(dtype).cuda().t()   # strided
    sB, sn = R.mean_scale(B), R.mean_scale(B * C)

    def ce(x, **kw):
        return R.cross_entropy(x, ta, loss_scale=sB, grad_scale=sB, **kw)

    def mix(x):
        return R.cross_entropy(x, ta, tb, R.f32(0.37), R.f32(0.1),
                               loss_scale=sB, grad_scale=sB)

    return x0, [
        ("cross_entropy", lambda x: FF.cross_entropy(x, ta), ce),
        ("cross_entropy_mix",
         lambda x: FF.cross_entropy(x, MixedTarget(ta, tb, lam),
                                    label_smoothing=0.1), mix),
        ("bce", lambda x: FF.bce_with_logits_const(x, 0.9),
         lambda x: R.bce_logits(x, R.f32(0.9), loss_scale=sn,
                                grad_scale=sn)),
        ("mse", lambda x: FF.mse_loss(x, t_mse),
         lambda x: R.mse(x, t_mse, loss_scale=sn, grad_scale=sn)),
    ]


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_scales_and_accumulates(dtype):
    """(loss * 0.5).backward(), then the same logits again with 0.25: the
    gradient is 0.75 of the oracle's.  Both factors are powers of two, so
    the two products are exact and the sum rounds once more."""
    worst = Worst()
    x0, routes = _routes(dtype)
    for name, call, oracle in routes:
        x = x0.cuda().requires_grad_(True)
        first = call(x)
        (first * 0.5).backward()
        (call(x) * 0.25).backward()
        ref = oracle(x.detach())
        gb = 0.75 * R.store_bound(dtype, ref.grad, ref.grad_bound)
        want = 0.75 * ref.grad
        worst.within(f"{name} grad", name, x.grad, want,
                     gb + _half_ulp(dtype) * (want.abs() + gb) + R.ETA)
        worst.within(f"{name} loss", name, first.detach(), ref.loss,
                     ref.loss_bound)
    worst.report(str(dtype))


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_label_smoothing_zero_reaches_the_plain_kernel(dtype):
    from flashy_amd import ops
    from flashy_amd.functional import cross_entropy
    x0, ta, _ = R.row_case(5, 65, dtype, "randn3")
    x, ta = x0.cuda().requires_grad_(True), ta.cuda()
    cross_entropy(x, ta, label_smoothing=0.0).backward()
    want = torch.empty_like(x0, device="cuda")
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    s = 1.0 / 5
    ops.cross_entropy_fwd_bwd(x.detach(), ta, want, loss, loss_scale=s,
                              grad_scale=s)
    assert torch.equal(x.grad, want)


# -- the four defects ---------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_input_gives_the_logical_gradient(dtype):
    """A transposed [C, B] base as input (and a transposed MSE target): the
    loss and the gradient, read logically, are the oracle's.  The gradient
    buffer used to take the input's strides while the kernel wrote row-major
    (and the mix entry refused the input)."""
    worst = Worst()
    x0, routes = _routes(dtype)
    for name, call, oracle in routes:
        base = x0.t().contiguous().cuda()                    # [C, B]
        x = base.permute(1, 0).detach().requires_grad_(True)
        assert not x.is_contiguous() and x.is_leaf
        loss = call(x)
        loss.backward()
        ref = oracle(x.detach())
        worst.within(f"{name} grad", name, x.grad, ref.grad,
                     R.store_bound(dtype, ref.grad, ref.grad_bound))
        worst.within(f"{name} loss", name, loss.detach(), ref.loss,
                     ref.loss_bound)
    worst.report(str(dtype))


@requires_gpu
@pytest.mark.parametrize("route", ["plain", "smoothed", "mixed", "accuracy"])
def test_strided_target_is_read_by_its_stride(route):
    """``pairs[:, 0]`` of a [B, 2] tensor whose other column holds different
    valid labels, which a stride-1 read would pick up."""
    import flashy_amd.functional as FF
    from flashy_amd.data import MixedTarget
    B, C, dtype = 5, 65, torch.float32
    x0, ta, tb = R.row_case(B, C, dtype, "randn3", neg_inf=False)
    pairs_a = torch.stack([ta, (ta + 7) % C], 1).cuda()
    pairs_b = torch.stack([tb, (tb + 11) % C], 1).cuda()
    sa, sb = pairs_a[:, 0], pairs_b[:, 0]
    assert not sa.is_contiguous()
    ta, tb = ta.cuda(), tb.cuda()
    s = R.mean_scale(B)
    x = x0.cuda().requires_grad_(True)
    if route == "accuracy":
        got = FF.accuracy(x.detach(), sa)
        assert got.item() == R.accuracy_count(x.detach(), ta) / B
        # and with every row a hit, which a stride-1 read would halve
        hits = x0.double().argmax(1).cuda()
        pairs_h = torch.stack([hits, (hits + 1) % C], 1)
        want = R.accuracy_count(x.detach(), hits)
        assert want >= B - 1
        assert FF.accuracy(x.detach(), pairs_h[:, 0]).item() == want / B
        return
    if route == "plain":
        loss = FF.cross_entropy(x, sa)
        ref = R.cross_entropy(x0.cuda(), ta, loss_scale=s, grad_scale=s)
    elif route == "smoothed":
        loss = FF.cross_entropy(x, sa, label_smoothing=0.1)
        ref = R.cross_entropy(x0.cuda(), ta, eps=R.f32(0.1), loss_scale=s,
                              grad_scale=s)
    else:
        lam = torch.full((), 0.37, dtype=torch.float32, device="cuda")
        loss = FF.cross_entropy(x, MixedTarget(sa, sb, lam))
        ref = R.cross_entropy(x0.cuda(), ta, tb, R.f32(0.37), loss_scale=s,
                              grad_scale=s)
    loss.backward()
    worst = Worst()
    worst.within("grad", route, x.grad, ref.grad, ref.grad_bound)
    worst.within("loss", route, loss.detach(), ref.loss, ref.loss_bound)
    worst.report(route)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])
def test_target_out_of_range_marks_no_class(mix, dtype):
    """Targets -1 and C: the row's gradient is the softmax alone and its loss
    is lse, in both kernels.  The logits are rows 1..B of a [B + 2, C]
    allocation and the rows next to the two hold 1e3, so the unguarded read
    the plain kernel used to do stays inside the allocation and shows in the
    loss."""
    from flashy_amd import ops
    B, C = 5, 65
    x0, ta, tb = R.row_case(B, C, dtype, "randn3", neg_inf=False)
    alloc = torch.full((B + 2, C), 1e3, dtype=dtype, device="cuda")
    alloc[1:B + 1] = x0.cuda()
    alloc[2] = 1e3                     # logits row 1, read by target -1 below
    alloc[5] = 1e3                     # logits row 4, read by target C above
    x = alloc[1:B + 1]
    assert x.is_contiguous()
    ta, tb = ta.cuda(), tb.cuda()
    ta[2], ta[3] = -1, C
    tb[2], tb[3] = C, -1
    ls, gs = R.mean_scale(B), R.f32(0.5 / B)
    buf, dl = _window((B, C), dtype)
    loss = _loss_sum()
    if mix:
        lam = torch.full((), 0.37, dtype=torch.float32, device="cuda")
        ops.cross_entropy_mix_fwd_bwd(x, ta, tb, lam, dl, loss, 0.1,
                                      loss_scale=ls, grad_scale=gs)
        ref = R.cross_entropy(x, ta, tb, R.f32(0.37), R.f32(0.1),
                              loss_scale=ls, grad_scale=gs, init=INIT)
    else:
        ops.cross_entropy_fwd_bwd(x, ta, dl, loss, loss_scale=ls,
                                  grad_scale=gs)
        ref = R.cross_entropy(x, ta, loss_scale=ls, grad_scale=gs, init=INIT)
    worst = Worst()
    worst.within("dlogits", "out of range", dl, ref.grad,
                 R.store_bound(dtype, ref.grad, ref.grad_bound))
    worst.within("loss", "out of range", loss[0], ref.loss, ref.loss_bound)
    _guards_intact("out of range", buf)
    worst.report(f"{'mix' if mix else 'plain'} {dtype}")


@requires_gpu
def test_mse_loss_rejects_a_shape_mismatch():
    """No broadcasting: the kernel runs over x.numel() elements of both."""
    from flashy_amd.functional import mse_loss
    x = torch.randn(64, 33, device="cuda", requires_grad=True)
    t = torch.randn(64, 1, device="cuda")
    with pytest.raises(ValueError):
        mse_loss(x, t)
