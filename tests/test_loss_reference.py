# Copyright (c) Flashy-AMD authors.
"""The float64 loss oracle (tests/loss_reference.py) against torch's own
float64 losses, and its bounds from both sides: torch's CPU fp32 losses lie
inside them on every case the GPU test runs, and a kernel that is wrong in
one of the listed ways lies outside.  No GPU.

A mutant is applied wherever what it changes enters the formula: C = 1 has an
identically zero gradient and loss (forward-only), the one-hot mutants need a
one-hot weight (eps < 1), the weight swap needs lam = 0.37 and rows with
ta != tb."""
import pytest
import torch
import torch.nn.functional as F

from tests import loss_reference as R

DTYPES = [pytest.param(d, id=str(d).split(".")[1]) for d in R.DTYPES]


def _close(got, want, rel=1e-12):
    scale = want.abs().max().clamp_min(1e-300)
    assert ((got - want).abs().max() <= rel * scale), (got, want)


# -- the oracle against torch float64 ----------------------------------------

@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("lam", R.LAMS)
@pytest.mark.parametrize("B,C", [(5, 65), (37, 1000), (4, 2)])
def test_cross_entropy_oracle_matches_torch_float64(B, C, lam, eps):
    x, ta, tb = R.row_case(B, C, torch.float32, "randn3", neg_inf=eps == 0)
    x64 = x.double().requires_grad_(True)
    want = lam * F.cross_entropy(x64, ta, label_smoothing=eps) \
        + (1 - lam) * F.cross_entropy(x64, tb, label_smoothing=eps)
    want.backward()
    got = R.cross_entropy(x, ta, tb, lam, eps, loss_scale=1.0 / B,
                          grad_scale=1.0 / B)
    _close(got.loss, want.detach())
    _close(got.grad, x64.grad)
    if lam == 1:  # the plain kernel's case
        plain = R.cross_entropy(x, ta, loss_scale=1.0 / B, grad_scale=1.0 / B,
                                eps=eps)
        _close(plain.grad, x64.grad)
        _close(plain.loss, want.detach())


def test_out_of_range_target_is_no_class():
    x, ta, _ = R.row_case(5, 65, torch.float32, "randn3", neg_inf=False)
    ta[2], ta[3] = -1, 65
    got = R.cross_entropy(x, ta, loss_scale=1.0, grad_scale=1.0)
    x64 = x.double()
    for r in (2, 3):
        _close(got.grad[r], torch.softmax(x64[r], 0))
        _close(got.rows[r], torch.logsumexp(x64[r], 0))


@pytest.mark.parametrize("target", R.BCE_TARGETS)
def test_bce_oracle_matches_torch_float64(target):
    x64 = R.bce_case(1025, torch.float32).double().requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(
        x64, torch.full_like(x64, target))
    want.backward()
    got = R.bce_logits(x64.detach(), target, loss_scale=1.0 / 1025,
                       grad_scale=1.0 / 1025)
    _close(got.loss, want.detach())
    _close(got.grad, x64.grad)


def test_mse_oracle_matches_torch_float64():
    x, t = R.mse_case(1025, torch.float32, "random")
    x64 = x.double().requires_grad_(True)
    want = F.mse_loss(x64, t.double())
    want.backward()
    got = R.mse(x, t, loss_scale=1.0 / 1025, grad_scale=1.0 / 1025)
    _close(got.loss, want.detach())
    _close(got.grad, x64.grad)


def test_accuracy_oracle_spells_out_ties():
    x, target = R.tie_case(torch.float32)
    assert R.accuracy_count(x, target) == 4
    for dtype in R.DTYPES:
        x, ta, _ = R.row_case(37, 1000, dtype, "randn3")
        assert R.accuracy_count(x, ta) == int(
            (x.float().argmax(1) == ta).sum())


# -- torch fp32 inside, mutants outside --------------------------------------

def _outside(mutant, ref, bound, dtype):
    return bool(((mutant.to(dtype).double() - ref).abs() > bound).any())


def _torch_fp32_rows(job, ls, gs):
    x32 = job.x.float().clone().requires_grad_(True)
    tb = job.ta if job.tb is None else job.tb
    lam = torch.tensor(1.0 if job.lam is None else job.lam)
    eps = job.eps
    total = lam * F.cross_entropy(x32, job.ta, label_smoothing=eps,
                                  reduction="sum") \
        + (1 - lam) * F.cross_entropy(x32, tb, label_smoothing=eps,
                                      reduction="sum")
    (total * torch.tensor(gs)).backward()
    return (total.detach() * torch.tensor(ls)), x32.grad


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_bounds_hold_torch_fp32_and_reject_mutants(dtype):
    n_mut = 0
    for job in R.row_jobs(dtype):
        B, C = job.x.shape
        ls, gs = R.mean_scale(B), R.f32(0.5 / B)
        ref = R.row_oracle(job, job.x, job.ta, job.tb, loss_scale=ls,
                           grad_scale=gs)
        gb = R.store_bound(dtype, ref.grad, ref.grad_bound)
        assert torch.isfinite(ref.loss) and torch.isfinite(ref.grad).all()
        loss32, grad32 = _torch_fp32_rows(job, ls, gs)
        assert not _outside(grad32, ref.grad, gb, dtype), job.name
        assert (loss32.double() - ref.loss).abs() <= ref.loss_bound, job.name
        if C == 1:  # forward-only: nothing to mutate
            assert not ref.grad.any() and ref.loss == 0, job.name
            continue

        def again(ta=job.ta, tb=job.tb, lam=job.lam, **kw):
            return R.row_oracle(job._replace(lam=lam), job.x, ta, tb,
                                loss_scale=ls, grad_scale=gs, **kw)

        mutants = {"zero": torch.zeros_like(ref.grad)}
        if C % 64:
            mutants["sum without the last column"] = \
                again(drop_last_in_sum=True).grad
        if job.eps < 1:
            tb1 = None if job.tb is None else (job.tb + 1) % C
            mutants["one-hot at tgt + 1"] = again((job.ta + 1) % C, tb1).grad
        unscaled = ref.grad.clone()
        unscaled[-1] /= gs
        mutants["last row unscaled"] = unscaled
        if job.eps > 0:
            mutants["eps / C dropped"] = \
                (ref.p - (ref.t - R.f32(job.eps) / C)) * gs
        if job.lam == 0.37 and job.eps < 1:
            assert bool((job.ta != job.tb).any()), job.name
            mutants["wa and wb swapped"] = again(lam=1 - 0.37).grad
        for what, g in mutants.items():
            assert _outside(g, ref.grad, gb, dtype), (job.name, what)
            n_mut += 1
        short = ref.loss - ref.rows[ref.rows.abs().argmax()]
        assert _outside(short, ref.loss, ref.loss_bound, torch.float32), \
            (job.name, "loss without one row")
    assert n_mut > 1000


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("target", R.BCE_TARGETS)
def test_bce_bounds_hold_torch_fp32_and_reject_mutants(dtype, target):
    for n in R.EW_SIZES + (R.EW_LARGE,):
        x = R.bce_case(n, dtype)
        ls, gs = R.mean_scale(n), R.f32(0.5 / n)
        t32 = R.f32(target)
        ref = R.bce_logits(x, t32, loss_scale=ls, grad_scale=gs)
        gb = R.store_bound(dtype, ref.grad, ref.grad_bound)
        x32 = x.float().clone().requires_grad_(True)
        total = F.binary_cross_entropy_with_logits(
            x32, torch.full_like(x32, target), reduction="sum")
        (total * torch.tensor(gs)).backward()
        assert not _outside(x32.grad, ref.grad, gb, dtype), n
        loss32 = (total.detach() * torch.tensor(ls)).double()
        assert (loss32 - ref.loss).abs() <= ref.loss_bound, n
        flipped = R.bce_logits(x, 1 - t32, loss_scale=ls, grad_scale=gs)
        mutants = {"zero": torch.zeros_like(ref.grad),
                   "target 1 - target": flipped.grad}
        unscaled = ref.grad.clone()
        unscaled[ref.grad.abs().argmax()] /= gs
        mutants["one element unscaled"] = unscaled
        for what, g in mutants.items():
            assert _outside(g, ref.grad, gb, dtype), (n, what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mse_bounds_hold_torch_fp32_and_reject_mutants(dtype):
    sizes = [(n, "random") for n in R.EW_SIZES + (R.EW_LARGE,)] \
        + [(R.MSE_STRETCH_N, "stretch")]
    for n, kind in sizes:
        x, t = R.mse_case(n, dtype, kind)
        ls, gs = R.mean_scale(n), R.f32(0.5 / n)
        ref = R.mse(x, t, loss_scale=ls, grad_scale=gs)
        gb = R.store_bound(dtype, ref.grad, ref.grad_bound)
        x32 = x.float().clone().requires_grad_(True)
        total = F.mse_loss(x32, t.float(), reduction="sum")
        (total * torch.tensor(gs)).backward()
        assert not _outside(x32.grad, ref.grad, gb, dtype), (n, kind)
        loss32 = (total.detach() * torch.tensor(ls)).double()
        assert (loss32 - ref.loss).abs() <= ref.loss_bound, (n, kind)
        unscaled = ref.grad.clone()
        unscaled[0] /= gs
        for what, g in {"zero": torch.zeros_like(ref.grad),
                        "without the factor 2": ref.grad / 2,
                        "first element unscaled": unscaled}.items():
            assert _outside(g, ref.grad, gb, dtype), (n, kind, what)
        if n <= 1025:
            d2 = (x.double() - t.double()) ** 2
            short = ref.loss - d2.max() * ls
            assert (short - ref.loss).abs() > ref.loss_bound, (n, kind)
    x, t = R.mse_case(65, dtype, "equal")
    ref = R.mse(x, t, loss_scale=1.0, grad_scale=1.0, init=1.5)
    assert ref.loss == 1.5 and not ref.grad.any()


# -- never looser than the tolerances it replaces -----------------------------
# The inputs of test_cross_entropy_gpu, test_bce_logits_gpu, test_mse_gpu
# (tests/test_ops_gpu.py) and test_cross_entropy_mix_kernel
# (tests/test_mix_gpu.py): the same seeds, shapes and recipes, drawn here from
# the CPU generator.  Those tests assert the same inequality on the tensors
# they actually draw.

def _old(dtype, ref):
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    return tol + tol * ref.abs()


def tighter(dtype, ref, bound) -> bool:
    return bool((bound <= _old(dtype, ref)).all())


def loss_tighter(dtype, ref, bound) -> bool:
    """The gradient bounds are tighter everywhere.  The fp32 loss bound is
    not: bound_sum = 4 (B + 1) u S alone is 1.5e-5 of the loss at B = 64,
    above the old rtol of 1e-5, so the four tests keep their old loss
    assertion and add the oracle's; only bf16 (2e-2) is claimed here."""
    return dtype == torch.float32 or tighter(dtype, ref, bound)


@pytest.mark.parametrize("dtype,B,C", [
    (torch.float32, 64, 10), (torch.bfloat16, 64, 10),
    (torch.float32, 128, 1000), (torch.bfloat16, 37, 1000)])
def test_new_bound_within_old_tolerance_cross_entropy(dtype, B, C):
    torch.manual_seed(1)
    x = (torch.randn(B, C) * 3).to(dtype)
    target = torch.randint(C, (B,))
    s = R.mean_scale(B)
    ref = R.cross_entropy(x, target, loss_scale=s, grad_scale=s)
    assert tighter(dtype, ref.grad,
                   R.store_bound(dtype, ref.grad, ref.grad_bound))
    assert loss_tighter(dtype, ref.loss, ref.loss_bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("target", [0.0, 1.0])
def test_new_bound_within_old_tolerance_bce(dtype, target):
    torch.manual_seed(2)
    x = (torch.randn(64, 33) * 2).to(dtype)
    s = R.mean_scale(x.numel())
    ref = R.bce_logits(x, target, loss_scale=s, grad_scale=s)
    assert tighter(dtype, ref.grad,
                   R.store_bound(dtype, ref.grad, ref.grad_bound))
    assert loss_tighter(dtype, ref.loss, ref.loss_bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_new_bound_within_old_tolerance_mse(dtype):
    torch.manual_seed(4)
    x = torch.randn(64, 33).to(dtype)
    t = torch.randn(64, 33).to(dtype)
    s = R.mean_scale(x.numel())
    ref = R.mse(x, t, loss_scale=s, grad_scale=s)
    assert tighter(dtype, ref.grad,
                   R.store_bound(dtype, ref.grad, ref.grad_bound))
    assert loss_tighter(dtype, ref.loss, ref.loss_bound)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 10, 33, 1000])
@pytest.mark.parametrize("B", [5, 64])
def test_new_bound_within_old_tolerance_mix(B, C, dtype, eps):
    torch.manual_seed(1)
    x = (torch.randn(B, C) * 3).to(dtype)
    ta = torch.randint(C, (B,))
    tb = ta.flip(0).contiguous()
    tb[:2] = ta[:2]
    s = R.mean_scale(B)
    for lam in (0.0, 1.0, 0.37):
        ref = R.cross_entropy(x, ta, tb, R.f32(lam), R.f32(eps), loss_scale=s,
                              grad_scale=s)
        assert tighter(dtype, ref.grad,
                       R.store_bound(dtype, ref.grad, ref.grad_bound))
        assert loss_tighter(dtype, ref.loss, ref.loss_bound)


def test_mse_loss_rejects_a_shape_mismatch_on_the_cpu_too():
    from flashy_amd.functional import mse_loss
    with pytest.raises(ValueError):
        mse_loss(torch.randn(64, 33), torch.randn(64, 1))
