# Copyright (c) Flashy-AMD authors.
"""Single-kernel BatchNorm for small-M layers (k_bn_fwd_small,
k_bn_bwd_small), forced through ops.bn_fwd_small / ops.bn_bwd_small so the
plan cannot route around them.

Forward: y, work and both running statistics are torch.equal to bn_finalize +
bn_apply on the same partials.

Backward: dz is torch.equal to the chain's.  dgamma/dbeta are held to a
float64 reference with a derived bound: any fp32 summation order of M terms
is within M * 2^-24 * S of the exact sum (S = float64 sum of the terms'
absolute values); 4x that also covers the few-ulp error of the fp32 xhat.
The chain is held to the same bound on the same inputs.  dx is held to
max|dx - ref64| / max|ref64| <= 2^-8 (one bf16 rounding), ref64 built from
the bf16-rounded dz the chain's apply reads.

Shapes: M = 1 and 70 (fewer rows than threads), 300 and 1030 (ragged tail
over several rows per thread; 1030 is also past the 4-rows-in-registers
form), C = 64 (smallest grid) and 192 (not a power of two).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

SHAPES = [(1, 1, 1, 64), (2, 7, 5, 192), (3, 10, 10, 64), (2, 5, 103, 192),
          (1, 10, 30, 192), (1, 10, 103, 64)]     # (N, H, W, C)
FLAGS = [(False, False, 0.0), (True, False, 0.0), (False, True, 0.0),
         (True, True, 0.0), (True, True, 0.2)]    # (relu, res, slope)
EPS, MOM = 1e-5, 0.1


def _bwd_forms():
    from flashy_amd import ops
    return [f for f in ops.BN_BWD_SMALL_FORMS if f != "chain"]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    N, H, W, C = shape
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    x = (rnd(N, H, W, C) * 1.5 + 0.3).to(torch.bfloat16)
    res = rnd(N, H, W, C).to(torch.bfloat16)
    dy = rnd(N, H, W, C).to(torch.bfloat16)
    gamma = 1.0 + 0.5 * rnd(C)
    beta = 0.3 * rnd(C)
    rmean = 0.1 * rnd(C)
    rvar = 1.0 + 0.1 * rnd(C).abs()
    return x, res, dy, gamma, beta, rmean, rvar


def _chain_fwd(partials, msplit, x, res, gamma, beta, rmean, rvar, relu,
               slope):
    from flashy_amd import ops
    M, C = x.numel() // x.shape[-1], x.shape[-1]
    work = torch.empty(4 * C, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    rm, rv = rmean.clone(), rvar.clone()
    ops.bn_finalize(partials, msplit, gamma, beta, rm, rv, work, M, C, EPS,
                    MOM, update_running=True)
    ops.bn_apply(x, res, y, work, M, C, relu, slope)
    return y, work, rm, rv


def _small_fwd(partials, msplit, x, res, gamma, beta, rmean, rvar, relu,
               slope):
    from flashy_amd import ops
    M, C = x.numel() // x.shape[-1], x.shape[-1]
    work = torch.full((4 * C,), float("nan"), device="cuda")
    y = torch.full_like(x, float("nan"))
    rm, rv = rmean.clone(), rvar.clone()
    ops.bn_fwd_small(partials, msplit, gamma, beta, rm, rv, work, x, res, y,
                     M, C, EPS, MOM, True, relu, slope)
    return y, work, rm, rv


def _assert_fwd_equal(a, b):
    for name, u, v in zip(("y", "work", "running_mean", "running_var"), a, b):
        assert torch.equal(u, v), (name, (u.float() - v.float()).abs().max())


@requires_gpu
@pytest.mark.parametrize("msplit", [1, 3, 4, 8])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fwd_bitwise(shape, flags, msplit):
    from flashy_amd import ops
    relu, has_res, slope = flags
    x, res, _, gamma, beta, rmean, rvar = _inputs(shape)
    M, C = x.numel() // shape[3], shape[3]
    partials = torch.empty(msplit * 2 * C, dtype=torch.float32, device="cuda")
    ops.bn_stats(x, partials, M, C, msplit)
    args = (partials, msplit, x, res if has_res else None, gamma, beta, rmean,
            rvar, relu, slope)
    _assert_fwd_equal(_small_fwd(*args), _chain_fwd(*args))


@requires_gpu
def test_fwd_bitwise_conv_partials():
    """Partials as the conv epilogue emits them (msplit = conv m-tiles)."""
    from flashy_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    N, H, W, C, K = 8, 84, 84, 192, 192     # tests/test_conv8_gpu.py FWD8_BN64
    xin = torch.randn(N, H, W, C, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(K, 1, 1, C, device="cuda", generator=g) * 0.1
         ).to(torch.bfloat16)
    d = ops.ConvDims.infer(xin, w, 2, 0)
    x = xin.new_empty((d.N, d.Ho, d.Wo, d.K))
    partials, msplit = ops.conv_fwd(xin, w, x, d, want_stats=True)
    gamma = 1.0 + 0.5 * torch.randn(K, device="cuda", generator=g)
    beta = 0.3 * torch.randn(K, device="cuda", generator=g)
    rmean, rvar = torch.zeros(K, device="cuda"), torch.ones(K, device="cuda")
    args = (partials, msplit, x, None, gamma, beta, rmean, rvar, True, 0.0)
    _assert_fwd_equal(_small_fwd(*args), _chain_fwd(*args))


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bwd_case(shape, flags):
    """Forward state, the chain's backward from zeroed grads, and the float64
    reference — computed once per (shape, flags) and left unchanged."""
    from flashy_amd import ops
    relu, has_res, slope = flags
    x, res, dy, gamma, beta, rmean, rvar = _inputs(shape)
    C = shape[3]
    M = x.numel() // C
    msplit = ops.bn_msplit(M, C)
    partials = torch.empty(msplit * 2 * C, dtype=torch.float32, device="cuda")
    ops.bn_stats(x, partials, M, C, msplit)
    y, work, _, _ = _chain_fwd(partials, msplit, x, res if has_res else None,
                               gamma, beta, rmean, rvar, relu, slope)
    # chain
    bpart = torch.empty(msplit * 2 * C, dtype=torch.float32, device="cuda")
    bsums = torch.empty(2 * C, dtype=torch.float32, device="cuda")
    dz, dx = torch.empty_like(dy), torch.empty_like(x)
    dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(beta)
    ops.bn_bwd_reduce(dy, y, x, work, dz, bpart, M, C, msplit, relu, slope)
    ops.bn_bwd_grads(bpart, msplit, bsums, dgamma, dbeta, C)
    ops.bn_bwd_apply(dz, x, work, bsums, dx, M, C)
    # float64 reference from the same bf16 inputs and the same fp32 work
    mean, invstd, scale = (work[i * C:(i + 1) * C].double() for i in range(3))
    factor = torch.ones(M, C, device="cuda", dtype=torch.float64)
    if relu:
        factor[y.reshape(M, C).float() <= 0] = float(torch.tensor(
            slope, dtype=torch.float32))
    g = dy.reshape(M, C).double() * factor
    xhat = (x.reshape(M, C).double() - mean) * invstd
    s, sx = g.sum(0), (g * xhat).sum(0)
    bound_s = 4 * M * 2.0 ** -24 * g.abs().sum(0)
    bound_sx = 4 * M * 2.0 ** -24 * (g * xhat).abs().sum(0)
    # pass 2 reads the bf16-rounded dz (fp32 product, then round-to-nearest)
    dz_ref = (dy.reshape(M, C).float() * factor.float()).to(torch.bfloat16)
    dx_ref = scale * (dz_ref.double() - s / M - xhat * sx / M)
    chain = dict(dz=dz, dx=dx, dgamma=dgamma, dbeta=dbeta)
    ref = dict(s=s, sx=sx, bound_s=bound_s, bound_sx=bound_sx,
               dz=dz_ref.reshape(dy.shape), dx=dx_ref)
    return y, work, chain, ref


def _dx_err(dx, ref):
    M, C = ref.shape
    return ((dx.reshape(M, C).double() - ref).abs().max()
            / ref.abs().max().clamp_min(1e-30)).item()


def _run_small(shape, flags, form, write_dz=True, dgamma0=None, dbeta0=None):
    from flashy_amd import ops
    relu, _, slope = flags
    x, _, dy, gamma, beta, _, _ = _inputs(shape)
    y, work, _, _ = _bwd_case(shape, flags)
    C = shape[3]
    M = x.numel() // C
    dz = torch.full_like(dy, -7.0)          # sentinel
    dx = torch.full_like(x, float("nan"))   # every element must be written
    dgamma = torch.zeros_like(gamma) if dgamma0 is None else dgamma0.clone()
    dbeta = torch.zeros_like(beta) if dbeta0 is None else dbeta0.clone()
    ops.bn_bwd_small(dy, y, x, work, dz, dgamma, dbeta, dx, M, C, relu, slope,
                     write_dz=write_dz, form=form)
    return dz, dx, dgamma, dbeta


@requires_gpu
@pytest.mark.parametrize("form", _bwd_forms())
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bwd(shape, flags, form):
    _, _, chain, ref = _bwd_case(shape, flags)
    dz, dx, dgamma, dbeta = _run_small(shape, flags, form)
    assert torch.equal(chain["dz"], ref["dz"])
    assert torch.equal(dz, chain["dz"])
    for name, got, chn, want, bound in (
            ("dbeta", dbeta, chain["dbeta"], ref["s"], ref["bound_s"]),
            ("dgamma", dgamma, chain["dgamma"], ref["sx"], ref["bound_sx"])):
        e_small = (got.double() - want).abs()
        e_chain = (chn.double() - want).abs()
        print(f"{name}: max err/bound small "
              f"{(e_small / bound.clamp_min(1e-300)).max().item():.3e} chain "
              f"{(e_chain / bound.clamp_min(1e-300)).max().item():.3e}")
        assert (e_chain <= bound).all(), name
        assert (e_small <= bound).all(), name
    e_chain, e_small = _dx_err(chain["dx"], ref["dx"]), _dx_err(dx, ref["dx"])
    print(f"dx rel err: chain {e_chain:.3e} small {e_small:.3e} "
          f"(bound {2.0 ** -8:.3e})")
    assert e_chain <= 2.0 ** -8
    assert e_small <= 2.0 ** -8


@requires_gpu
@pytest.mark.parametrize("form", _bwd_forms())
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]])
def test_bwd_accumulates_repeats_and_skips_dz(shape, form):
    flags = FLAGS[4]
    x, _, _, gamma, beta, _, _ = _inputs(shape)
    dz, dx, dgamma, dbeta = _run_small(shape, flags, form)
    # accumulation: one fp32 add of the same sums onto what was there
    g0, b0 = gamma * 3.0 + 1.0, beta - 2.0
    _, _, dgamma1, dbeta1 = _run_small(shape, flags, form, dgamma0=g0,
                                       dbeta0=b0)
    assert torch.equal(dgamma1, g0 + dgamma)
    assert torch.equal(dbeta1, b0 + dbeta)
    assert not torch.equal(dgamma1, dgamma)
    # determinism
    again = _run_small(shape, flags, form)
    for u, v in zip((dz, dx, dgamma, dbeta), again):
        assert torch.equal(u, v)
    # without WRITE_DZ the buffer is untouched and nothing else changes
    dz2, dx2, dgamma2, dbeta2 = _run_small(shape, flags, form, write_dz=False)
    assert torch.equal(dz2, torch.full_like(dz2, -7.0))
    assert torch.equal(dx2, dx)
    assert torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta)


@requires_gpu
def test_forms_refuse_what_they_cannot_run():
    from flashy_amd import ops
    assert ops.bn_small_plan(1024, 60) == ("chain", "chain")    # C % 8
    assert ops.bn_small_plan(16384, 128) == ("chain", "chain")  # 16 blocks
    t = torch.zeros(8, 60, device="cuda", dtype=torch.bfloat16)
    f = torch.zeros(4 * 60, device="cuda")
    with pytest.raises(ValueError):
        ops.bn_fwd_small(f, 1, f, f, f, f, f, t, None, t.clone(), 8, 60, EPS,
                         MOM, True, False)
    with pytest.raises(ValueError):
        ops.bn_bwd_small(t, t, t, f, t.clone(), f, f.clone(), t.clone(), 8, 60,
                         False)
    # more rows than a thread keeps in registers
    t = torch.zeros(4097, 64, device="cuda", dtype=torch.bfloat16)
    f = torch.zeros(4 * 64, device="cuda")
    with pytest.raises(ValueError):
        ops.bn_bwd_small(t, t, t, f, t.clone(), f, f.clone(), t.clone(), 4097,
                         64, False)


# ---------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------

def _count_calls(monkeypatch, names):
    from flashy_amd import ops
    calls = {n: 0 for n in names}
    for n in names:
        def wrapped(*a, _n=n, _f=getattr(ops, n), **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, n, wrapped)
    return calls


@requires_gpu
@pytest.mark.parametrize("relu,res", [(False, False), (True, True)])
@pytest.mark.parametrize("shape,small", [((4, 8, 8, 64), True),
                                         ((16, 32, 32, 64), False)])
def test_module_matches_fp32_reference(monkeypatch, shape, small, relu, res):
    """tests/test_conv_gpu.py::test_bn_fwd_bwd's reference and tolerances, on
    a shape the plan accepts and on one it declines."""
    from flashy_amd import nn as fnn
    from flashy_amd import ops
    N, H, W, C = shape
    M = N * H * W
    assert (ops.bn_small_plan(M, C) != ("chain", "chain")) == small
    calls = _count_calls(monkeypatch, ["bn_fwd_small", "bn_bwd_small",
                                       "bn_finalize", "bn_bwd_reduce"])
    torch.manual_seed(4)
    x16 = torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16)
    r16 = torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16) \
        if res else None
    bn = fnn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.mul_(1.5)
        bn.bias.add_(0.3)
    x = x16.detach().requires_grad_(True)
    rr = r16.detach().requires_grad_(True) if res else None
    y = bn(x, res=rr, relu=relu)
    dy = torch.randn_like(y).to(torch.bfloat16)
    y.backward(dy)
    fwd_form, bwd_form = ops.bn_small_plan(M, C)
    assert calls["bn_fwd_small"] == (fwd_form == "small")
    assert calls["bn_finalize"] == (fwd_form != "small")
    assert calls["bn_bwd_small"] == (bwd_form != "chain")
    assert calls["bn_bwd_reduce"] == (bwd_form == "chain")

    xr = x16.float().requires_grad_(True)
    g = bn.weight.detach().float().clone().requires_grad_(True)
    b = bn.bias.detach().float().clone().requires_grad_(True)
    flat = xr.reshape(M, C)
    mean = flat.mean(0)
    var = flat.var(0, unbiased=False)
    ref = (flat - mean) * torch.rsqrt(var + bn.eps) * g + b
    if res:
        ref = ref + r16.float().reshape(M, C)
    if relu:
        ref = torch.relu(ref)
    ref = ref.reshape(N, H, W, C)
    ref.backward(dy.float())
    tol = 5e-2
    assert (y.float() - ref).abs().max().item() < tol
    assert (x.grad.float() - xr.grad).abs().max().item() < tol
    assert torch.allclose(bn.weight.grad, g.grad, atol=1.0, rtol=2e-2)
    assert torch.allclose(bn.bias.grad, b.grad, atol=1.0, rtol=2e-2)
    if res:
        ref_dres = dy.float() * (ref > 0).float() if relu else dy.float()
        assert (rr.grad.float() - ref_dres).abs().max().item() < tol


@requires_gpu
def test_eval_mode_keeps_the_chain(monkeypatch):
    from flashy_amd import nn as fnn
    from flashy_amd import ops
    N, H, W, C = 4, 8, 8, 64
    M = N * H * W
    assert ops.bn_small_plan(M, C) != ("chain", "chain")
    x16, r16, dy, gamma, beta, rmean, rvar = _inputs((N, H, W, C))
    bn = fnn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rmean)
        bn.running_var.copy_(rvar)
    bn.eval()
    calls = _count_calls(monkeypatch, ["bn_fwd_small", "bn_bwd_small"])
    x = x16.detach().requires_grad_(True)
    rr = r16.detach().requires_grad_(True)
    y = bn(x, res=rr, relu=True)
    y.backward(dy)
    assert calls == {"bn_fwd_small": 0, "bn_bwd_small": 0}
    assert torch.equal(bn.running_mean, rmean)
    assert torch.equal(bn.running_var, rvar)
    # the chain called directly on the eval-mode coefficients
    invstd = torch.rsqrt(rvar + bn.eps)
    scale = gamma * invstd
    work = torch.cat([rmean, invstd, scale, beta - rmean * scale])
    y_c = torch.empty_like(x16)
    ops.bn_apply(x16, r16, y_c, work, M, C, True, 0.0)
    msplit = ops.bn_msplit(M, C)
    part = torch.empty(msplit * 2 * C, dtype=torch.float32, device="cuda")
    bsums = torch.empty(2 * C, dtype=torch.float32, device="cuda")
    dz = torch.empty_like(dy)
    dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(beta)
    ops.bn_bwd_reduce(dy, y_c, x16, work, dz, part, M, C, msplit, True, 0.0)
    ops.bn_bwd_grads(part, msplit, bsums, dgamma, dbeta, C)
    assert torch.equal(y, y_c)
    # running statistics do not depend on x: dx = scale * dz, one fp32
    # product and one rounding (not the training formula's batch terms)
    assert torch.equal(x.grad, (scale * dz.float()).to(torch.bfloat16))
    assert torch.equal(rr.grad, dz)
    assert torch.equal(bn.weight.grad, dgamma)
    assert torch.equal(bn.bias.grad, dbeta)


@requires_gpu
def test_graph_replay_equals_eager():
    """Forward + backward of one BatchNorm2d under CapturedStep: three
    replays on changing input equal three eager steps bit for bit."""
    import copy
    from flashy_amd import nn as fnn
    from flashy_amd import ops
    from flashy_amd.graph import CapturedStep
    N, H, W, C = 4, 8, 8, 64
    assert ops.bn_small_plan(N * H * W, C) != ("chain", "chain")
    g = torch.Generator(device="cuda").manual_seed(3)
    xs = [torch.randn(N, H, W, C, device="cuda", generator=g
                      ).to(torch.bfloat16) for _ in range(4)]
    dy = torch.randn(N, H, W, C, device="cuda", generator=g).to(torch.bfloat16)
    bn = fnn.BatchNorm2d(C).cuda().train()
    for p in bn.parameters():
        p.grad = torch.zeros_like(p)
    eager = copy.deepcopy(bn)
    for p in eager.parameters():
        p.grad = torch.zeros_like(p)
    state0 = copy.deepcopy(bn.state_dict())
    static_x = xs[3].clone()
    out = {}

    def make_step(mod, src):
        def step():
            for p in mod.parameters():
                p.grad.zero_()
            x = src.detach().requires_grad_(True)
            y = mod(x, relu=True)
            y.backward(dy)
            out["y"], out["dx"] = y, x.grad
        return step

    graphed = CapturedStep(make_step(bn, static_x), warmup=1).capture()
    g_y, g_dx = out["y"], out["dx"]          # the graph's static outputs
    with torch.no_grad():                    # undo the warmup's running update
        bn.load_state_dict(state0)
    eager_step = make_step(eager, static_x)
    for i in range(3):
        static_x.copy_(xs[i])
        graphed()
        torch.cuda.synchronize()
        got = [g_y.clone(), g_dx.clone(), bn.weight.grad.clone(),
               bn.bias.grad.clone(), bn.running_mean.clone(),
               bn.running_var.clone()]
        eager_step()
        want = [out["y"], out["dx"], eager.weight.grad, eager.bias.grad,
                eager.running_mean, eager.running_var]
        for k, (u, v) in enumerate(zip(got, want)):
            assert torch.equal(u, v), (i, k)
