# Copyright (c) Flashy-AMD authors.
"""BatchNorm backward with a generalised gradient source, dy = A [+ B]
(k_bn_bwd_reduce, k_bn_bwd_small): A a bf16 tensor or the fp32 slices of a
split-K dgrad, B a second bf16 gradient.

Kernel level.  The fused call is torch.equal to the chain it replaces
(ops.splitk_combine, torch.add, the old call) on dz, partials, dgamma, dbeta
(accumulated onto non-zero gradients) and dx, and is held to the float64
oracle of tests/bn_reference.py with its bounds, dy taken in float64 from the
bf16-rounded combine and add.  With slope 0 dz is dy or 0, so it equals the
oracle's exactly.

Shapes (M, C): (50, 64) M not a multiple of 32; (1024, 128) the small form's
last row slot; (4100, 128), chain form only: ragged last m_per_block and past
the small form's limit.  About half of y is non-positive.

Block level.  A BatchNorm2d feeding a downsample block 64 -> 128 and two
NativeBasicBlocks at C = 128, 8x8, N = 2, switch on against switch off:
every gradient torch.equal, no bf16 add and no k_splitk_combine launch in the
fused backward (but for a workspace above the row limit of a single-kernel
backward, which keeps its combine by design), once more under CapturedStep;
and the paths that keep the unfused chain.
"""
import functools

import pytest
import torch

from tests import bn_reference as R

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

SMALL_SHAPES = [(50, 64), (1024, 128)]
CHAIN_SHAPES = SMALL_SHAPES + [(4100, 128)]
SOURCES = [(zn, has_b) for zn in (0, 2, 5) for has_b in (False, True)]
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _inputs(M, C):
    g = torch.Generator(device="cuda").manual_seed(11 + M + C)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    x = (rnd(M, C) * 1.5 + 0.3).to(torch.bfloat16)
    y = rnd(M, C).to(torch.bfloat16)            # the mask: half non-positive
    a = rnd(M, C).to(torch.bfloat16)
    b = rnd(M, C).to(torch.bfloat16)
    ws = rnd(5, M, C) * 0.6                     # fp32 slices; zn uses a prefix
    gamma = 1.0 + 0.5 * rnd(C)
    mean = x.float().mean(0)
    invstd = torch.rsqrt(x.float().var(0, unbiased=False) + EPS)
    scale = gamma * invstd
    work = torch.cat([mean, invstd, scale, 0.3 * rnd(C) - mean * scale])
    g0, b0 = 3.0 * rnd(C) + 1.0, rnd(C) - 2.0   # gradients already there
    return x, y, a, b, ws, work, g0, b0


@functools.lru_cache(maxsize=None)
def _unfused_dy(M, C, zn, has_b):
    """The dy the unfused chain materialises: combine, then add."""
    from flashy_amd import ops
    _, _, a, b, ws, _, _, _ = _inputs(M, C)
    if zn:
        a = torch.empty_like(a)
        ops.splitk_combine(ws[:zn].contiguous(), a, zn)
    return torch.add(a, b) if has_b else a


def _sources(M, C, zn, has_b):
    _, _, a, b, ws, _, _, _ = _inputs(M, C)
    src = ws[:zn].contiguous() if zn else a
    return src, dict(dy_b=b if has_b else None, zn=zn)


def _chain(M, C, dy, relu, kw, dgamma, dbeta):
    from flashy_amd import ops
    x, y, _, _, _, work, _, _ = _inputs(M, C)
    msplit = ops.bn_msplit(M, C)
    partials = torch.full((msplit * 2 * C,), float("nan"), device="cuda")
    bsums = torch.empty(2 * C, dtype=torch.float32, device="cuda")
    dz = torch.full_like(x, float("nan"))
    dx = torch.full_like(x, float("nan"))
    ops.bn_bwd_reduce(dy, y, x, work, dz, partials, M, C, msplit, relu, 0.0,
                      **kw)
    ops.bn_bwd_grads(partials, msplit, bsums, dgamma, dbeta, C)
    ops.bn_bwd_apply(dz, x, work, bsums, dx, M, C)
    return dict(dz=dz, partials=partials, dgamma=dgamma, dbeta=dbeta, dx=dx)


def _small(M, C, dy, relu, write_dz, kw, dgamma, dbeta):
    from flashy_amd import ops
    x, y, _, _, _, work, _, _ = _inputs(M, C)
    dz = torch.full_like(x, -7.0)               # sentinel
    dx = torch.full_like(x, float("nan"))
    ops.bn_bwd_small(dy, y, x, work, dz, dgamma, dbeta, dx, M, C, relu, 0.0,
                     write_dz=write_dz, **kw)
    return dict(dz=dz, dgamma=dgamma, dbeta=dbeta, dx=dx)


@functools.lru_cache(maxsize=None)
def _case(form, M, C, zn, has_b, relu, write_dz=True):
    """(unfused, fused from the same non-zero gradients, fused from zero
    gradients) — computed once and left unchanged."""
    _, _, _, _, _, _, g0, b0 = _inputs(M, C)
    src, kw = _sources(M, C, zn, has_b)
    dy = _unfused_dy(M, C, zn, has_b)
    if form == "chain":
        run = lambda d, k, g, b: _chain(M, C, d, relu, k, g, b)  # noqa: E731
    else:
        run = lambda d, k, g, b: _small(M, C, d, relu, write_dz, k,  # noqa
                                        g, b)
    z = torch.zeros_like
    return (run(dy, {}, g0.clone(), b0.clone()),
            run(src, kw, g0.clone(), b0.clone()),
            run(src, kw, z(g0), z(b0)))


def _assert_bitwise(unfused, fused):
    for name in unfused:
        u, v = unfused[name], fused[name]
        assert torch.equal(u, v), \
            (name, (u.float() - v.float()).abs().max().item())


def _assert_oracle(M, C, zn, has_b, relu, out, dz_written=True):
    x, y, _, _, _, work, _, _ = _inputs(M, C)
    dy = _unfused_dy(M, C, zn, has_b)
    mean, invstd, scale = (work[i * C:(i + 1) * C] for i in range(3))
    exact = R.bwd_train64(x, dy, y, mean, invstd, scale, relu, 0.0)
    dz16 = exact.dz.to(torch.bfloat16)
    assert torch.equal(dz16.double(), exact.dz)     # slope 0: dy or 0
    if dz_written:
        assert torch.equal(out["dz"], dz16)
    ref = R.bwd_train64(x, dy, y, mean, invstd, scale, relu, 0.0,
                        dz_apply=dz16)
    for name, got, want, bound in (("dbeta", out["dbeta"], ref.s, ref.bound_s),
                                   ("dgamma", out["dgamma"], ref.sx,
                                    ref.bound_sx)):
        err = (got.double() - want).abs()
        print(f"{name}: max err/bound "
              f"{(err / bound.clamp_min(1e-300)).max().item():.3e}")
        assert (err <= bound).all(), name
    bound = R.dx_bound(ref, scale, dz16, sums_exact=False)
    err = (out["dx"].double() - ref.dx).abs()
    print(f"dx: max err/bound "
          f"{(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all()


@requires_gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("zn,has_b", SOURCES)
@pytest.mark.parametrize("M,C", CHAIN_SHAPES)
def test_reduce_bitwise(M, C, zn, has_b, relu):
    unfused, fused, _ = _case("chain", M, C, zn, has_b, relu)
    _, _, _, _, _, _, g0, _ = _inputs(M, C)
    assert not torch.equal(fused["dgamma"], g0)
    _assert_bitwise(unfused, fused)


@requires_gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("zn,has_b", SOURCES)
@pytest.mark.parametrize("M,C", CHAIN_SHAPES)
def test_reduce_oracle(M, C, zn, has_b, relu):
    _, _, fused0 = _case("chain", M, C, zn, has_b, relu)
    _assert_oracle(M, C, zn, has_b, relu, fused0)


@requires_gpu
@pytest.mark.parametrize("write_dz", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("zn,has_b", SOURCES)
@pytest.mark.parametrize("M,C", SMALL_SHAPES)
def test_small_bitwise(M, C, zn, has_b, relu, write_dz):
    unfused, fused, _ = _case("small", M, C, zn, has_b, relu, write_dz)
    _, _, _, _, _, _, g0, _ = _inputs(M, C)
    assert not torch.equal(fused["dgamma"], g0)
    _assert_bitwise(unfused, fused)
    if not write_dz:
        assert torch.equal(fused["dz"], torch.full_like(fused["dz"], -7.0))
    # the small form against the chain on the same sources: dz agrees bit
    # for bit (test_bn_small_gpu.py holds that for the plain source)
    _, chain, _ = _case("chain", M, C, zn, has_b, relu)
    if write_dz:
        assert torch.equal(fused["dz"], chain["dz"])


@requires_gpu
@pytest.mark.parametrize("write_dz", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("zn,has_b", SOURCES)
@pytest.mark.parametrize("M,C", SMALL_SHAPES)
def test_small_oracle(M, C, zn, has_b, relu, write_dz):
    _, _, fused0 = _case("small", M, C, zn, has_b, relu, write_dz)
    _assert_oracle(M, C, zn, has_b, relu, fused0, dz_written=write_dz)


@requires_gpu
def test_sources_are_checked_before_a_launch():
    from flashy_amd import ops
    M, C = 50, 64
    x, y, a, b, ws, work, g0, b0 = _inputs(M, C)
    msplit = ops.bn_msplit(M, C)
    part = torch.empty(msplit * 2 * C, dtype=torch.float32, device="cuda")
    dz, dx = torch.empty_like(x), torch.empty_like(x)
    bad = [dict(dy=ws[:2].contiguous(), zn=3),          # too few slices
           dict(dy=a, zn=2),                            # bf16 as a workspace
           dict(dy=ws[0].contiguous(), zn=0),           # fp32 as a tensor
           dict(dy=a, zn=0, dy_b=b[:-1]),               # short B
           dict(dy=a, zn=0, dy_b=b.float())]
    for kw in bad:
        kw = dict(kw)
        dy = kw.pop("dy")
        with pytest.raises(ValueError):
            ops.bn_bwd_reduce(dy, y, x, work, dz, part, M, C, msplit, True,
                              0.0, **kw)
        with pytest.raises(ValueError):
            ops.bn_bwd_small(dy, y, x, work, dz, g0.clone(), b0.clone(), dx, M,
                             C, True, 0.0, **kw)


# ---------------------------------------------------------------------------
# block level
# ---------------------------------------------------------------------------

class _Trunk(torch.nn.Module):
    """BatchNorm2d -> downsample block 64 -> 128 -> two blocks at 128."""

    def __init__(self, head: str = "bn"):
        super().__init__()
        from flashy_amd import nn as fnn
        from flashy_amd.models.resnet_native import (NativeBasicBlock,
                                                      chain_blocks)
        self.head = head
        self.bn0 = fnn.BatchNorm2d(64)
        self.blocks = torch.nn.Sequential(
            NativeBasicBlock(64, 128, 2, downsample=True),
            NativeBasicBlock(128, 128), NativeBasicBlock(128, 128))
        chain_blocks(self.blocks)

    def forward(self, x):
        if self.head == "bn":
            h = self.bn0(x, relu=True, split=True)
        else:                       # a block input that is no BatchNorm's
            h = x
        return self.blocks(h)


def _keep_conv_outputs(model, store):
    """Every conv output's gradient is a BatchNorm's dx: retained in both
    modes (a BatchNorm output's own gradient is never materialised when its
    two readers' gradients stay un-summed)."""
    from flashy_amd import nn as fnn

    def hook(mod, args, out):
        if out.requires_grad:
            out.retain_grad()
            store.append(out)
    return [m.register_forward_hook(hook) for m in model.modules()
            if isinstance(m, fnn.Conv2d)]


def _trunk_inputs(C=64, hw=16):
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(2, hw, hw, C, device="cuda", generator=g
                    ).to(torch.bfloat16)
    dy = torch.randn(2, 8, 8, 128, device="cuda", generator=g
                     ).to(torch.bfloat16)
    return x, dy


def _make_trunk(head="bn", seed=3):
    torch.manual_seed(seed)
    model = _Trunk(head).cuda().train()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.2 * torch.randn_like(p))
    return model


def _backward(model, x16, dy, fuse, monkeypatch, count=None):
    """One forward + backward from zeroed gradients; returns every gradient
    by name."""
    from flashy_amd import nn as fnn
    monkeypatch.setattr(fnn, "_FUSE_GRAD_SOURCES", fuse)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    acts = []
    hooks = _keep_conv_outputs(model, acts)
    x = x16.detach().requires_grad_(True)
    out = model(x)
    if count is not None:
        with torch.profiler.profile(
                activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            out.backward(dy)
        count["add"] = sum(e.count for e in prof.key_averages()
                           if e.key in ("aten::add", "aten::add_"))
    else:
        out.backward(dy)
    for h in hooks:
        h.remove()
    grads = {"out": out.detach().clone(), "x": x.grad}
    grads.update({f"act{i}": a.grad for i, a in enumerate(acts)})
    grads.update({n: p.grad.clone() for n, p in model.named_parameters()})
    return grads     # None where no gradient flows (input_grad=False)


def _count_ops(monkeypatch, names):
    from flashy_amd import ops
    calls = {n: [] for n in names}
    for n in names:
        def wrapped(*a, _n=n, _f=getattr(ops, n), **k):
            r = _f(*a, **k)
            calls[_n].append((a, r))
            return r
        monkeypatch.setattr(ops, n, wrapped)
    return calls


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
            continue
        assert torch.equal(a[k], b[k]), \
            (k, (a[k].float() - b[k].float()).abs().max().item())


@requires_gpu
def test_blocks_fused_equals_unfused(monkeypatch):
    from flashy_amd import nn as fnn
    from flashy_amd import ops
    monkeypatch.setenv("FLASHY_WGRAD_SPLITS", "1")
    # C = 128 at 3x3 is 18 stages: the stride-1 dgrads run split-K at M = 128
    assert ops._splitk_plan(2 * 8 * 8, 128 // 64, 18) >= 2
    model = _make_trunk()
    x16, dy = _trunk_inputs()
    calls = _count_ops(monkeypatch, ["conv_dgrad", "splitk_combine"])
    n_add = {}
    unfused = _backward(model, x16, dy, False, monkeypatch, n_add)
    # the detectors see the unfused chain: 3 block inputs summed by autograd,
    # the 5 stride-1 3x3 dgrads at C = 128 combined by their own kernel
    assert n_add["add"] == 3, n_add
    def rows(c):                        # (ws, out, zn) -> M * zn
        (_, out, zn), _ = c
        return out.numel() // out.shape[-1] * zn

    n_splitk = len(calls["splitk_combine"])
    small_m128 = sum(rows(c) <= fnn._SMALL_FORM_WS_ROWS
                     for c in calls["splitk_combine"])
    assert small_m128 == 5
    assert all(r is None for _, r in calls["conv_dgrad"])
    for c in calls.values():
        c.clear()
    fused = _backward(model, x16, dy, True, monkeypatch, n_add)
    assert n_add["add"] == 0, n_add
    # no combine kernel is left but for a workspace past the row limit of
    # the single-kernel backward that would read it (nn._SMALL_FORM_WS_ROWS:
    # the downsample block's stride-2 conv1, M = 512 in front of bn0)
    assert all(rows(c) > fnn._SMALL_FORM_WS_ROWS
               for c in calls["splitk_combine"])
    assert len(calls["splitk_combine"]) == n_splitk - 5
    assert sum(r is not None for _, r in calls["conv_dgrad"]) == 5
    assert all(v is not None for v in fused.values())
    _assert_same(unfused, fused)


@requires_gpu
def test_blocks_graph_replay_equals_eager(monkeypatch):
    from flashy_amd import nn as fnn
    from flashy_amd.graph import CapturedStep
    monkeypatch.setenv("FLASHY_WGRAD_SPLITS", "1")
    monkeypatch.setattr(fnn, "_FUSE_GRAD_SOURCES", True)
    model = _make_trunk()
    x16, dy = _trunk_inputs()
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    out = {}

    def step():
        for p in model.parameters():
            p.grad.zero_()
        x = x16.detach().requires_grad_(True)
        model(x).backward(dy)
        out["dx"] = x.grad

    graphed = CapturedStep(step, warmup=1).capture()
    g_dx = out["dx"]
    got = []
    for _ in range(2):
        graphed()
        torch.cuda.synchronize()
        got.append([g_dx.clone()] + [p.grad.clone()
                                     for p in model.parameters()])
    with torch.no_grad():
        model.load_state_dict(state0)
    step()
    want = [out["dx"]] + [p.grad for p in model.parameters()]
    for replay in got:
        for k, (u, v) in enumerate(zip(replay, want)):
            assert torch.equal(u, v), k


@requires_gpu
@pytest.mark.parametrize("case", ["plain_input", "frozen_bn", "no_input_grad"])
def test_fallbacks_match_unfused(monkeypatch, case):
    monkeypatch.setenv("FLASHY_WGRAD_SPLITS", "1")
    x16, dy = _trunk_inputs()
    model = _make_trunk("plain" if case == "plain_input" else "bn")
    if case == "frozen_bn":
        # eval mode: running statistics, dx = scale * dz, the chain kernels
        with torch.no_grad():
            for m in model.modules():
                if hasattr(m, "running_var"):
                    m.running_var.add_(0.3 * torch.rand_like(m.running_var))
                    m.running_mean.add_(0.1)
        model.eval()
    if case == "no_input_grad":
        model.blocks[1].conv1.input_grad = False
        model.blocks[2].conv2.input_grad = False
    unfused = _backward(model, x16, dy, False, monkeypatch)
    fused = _backward(model, x16, dy, True, monkeypatch)
    _assert_same(unfused, fused)


@requires_gpu
def test_lost_hand_over_raises(monkeypatch):
    """A BatchNorm output read twice on one edge while its conv defers the
    combine: autograd sums into the unwritten dx, and backward refuses."""
    from flashy_amd import nn as fnn
    monkeypatch.setattr(fnn, "_FUSE_GRAD_SOURCES", True)
    torch.manual_seed(0)
    bn = fnn.BatchNorm2d(128).cuda().train()
    conv = fnn.Conv2d(128, 128, 3, 1, 1).cuda()
    x16 = torch.randn(2, 8, 8, 128, device="cuda").to(torch.bfloat16)
    x = x16.detach().requires_grad_(True)
    h = bn(x, relu=True)
    out = conv(h, sole_reader=True) + h         # not the sole reader
    with pytest.raises(RuntimeError, match="deferred its combine"):
        out.backward(torch.ones_like(out))


@requires_gpu
def test_conv_dgrad_defer_and_row_limit():
    """The deferred slices combine to the dx the dgrad writes itself, and a
    workspace above the reader's row limit is combined by the dgrad."""
    from flashy_amd import ops
    g = torch.Generator(device="cuda").manual_seed(2)
    dout = torch.randn(2, 8, 8, 128, device="cuda", generator=g
                       ).to(torch.bfloat16)
    w = (0.05 * torch.randn(128, 3, 3, 128, device="cuda", generator=g)
         ).to(torch.bfloat16)
    wt = w.permute(1, 2, 3, 0).contiguous()         # RSCK
    d = ops.ConvDims.infer(dout, w, 1, 1)
    M = 2 * 8 * 8
    dx = torch.full_like(dout, float("nan"))
    assert ops.conv_dgrad(dout, wt, dx, d) is None
    dx1 = torch.full_like(dout, float("nan"))
    ws, zn = ops.conv_dgrad(dout, wt, dx1, d, defer_combine=True)
    assert zn >= 2 and ws.numel() == zn * M * 128
    assert torch.isnan(dx1).all()                   # left unwritten
    ops.splitk_combine(ws, dx1, zn)
    assert torch.equal(dx1, dx)
    dx2 = torch.full_like(dout, float("nan"))
    assert ops.conv_dgrad(dout, wt, dx2, d, defer_combine=True,
                          defer_max_rows=M * zn) is not None
    assert ops.conv_dgrad(dout, wt, dx2, d, defer_combine=True,
                          defer_max_rows=M * zn - 1) is None
    assert torch.equal(dx2, dx)
