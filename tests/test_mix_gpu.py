# Copyright (c) Flashy-AMD authors.
"""GPU tests of the batch-mixing kernels behind flashy_amd.data.DeviceMix and
of the mixed / smoothed cross-entropy kernel.

The mixing checks are bitwise on bf16 payloads against the CPU torch path at
the same row or counter value — hand-written rows (edge boxes, out-of-range
rows), eager draws, captured into a HIP graph and replayed, after a state
restore.  Bitwise comparison is sound because the kernel rounds ``lam * a``,
``oml * b`` and their sum separately, exactly as the torch expression does.
The loss is compared with the two-term torch formula on fp32 copies at the
tolerances tests/test_ops_gpu.py uses for cross-entropy."""
import struct

import pytest
import torch
from torch.nn import functional as F

from flashy_amd import ops
from flashy_amd.data import DeviceMix, MixedTarget
from flashy_amd.functional import cross_entropy
from tests import loss_reference as R

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

SHAPES = [(5, 7, 7, 3), (1, 4, 4, 3), (2, 8, 8, 64), (4, 6, 5, 8),
          (6, 9, 12, 3)]
BIG = (48, 224, 224, 3)          # the grid-stride loop iterates
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def _batch(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).bfloat16()


def _bits(t):
    return t.cpu().view(torch.int16)


def _assert_same(got, want):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape
    bad = int((got != want).sum())
    assert bad == 0, f"{bad} of {got.numel()} bf16 payloads differ"


def _f32_bits(lam):
    return struct.unpack("i", struct.pack("f", lam))[0]


def _row_lam(row):
    return struct.unpack("f", struct.pack("i", row[5]))[0]


def _hand_rows(H, W):
    """(name, row, clamped row or None) for an H x W image."""
    one = _f32_bits(1.0)
    rows = [(f"mixup lam {lam}", [1, 0, 0, 0, 0, _f32_bits(lam), 0, 0], None)
            for lam in (0.0, 1.0, 0.5, 0.3)]
    boxes = {
        "none": (0, 0, 0, 0, 0),
        "empty box": (2, 2, 2, 1, 3),
        "empty row range": (2, 0, 0, 0, W),
        "full image": (2, 0, H, 0, W),
        "one pixel": (2, H // 2, H // 2 + 1, W // 2, W // 2 + 1),
        "last pixel": (2, H - 1, H, W - 1, W),
        "top left": (2, 0, H // 2, 0, W // 2),
        "top right": (2, 0, H // 2, W - W // 2, W),
        "bottom left": (2, H - H // 2, H, 0, W // 2),
        "bottom right": (2, H - H // 2, H, W - W // 2, W),
        "odd edges": (2, 1, H - 1, 1, W - 2),
        "full rows": (2, 1, 3, 0, W),
        "one column": (2, 0, H, 1, 2),
    }
    rows += [(name, [*box, one, 0, 0], None) for name, box in boxes.items()]
    # out of range: the result must be that of the clamped row
    rows += [
        ("beyond every side", [2, -5, H + 9, -3, W + 100, one, 0, 0],
         [2, 0, H, 0, W, one, 0, 0]),
        ("extreme values", [2, INT_MIN, INT_MAX, INT_MIN, INT_MAX, one, 0, 0],
         [2, 0, H, 0, W, one, 0, 0]),
        ("reversed", [2, 3, 1, W, 0, one, 0, 0], [2, 3, 3, W, W, one, 0, 0]),
        ("past the bottom right", [2, H + 1, H + 5, W + 1, W + 5, one, 0, 0],
         [2, H, H, W, W, one, 0, 0]),
        ("partly outside", [2, 1, H + 7, -2, W - 1, one, 0, 0],
         [2, 1, H, 0, W - 1, one, 0, 0]),
        ("unknown mode", [7, 0, H, 0, W, _f32_bits(0.5), 0, 0],
         [0, 0, 0, 0, 0, one, 0, 0]),
    ]
    return rows


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_batch_mix_hand_written_rows(shape):
    H, W = shape[1:3]
    x0 = _batch(shape, seed=3)
    row_dev = torch.zeros(8, dtype=torch.int32, device="cuda")
    for name, row, clamped in _hand_rows(H, W):
        want = x0.clone()
        DeviceMix._reference(want, row)
        if clamped is not None:
            alt = x0.clone()
            DeviceMix._reference(alt, clamped)
            assert torch.equal(_bits(want), _bits(alt)), name
        got = x0.cuda()
        row_dev.copy_(torch.tensor(row, dtype=torch.int32))
        ops.batch_mix(got, row_dev)
        got, want = _bits(got), _bits(want)
        bad = int((got != want).sum())
        assert bad == 0, f"{name}: {bad} of {got.numel()} payloads differ"
    torch.cuda.synchronize()


@requires_gpu
def test_batch_mix_rejects_bad_arguments():
    x = _batch((2, 4, 4, 3)).cuda()
    row = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError):
        ops.batch_mix(x.float(), row)
    with pytest.raises(AssertionError):
        ops.batch_mix(x.permute(0, 3, 1, 2), row)
    with pytest.raises(AssertionError):
        ops.batch_mix(x, row.long())
    with pytest.raises(AssertionError):
        ops.batch_mix(x, torch.zeros(9, dtype=torch.int32,
                                     device="cuda")[1:])     # misaligned
    mixer = DeviceMix(mixup_alpha=1.0, device="cuda")
    with pytest.raises(TypeError, match="bfloat16"):
        mixer(x.float(), torch.arange(2, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        mixer(x.permute(0, 2, 1, 3), torch.arange(2, device="cuda"))
    with pytest.raises(ValueError, match="cpu"):
        mixer(x.cpu(), torch.arange(2))
    assert mixer.step == 0


MODES = {
    "mixup": dict(mixup_alpha=0.8),
    "cutmix": dict(cutmix_alpha=1.0),
    "both": dict(mixup_alpha=0.2, cutmix_alpha=1.0),
}


@requires_gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", SHAPES + [BIG])
def test_eager_matches_cpu_at_consecutive_steps(shape, mode):
    gpu = DeviceMix(seed=11, device="cuda", **MODES[mode])
    cpu = DeviceMix(seed=11, device="cpu", **MODES[mode])
    n = shape[0]
    target = torch.arange(n)
    for step in range(3):
        x = _batch(shape, seed=step)
        got = x.cuda()
        out = gpu(got, target.cuda())
        want_t = cpu(x, target)
        _assert_same(got, x)
        row = gpu.last_row.cpu().tolist()
        assert row == gpu.row_at(step, shape[1:3]) == cpu.last_row.tolist()
        assert out.lam.is_cuda and out.lam.dtype == torch.float32
        assert float(out.lam) == _row_lam(row) == float(want_t.lam)
        assert torch.equal(out.target_b.cpu(), target.flip(0))
    assert gpu.state_dict() == {"seed": 11, "step": 3} == cpu.state_dict()


def _seed_with_distinct_rows(kw, size, start):
    """A seed (chosen on the CPU) whose rows at start..start+2 hold both
    modes and three different lam values."""
    for seed in range(64):
        probe = DeviceMix(seed=seed, device="cpu", **kw)
        rows = [probe.row_at(start + k, size) for k in range(3)]
        if {r[0] for r in rows} == {1, 2} and len({r[5] for r in rows}) == 3:
            return seed
    raise AssertionError("no seed with three distinct rows")


@requires_gpu
def test_captured_replay_draws_fresh_rows_and_feeds_the_loss():
    """Draw, mix, counter bump and the mixed loss captured once, replayed
    three times: every replay matches the CPU path at the NEXT step, so the
    row — and the lam the loss kernel reads — follow the device counter."""
    shape, classes, eps, start = (8, 16, 16, 3), 10, 0.1, 5
    kw = MODES["both"]
    seed = _seed_with_distinct_rows(kw, shape[1:3], start)
    gpu = DeviceMix(seed=seed, device="cuda", **kw)
    cpu = DeviceMix(seed=seed, device="cpu", **kw)
    g = torch.Generator().manual_seed(0)
    target = torch.randint(classes, (shape[0],), generator=g)
    logits = torch.randn(shape[0], classes, generator=g)
    static_x = torch.zeros(shape, dtype=torch.bfloat16, device="cuda")
    static_t = target.cuda()
    static_logits = logits.cuda()

    def step():
        mixed = gpu(static_x, static_t)
        return cross_entropy(static_logits, mixed, label_smoothing=eps)

    step()                                   # load the kernels before capture
    torch.cuda.synchronize()
    gpu.load_state_dict({"seed": seed, "step": start})
    cpu.load_state_dict({"seed": seed, "step": start})
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):            # one stream, no branches
        loss = step()
    assert gpu.step == start                 # capture runs nothing

    def expect(k):
        """CPU path at counter start + k on the batch of replay k."""
        x = _batch(shape, seed=100 + k)
        want = x.clone()
        lam = float(cpu(want, target).lam)
        ref = (lam * F.cross_entropy(logits, target, label_smoothing=eps)
               + (1 - lam) * F.cross_entropy(logits, target.flip(0),
                                             label_smoothing=eps))
        return x, want, cpu.last_row.tolist(), ref

    outs, losses = [], []
    for k in range(3):
        x, want, row, ref = expect(k)
        static_x.copy_(x.cuda())
        graph.replay()
        _assert_same(static_x, want)
        assert gpu.last_row.cpu().tolist() == row
        assert torch.allclose(loss.cpu(), ref, atol=1e-5, rtol=1e-5), \
            (k, loss.item(), ref.item())
        outs.append(static_x.clone())
        losses.append(loss.item())
    assert gpu.step == start + 3
    assert len(set(losses)) == 3

    # restore: the replay reproduces the earlier step
    gpu.load_state_dict({"seed": seed, "step": start + 1})
    static_x.copy_(_batch(shape, seed=101).cuda())
    graph.replay()
    _assert_same(static_x, outs[1])
    # (the loss is an atomic sum over rows: equal up to the order of adds)
    assert abs(loss.item() - losses[1]) <= 1e-6 * abs(losses[1])
    assert gpu.step == start + 2


# -- the loss kernel --------------------------------------------------------

def _within_oracle(dtype, tol, loss, grad, ref):
    """The loss and the gradient within the float64 oracle's bounds
    (tests/loss_reference.py).  The gradient bound is elementwise no looser
    than the ``atol = rtol = tol`` it replaces, asserted on these very
    inputs; the fp32 loss bound can be, so the old loss assertion stays."""
    bound = R.store_bound(dtype, ref.grad, ref.grad_bound)
    assert bool((bound <= tol + tol * ref.grad.abs()).all())
    assert torch.isfinite(grad).all()
    err = (grad.double() - ref.grad).abs()
    assert bool((err <= bound).all()), err.max().item()
    assert (loss.double() - ref.loss).abs() <= ref.loss_bound


def _reference_loss(x32, ta, tb, lam, eps):
    return (lam * F.cross_entropy(x32, ta, label_smoothing=eps)
            + (1 - lam) * F.cross_entropy(x32, tb, label_smoothing=eps))


@requires_gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 10, 33, 1000])
@pytest.mark.parametrize("B", [5, 64])
def test_cross_entropy_mix_kernel(B, C, dtype, eps):
    torch.manual_seed(1)
    base = (torch.randn(B, C, device="cuda") * 3).to(dtype)
    ta = torch.randint(C, (B,), device="cuda")
    tb = ta.flip(0).contiguous()
    tb[:2] = ta[:2]                              # rows with ta == tb
    assert bool((ta != tb).any()) or C == 1
    lam_dev = torch.ones((), dtype=torch.float32, device="cuda")
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    for lam in (0.0, 1.0, 0.37):
        lam_dev.fill_(lam)                       # the same tensor every time
        logits = base.clone().requires_grad_(True)
        loss = cross_entropy(logits, MixedTarget(ta, tb, lam_dev),
                             label_smoothing=eps)
        loss.backward()
        ref_in = base.float().clone().requires_grad_(True)
        ref = _reference_loss(ref_in, ta, tb, lam, eps)
        ref.backward()
        err = (logits.grad.float() - ref_in.grad).abs().max().item()
        print(f"lam {lam}: loss {loss.item():.6f} ref {ref.item():.6f} "
              f"max grad error {err:.3g}")
        assert torch.allclose(loss.float(), ref, atol=tol, rtol=tol)
        _within_oracle(dtype, tol, loss.detach(), logits.grad,
                       R.cross_entropy(base, ta, tb, R.f32(lam), R.f32(eps),
                                       loss_scale=R.mean_scale(B),
                                       grad_scale=R.mean_scale(B)))
    # smoothing alone, plain target
    logits = base.clone().requires_grad_(True)
    loss = cross_entropy(logits, ta, label_smoothing=eps)
    loss.backward()
    ref_in = base.float().clone().requires_grad_(True)
    ref = F.cross_entropy(ref_in, ta, label_smoothing=eps)
    ref.backward()
    assert torch.allclose(loss.float(), ref, atol=tol, rtol=tol)
    _within_oracle(dtype, tol, loss.detach(), logits.grad,
                   R.cross_entropy(base, ta, eps=R.f32(eps),
                                   loss_scale=R.mean_scale(B),
                                   grad_scale=R.mean_scale(B)))


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C", [(1, 10), (64, 10), (37, 1000)])
def test_plain_cross_entropy_still_runs_the_plain_kernel(dtype, B, C):
    """``cross_entropy(logits, target)`` equals a direct launch of
    ``k_cross_entropy`` bit for bit: the gradient always, the loss where its
    atomic sum has one order (one row)."""
    torch.manual_seed(2)
    logits = (torch.randn(B, C, device="cuda") * 3).to(dtype)
    target = torch.randint(C, (B,), device="cuda")
    want_grad = torch.empty_like(logits)
    want_loss = torch.zeros((), dtype=torch.float32, device="cuda")
    ops.cross_entropy_fwd_bwd(logits, target, want_grad, want_loss,
                              loss_scale=1.0 / B, grad_scale=1.0 / B)
    for kw in ({}, {"label_smoothing": 0.0}):
        x = logits.clone().requires_grad_(True)
        loss = cross_entropy(x, target, **kw)
        loss.backward()
        assert torch.equal(x.grad, want_grad)
        if B == 1:
            assert torch.equal(loss, want_loss)
        else:
            assert torch.allclose(loss, want_loss, atol=0, rtol=1e-6)


# -- end to end -------------------------------------------------------------

@requires_gpu
def test_native_step_with_ingest_mix_and_smoothed_loss_under_capture():
    from flashy_amd.data import DeviceAugment
    from flashy_amd.graph import CapturedStep
    from flashy_amd.models import native_resnet18
    from flashy_amd.optim import FusedSGD
    torch.manual_seed(0)
    n = 16
    model = native_resnet18(10).cuda().train()
    optim = FusedSGD(model.parameters(), lr=0.01, momentum=0.9,
                     bf16_mirror=True)
    model.enable_wt_cache()
    augment = DeviceAugment(32, pad=4, mean=(0.4914, 0.4822, 0.4465),
                            std=(0.2023, 0.1994, 0.2010), seed=1,
                            device="cuda")
    mixer = DeviceMix(mixup_alpha=0.2, cutmix_alpha=1.0, seed=1,
                      device="cuda")
    g = torch.Generator().manual_seed(0)
    static_img = torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8,
                               generator=g).cuda()
    static_label = torch.randint(10, (n,), generator=g).cuda()

    def step():
        optim.zero_grad(set_to_none=False)
        x = augment(static_img)
        target = mixer(x, static_label)
        loss = cross_entropy(model(x), target, label_smoothing=0.1)
        loss.backward()
        optim.step()
        return loss

    graphed = CapturedStep(step, warmup=3).capture()
    mixer.load_state_dict({"seed": 1, "step": 0})
    losses = []
    for _ in range(5):
        losses.append(graphed().item())
    print("losses", losses)
    assert all(torch.isfinite(torch.tensor(losses)))
    assert len(set(losses)) == 5
    assert mixer.step == 5
    assert mixer.last_row.cpu().tolist() == mixer.row_at(4, (32, 32))
