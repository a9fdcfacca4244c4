# Copyright (c) Flashy-AMD authors.
"""GPU tests of k_resized_crop_draw / k_resized_crop behind
flashy_amd.data.DeviceResizedCrop: boxes equal to the host mirror and bf16
payloads bitwise equal to the CPU torch path at the same counter value —
eager, in eval mode, captured into a HIP graph and replayed, after a state
restore — plus the hand-off into the native model.

Bitwise comparison is sound because the draw is integer-only, the
accumulator is an exact integer, and the kernel's single fused multiply-add
rounds like the host's fp64 path for every accumulator value (checked
exhaustively in tests/test_resized_crop.py)."""
import pytest
import torch

from flashy_amd.data import DeviceResizedCrop

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

NORMS = {
    "identity": dict(mean=(0., 0., 0.), std=(1 / 255, 1 / 255, 1 / 255)),
    "cifar": dict(mean=(0.4914, 0.4822, 0.4465),
                  std=(0.2023, 0.1994, 0.2010)),
    "imagenet": dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)),
}


def _pair(out_size, **kw):
    """The same augment on the GPU and on the CPU (the oracle)."""
    return (DeviceResizedCrop(out_size, device="cuda", **kw),
            DeviceResizedCrop(out_size, device="cpu", **kw))


def _batch(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)


def _bits(t):
    return t.cpu().view(torch.int16)


def _assert_same(got, want):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape
    bad = int((got != want).sum())
    assert bad == 0, f"{bad} of {got.numel()} bf16 payloads differ"


TINY = dict(scale=(0.01, 0.05))      # boxes of 1 and 2 pixels a side

# n, (h, w), out_size, norm, extra
SHAPES = [
    (5, (9, 11), (6, 7), "imagenet", {}),        # odd width: scalar stores
    (3, (16, 16), 8, "cifar", {}),
    (4, (8, 8), 12, "identity", TINY),           # upscale, 1-pixel boxes
    (64, (40, 56), 32, "cifar", {}),
    (5, (8, 64), 8, "imagenet", dict(scale=(0.9, 1.0))),   # fallback
    (48, (256, 256), 224, "imagenet", {}),       # grid-stride loop iterates
    (5, (9, 11), (6, 7), "identity", dict(flip=0.0)),
    (5, (9, 11), (6, 7), "cifar", dict(flip=1.0)),
    (3, (16, 16), 8, "identity", dict(flip=1.0)),
    (4, (8, 8), 12, "imagenet", dict(flip=0.0, **TINY)),
]


@requires_gpu
@pytest.mark.parametrize("n,size,out,norm,extra", SHAPES)
def test_eager_matches_cpu_at_consecutive_steps(n, size, out, norm, extra):
    gpu, cpu = _pair(out, seed=7, **NORMS[norm], **extra)
    fell_back = one_pixel = False
    for step in range(3):
        src = _batch(n, *size, seed=step)
        got = gpu(src.cuda())
        assert got.dtype == torch.bfloat16 and got.is_cuda
        assert tuple(got.shape) == (n, *gpu.out_size, 3)
        boxes, fallback = cpu.boxes_at(step, n, size)
        last = gpu.last_boxes
        assert last.dtype == torch.int32 and last.is_cuda
        assert tuple(last.shape) == (n, 8)
        assert torch.equal(last[:, :5].cpu().long(), boxes)
        assert torch.equal(last[:, 7].cpu() != 0, fallback)
        _assert_same(got, cpu(src))
        assert torch.equal(last.cpu(), cpu.last_boxes)
        fell_back = fell_back or bool(fallback.all())
        one_pixel = one_pixel or int(boxes[:, 2:4].min()) == 1
        if "flip" in extra:
            assert bool(boxes[:, 4].all()) == (extra["flip"] == 1.0)
            assert bool(boxes[:, 4].any()) == (extra["flip"] == 1.0)
    assert gpu.state_dict() == {"seed": 7, "step": 3}
    assert cpu.state_dict() == gpu.state_dict()
    # the cases exercise what their comments claim
    assert fell_back == (size == (8, 64))
    if size == (8, 8):
        assert one_pixel


@requires_gpu
@pytest.mark.parametrize("n,size,out,norm,extra", SHAPES[:4])
def test_eval_mode_is_centre_box_without_counter(n, size, out, norm, extra):
    gpu, cpu = _pair(out, seed=7, **NORMS[norm], **extra)
    src = _batch(n, *size, seed=9)
    _assert_same(gpu(src.cuda(), train=False), cpu(src, train=False))
    assert torch.equal(gpu.last_boxes.cpu(), cpu.last_boxes)
    assert int(gpu.last_boxes[:, 4].sum()) == 0
    assert gpu.state_dict()["step"] == 0
    assert gpu.step == 0


@requires_gpu
def test_out_buffer_is_written_in_place():
    gpu, cpu = _pair(8, **NORMS["cifar"])
    src = _batch(5, 12, 12)
    out = torch.zeros(5, 8, 8, 3, dtype=torch.bfloat16, device="cuda")
    assert gpu(src.cuda(), out=out) is out
    _assert_same(out, cpu(src))


@requires_gpu
def test_captured_replay_draws_fresh_boxes():
    """Draw, resample and counter bump captured once, replayed three times:
    every replay matches the CPU path at the NEXT step, so the boxes are a
    function of the device counter and not frozen at capture."""
    n, size = 64, (40, 56)
    gpu, cpu = _pair(32, seed=3, **NORMS["cifar"])
    static_src = torch.zeros(n, *size, 3, dtype=torch.uint8, device="cuda")
    static_out = torch.zeros(n, 32, 32, 3, dtype=torch.bfloat16,
                             device="cuda")
    gpu(static_src, out=static_out)          # load the kernels before capture
    torch.cuda.synchronize()
    start = 5
    gpu.load_state_dict({"seed": 3, "step": start})
    cpu.load_state_dict({"seed": 3, "step": start})

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):            # one stream, no branches
        gpu(static_src, out=static_out)
    # capturing records the launches without running them
    assert gpu.state_dict()["step"] == start

    outs, draws = [], []
    for k in range(3):
        src = _batch(n, *size, seed=100 + k)
        static_src.copy_(src.cuda())
        graph.replay()
        outs.append(static_out.clone())
        _assert_same(outs[-1], cpu(src))
        draws.append(gpu.last_boxes.cpu().clone())
        assert torch.equal(draws[-1][:, :5].long(),
                           gpu.boxes_at(start + k, n, size)[0])
    assert gpu.state_dict() == {"seed": 3, "step": start + 3}
    for a in range(3):
        for b in range(a + 1, 3):
            assert not torch.equal(draws[a], draws[b])
            assert not torch.equal(_bits(outs[a]), _bits(outs[b]))

    # the same source again: only the counter differs, and the output moves
    graph.replay()
    _assert_same(static_out, cpu(src))
    assert not torch.equal(_bits(static_out), _bits(outs[-1]))


@requires_gpu
def test_other_batch_sizes_leave_a_captured_graph_its_boxes():
    """Capture at N = 16, call eagerly at N = 5 (a last partial batch) and in
    eval mode at N = 7, then replay: the graph still writes and reads the
    boxes buffer it was captured with, which the object keeps for its whole
    life, so the replay matches the CPU path and nothing else is allocated
    there; ``last_boxes`` names the buffer of the latest call."""
    a, b, c, size = 16, 5, 7, (20, 24)
    gpu, cpu = _pair((6, 7), seed=13, **NORMS["imagenet"])
    static_src = torch.zeros(a, *size, 3, dtype=torch.uint8, device="cuda")
    static_out = torch.zeros(a, 6, 7, 3, dtype=torch.bfloat16, device="cuda")
    gpu(static_src, out=static_out)          # load the kernels before capture
    torch.cuda.synchronize()
    gpu.load_state_dict({"seed": 13, "step": 0})
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gpu(static_src, out=static_out)
    assert tuple(gpu.last_boxes.shape) == (a, 8)
    # only the address is kept here: a reference held by the test would
    # itself keep the buffer alive and hide a release by the object
    ptr_a = gpu.last_boxes.data_ptr()

    step = 0
    for k in range(3):
        # a replay at N = a ...
        src = _batch(a, *size, seed=50 + k)
        static_src.copy_(src.cuda())
        graph.replay()
        _assert_same(static_out, cpu(src))
        step += 1
        # ... then other batch sizes through the same object, eagerly
        src_b = _batch(b, *size, seed=70 + k)
        _assert_same(gpu(src_b.cuda()), cpu(src_b))
        assert tuple(gpu.last_boxes.shape) == (b, 8)
        assert torch.equal(gpu.last_boxes.cpu(), cpu.last_boxes)
        step += 1
        src_c = _batch(c, *size, seed=90 + k)
        _assert_same(gpu(src_c.cuda(), train=False), cpu(src_c, train=False))
        assert tuple(gpu.last_boxes.shape) == (c, 8)
        assert torch.equal(gpu.last_boxes.cpu(), cpu.last_boxes)
        # fresh allocations of the boxes' size must not land on the
        # captured buffer: the object still owns it
        junk = [torch.full((a, 8), -1, dtype=torch.int32, device="cuda")
                for _ in range(8)]
        assert all(j.data_ptr() != ptr_a for j in junk)
        del junk
    assert gpu.state_dict() == {"seed": 13, "step": step}
    # an eager call at N = a comes back to the captured buffer
    src = _batch(a, *size, seed=99)
    _assert_same(gpu(src.cuda()), cpu(src))
    assert gpu.last_boxes.data_ptr() == ptr_a
    assert torch.equal(gpu.last_boxes.cpu(), cpu.last_boxes)


@requires_gpu
def test_load_state_dict_sets_the_device_counter():
    gpu, cpu = _pair(8, seed=1, **NORMS["imagenet"])
    gpu.load_state_dict({"seed": 21, "step": 1000})
    cpu.load_state_dict({"seed": 21, "step": 1000})
    assert gpu.state_dict() == {"seed": 21, "step": 1000}
    src = _batch(5, 12, 12)
    _assert_same(gpu(src.cuda()), cpu(src))
    assert torch.equal(gpu.last_boxes[:, :5].cpu().long(),
                       cpu.boxes_at(1000, 5, (12, 12))[0])
    assert gpu.state_dict()["step"] == 1001


@requires_gpu
def test_cuda_argument_validation():
    gpu = DeviceResizedCrop(8, device="cuda")
    with pytest.raises(ValueError, match="cpu"):
        gpu(_batch(2, 8, 8))                                  # host tensor
    with pytest.raises(TypeError, match="uint8"):
        gpu(_batch(2, 8, 8).cuda().float())
    assert gpu.state_dict()["step"] == 0 and gpu.last_boxes is None


@requires_gpu
def test_native_model_takes_the_resampled_output():
    """bf16 NHWC from the kernel and the CPU path's result as normalized
    fp32 NCHW through the model's usual entry give bitwise equal logits."""
    from flashy_amd.models import native_resnet18
    torch.manual_seed(0)
    model = native_resnet18(10).cuda().eval()
    gpu, cpu = _pair(32, **NORMS["cifar"])
    src = _batch(4, 40, 40, seed=4)
    with torch.no_grad():
        direct = model(gpu(src.cuda(), train=False))
        nchw = cpu(src, train=False).float().permute(0, 3, 1, 2).contiguous()
        usual = model(nchw.cuda())
    assert torch.isfinite(direct).all()
    assert torch.equal(direct, usual)
