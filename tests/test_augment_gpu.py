# Copyright (c) Flashy-AMD authors.
"""GPU tests of the fused image-ingest kernel behind
flashy_amd.data.DeviceAugment: bitwise (bf16 payload) against the CPU torch
path at the same counter value — eager, captured into a HIP graph and
replayed, after a state restore — plus the uint8 prefetch path and the
hand-off into the native model.

Bitwise comparison is sound because an output element depends only on
(u8 value, channel): for the three normalizations used here the exact fused
multiply-add, the fp64 torch path and separate fp32 multiply + add round to
the same bf16 for all 768 combinations (checked exhaustively on the CPU)."""
import pytest
import torch

from flashy_amd.data import DeviceAugment, DevicePrefetcher

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
    return (DeviceAugment(out_size, device="cuda", **kw),
            DeviceAugment(out_size, device="cpu", **kw))


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


@requires_gpu
@pytest.mark.parametrize("norm", sorted(NORMS))
def test_all_256_values_through_every_channel(norm):
    """Every (u8 value, channel) pair, as image pixels and as the fill."""
    src = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1)
    src = src.expand(1, 16, 16, 3).contiguous()
    gpu, cpu = _pair(16, **NORMS[norm])
    _assert_same(gpu(src.cuda(), train=False), cpu(src, train=False))
    if norm == "identity":  # outputs are the integers 0..255, exact in bf16
        assert torch.equal(gpu(src.cuda(), train=False).float().cpu(),
                           src.float())
    for fill in (0, 1, 127, 128, 254, 255):
        gpu, cpu = _pair(16, pad=3, fill=fill, **NORMS[norm])
        _assert_same(gpu(src.cuda()), cpu(src))


# n, (h, w), out_size, pad, norm, extra
SHAPES = [
    (5, (8, 8), 8, 2, "identity", {}),
    (3, (10, 12), 8, 0, "cifar", {}),
    (4, (9, 9), (6, 7), 1, "imagenet", {}),      # odd width: scalar stores
    (64, (32, 32), 32, 4, "cifar", {}),          # the example's shape
    (48, (256, 256), 224, 0, "imagenet", {}),    # grid-stride loop iterates
    (5, (8, 8), 8, 2, "cifar", dict(fill=7)),
    (4, (9, 9), (6, 7), 1, "identity", dict(fill=7)),
    (5, (8, 8), 8, 2, "imagenet", dict(flip=0.0)),
    (5, (8, 8), 8, 2, "identity", dict(flip=1.0)),
    (4, (9, 9), (6, 7), 1, "cifar", dict(flip=1.0)),
]


@requires_gpu
@pytest.mark.parametrize("n,size,out,pad,norm,extra", SHAPES)
def test_eager_matches_cpu_at_consecutive_steps(n, size, out, pad, norm,
                                                extra):
    gpu, cpu = _pair(out, pad=pad, seed=7, **NORMS[norm], **extra)
    for step in range(3):
        src = _batch(n, *size, seed=step)
        got = gpu(src.cuda())
        assert got.dtype == torch.bfloat16 and got.is_cuda
        assert tuple(got.shape) == (n, *gpu.out_size, 3)
        _assert_same(got, cpu(src))
    assert gpu.state_dict() == {"seed": 7, "step": 3}
    assert cpu.state_dict() == gpu.state_dict()


@requires_gpu
@pytest.mark.parametrize("n,size,out,pad,norm,extra", SHAPES[:5])
def test_eval_mode_is_centre_crop_without_counter(n, size, out, pad, norm,
                                                  extra):
    gpu, cpu = _pair(out, pad=pad, seed=7, fill=7, **NORMS[norm])
    src = _batch(n, *size, seed=9)
    _assert_same(gpu(src.cuda(), train=False), cpu(src, train=False))
    assert gpu.state_dict()["step"] == 0


@requires_gpu
def test_out_buffer_is_written_in_place():
    gpu, cpu = _pair(8, pad=2, **NORMS["cifar"])
    src = _batch(5, 8, 8)
    out = torch.zeros(5, 8, 8, 3, dtype=torch.bfloat16, device="cuda")
    assert gpu(src.cuda(), out=out) is out
    _assert_same(out, cpu(src))


@requires_gpu
def test_captured_replay_draws_fresh_parameters():
    """The ingest and its counter bump captured once, replayed three times:
    every replay matches the CPU path at the NEXT step, so the draw is a
    function of the device counter and not frozen at capture."""
    n, size = 64, (32, 32)
    gpu, cpu = _pair(32, pad=4, seed=3, **NORMS["cifar"])
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
        draws.append(gpu.params_at(start + k, n, size))
    assert gpu.state_dict() == {"seed": 3, "step": start + 3}
    for a in range(3):
        for b in range(a + 1, 3):
            assert not torch.equal(_bits(outs[a]), _bits(outs[b]))
            assert not all(torch.equal(x, y)
                           for x, y in zip(draws[a], draws[b]))

    # the same source again: only the counter differs, and the output moves
    graph.replay()
    _assert_same(static_out, cpu(src))
    assert not torch.equal(_bits(static_out), _bits(outs[-1]))


@requires_gpu
def test_load_state_dict_sets_the_device_counter():
    gpu, cpu = _pair(8, pad=2, seed=1, **NORMS["imagenet"])
    gpu.load_state_dict({"seed": 21, "step": 1000})
    cpu.load_state_dict({"seed": 21, "step": 1000})
    assert gpu.state_dict() == {"seed": 21, "step": 1000}
    src = _batch(5, 8, 8)
    _assert_same(gpu(src.cuda()), cpu(src))
    assert gpu.state_dict()["step"] == 1001


@requires_gpu
def test_cuda_argument_validation():
    gpu = DeviceAugment(8, pad=2, device="cuda")
    with pytest.raises(ValueError, match="cpu"):
        gpu(_batch(2, 8, 8))                                  # host tensor
    with pytest.raises(TypeError, match="uint8"):
        gpu(_batch(2, 8, 8).cuda().float())
    with pytest.raises(ValueError, match=r"\(7, 7\)"):
        gpu(_batch(2, 3, 3).cuda())
    assert gpu.state_dict()["step"] == 0


@requires_gpu
def test_prefetcher_carries_uint8_batches():
    host = [(_batch(4, 8, 8, seed=s).pin_memory(),
             torch.full((4,), s, dtype=torch.long).pin_memory())
            for s in range(5)]
    seen = 0
    for k, (img, label) in enumerate(DevicePrefetcher(iter(host), "cuda")):
        assert img.is_cuda and img.dtype == torch.uint8
        assert torch.equal(img.cpu(), host[k][0])
        assert torch.equal(label.cpu(), host[k][1])
        seen += 1
    assert seen == 5


@requires_gpu
def test_native_model_takes_the_ingest_output():
    """bf16 NHWC from the kernel and the same image as normalized fp32 NCHW
    through the model's usual entry give bitwise equal logits."""
    from flashy_amd.models import native_resnet18
    torch.manual_seed(0)
    model = native_resnet18(10).cuda().eval()
    gpu, cpu = _pair(32, pad=4, **NORMS["cifar"])
    src = _batch(4, 32, 32, seed=4)
    with torch.no_grad():
        direct = model(gpu(src.cuda(), train=False))
        nchw = cpu(src, train=False).float().permute(0, 3, 1, 2).contiguous()
        usual = model(nchw.cuda())
    assert torch.isfinite(direct).all()
    assert torch.equal(direct, usual)
