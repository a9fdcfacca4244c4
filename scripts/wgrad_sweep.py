# Time ops.conv_wgrad on the flagship (ResNet-18 CIFAR b64) body/downsample
# shapes and the ResNet-50/224 shapes.
#   python scripts/wgrad_sweep.py            per-shape us at the default dispatch
#   python scripts/wgrad_sweep.py --sweep    block target (n_splits) x MG grid,
#                                            one row per staging pipeline
# MG is pinned through FLASHY_WGRAD_MG, the pipeline through FLASHY_WGRAD_DMA
# (0 = register-staged k_conv_wgrad, 1 = k_conv_wgrad_dma); the launcher reads
# both on every call.  Shapes that run k_conv_wgrad8 ignore them.
import os
import sys
import torch
sys.path.insert(0, ".")
from flashy_amd import ops  # noqa: E402

SHAPES = {  # name: (N,H,W,C,K,R,stride)
    "c10-l1": (64, 32, 32, 64, 64, 3, 1),
    "c10-l2s2": (64, 32, 32, 64, 128, 3, 2),
    "c10-l2": (64, 16, 16, 128, 128, 3, 1),
    "c10-l3s2": (64, 16, 16, 128, 256, 3, 2),
    "c10-l3": (64, 8, 8, 256, 256, 3, 1),
    "c10-l4s2": (64, 8, 8, 256, 512, 3, 2),
    "c10-l4": (64, 4, 4, 512, 512, 3, 1),
    "c10-ds2": (64, 32, 32, 64, 128, 1, 2),
    "c10-ds3": (64, 16, 16, 128, 256, 1, 2),
    "c10-ds4": (64, 8, 8, 256, 512, 1, 2),
    "r50-l1c2": (64, 56, 56, 64, 64, 3, 1),
    "r50-l2c2": (64, 28, 28, 128, 128, 3, 1),
    "r50-l1c3": (64, 56, 56, 64, 256, 1, 1),
    "r50-l3c2": (64, 14, 14, 256, 256, 3, 1),
}
FORMS = {"reg": "0", "dma": "1"}   # pipeline name: FLASHY_WGRAD_DMA
PINS = ("FLASHY_WGRAD_MG", "FLASHY_WGRAD_DMA")
ITERS = 50


def time_us(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS * 1000


def pin(mg, form):
    os.environ["FLASHY_WGRAD_MG"] = str(mg)
    os.environ["FLASHY_WGRAD_DMA"] = FORMS[form]


def unpin():
    for name in PINS:
        os.environ.pop(name, None)


sweep = "--sweep" in sys.argv
for name, (N, H, W, C, K, R, st) in SHAPES.items():
    pad = R // 2
    x = torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16)
    w = (torch.randn(K, R, R, C, device="cuda") * 0.1).to(torch.bfloat16)
    d = ops.ConvDims.infer(x, w, st, pad)
    dy = torch.randn(N, d.Ho, d.Wo, K, device="cuda").to(torch.bfloat16)
    dw = torch.zeros(K, R, R, C, device="cuda", dtype=torch.float32)
    tiles = (K // 64) * (R * R * C // 64)
    M = d.N * d.Ho * d.Wo
    print(f"{name} M={M} tiles={tiles}: {ops.conv_wgrad_form(d)} default "
          f"{time_us(lambda: ops.conv_wgrad(x, dy, dw, d)):.1f}us", flush=True)
    if not sweep or ops.conv_wgrad_form(d) == "wgrad8":
        continue
    for form in FORMS:
        out = [f"  {form:6}"]
        for target in (512, 768, 1024, 2048):
            ns = max(1, min(target // tiles, 128, M // 32 or 1))
            cell = []
            for mg in (1, 2, 4):
                pin(mg, form)
                t = time_us(lambda: ops.conv_wgrad(x, dy, dw, d, n_splits=ns))
                unpin()
                cell.append(f"{t:.1f}")
            out.append(f"z{ns} " + "/".join(cell))
        print("  ".join(out), flush=True)
