# Time ops.conv_wgrad on the flagship (ResNet-18 CIFAR b64) body/downsample
# shapes and the ResNet-50/224 shapes.
#   python scripts/wgrad_sweep.py            per-shape us at the default dispatch
#   python scripts/wgrad_sweep.py --sweep    block target (n_splits) x MG grid
# MG is pinned through FLASHY_WGRAD_MG (read by the launcher on every call;
# builds without wave groups ignore it, so run those without --sweep).
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
    out = [f"{name} M={M} tiles={tiles}:",
           f"default {time_us(lambda: ops.conv_wgrad(x, dy, dw, d)):.1f}us"]
    if sweep:
        for target in (512, 640, 768, 1024, 2048):
            ns = max(1, min(target // tiles, 128, M // 32 or 1))
            cell = []
            for mg in (1, 2, 4):
                os.environ["FLASHY_WGRAD_MG"] = str(mg)
                t = time_us(lambda: ops.conv_wgrad(x, dy, dw, d, n_splits=ns))
                cell.append(f"{t:.1f}")
            os.environ.pop("FLASHY_WGRAD_MG")
            out.append(f"z{ns} mg1/2/4 " + "/".join(cell))
    print("  ".join(out), flush=True)
