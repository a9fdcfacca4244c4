# Time the grouped 3x3 conv kernels (csrc/conv_group.hip) on ResNeXt-50
# 32x4d's grouped shapes at batch 64 / 224 px, in a hot loop (no tracing),
# against torch's conv (groups=32, channels-last bf16) on the same machine,
# and print the bytes each direction must move over its time.  Each call's
# result is also compared with torch's (max |a - b| / max |b|).
#   python scripts/gconv_sweep.py                 all shapes, one process each
#   python scripts/gconv_sweep.py --shape l2s2    one shape, in-process
# The ops.gconv_* calls are timed as the module runs them: forward and
# backward-data include the operand expansion, the weight gradient includes
# its combine.  Each shape runs in a child process under its own `timeout`;
# the first child that fails ends the sweep.
import subprocess
import sys

GROUPS = 32
SHAPES = {  # name: (N, H, W, C, stride)
    "l1": (64, 56, 56, 128, 1),
    "l2s2": (64, 56, 56, 256, 2),
    "l2": (64, 28, 28, 256, 1),
    "l3s2": (64, 28, 28, 512, 2),
    "l3": (64, 14, 14, 512, 1),
    "l4s2": (64, 14, 14, 1024, 2),
    "l4": (64, 7, 7, 1024, 1),
}
ITERS = 50
CHILD_TIMEOUT = 150


def run_shape(name):
    import torch
    sys.path.insert(0, ".")
    from flashy_amd import ops
    aten = torch.ops.aten

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

    def rel(a, b):
        return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()

    N, H, W, C, st = SHAPES[name]
    cg = C // GROUPS
    d = ops.ConvDims(N, H, W, C, C, 3, 3, (H - 1) // st + 1, (W - 1) // st + 1,
                     st, 1)
    torch.manual_seed(3)
    x = torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16)
    w = (torch.randn(C, 3, 3, cg, device="cuda") * 0.1).to(torch.bfloat16)
    dy = torch.randn(N, d.Ho, d.Wo, C, device="cuda").to(torch.bfloat16)
    y = torch.empty_like(dy)
    dx = torch.empty_like(x)
    dw = torch.zeros(C, 3, 3, cg, device="cuda")
    # torch's views of the same bytes: NCHW shape, channels-last strides
    xt, dyt, wt = (t.permute(0, 3, 1, 2) for t in (x, dy, w))

    def t_bwd(mask):
        return aten.convolution_backward(dyt, xt, wt, None, [st, st], [1, 1],
                                         [1, 1], False, [0, 0], GROUPS, mask)

    runs = {
        "fwd": (lambda: ops.gconv_fwd(x, w, y, d, GROUPS),
                lambda: torch.nn.functional.conv2d(xt, wt, None, st, 1, 1,
                                                   GROUPS),
                x.numel() * 2 + y.numel() * 2),
        "dgrad": (lambda: ops.gconv_dgrad(dy, w, dx, d, GROUPS),
                  lambda: t_bwd([True, False, False]),
                  dy.numel() * 2 + dx.numel() * 2),
        "wgrad": (lambda: ops.gconv_wgrad(x, dy, dw, d, GROUPS),
                  lambda: t_bwd([False, True, False]),
                  x.numel() * 2 + dy.numel() * 2),
    }
    # same results first
    ops.gconv_fwd(x, w, y, d, GROUPS)
    ops.gconv_dgrad(dy, w, dx, d, GROUPS)
    ops.gconv_wgrad(x, dy, dw, d, GROUPS)
    errs = (rel(y, runs["fwd"][1]().permute(0, 2, 3, 1)),
            rel(dx, t_bwd([True, False, False])[0].permute(0, 2, 3, 1)),
            rel(dw, t_bwd([False, True, False])[1].permute(0, 2, 3, 1)))
    out = [f"{name} {N}x{H}x{W}x{C} s{st}:",
           "vs torch %.1e %.1e %.1e" % errs]
    for direction, (ours, theirs, nbytes) in runs.items():
        a, b = time_us(ours), time_us(theirs)
        out.append(f"{direction} {a:.1f} us (torch {b:.1f}) "
                   f"{nbytes / a / 1e3:.0f} GB/s")
    print("  ".join(out), flush=True)


if __name__ == "__main__":
    if "--shape" in sys.argv:
        run_shape(sys.argv[sys.argv.index("--shape") + 1])
        sys.exit(0)
    for name in SHAPES:
        rc = subprocess.run(
            ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable,
             __file__, "--shape", name]).returncode
        if rc:
            print(f"{name}: exit status {rc}; sweep stopped", flush=True)
            sys.exit(rc)
