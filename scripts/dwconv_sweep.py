# Time the depthwise conv kernels (csrc/conv_depthwise.hip) on MobileNet /
# EfficientNet / ConvNeXt shapes at batch 64, in a hot loop (no tracing),
# against torch's conv (groups=C, channels-last bf16) on the same machine,
# and print the bytes each direction must move over its time.  Each call's
# result is also compared with torch's (max |a - b| / max |b|).
#   python scripts/dwconv_sweep.py                 all shapes, one process each
#   python scripts/dwconv_sweep.py --shape e5s2    one shape, in-process
# The ops.dwconv_* calls are timed as the module runs them: the weight
# gradient includes its workspace allocation and its combine.  Each shape runs
# in a child process under its own `timeout`; the first child that fails ends
# the sweep.
import subprocess
import sys

SHAPES = {  # name: (N, H, W, C, k, stride)
    "m32": (64, 112, 112, 32, 3, 1),
    "m96s2": (64, 112, 112, 96, 3, 2),
    "m144": (64, 56, 56, 144, 3, 1),
    "e240": (64, 28, 28, 240, 5, 1),
    "e672s2": (64, 14, 14, 672, 5, 2),
    "c96": (64, 56, 56, 96, 7, 1),
    "c384": (64, 14, 14, 384, 7, 1),
    "c768": (64, 7, 7, 768, 7, 1),
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

    N, H, W, C, k, st = SHAPES[name]
    p = k // 2
    d = ops.ConvDims(N, H, W, C, C, k, k, (H - 1) // st + 1, (W - 1) // st + 1,
                     st, p)
    torch.manual_seed(3)
    x = torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16)
    w = (torch.randn(C, k, k, 1, device="cuda") * 0.1).to(torch.bfloat16)
    dy = torch.randn(N, d.Ho, d.Wo, C, device="cuda").to(torch.bfloat16)
    y = torch.empty_like(dy)
    dx = torch.empty_like(x)
    dw = torch.zeros(C, k, k, 1, device="cuda")
    # torch's views of the same bytes: NCHW shape, channels-last strides
    xt, dyt, wt = (t.permute(0, 3, 1, 2) for t in (x, dy, w))

    def t_bwd(mask):
        return aten.convolution_backward(dyt, xt, wt, None, [st, st], [p, p],
                                         [1, 1], False, [0, 0], C, mask)

    runs = {
        "fwd": (lambda: ops.dwconv_fwd(x, w, y, d),
                lambda: torch.nn.functional.conv2d(xt, wt, None, st, p, 1, C),
                x.numel() * 2 + y.numel() * 2),
        "dgrad": (lambda: ops.dwconv_dgrad(dy, w, dx, d),
                  lambda: t_bwd([True, False, False]),
                  dy.numel() * 2 + dx.numel() * 2),
        "wgrad": (lambda: ops.dwconv_wgrad(x, dy, dw, d),
                  lambda: t_bwd([False, True, False]),
                  x.numel() * 2 + dy.numel() * 2),
    }
    # same results first
    ops.dwconv_fwd(x, w, y, d)
    ops.dwconv_dgrad(dy, w, dx, d)
    ops.dwconv_wgrad(x, dy, dw, d)
    errs = (rel(y, runs["fwd"][1]().permute(0, 2, 3, 1)),
            rel(dx, t_bwd([True, False, False])[0].permute(0, 2, 3, 1)),
            rel(dw, t_bwd([False, True, False])[1].permute(0, 2, 3, 1)))
    out = [f"{name} {N}x{H}x{W}x{C} k{k} s{st}:",
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
