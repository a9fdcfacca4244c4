# Time the pointwise conv kernels (csrc/conv_point.hip) on ConvNeXt-T's
# off-grid convs at batch 64, in a hot loop (no tracing), against torch's own
# bf16 F.linear (p = 1) / F.conv2d (p = 2) and their backward on the same
# tensors, same machine, same process.  Next to each time: the traffic floor,
# the bytes a direction reads once plus the bytes it writes once (weights
# included, the wgrad workspace not) over HBM_GBS.  Each call cycles through
# SETS copies of its activations, so the timed set (0.5-0.8 GB) does not sit
# in the 256 MB last-level cache.  Each call's result is also compared with
# torch's (max |a - b| / max |b|).
#   python scripts/pwconv_sweep.py                 all shapes, one process each
#   python scripts/pwconv_sweep.py --shape mlp1    one shape, in-process
# The ops.pwconv_* calls are timed as the module runs them: the weight
# gradient includes its workspace allocation and its combine.  Each shape runs
# in a child process under its own `timeout`; the first child that fails ends
# the sweep.
import subprocess
import sys

SHAPES = {  # name: (N, H, W, C, p, K)
    "mlp1": (64, 56, 56, 96, 1, 384),
    "mlp2": (64, 56, 56, 384, 1, 96),
    "down": (64, 56, 56, 96, 2, 192),
}
ITERS = 1000
SETS = 4
HBM_GBS = 8000.0    # the part's public HBM3E rate
CHILD_TIMEOUT = 150


def run_shape(name):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ".")
    from flashy_amd import ops
    aten = torch.ops.aten

    def time_us(fn):
        for i in range(2 * SETS):
            fn(i % SETS)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(True), torch.cuda.Event(True)
        s.record()
        for i in range(ITERS):
            fn(i % SETS)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / ITERS * 1000

    def rel(a, b):
        return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()

    N, H, W, C, p, K = SHAPES[name]
    d = ops.ConvDims(N, H, W, C, K, p, p, H // p, W // p, p, 0)
    torch.manual_seed(3)
    w = (torch.randn(K, p, p, C, device="cuda") * 0.1).to(torch.bfloat16)
    xs = [torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16)
          for _ in range(SETS)]
    dys = [torch.randn(N, d.Ho, d.Wo, K, device="cuda").to(torch.bfloat16)
           for _ in range(SETS)]
    ys = [torch.empty_like(t) for t in dys]
    dxs = [torch.empty_like(t) for t in xs]
    dw = torch.zeros(K, p, p, C, device="cuda")
    wt = w.permute(0, 3, 1, 2)      # torch's view of the same bytes
    w2 = w.view(K, C) if p == 1 else None

    def t_fwd(i):
        if p == 1:
            return F.linear(xs[i], w2)
        return F.conv2d(xs[i].permute(0, 3, 1, 2), wt, None, p)

    def t_bwd(i, mask):
        if p == 1:      # the two GEMMs F.linear's backward runs
            if mask[0]:
                return dys[i].view(-1, K) @ w2
            return dys[i].view(-1, K).t() @ xs[i].view(-1, C)
        return aten.convolution_backward(
            dys[i].permute(0, 3, 1, 2), xs[i].permute(0, 3, 1, 2), wt, None,
            [p, p], [0, 0], [1, 1], False, [0, 0], 1, mask)

    wb = w.numel() * 2
    runs = {
        "fwd": (lambda i: ops.pwconv_fwd(xs[i], w, ys[i], d), t_fwd,
                xs[0].numel() * 2 + ys[0].numel() * 2 + wb),
        "dgrad": (lambda i: ops.pwconv_dgrad(dys[i], w, dxs[i], d),
                  lambda i: t_bwd(i, [True, False, False]),
                  dys[0].numel() * 2 + dxs[0].numel() * 2 + wb),
        "wgrad": (lambda i: ops.pwconv_wgrad(xs[i], dys[i], dw, d),
                  lambda i: t_bwd(i, [False, True, False]),
                  xs[0].numel() * 2 + dys[0].numel() * 2 + 2 * wb),
    }
    # same results first
    ops.pwconv_fwd(xs[0], w, ys[0], d)
    ops.pwconv_dgrad(dys[0], w, dxs[0], d)
    ops.pwconv_wgrad(xs[0], dys[0], dw, d)
    ty, tdx, tdw = t_fwd(0), t_bwd(0, [True, False, False]), \
        t_bwd(0, [False, True, False])
    if p == 2:
        ty, tdx, tdw = (t.permute(0, 2, 3, 1) for t in (ty, tdx[0], tdw[1]))
    errs = (rel(ys[0], ty.reshape(ys[0].shape)),
            rel(dxs[0], tdx.reshape(dxs[0].shape)),
            rel(dw, tdw.reshape(dw.shape)))
    out = [f"{name} {N}x{H}x{W}x{C} p{p} K{K}:",
           "vs torch %.1e %.1e %.1e" % errs]
    for direction, (ours, theirs, nbytes) in runs.items():
        a, b = time_us(ours), time_us(theirs)
        out.append(f"{direction} {a:.1f} us (torch {b:.1f}, floor "
                   f"{nbytes / HBM_GBS / 1e3:.1f}) {nbytes / a / 1e3:.0f} GB/s")
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
