# Time the stride-2 backward-data forms per shape in a hot loop (no tracing):
# the previous dispatch (4-wave parity / generic / generic split-K + combine,
# rebuilt here from the public bindings), the current ops.conv_dgrad, and
# every form ops.conv_dgrad_s2_form can force on the shape.
#   python scripts/dgrad_s2_sweep.py              all shapes, one process each
#   python scripts/dgrad_s2_sweep.py --passes 2   the whole table twice
#   python scripts/dgrad_s2_sweep.py --shape c10-l4s2   one shape, in-process
# Each shape runs in a child process under its own `timeout`; the first
# child that fails ends the sweep.
import subprocess
import sys

SHAPES = {  # name: (N,H,W,C,K,R,stride,pad) of the conv whose dx is computed
    "c10-l2s2": (64, 32, 32, 64, 128, 3, 2, 1),
    "c10-l3s2": (64, 16, 16, 128, 256, 3, 2, 1),
    "c10-l4s2": (64, 8, 8, 256, 512, 3, 2, 1),
    "c10-ds2": (64, 32, 32, 64, 128, 1, 2, 0),
    "c10-ds3": (64, 16, 16, 128, 256, 1, 2, 0),
    "c10-ds4": (64, 8, 8, 256, 512, 1, 2, 0),
    "r50-l2s2": (64, 56, 56, 128, 128, 3, 2, 1),
    "r50-l3s2": (64, 28, 28, 256, 256, 3, 2, 1),
    "r50-l4s2": (64, 14, 14, 512, 512, 3, 2, 1),
    "r50-ds2": (64, 56, 56, 256, 512, 1, 2, 0),
    "r50-ds3": (64, 28, 28, 512, 1024, 1, 2, 0),
    "r50-ds4": (64, 14, 14, 1024, 2048, 1, 2, 0),
}
ITERS = 50
CHILD_TIMEOUT = 120


def previous_dispatch(ops, ext, dy, wt, dx, d):
    """The dispatch before the stride-2 plan: SCAT2 from 104 blocks, split-K
    decided first from the zero-filled stage count, then the 4-wave parity
    kernel for 3x3, else the generic kernel."""
    M = d.N * d.H * d.W
    stages = d.R * d.S * d.K // 64
    zn = 0
    if not ext.conv8_eligible(*d, True):
        zn = ops._splitk_plan(M, d.C // 64, stages)
    if zn:
        spz = (stages + zn - 1) // zn
        zeff = (stages + spz - 1) // spz
        ws = dy.new_empty(zeff * M * d.C).float()

        def run():
            ext.conv_dgrad_splitk(dy.data_ptr(), wt.data_ptr(), ws.data_ptr(),
                                  *d, spz, ops._stream())
            ext.splitk_combine(ws.data_ptr(), dx.data_ptr(), M * d.C, zeff,
                               False, ops._stream())
        return f"splitk-z{zeff}", run
    if d.R == 1:
        mt = (d.N * d.Ho * d.Wo + 255) // 256
        for bn in (128, 64):
            if d.C % bn == 0 and mt * (d.C // bn) >= 104 and \
                    d.H % 2 == 0 and d.W % 2 == 0:
                return f"scat2-{bn}", lambda: ops.conv_dgrad_s2_form(
                    dy, wt, dx, d, "scat2", bn)
        return "generic", lambda: ops.conv_dgrad_s2_form(dy, wt, dx, d,
                                                         "generic", 0)
    Mc = d.N * ((d.H + 1) // 2) * ((d.W + 1) // 2)
    bm = 32
    for cand in (128, 64):
        if (Mc + cand - 1) // cand * (d.C // 64) * 4 >= 208:
            bm = cand
            break
    return f"par4-{bm}", lambda: ops.conv_dgrad_s2_form(dy, wt, dx, d,
                                                        "par4", bm)


def run_shape(name):
    import torch
    sys.path.insert(0, ".")
    from flashy_amd import ops
    ext = ops.require()

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

    N, H, W, C, K, R, st, pad = SHAPES[name]
    Ho = (H + 2 * pad - R) // st + 1
    Wo = (W + 2 * pad - R) // st + 1
    d = ops.ConvDims(N, H, W, C, K, R, R, Ho, Wo, st, pad)
    dy = torch.randn(N, Ho, Wo, K, device="cuda").to(torch.bfloat16)
    wt = (torch.randn(R, R, C, K, device="cuda") * 0.1).to(torch.bfloat16)
    dx = torch.empty(N, H, W, C, device="cuda", dtype=torch.bfloat16)
    prev_name, prev = previous_dispatch(ops, ext, dy, wt, dx, d)
    plan = "%s-%d" % ops.conv_dgrad_s2_plan(d)
    out = [f"{name}:", f"previous[{prev_name}] {time_us(prev):.1f}",
           f"current[{plan}] "
           f"{time_us(lambda: ops.conv_dgrad(dy, wt, dx, d)):.1f}"]
    forms = [("generic", 0), ("par8", 64), ("par8", 128),
             ("par4", 128), ("par4", 64), ("par4", 32)]
    if R == 1:
        forms += [("scat2", 64), ("scat2", 128)]
    for form, tile in forms:
        if tile > 64 and form != "par4" and C % tile:
            continue
        t = time_us(lambda: ops.conv_dgrad_s2_form(dy, wt, dx, d, form, tile))
        out.append(f"{form}-{tile} {t:.1f}")
    print("  ".join(out) + "  (us)", flush=True)


if __name__ == "__main__":
    if "--shape" in sys.argv:
        run_shape(sys.argv[sys.argv.index("--shape") + 1])
        sys.exit(0)
    passes = int(sys.argv[sys.argv.index("--passes") + 1]) \
        if "--passes" in sys.argv else 1
    for p in range(passes):
        print(f"# pass {p + 1}", flush=True)
        for name in SHAPES:
            rc = subprocess.run(
                ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable,
                 __file__, "--shape", name]).returncode
            if rc:
                print(f"{name}: exit status {rc}; sweep stopped", flush=True)
                sys.exit(rc)
