# Time the 8-wave conv kernels per shape and direction in a hot loop (no
# tracing): what ops.conv_fwd / ops.conv_dgrad run today, against every tile
# ops.conv8_form can force (BM 256 / 128 x BN 128 / 64) at split factors
# 1 (single pass) to 8, each with the combine it needs (forward: the
# BN-partials combine, as in a conv that feeds BatchNorm).
#   python scripts/splitk_sweep.py               all shapes, one process each
#   python scripts/splitk_sweep.py --passes 2    the whole table twice
#   python scripts/splitk_sweep.py --shape c10-l4   one shape, in-process
# Each shape runs in a child process under its own `timeout`; the first
# child that fails ends the sweep.
import subprocess
import sys

SHAPES = {  # name: (N,H,W,C,K,R,stride,pad)
    "c10-l3": (64, 8, 8, 256, 256, 3, 1, 1),
    "c10-l4": (64, 4, 4, 512, 512, 3, 1, 1),
    "c10-l3s2": (64, 16, 16, 128, 256, 3, 2, 1),
    "c10-l4s2": (64, 8, 8, 256, 512, 3, 2, 1),
    "c10-ds2": (64, 32, 32, 64, 128, 1, 2, 0),
    "c10-ds3": (64, 16, 16, 128, 256, 1, 2, 0),
    "c10-ds4": (64, 8, 8, 256, 512, 1, 2, 0),
    "r50c-l3a": (64, 8, 8, 1024, 256, 1, 1, 0),
    "r50c-l4c": (64, 4, 4, 512, 2048, 1, 1, 0),
    "r50-l3": (64, 14, 14, 256, 256, 3, 1, 1),
    "r50-l4": (64, 7, 7, 512, 512, 3, 1, 1),
    "r50-l4a": (64, 7, 7, 2048, 512, 1, 1, 0),
}
ZNS = (1, 2, 3, 4, 5, 6, 8)
ITERS = 30
CHILD_TIMEOUT = 240


def run_shape(name):
    import torch
    sys.path.insert(0, ".")
    from flashy_amd import ops
    ext = ops.require()

    def time_us(fn):
        for _ in range(3):
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
    x = torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16)
    w = (torch.randn(K, R, R, C, device="cuda") * 0.1).to(torch.bfloat16)
    d = ops.ConvDims.infer(x, w, st, pad)
    dy = torch.randn(N, d.Ho, d.Wo, K, device="cuda").to(torch.bfloat16)
    wt = w.new_empty((d.R, d.S, d.C, d.K))
    ops.weight_transpose(w, wt)
    for dgrad in (False, True):
        M = d.N * d.H * d.W if dgrad else d.N * d.Ho * d.Wo
        cols = d.C if dgrad else d.K
        stages = d.R * d.S * (d.K if dgrad else d.C) // 64
        out = torch.empty(M * cols, device="cuda", dtype=torch.bfloat16)
        a, ww = (dy, wt) if dgrad else (x, w)
        if dgrad:
            cur = time_us(lambda: ops.conv_dgrad(dy, wt, out, d))
        else:
            cur = time_us(lambda: ops.conv_fwd(x, w, out, d, want_stats=True))
        head = (f"{name} {'dgrad' if dgrad else 'fwd'} (M={M}, cols={cols}, "
                f"stages={stages}): current {cur:.1f}")
        print(head, flush=True)
        msplit = ops.bn_msplit(M, cols)
        partials = torch.empty(2 * cols * max(msplit, (M + 127) // 128),
                               device="cuda")
        for bm in (256, 128):
            for bn in (128, 64):
                if cols % bn:
                    continue
                line = [f"  bm{bm} bn{bn}:"]
                seen = set()
                for zn in ZNS:
                    if zn > stages:
                        continue
                    spz = (stages + zn - 1) // zn
                    zeff = (stages + spz - 1) // spz
                    if zeff in seen:
                        continue
                    seen.add(zeff)
                    if zeff == 1:
                        def fn():
                            ops.conv8_form(a, ww, out, d, dgrad, bm, bn,
                                           bn_ws=None if dgrad else partials)
                    else:
                        ws = torch.empty(zeff * M * cols, device="cuda")

                        def fn(ws=ws, spz=spz, zeff=zeff):
                            ops.conv8_form(a, ww, ws, d, dgrad, bm, bn,
                                           spz=spz)
                            if dgrad:
                                ops.splitk_combine(ws, out, zeff)
                            else:
                                ext.splitk_combine_stats(
                                    ws.data_ptr(), out.data_ptr(),
                                    partials.data_ptr(), M, cols, zeff,
                                    msplit, ops._stream())
                    line.append(f"z{zeff} {time_us(fn):.1f}")
                print("  ".join(line), flush=True)


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
