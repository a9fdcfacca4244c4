# Copyright (c) Flashy-AMD authors.
"""CPU-checkable pieces of the ops layer: dim inference and launch plans."""
import pytest
import torch

from flashy_amd import ops


def test_convdims_infer_asymmetric():
    x = torch.zeros(2, 17, 9, 8)
    w = torch.zeros(32, 5, 3, 8)            # R=5, S=3
    d = ops.ConvDims.infer(x, w, stride=2, pad=1)
    assert (d.R, d.S) == (5, 3)
    assert d.Ho == (17 + 2 - 5) // 2 + 1
    assert d.Wo == (9 + 2 - 3) // 2 + 1


def test_splitk_plan_regimes():
    # big-M short-K: single pass
    assert ops._splitk_plan(65536, 1, 9) == 0
    # tiny reductions never split
    assert ops._splitk_plan(128, 1, 2) == 0
    # underfilled grid: split for fill
    zn = ops._splitk_plan(1024, 8, 72)
    assert 2 <= zn <= 8
    # full grid + long reduction: split for the K length (measured 20-25%)
    zn = ops._splitk_plan(3136, 8, 72)
    assert zn == 5
    # cap at 8
    assert ops._splitk_plan(64, 1, 200) <= 8


def test_needs_build_sees_every_header(tmp_path, monkeypatch):
    """An edit to ANY csrc header (the 8-wave kernel core lives in one) must
    invalidate the built extension.  Paths are redirected to a scratch
    directory; nothing is compiled."""
    import os
    from flashy_amd.ops import build
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    for name in ("a.hip", "ext.cpp", "common.h", "conv8.h"):
        (csrc / name).write_text("// stub\n")
        os.utime(csrc / name, (1000, 1000))
    so = tmp_path / "_hip_ops.so"
    so.write_bytes(b"")
    os.utime(so, (2000, 2000))
    monkeypatch.setattr(build, "CSRC", csrc)
    monkeypatch.setattr(build, "so_path", lambda: so)
    assert not build.needs_build()
    for name in ("conv8.h", "common.h", "a.hip", "ext.cpp"):
        os.utime(csrc / name, (3000, 3000))
        assert build.needs_build(), name
        os.utime(csrc / name, (1000, 1000))
    assert not build.needs_build()
    so.unlink()
    assert build.needs_build()


def test_underfill_zn():
    # r4-class dgrad (64,7,7,512,192,3x3): 52 tiles, 27 stages -> 3 slices
    assert ops._underfill_zn(3136, 512, 27) == 3
    assert ops._underfill_zn(3136, 512, 15) == 0     # short reduction
    assert ops._underfill_zn(64 * 56 * 56, 256, 64) == 0   # grid already full


def test_bn_wrappers_refuse_widths_before_touching_the_extension(monkeypatch):
    """The reductions walk 64-channel groups, the rest 8-channel octets; the
    check runs before the extension is even loaded, so nothing is launched."""
    def no_ext():
        raise AssertionError("extension reached")

    monkeypatch.setattr(ops, "require", no_ext)
    t = torch.zeros(8)
    for C in (0, 8, 32, 96):
        with pytest.raises(ValueError):
            ops.bn_stats(t, t, 4, C, 1)
        with pytest.raises(ValueError):
            ops.bn_bwd_reduce(t, t, t, t, t, t, 4, C, 1, False)
    for C in (0, 4, 12, 60):
        with pytest.raises(ValueError):
            ops.bn_finalize(t, 1, t, t, t, t, t, 4, C, 1e-5, 0.1, False)
        with pytest.raises(ValueError):
            ops.bn_apply(t, None, t, t, 4, C, False)
        with pytest.raises(ValueError):
            ops.bn_bwd_grads(t, 1, t, t, t, C)
        with pytest.raises(ValueError):
            ops.bn_bwd_apply(t, t, t, t, t, 4, C)
    # accepted widths get as far as the extension
    for call in (lambda: ops.bn_stats(t, t, 4, 128, 1),
                 lambda: ops.bn_apply(t, None, t, t, 4, 40, False)):
        with pytest.raises(AssertionError, match="extension reached"):
            call()


def test_bn_msplit_alignment():
    for M, C in [(65536, 64), (16384, 128), (1024, 512), (48, 64)]:
        ms = ops.bn_msplit(M, C)
        assert ms >= 1
        if ms >= 4:
            assert ms % 4 == 0   # float4-aligned partial rows
        assert ms <= max(1, (M + 31) // 32)
