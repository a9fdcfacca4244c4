# Copyright (c) Flashy-AMD authors.
"""In-tree build of the gfx950 native extension.

``python -m flashy_amd.ops.build`` compiles csrc/*.hip + ext.cpp with hipcc
(--offload-arch=gfx950) into ``flashy_amd/ops/_hip_ops.<abi>.so``.  The .so
lives in the source tree (it is .gitignored but ships to the GPU box with the
gpurun snapshot).  hipcc cross-compiles without a GPU, so this runs on the
CPU-only build box too.
"""
from __future__ import annotations

import os
import subprocess
import sys
import sysconfig
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

HERE = Path(__file__).resolve().parent
CSRC = HERE / "csrc"
ARCH = "gfx950"
# Translation units built without packed fp32 instructions (v_pk_add_f32,
# v_pk_mul_f32, v_pk_fma_f32).  Each lane's arithmetic is the same IEEE
# operation either way, so results do not move; these kernels are bound by
# memory and launch latency, not by the VALU.  New kernel code goes here.
SCALAR_FP32 = {"batchnorm.hip"}
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]


def so_path() -> Path:
    suffix = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    return HERE / f"_hip_ops{suffix}"


def sources() -> list:
    return sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.cpp"))


def needs_build() -> bool:
    out = so_path()
    if not out.exists():
        return True
    # every header counts: the 8-wave kernel core lives in conv8.h
    newest = max(p.stat().st_mtime
                 for p in sources() + sorted(CSRC.glob("*.h")))
    return out.stat().st_mtime < newest


def build(verbose: bool = True, force: bool = False) -> Path:
    out = so_path()
    if not force and not needs_build():
        if verbose:
            print(f"[flashy_amd.ops.build] up to date: {out}")
        return out
    import pybind11
    py_include = sysconfig.get_paths()["include"]
    base = [
        "hipcc", f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC",
        "-DNDEBUG",
        f"-I{py_include}", f"-I{pybind11.get_include()}", f"-I{CSRC}",
    ]

    def run(cmd: list) -> None:
        if verbose:
            print("[flashy_amd.ops.build]", " ".join(cmd))
        subprocess.run(cmd, check=True)

    # one object per source (flags differ per file), a few at a time, then
    # one link; the objects live in a temporary folder, not in the tree
    with tempfile.TemporaryDirectory(prefix="flashy_amd_build_") as tmp:
        def compile_one(src: Path) -> str:
            obj = str(Path(tmp) / (src.name + ".o"))
            flags = NO_PACKED_FP32 if src.name in SCALAR_FP32 else []
            run(base + flags + ["-c", str(src), "-o", obj])
            return obj

        jobs = max(1, min(8, os.cpu_count() or 1))
        with ThreadPoolExecutor(jobs) as pool:
            objs = list(pool.map(compile_one, sources()))
        run(["hipcc", f"--offload-arch={ARCH}", "-fPIC", "-shared", *objs,
             "-o", str(out)])
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv)
