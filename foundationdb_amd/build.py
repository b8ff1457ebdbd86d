"""Build the in-tree HIP extension libfdbcs.so for gfx950 (hipcc cross-compiles; no GPU needed)."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libfdbcs.so")
# The engine's sources, named here once: roofline.BUILD_SOURCES (the build id of profile files) and
# scripts/build_variant.sh (same-box A/B libraries) read these lists.
SOURCES = ["engine.cpp", "transfer.cpp", "ingest.cpp", "verify.cpp", "kernels.hip", "transfer.hip", "ingest.hip",
           "verify.hip"]
HEADERS = ["dkey.h", "engine.h", "engine_impl.h", "transfer.h", "ingest.h", "verify.h", "search.h", "scan.h",
           "launch.h", "lane_xor.h"]
PUBLIC_HEADER = "include/fdb_conflict_set.h"  # relative to the repository root
ARCH = os.environ.get("FDBCS_OFFLOAD_ARCH", "gfx950")


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.join(ROOT, PUBLIC_HEADER)]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        return LIB
    objs = []
    hipcc = _hipcc()
    common = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
              "-mllvm", "-disable-promote-alloca-to-lds"]
    for src in SOURCES:
        obj = os.path.join(CSRC, src + ".o")  # transfer.cpp and transfer.hip: the suffix stays in the name
        cmd = [hipcc, *common, "-c", os.path.join(CSRC, src), "-o", obj]
        if src.endswith(".cpp"):
            cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "-Wall", "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
        objs.append(obj)
    tmp = LIB + ".tmp"
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp, *objs]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    print(LIB)
