"""Build recipe for libpgf_hip.so (hipcc, gfx950 only; cross-compiles without a GPU)."""

from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libpgf_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

# The contraction rule.  The files of NO_CONTRACT must not contract a*b+c into fma: active-set masks
# and matrix entries are compared bit-for-bit with numpy expressions, and the fixed-order sums of
# pgf_step_dev.h / pgf_reduce_dev.h give equal bits wherever they are included.  Every file that
# includes one of those two headers belongs here (tests/test_build_sources.py checks it).
NO_CONTRACT = [
    "pgf_kernels.hip",
    "pgf_guard_kernels.hip",
    "pgf_batch_kernels.hip",
    "pgf_sparse.hip",
    "pgf_line_search.hip",
    "pgf_batch_line_search.hip",
    "pgf_border.hip",
    "pgf_border_large.hip",
    "pgf_unsym.hip",
    "pgf_api.hip",
    "pgf_api_factor.hip",
    "pgf_api_guard.hip",
    "pgf_api_step.hip",
    "pgf_api_band.hip",
    "pgf_api_band_setup.hip",
    "pgf_api_line_search.hip",
    "pgf_api_unsym.hip",
    "pgf_api_batch.hip",
    "pgf_api_band_batch.hip",
    "pgf_api_batch_ctl.hip",
    "pgf_api_batch_line_search.hip",
    "pgf_api_batch_read.hip",
    "pgf_api_comm.hip",
    "pgf_api_aux.hip",
]
# The factorisations and the wide band contract freely; what must be bit-exact inside them switches
# contraction off itself (pgf_head_dev.h).
CONTRACT = [
    "pgf_band_wide.hip",
    "pgf_ldlt.hip",
    "pgf_factor2.hip",
    "pgf_update_plan.hip",
    "pgf_lu.hip",
]
# (source, extra flags)
SOURCES = [(s, ["-ffp-contract=off"]) for s in NO_CONTRACT] + [(s, []) for s in CONTRACT]
COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function"]


def _newer(target, deps):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "pgf_hip.h"))
    objs = []
    for src, extra in SOURCES:
        sp = os.path.join(CSRC, src)
        op = os.path.join(CSRC, src.replace(".hip", ".o"))
        if force or not _newer(op, [sp] + headers):
            cmd = [HIPCC, *COMMON, *extra, "-c", sp, "-o", op]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
        objs.append(op)
    if force or not _newer(LIB, objs):
        cmd = [HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", *objs, "-o", LIB]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
