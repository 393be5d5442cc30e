"""Times the Standard / Extended / Asymmetric formulations on one MI355X (median of --reps after
--warmup warm-ups, the convention of SURVEY.md 8d), at config 2b (n = 4096, m = 1024, 25 % boxed)
and at n = 1024, m = 256, per kind:

  (a) a Full step through the plugin classes with PGF_UNSYM_HOST=1 (host assembly with scipy, the
      dense matrix uploaded to the stand-alone LU: what the classes did before the device path);
  (b) the same step on the device path;
  (c) a DeviceNewton Full step;
  (d) the assembly kernel alone (HIP events, pgf_profile_read_ex), with its algorithmic bytes --
      H read once (n^2; Standard also G), J twice, (n + m)^2 doubles written -- and the bandwidth
      they imply;
  and, for the bound on (c): the LU's own factor + solve time (HipLinearSolver(symmetric=False) on
  the downloaded matrix: wall time of constructor + one solve, minus the separately measured
  upload of the same bytes) plus a Symmetric-path Full step outside its factorisation (step wall
  time minus the profiled factor_ms).

Writes profiles/unsym_device_assembly.json (or --out).

    python tools/time_unsym.py [--sizes 4096x1024,1024x256] [--reps 20] [--warmup 3]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import pygradflow_amd as pgf  # noqa: E402
from pygradflow_amd import _lib, problems  # noqa: E402
from pygradflow_amd.newton import newton_method  # noqa: E402

KINDS = ("Standard", "Extended", "Asymmetric")


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def plugin_step_ms(prob, kind, host, reps, warmup):
    """One FullNewtonMethod.step at the outer iterate (mask, derivatives, assembly, LU, solve)."""
    if host:
        os.environ["PGF_UNSYM_HOST"] = "1"
    else:
        os.environ.pop("PGF_UNSYM_HOST", None)
    n, m = prob.num_vars, prob.num_cons
    params = pgf.Params(newton_type="Full", step_solver_type=kind)
    orig = pgf.Iterate(prob, params, np.zeros(n), np.zeros(m))
    method = newton_method(prob, params, orig, 1.0, 1.0)
    try:
        ms = median_ms(lambda: method.step(orig), reps, warmup)
        stats = method.step_solver.unsym_stats()
    finally:
        method.step_solver.close()
        os.environ.pop("PGF_UNSYM_HOST", None)
    return ms, stats


def device_newton(prob, kind, reps, warmup):
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    dn = pgf.DeviceNewton(prob, "Full", x0, y0, 1.0, 1.0, step_solver_type=kind)
    out = {}
    try:
        def one():
            dn.set_point(x0, y0)
            dn.step()

        out["step_ms"] = median_ms(one, reps, warmup)
        if kind != "Symmetric":
            dn.profile(True)
            rec = np.zeros(16)
            _lib.check(dn._lib.pgf_profile_read_ex(dn._hd.h, _lib.dptr(rec), rec.size), dn._hd.h)
            for _ in range(reps):
                one()
            _lib.check(dn._lib.pgf_profile_read_ex(dn._hd.h, _lib.dptr(rec), rec.size), dn._hd.h)
            dn.profile(False)
            launches = max(1.0, rec[15])
            asm_ms = rec[14] / launches
            # H once (n^2; device-resident Standard reads G = J'J beside it), J twice, M written
            gram = n * n if (kind == "Standard" and m) else 0
            nbytes = 8.0 * (float(n) * n + gram + 2.0 * m * n + float(n + m) ** 2)
            out.update(assembly_ms=asm_ms, assembly_launches=int(rec[15]), assembly_bytes=nbytes,
                       assembly_TBps=nbytes / (asm_ms * 1e-3) / 1e12 if asm_ms > 0 else None)
            M = dn.newton_matrix()
            # the LU alone on the same matrix: constructor (upload + factor) + one solve, and the
            # upload of the same bytes measured separately
            rhs = np.ones(n + m)

            def lu():
                sv = pgf.HipLinearSolver(M, symmetric=False)
                sv.solve(rhs)
                sv.close()

            out["lu_upload_factor_solve_ms"] = median_ms(lu, max(5, reps // 4), 1)
            import torch

            t = torch.from_numpy(M)

            def upload():
                t.to("cuda")
                torch.cuda.synchronize()

            out["matrix_upload_ms"] = median_ms(upload, max(5, reps // 4), 1)
            out["lu_factor_solve_ms"] = out["lu_upload_factor_solve_ms"] - out["matrix_upload_ms"]
        else:
            dn.profile(True)
            dn.profile_read()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                one()
                ts.append((time.perf_counter() - t0) * 1e3)
            rec = dn.profile_read()
            dn.profile(False)
            out["profiled_step_ms"] = statistics.median(ts)
            out["factor_ms"] = rec["factor_ms"] / reps
            out["step_outside_factor_ms"] = out["profiled_step_ms"] - out["factor_ms"]
    finally:
        dn.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096x1024,1024x256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=None, help="repetitions of (a); default --reps")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "unsym_device_assembly.json"))
    args = ap.parse_args()
    _lib.require_gpu()
    result = {"reps": args.reps, "warmup": args.warmup, "sizes": {}}
    for size in args.sizes.split(","):
        n, m = (int(v) for v in size.split("x"))
        prob = problems.dense_qp(n, m, seed=0, boxed_frac=0.25)
        rec = {"symmetric": device_newton(prob, "Symmetric", args.reps, args.warmup)}
        for kind in KINDS:
            a_ms, a_stats = plugin_step_ms(prob, kind, True, args.host_reps or args.reps, args.warmup)
            b_ms, b_stats = plugin_step_ms(prob, kind, False, args.reps, args.warmup)
            c = device_newton(prob, kind, args.reps, args.warmup)
            bound = c["lu_factor_solve_ms"] + rec["symmetric"]["step_outside_factor_ms"]
            rec[kind] = {"a_plugin_host_ms": a_ms, "a_bytes_from_host": a_stats[2],
                         "b_plugin_device_ms": b_ms, "b_bytes_from_host": b_stats[2],
                         "c_device_newton_ms": c["step_ms"], "c_bound_ms": bound,
                         "b_faster_than_a": b_ms < a_ms, "c_faster_than_a": c["step_ms"] < a_ms,
                         "c_within_bound": c["step_ms"] <= bound, **c}
            print(size, kind, json.dumps(rec[kind]), flush=True)
        result["sizes"][size] = rec
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
