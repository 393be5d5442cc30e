#!/usr/bin/env python3
"""Timing of the Globalized policy in the device batch (GPU; recorded, not asserted).

Method of tools/time_line_search.py: medians of REPS steps from the same point after
WARMUP steps, host clock around calls that end in a wait, min and max recorded.  Per workload and
batch size B (64 and 256), dt = 10, rho = 1, from x0 = y0 = 0: one Globalized step is taken and
accepted as the outer point; every measured step starts from that outer point again (a rejected
``advance_outer_each`` puts the instances back, outside the timed window), so each is the first
Newton step of an outer step and a Globalized one includes the evaluation of g, c at the outer
point.

  globalized   ``pgf_batch_step_async`` + ``pgf_batch_sync`` with PGF_STEP_LINE_SEARCH on a batch
               created with ``line_search=True``
  full         the Full step of the same batch from the same point
  sequential   the loop of single handles (``sequential=True, line_search=True``), Globalized

Workloads: ``box_qp(4096)`` band batch, ``multistate_ocp(200, 8, 4)`` wide batch,
``dense_qp(1024, 256, boxed_frac=0.5)`` dense batch (every instance the same problem: the launches do
not depend on the values).  One JSON line per (workload, B, route) to
profiles/batch_line_search_timing.jsonl with the trial counts of the measured step.

Usage:  python tools/time_batch_line_search.py [--reps 25] [--warmup 5] [--sizes 64,256] [--out FILE]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DT, RHO = 10.0, 1.0


def _workloads():
    from pygradflow_amd import problems as P

    band = P.box_qp(4096)
    band.pgf_force_band = True
    wide = P.multistate_ocp(200, 8, 4)
    wide.pgf_force_band = True
    dense = P.dense_qp(1024, 256, seed=1, boxed_frac=0.5)
    return [("box_qp(4096) band", band, dict()), ("multistate_ocp(200,8,4) wide", wide, dict(wide_band=True)),
            ("dense_qp(1024,256,boxed_frac=0.5) dense", dense, dict())]


def _timed(step, back, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        back()
        t0 = time.perf_counter()
        step()
        el = 1e3 * (time.perf_counter() - t0)
        if i >= warmup:
            ms.append(el)
    return ms


def measure(name, prob, kw, B, reps, warmup, out):
    import ctypes as C

    from pygradflow_amd import _lib
    from pygradflow_amd.batched import BatchedDeviceNewton
    from pygradflow_amd.newton import _POLICY_BITS

    lib = _lib.load()
    dts, rhos, rejected = np.full(B, DT), np.full(B, RHO), np.zeros(B, dtype=np.bool_)

    def line(route, ms, **extra):
        rec = dict(workload=name, B=B, route=route, reps=len(ms), median_ms=float(np.median(ms)),
                   min_ms=float(np.min(ms)), max_ms=float(np.max(ms)),
                   steps_per_s=1e3 * B / float(np.median(ms)), **extra)
        print(json.dumps(rec), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    bn = BatchedDeviceNewton(lambda i: prob, B, "Globalized", DT, RHO, line_search=True, **kw)
    try:
        bn.step_local()
        bn.advance_outer()  # the point the first step reached is the outer point of what follows
        status = np.zeros(B, dtype=np.int32)
        ip = C.POINTER(C.c_int)

        def back():
            bn.advance_outer_each(dts, rhos, rejected)

        def step(policy):
            _lib.check(lib.pgf_batch_step_async(bn._b, policy, bn.tau), batch=bn._b)
            _lib.check(lib.pgf_batch_sync(bn._b, status.ctypes.data_as(ip), None, None), batch=bn._b)

        ms = _timed(lambda: step(_POLICY_BITS["Globalized"]), back, reps, warmup)
        ls = bn.line_search()
        launches, waits = bn.line_search_stats()
        line("globalized", ms, trials_min=int(ls["trials"].min()), trials_max=int(ls["trials"].max()),
             failed=int(np.sum(status == _lib.PGF_LINE_SEARCH)), stage_launches=launches, host_waits=waits,
             band_block=bn.band_block)
        ms = _timed(lambda: step(_POLICY_BITS["Full"]), back, reps, warmup)
        line("full", ms)
    finally:
        bn.close()
    sq = BatchedDeviceNewton(lambda i: prob, B, "Globalized", DT, RHO, line_search=True, sequential=True)
    try:
        from pygradflow_amd.errors import LineSearchError

        def loop():  # (the handles' steps alone: no residual norms, which the batch's window has not either)
            for s in sq.solvers:
                try:
                    s.step()
                except LineSearchError:
                    pass

        sq.step_local()
        sq.advance_outer()
        ms = _timed(loop, lambda: sq.advance_outer_each(dts, rhos, rejected), reps, warmup)
        ls = sq.line_search()
        line("sequential", ms, trials_min=int(ls["trials"].min()), trials_max=int(ls["trials"].max()))
    finally:
        sq.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_line_search_timing.jsonl"))
    args = ap.parse_args()
    open(args.out, "w").close()
    for name, prob, kw in _workloads():
        for B in [int(s) for s in args.sizes.split(",")]:
            measure(name, prob, kw, B, args.reps, args.warmup, args.out)


if __name__ == "__main__":
    main()
