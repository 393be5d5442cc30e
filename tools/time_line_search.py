#!/usr/bin/env python3
"""Timing of the Globalized policy's device line search (GPU; recorded, not asserted).

For ``dense_qp(4096, 1024)`` (half the variables boxed) and the banded ``box_qp(16384)``, dt = 10,
rho = 1, from x0 = 0: one Globalized step is taken, and the step from the point it reaches is then
measured REPS times (the point is put back before each, outside the timed window):

  globalized   ``DeviceNewton("Globalized").step()``, host clock around a call that ends in a wait
  full         the ``Full`` step of the same handle from the same point
  stage        the line-search stage alone -- the direction's images, k_ls_ladder, k_ls_finish --
               from the event pair around it (``pgf_debug_line_search_ms``), in a pass of its own
               with the handle's profiling events on
  host         the route before this stage existed: ``GlobalizedNewtonMethod`` on the host over
               ``HipStepSolver`` (derivatives resident), one residual round trip per trial

A step whose search fails costs the same launches and is timed like any other; ``trials`` says
what it did.  One JSON line per (workload, route) to profiles/line_search_timing.jsonl: median,
min and max in ms over REPS >= 20 steps after WARMUP.  The host route takes seconds per step on
the dense workload (every trial evaluates g and c on the host, every step assembles the generalised
Jacobian with ``scipy.sparse.bmat``): it stops after HOST_SECONDS of timed steps, and its line
says how many it made (``reps``).

Usage:  python tools/time_line_search.py [--reps 25] [--warmup 5] [--out FILE]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _timed(fn, before, reps, warmup, seconds=None):
    ms = []
    for i in range(warmup + reps):
        before()
        t0 = time.perf_counter()
        fn()
        el = 1e3 * (time.perf_counter() - t0)
        if i >= warmup:
            ms.append(el)
        if seconds is not None:
            print(f"  host step {i}: {el:.1f} ms", flush=True)
            if len(ms) >= 3 and sum(ms) > 1e3 * seconds:
                break
    return ms


OUT = [None]


def _line(workload, route, ms, **extra):
    rec = dict(workload=workload, route=route, reps=len(ms), median_ms=float(np.median(ms)),
               min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), **extra)
    print(json.dumps(rec), flush=True)
    with open(OUT[0], "a") as f:
        f.write(json.dumps(rec) + "\n")
    return rec


def measure(workload, prob, dt, reps, warmup, host_seconds):
    import pygradflow_amd as pgf
    from pygradflow_amd.errors import LineSearchError

    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    dn = pgf.DeviceNewton(prob, "Globalized", x0, y0, dt, 1.0)

    def step():
        try:
            dn.step()
        except LineSearchError:
            pass

    step()
    x1, y1 = dn.point()
    first = dn.line_search()["trials"]

    def back():
        dn.set_point(x1, y1)

    out = []
    dn.kind = "Globalized"
    ms = _timed(step, back, reps, warmup)
    trials = dn.line_search()["trials"]
    out.append(_line(workload, "globalized", ms, trials=trials, first_step_trials=first, n=n, m=m, dt=dt,
                     banded=bool(dn.sparse)))
    dn.kind = "Full"
    out.append(_line(workload, "full", _timed(lambda: dn.step(), back, reps, warmup), n=n, m=m, dt=dt))
    dn.kind = "Globalized"
    dn.profile(2)
    stage = []
    for i in range(warmup + reps):
        back()
        step()
        if i >= warmup:
            stage.append(dn.line_search_ms())
    dn.profile(False)
    out.append(_line(workload, "stage", stage, trials=trials, n=n, m=m, dt=dt))
    dn.close()

    # the host policy over the plug-in step solver, from the same point
    params = pgf.Params(newton_type=pgf.NewtonType.Globalized)
    orig = pgf.Iterate(prob, params, x0, y0)
    method = pgf.newton_method(prob, params, orig, dt, 1.0)
    it1 = pgf.Iterate(prob, params, x1, y1)

    def host_step():
        try:
            method.step(it1)
        except Exception as e:
            if str(e) != "Line search failed to converge":
                raise

    out.append(_line(workload, "host", _timed(host_step, lambda: None, reps, 1, seconds=host_seconds),
                     trials=trials, n=n, m=m, dt=dt))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "line_search_timing.jsonl"))
    ap.add_argument("--host-seconds", type=float, default=60.0)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script)")
    args = ap.parse_args()
    assert args.reps >= 20 or args.small
    from pygradflow_amd import problems

    nd, md, nb = (4096, 1024, 16384) if not args.small else (96, 24, 300)
    dense = problems.dense_qp(nd, md, seed=0, boxed_frac=0.5)
    band = problems.box_qp(nb)
    band.pgf_force_band = True
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    OUT[0] = args.out
    open(args.out, "w").close()
    measure(f"box_qp({nb}) banded", band, 10.0, args.reps, args.warmup, args.host_seconds)
    measure(f"dense_qp({nd}, {md}, boxed_frac=0.5)", dense, 10.0, args.reps, args.warmup, args.host_seconds)


if __name__ == "__main__":
    main()
