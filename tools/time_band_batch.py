"""Banded device batch against the loop over single handles: Newton steps of B banded instances of
one pattern, ``BatchedDeviceNewton`` as a band batch and with ``sequential=True``, alternated in one
session.

    python tools/time_band_batch.py [--steps 200] [--warmup 20] [--reps 7] [--batches 1,8,64,256]
                                    [--workloads sparse_ocp,multistate_ocp,box_qp] [--out FILE]
                                    [--policy Full|Simplified] [--routes batch,sequential]

The workloads ``multistate_ocp_w16``, ``_w32``, ``_w64`` are on the wide route (block sizes 16, 32,
64): their batch is created with ``wide_band=True`` and their rows go to
profiles/band_batch_wide_timing.jsonl unless --out says otherwise.  --policy Simplified times the
steps behind the first one of an outer step: the solve phase against kept factors on the wide
route (the batch's lean step).  --routes with one route times that route alone (no ratio line).

A step is ``step_local()``: the Newton step of every instance, its host synchronisation and the
residual norms of the new points -- what a controller pays per step on either route.  One JSON line
per (workload, B, route) with the median, minimum and maximum over the repetitions of the time per
step and the instance-steps per second at the median, appended to --out (default
profiles/band_batch_timing.jsonl) and printed; after both routes of a (workload, B) a line
``"route": "ratio"`` with sequential / batch and whether the batch's median lies below the
sequential one by more than both spreads (max - min) together.
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
from pygradflow_amd import problems  # noqa: E402
from pygradflow_amd.batched import BatchedDeviceNewton  # noqa: E402

WORKLOADS = {
    "sparse_ocp": ("sparse_ocp(1000)", lambda i: problems.sparse_ocp(1000, seed=i)),  # N = 3000
    "multistate_ocp": ("multistate_ocp(200, 3, 1)", lambda i: problems.multistate_ocp(200, 3, 1, seed=i)),
    "box_qp": ("box_qp(4096)", lambda i: problems.box_qp(4096, seed=i)),
    # the wide route: half-bandwidths 10, 22, 46 -> block sizes 16, 32, 64
    "multistate_ocp_w16": ("multistate_ocp(200, 4, 2)", lambda i: problems.multistate_ocp(200, 4, 2, seed=i)),  # N = 2000
    "multistate_ocp_w32": ("multistate_ocp(200, 8, 4)", lambda i: problems.multistate_ocp(200, 8, 4, seed=i)),  # N = 4000
    "multistate_ocp_w64": ("multistate_ocp(100, 16, 8)", lambda i: problems.multistate_ocp(100, 16, 8, seed=i)),  # N = 4000
}
WIDE = ("multistate_ocp_w16", "multistate_ocp_w32", "multistate_ocp_w64")


def timed(run, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        status, _, _ = run.step_local()  # (ends in the step's host synchronisation)
    dt = (time.perf_counter() - t0) / steps
    assert not status.any(), status
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--workloads", default="sparse_ocp,multistate_ocp,box_qp")
    ap.add_argument("--out", default=None)
    ap.add_argument("--policy", default="Full", choices=("Full", "Simplified"))
    ap.add_argument("--routes", default="batch,sequential")
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",")]
    keys = a.workloads.split(",")
    routes = a.routes.split(",")
    assert routes and set(routes) <= {"batch", "sequential"}, routes
    if a.out is None:
        name = "band_batch_wide_timing.jsonl" if all(k in WIDE for k in keys) else "band_batch_timing.jsonl"
        a.out = os.path.join(REPO, "profiles", name)
    out = open(a.out, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for key in keys:
        name, make = WORKLOADS[key]
        probs = []
        for B in batches:
            while len(probs) < B:
                p = make(len(probs))
                p.pgf_force_band = True
                probs.append(p)
            runs = {r: BatchedDeviceNewton(lambda i: probs[i], B, a.policy, 1.0, 1.0, sequential=(r == "sequential"),
                                           wide_band=key in WIDE) for r in routes}
            assert "batch" not in runs or runs["batch"].band
            N = probs[0].num_vars + probs[0].num_cons
            for run in runs.values():
                timed(run, a.warmup)
            # both routes have taken the same steps: the same points, or the comparison is void
            same = None
            if len(runs) == 2:
                xb, yb = runs["batch"].points()
                xs, ys = runs["sequential"].points()
                same = bool(np.array_equal(xb, xs) and np.array_equal(yb, ys))
            times = {r: [] for r in runs}
            for _ in range(a.reps):  # alternated: other people's work shares the host
                for r, run in runs.items():
                    times[r].append(timed(run, a.steps))
            rows = {}
            for r, ts in times.items():
                med = statistics.median(ts)
                rows[r] = {"workload": name, "N": N, "B": B, "route": r, "policy": a.policy, "steps": a.steps,
                           "reps": a.reps,
                           "median_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts),
                           "instance_steps_per_s": B / med, "points_bit_identical": same}
                emit(rows[r])
            if len(rows) == 2:
                b, s = rows["batch"], rows["sequential"]
                spreads = (b["max_ms"] - b["min_ms"]) + (s["max_ms"] - s["min_ms"])
                emit({"workload": name, "N": N, "B": B, "route": "ratio", "policy": a.policy,
                      "sequential_over_batch": s["median_ms"] / b["median_ms"],
                      "batch_below_sequential_by_more_than_both_spreads":
                          bool(s["median_ms"] - b["median_ms"] > spreads)})
            for run in runs.values():
                run.close()
    out.close()


if __name__ == "__main__":
    main()
