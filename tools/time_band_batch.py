"""Banded device batch against the loop over single handles: Newton steps of B banded instances of
one pattern, ``BatchedDeviceNewton`` as a band batch and with ``sequential=True``, alternated in one
session.

    python tools/time_band_batch.py [--steps 200] [--warmup 20] [--reps 7] [--batches 1,8,64,256]
                                    [--workloads sparse_ocp,multistate_ocp,box_qp,budget_box_qp,bordered_lq_k4,
                                                 ocp_gp_w32,...]
                                    [--out FILE]
                                    [--policy Full|Simplified] [--routes batch,sequential]
    python tools/time_band_batch.py --controller [--iterations 20] [--warmup 3] [--reps 5]
                                    [--batches 1,8,64,256] [--workloads sparse_ocp,multistate_ocp_w32]
                                    [--policies Full,Simplified] [--lamb-min 1e-3] [--refine] [--out FILE]

The workloads ``multistate_ocp_w16``, ``_w32``, ``_w64`` are on the wide route (block sizes 16, 32,
64): their batch is created with ``wide_band=True`` and their rows go to
profiles/band_batch_wide_timing.jsonl unless --out says otherwise.  --policy Simplified times the
steps behind the first one of an outer step: the solve phase against kept factors on the wide
route (the batch's lean step).  --routes with one route times that route alone (no ratio line).

The workloads ``budget_box_qp`` (k = 1), ``bordered_lq_k4`` and ``bordered_lq_k64`` are BORDERED bands
on the narrow route: their batch is created with ``border=True`` and their rows go to
profiles/band_batch_border_timing.jsonl unless --out says otherwise.  (``bordered_lq`` with a band
of half-width 3 in H comes out of the plan's ordering with half-bandwidth 9, the wide route, which
a bordered batch refuses: the two workloads have half-width 2, half-bandwidth 6.)  Under Simplified
every step behind the first runs the solve phase alone, without a factor-phase launch.

The workloads ``ocp_gp_w16``, ``_w32``, ``_w64`` (``ocp_global_parameter`` with three global
parameters and the automatic border: k = 3 on block sizes 16, 32, 64) and ``bordered_lq_w16``
(``bordered_lq(3000, 3, 1000, 2, 2)``: k = 4, half-bandwidth 9, block size 16) are BORDERED bands on
the WIDE route: their batch is created with ``wide_border=True`` and their rows go to
profiles/band_batch_wide_border_timing.jsonl unless --out says otherwise.

A step is ``step_local()``: the Newton step of every instance, its host synchronisation and the
residual norms of the new points -- what a controller pays per step on either route.  One JSON line
per (workload, B, route) with the median, minimum and maximum over the repetitions of the time per
step and the instance-steps per second at the median, appended to --out (default
profiles/band_batch_timing.jsonl) and printed; after both routes of a (workload, B) a line
``"route": "ratio"`` with sequential / batch and whether the batch's median lies below the
sequential one by more than both spreads (max - min) together.

--controller times the step controller that drives such a batch instead: one outer iteration (two
Newton steps and the controller's decisions) of the host-driven ``BatchedDistanceRatioController``
on a band batch against ``DeviceResidentDistanceRatioController`` on its twin created with
``band_ctl=True``, alternated in one session.  A repetition is ``--iterations`` outer iterations: on
the host route that many ``step()`` calls (three host synchronisations each), on the device route one
``run(iterations)`` -- one ``ctl_iterate`` and one ``ctl_read``.  One JSON line per (workload,
policy, B, route) with the median, minimum and maximum time per outer iteration, appended to --out
(default profiles/band_batch_ctl_timing.jsonl); the ratio line also says whether the accept flags
of all iterations were equal on both routes and the largest relative difference of lambda.
--lamb-min is the controller's floor for lambda (``Params.lamb_min``; the library's default is 1e-12).
These workloads converge after one Newton step in most iterations, so lambda halves until it reaches
the floor; left to the default it falls to where the accuracy guard fires (from about 1e-6), and
then the host route repairs instances on their handles where the device route rejects the step: the
two routes no longer do the same work, which the ratio line shows (``host_repaired``,
``device_guard_rejects``, ``accept_flags_equal``).

--controller takes the bordered workloads too (narrow and wide): the device route's batch is then
created with ``border_ctl=True`` beside the route's own flags, and the rows go to
profiles/band_batch_ctl_border_timing.jsonl unless --out says otherwise.  --refine adds a third
route, ``device_refine``: a second device-resident twin created with ``ctl_refine=True``, which
refines an instance above ``refine_tol`` inside the loop as the host route repairs it on its handle.
Its row carries the refined steps and rounds; the ratio line has ``refine_over_device`` (the price
of the two rounds of launches per step when nothing refines, what the flag buys when the plain
device route rejects), whether its accept flags equal the host route's and its largest relative
difference of lambda from the host route.  Rows go to profiles/band_batch_ctl_refine_timing.jsonl.
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
    # bordered bands on the narrow route: k = 1, 4, 64 border nodes
    "budget_box_qp": ("budget_box_qp(4096)", lambda i: _bordered(problems.budget_box_qp(4096, seed=i))),  # N = 4097
    "bordered_lq_k4": ("bordered_lq(3000, 2, 1000, 2, 2)", lambda i: _bordered_lq(3000, 2, 1000, 2, 2, i)),  # N = 4004
    "bordered_lq_k64": ("bordered_lq(3000, 2, 1000, 32, 32)", lambda i: _bordered_lq(3000, 2, 1000, 32, 32, i)),  # N = 4064
    # bordered bands on the wide route: k = 3 global parameters on blocks 16, 32, 64; k = 4 on block 16
    "ocp_gp_w16": ("ocp_global_parameter(200, 4, 2, 3)",
                   lambda i: _bordered(problems.ocp_global_parameter(200, 4, 2, 3, seed=i))),  # N = 2003
    "ocp_gp_w32": ("ocp_global_parameter(200, 8, 4, 3)",
                   lambda i: _bordered(problems.ocp_global_parameter(200, 8, 4, 3, seed=i))),  # N = 4003
    "ocp_gp_w64": ("ocp_global_parameter(100, 16, 8, 3)",
                   lambda i: _bordered(problems.ocp_global_parameter(100, 16, 8, 3, seed=i))),  # N = 4003
    "bordered_lq_w16": ("bordered_lq(3000, 3, 1000, 2, 2)", lambda i: _bordered_lq(3000, 3, 1000, 2, 2, i)),  # N = 4004
}
WIDE = ("multistate_ocp_w16", "multistate_ocp_w32", "multistate_ocp_w64")
BORDERED = ("budget_box_qp", "bordered_lq_k4", "bordered_lq_k64")
WIDE_BORDERED = ("ocp_gp_w16", "ocp_gp_w32", "ocp_gp_w64", "bordered_lq_w16")


def _bordered(prob):
    prob.pgf_border = "auto"
    return prob


def _bordered_lq(n0, bw, mloc, kv, kc, seed):
    from tests.band_util import bordered_lq  # (the generator the bordered tests share)

    return bordered_lq(n0, bw, mloc, kv, kc, seed)


def timed(run, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        status, _, _ = run.step_local()  # (ends in the step's host synchronisation)
    dt = (time.perf_counter() - t0) / steps
    assert not status.any(), status
    return dt


def controller_rows(a, emit):
    """--controller: see the module docstring."""
    from pygradflow_amd import step_control as SC
    from pygradflow_amd.params import Params

    total = a.warmup + a.reps * a.iterations
    for key in a.workloads.split(","):
        name, make = WORKLOADS[key]
        probs = []
        for pol in a.policies.split(","):
            for B in [int(v) for v in a.batches.split(",")]:
                while len(probs) < B:
                    p = make(len(probs))
                    p.pgf_force_band = True
                    probs.append(p)
                par = Params(newton_type=pol, lamb_init=1.0, lamb_min=a.lamb_min)
                bordered = key in BORDERED + WIDE_BORDERED
                route_flags = dict(wide_band=key in WIDE, border=key in BORDERED, wide_border=key in WIDE_BORDERED)
                host_b, dev_b = (BatchedDeviceNewton(lambda i: probs[i], B, pol, 1.0, 1.0, band_ctl=ctl,
                                                     border_ctl=ctl and bordered, **route_flags)
                                 for ctl in (False, True))
                assert host_b.band and dev_b.band and (dev_b.band_border > 0) == bordered
                host = SC.BatchedDistanceRatioController(host_b, par, rho=1.0)
                dev = SC.DeviceResidentDistanceRatioController(dev_b, par, rho=1.0, max_iterations=total)
                ref_b = ref = None
                if a.refine:
                    ref_b = BatchedDeviceNewton(lambda i: probs[i], B, pol, 1.0, 1.0, band_ctl=True,
                                                border_ctl=bordered, ctl_refine=True, **route_flags)
                    ref = SC.DeviceResidentDistanceRatioController(ref_b, par, rho=1.0, max_iterations=total)
                rec = []

                def host_iters(k):
                    t0 = time.perf_counter()
                    for _ in range(k):
                        rec.append(host.step())
                    return (time.perf_counter() - t0) / k

                def dev_iters(k):
                    t0 = time.perf_counter()
                    dev.run(k)  # (ends in ctl_read: the one host synchronisation)
                    return (time.perf_counter() - t0) / k

                def ref_iters(k):
                    t0 = time.perf_counter()
                    ref.run(k)
                    return (time.perf_counter() - t0) / k

                routes = {"host_driven": host_iters, "device_resident": dev_iters}
                if a.refine:
                    routes["device_refine"] = ref_iters
                for run in routes.values():
                    run(a.warmup)
                times = {r: [] for r in routes}
                for _ in range(a.reps):  # alternated: other people's work shares the host
                    for r, run in routes.items():
                        times[r].append(run(a.iterations))
                used = np.array([r[0] for r in rec])
                nxt = np.array([r[1] for r in rec])
                acc = np.array([r[2] for r in rec])
                h = dev.history
                flags_equal = bool(np.array_equal(h[:, :, 2] != 0.0, acc))
                lamb_diff = float(max(np.max(np.abs(h[:, :, 0] - used) / used), np.max(np.abs(h[:, :, 1] - nxt) / nxt)))
                piv, grd = dev_b.ctl_stats()
                N = probs[0].num_vars + probs[0].num_cons
                rows = {}
                for r, ts in times.items():
                    med = statistics.median(ts)
                    rows[r] = {"workload": name, "N": N, "B": B, "route": r, "policy": pol, "lamb_min": a.lamb_min,
                               "iterations": a.iterations, "warmup": a.warmup, "reps": a.reps,
                               "median_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}
                    if r == "device_refine":
                        steps, rounds = ref_b.ctl_refine_stats()
                        rows[r].update(refined_steps=int(steps.sum()), rounds=int(rounds.sum()),
                                       guard_rejects=int(ref_b.ctl_stats()[1].sum()))
                    emit(rows[r])
                d, s = rows["device_resident"], rows["host_driven"]
                spreads = (d["max_ms"] - d["min_ms"]) + (s["max_ms"] - s["min_ms"])
                extra = {}
                if a.refine:
                    f, hr = rows["device_refine"], ref.history
                    both = (d["max_ms"] - d["min_ms"]) + (f["max_ms"] - f["min_ms"])
                    extra = {"refine_over_device": f["median_ms"] / d["median_ms"],
                             "refine_differs_from_device_by_more_than_both_spreads":
                                 bool(abs(f["median_ms"] - d["median_ms"]) > both),
                             "host_over_refine": s["median_ms"] / f["median_ms"],
                             "refine_accept_flags_equal": bool(np.array_equal(hr[:, :, 2] != 0.0, acc)),
                             "refine_max_rel_lambda_diff": float(max(np.max(np.abs(hr[:, :, 0] - used) / used),
                                                                     np.max(np.abs(hr[:, :, 1] - nxt) / nxt)))}
                emit({"workload": name, "N": N, "B": B, "route": "ratio", "policy": pol, **extra,
                      "host_over_device": s["median_ms"] / d["median_ms"],
                      "device_below_host_by_more_than_both_spreads": bool(s["median_ms"] - d["median_ms"] > spreads),
                      "accept_flags_equal": flags_equal, "max_rel_lambda_diff": lamb_diff,
                      "accepted_share": float(acc.mean()), "host_repaired": host_b.repaired(),
                      "device_pivot_rejects": int(piv.sum()), "device_guard_rejects": int(grd.sum())})
                host_b.close()
                dev_b.close()
                if ref_b is not None:
                    ref_b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--controller", action="store_true")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--policies", default="Full,Simplified")
    ap.add_argument("--lamb-min", type=float, default=1e-3)
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--workloads", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--policy", default="Full", choices=("Full", "Simplified"))
    ap.add_argument("--routes", default="batch,sequential")
    a = ap.parse_args()
    if a.warmup is None:
        a.warmup = 3 if a.controller else 20
    if a.reps is None:
        a.reps = 5 if a.controller else 7
    if a.workloads is None:
        a.workloads = "sparse_ocp,multistate_ocp_w32" if a.controller else "sparse_ocp,multistate_ocp,box_qp"
    batches = [int(v) for v in a.batches.split(",")]
    keys = a.workloads.split(",")
    routes = a.routes.split(",")
    assert routes and set(routes) <= {"batch", "sequential"}, routes
    if a.out is None:
        name = "band_batch_wide_timing.jsonl" if all(k in WIDE for k in keys) else "band_batch_timing.jsonl"
        if all(k in BORDERED for k in keys):
            name = "band_batch_border_timing.jsonl"
        if all(k in WIDE_BORDERED for k in keys):
            name = "band_batch_wide_border_timing.jsonl"
        if a.controller:
            name = "band_batch_ctl_timing.jsonl"
            if all(k in BORDERED + WIDE_BORDERED for k in keys):
                name = "band_batch_ctl_border_timing.jsonl"
            if a.refine:
                name = "band_batch_ctl_refine_timing.jsonl"
        a.out = os.path.join(REPO, "profiles", name)
    out = open(a.out, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    if a.controller:
        controller_rows(a, emit)
        out.close()
        return
    for key in keys:
        name, make = WORKLOADS[key]
        probs = []
        for B in batches:
            while len(probs) < B:
                p = make(len(probs))
                p.pgf_force_band = True
                probs.append(p)
            runs = {r: BatchedDeviceNewton(lambda i: probs[i], B, a.policy, 1.0, 1.0, sequential=(r == "sequential"),
                                           wide_band=key in WIDE, border=key in BORDERED,
                                           wide_border=key in WIDE_BORDERED) for r in routes}
            assert "batch" not in runs or runs["batch"].band
            assert "batch" not in runs or (runs["batch"].band_border > 0) == (key in BORDERED + WIDE_BORDERED)
            assert "batch" not in runs or key not in WIDE_BORDERED or runs["batch"].band_block > 8
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
