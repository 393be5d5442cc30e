"""Times the bordered-band route (csrc/pgf_border.hip) on one MI355X, one process, DeviceNewton
steps from zero (median of --reps after --warmup warm-ups, the convention of SURVEY.md 8d):

  budget_box_qp(16 384)                 bordered route (pgf_border = "auto"), Full and Simplified
  the same problem                      dense route (no pgf_border: what the code did before), Full and Simplified
  budget_box_qp(100 000)                bordered route (no dense matrix of that size exists)
  ocp_global_parameter(5000, 8, 4, 4)   bordered route, wide remainder (B = 32)
  bordered_lq(20 000, bw 12, k = 16)    bordered route, wide remainder (B = 16), the tests' generator
                                        (--wide-only: the two wide remainders alone)

On a wide remainder Y = inv(B) C is one panel solve against the kept factors of one reduction of B
(factor / solve split of pgf_band_wide.hip on), or k whole reductions (split off).

Per workload: wall time of a step (each step waits for the device once, so this is device time plus
the launch overhead), and from HIP events (pgf_profile_read_ex) the device time of the factor
phase (Y = inv(B) C, C'Y, L D L' of S: ``factor_ms``) and of the solve phase (one banded reduction
plus the border kernels and the residual: ``solve_ms``).  For the 8 x 8 routes the algorithmic
bytes of the multi-right-hand-side reduction are set against the factor phase's device time: a
lower bound on its bandwidth, since the span also holds the C'Y product and the factor of S.
The first Full step of every bordered workload is compared with the CPU reference implementation
of the step (tests' oracle) unless --no-check.

Writes one JSON line per workload to profiles/border_band_timing.jsonl (or --out).

    timeout -k 10 900 python tools/time_border.py [--reps 20] [--warmup 3]
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


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def panel_bytes(Nb, kp):
    """Algorithmic bytes of the multi-right-hand-side reduction: per block of 8 rows the extraction
    (D, L, U and the 8 x kp panel written), one level as a kept block (its own and both neighbours'
    D, L, U and panels read, its own and one inverse written) and one back-substitution (inverse,
    L, U and three panels read, one written)."""
    nb = (Nb + 7) // 8
    blk, pan = 3 * 512, 64 * kp
    return nb * ((blk + pan) + (4 * (blk + pan) + 512) + (blk + 4 * pan))


def agreement(prob):
    """Largest relative deviation of x, y of one Full step from the CPU reference step."""
    from oracle import newton_oracle as O

    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    rec = O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, 1)[0]
    dn = pgf.DeviceNewton(prob, "Full", x0, y0, 1.0, 1.0)
    dn.step()
    x, y = dn.point()
    same = bool(np.array_equal(dn.mask(), rec["mask"]))
    dn.close()
    rel = lambda a, b: float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))  # noqa: E731
    return {"mask_identical": same, "x_rel": rel(x, rec["xn"]), "y_rel": rel(y, rec["yn"]),
            "active": int(np.count_nonzero(rec["mask"]))}


def time_policy(prob, policy, reps, warmup, profile):
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    dn = pgf.DeviceNewton(prob, policy, x0, y0, 1.0, 1.0)
    out = {}
    try:
        def one():
            dn.set_point(x0, y0)
            dn.step()

        out["step_ms"] = median_ms(one, reps, warmup)
        if profile:
            dn.profile(True)
            dn.profile_read()
            before = dn.border_stats()
            for _ in range(reps):
                one()
            rec = dn.profile_read()
            after = dn.border_stats()
            dn.profile(False)
            out["factor_ms"] = rec["factor_ms"] / reps
            out["solve_ms"] = rec["update_ms"] / reps
            out["factor_phases_per_step"] = (after[1] - before[1]) / reps
            out["solve_phases_per_step"] = (after[2] - before[2]) / reps
    finally:
        dn.close()
    return out


def workload(name, prob, bordered, reps, warmup, check):
    n, m = prob.num_vars, prob.num_cons
    rec = {"workload": name, "n": n, "m": m, "route": "bordered" if bordered else "dense"}
    if bordered:
        if getattr(prob, "pgf_border", None) is None:
            prob.pgf_border = "auto"
        dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
        plan = dn._hd.plan
        panels = 0
        if hasattr(dn, "band_stats"):  # wide remainder: did the factor phase run a panel solve?
            before = dn.band_stats()[2]
            dn.step()
            panels = dn.band_stats()[2] - before
        dn.close()
        y_route = "repeated solves"
        if plan.block_size == 8 and os.environ.get("PGF_BORDER_MULTI") != "0":
            y_route = "multi-rhs reduction"
        elif panels:
            y_route = "panel solve against kept factors"
        rec.update(k=plan.k, kp=plan.kp, Nb=plan.Nb, bw=plan.bw, block=plan.block_size, y_route=y_route)
        if check:
            rec["reference_agreement"] = agreement(prob)
    for pol in ("Full", "Simplified"):
        rec[pol] = time_policy(prob, pol, reps, warmup, profile=bordered)
    if bordered and rec["y_route"] == "multi-rhs reduction" and rec["Full"]["factor_ms"] > 0:
        nbytes = panel_bytes(plan.Nb, plan.kp)
        rec["panel_reduction_bytes"] = nbytes
        rec["panel_reduction_TBps_lower_bound"] = nbytes / (rec["Full"]["factor_ms"] * 1e-3) / 1e12
    rec["simplified_cheaper_than_full"] = rec["Simplified"]["step_ms"] < rec["Full"]["step_ms"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dense-reps", type=int, default=5, help="repetitions of the dense route (about 10 ms a step)")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--wide-only", action="store_true", help="only the wide-remainder workloads")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "border_band_timing.jsonl"))
    args = ap.parse_args()
    _lib.require_gpu()
    recs = []

    def wide():
        from tests.band_util import bordered_lq

        recs.append(workload("ocp_global_parameter(5000,8,4,4)", problems.ocp_global_parameter(5000, 8, 4, 4),
                             True, args.reps, args.warmup, not args.no_check))
        recs.append(workload("bordered_lq(20000,bw=12,k=16,B=16)", bordered_lq(20000, 12, 0, 8, 8, 1, block=16),
                             True, args.reps, args.warmup, not args.no_check))

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in recs:
                f.write(json.dumps(rec, sort_keys=True) + "\n")
        print(json.dumps({"written": args.out}))

    if args.wide_only:
        wide()
        return write()
    a = workload("budget_box_qp(16384)", problems.budget_box_qp(16384), True, args.reps, args.warmup,
                 not args.no_check)
    recs.append(a)
    b = workload("budget_box_qp(16384)", problems.budget_box_qp(16384), False, args.dense_reps, 1, False)
    b["bordered_full_faster_than_dense_full"] = a["Full"]["step_ms"] < b["Full"]["step_ms"]
    b["dense_over_bordered_full"] = b["Full"]["step_ms"] / a["Full"]["step_ms"]
    recs.append(b)
    recs.append(workload("budget_box_qp(100000)", problems.budget_box_qp(100000), True, args.reps, args.warmup,
                         not args.no_check))
    wide()
    write()


if __name__ == "__main__":
    main()
