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

--large: the large border (csrc/pgf_border_large.hip, ``pgf_border_limit``) instead, into
profiles/border_large_timing.jsonl:

  bordered_lq(20 000, bw 12) with k = 128, 512, 1024   explicit border, block 16
  multistate_ocp(300, 24, 8)                           automatic border (k = 299)

each on the large-border route and, the same problem without ``pgf_border``, on the dense route
(what the code did with it before the large border existed; n + m <= 60 000): step time (median and
quartiles), device time of the phases, the ratio dense / large border, and the Gram launch alone
(``pgf_debug_border_gram_time``) in TF at 2 Nb kp^2 / 2 useful flops.  One more row sets the MFMA
Gram kernel against the small border's FMA kernel on the same C and Y at kp = 64.

    timeout -k 10 900 python tools/time_border.py --large [--reps 20] [--dense-reps 3]
    timeout -k 10 600 python tools/time_border.py --large --only k1024   # one workload, appended
"""

import argparse
import ctypes as C
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
from pygradflow_amd.step_solver import DENSE_LIMIT  # noqa: E402


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def spread_ms(fn, reps, warmup):
    """(median, lower quartile, upper quartile, min) of the wall time of fn in ms."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    q = statistics.quantiles(ts, n=4) if len(ts) >= 4 else [min(ts), statistics.median(ts), max(ts)]
    return {"median": statistics.median(ts), "q1": q[0], "q3": q[2], "min": min(ts), "reps": len(ts)}


def gram_time(dn, launches=200, samples=7):
    """Per launch of the MFMA Gram kernel and of the FMA kernel (None beyond kp = 64) on the handle's
    last factor phase: ``samples`` windows of ``launches`` back-to-back launches each (a window of
    milliseconds, not of a few launches), as {"median", "min", "max"} of the windows' means in ms.
    The operands are the same C and Y every launch: whatever of their 16 Nb kp bytes fits stays in
    L2 / Infinity Cache, so these are warm-cache figures, not what the first launch of a factor
    phase sees."""
    ms = {"mfma": [], "fma": []}
    for _ in range(samples):
        a, b = C.c_double(0.0), C.c_double(0.0)
        _lib.check(dn._lib.pgf_debug_border_gram_time(dn._hd.h, launches, C.byref(a), C.byref(b)), dn._hd.h,
                   "pgf_debug_border_gram_time")
        ms["mfma"].append(a.value)
        if b.value >= 0:
            ms["fma"].append(b.value)
    spread = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v),  # noqa: E731
                        "launches_per_window": launches, "windows": len(v)} if v else None
    return spread(ms["mfma"]), spread(ms["fma"])


def strip_border(prob):
    """The same problem without border settings: the dense route while n + m <= 60 000."""
    return problems.LinearQuadraticProblem(prob.hess_sparse(), prob.q, prob.jac_sparse(), prob.b, prob.var_lb,
                                           prob.var_ub)


def large_workload(name, prob, reps, warmup, dense_reps, check):
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    prob.pgf_border_limit = 1024
    rec = {"workload": name, "n": n, "m": m}
    if check:
        rec["reference_agreement"] = agreement(prob)
    first = None
    for pol in ("Full", "Simplified"):
        dn = pgf.DeviceNewton(prob, pol, x0, y0, 1.0, 1.0)
        plan = dn._hd.plan
        rec.update(k=plan.k, kp=plan.kp, Nb=plan.Nb, bw=plan.bw, block=plan.block_size)
        if first is None:
            dn.step()
            first = dn.point()

        def one():
            dn.set_point(x0, y0)
            dn.step()

        out = {"step_ms": spread_ms(one, reps, warmup)}
        dn.profile(True)
        dn.profile_read()
        for _ in range(reps):
            one()
        pr = dn.profile_read()
        dn.profile(False)
        out["factor_ms"] = pr["factor_ms"] / reps
        out["solve_ms"] = pr["update_ms"] / reps
        if pol == "Full":
            ms, _ = gram_time(dn)
            flops = 2.0 * plan.Nb * plan.kp * plan.kp / 2.0
            rec["gram"] = {"ms": ms, "useful_flops": flops, "TF": flops / (ms["median"] * 1e-3) / 1e12,
                           "operand_bytes": 16.0 * plan.Nb * plan.kp, "cache": "warm (same C, Y every launch)"}
        dn.close()
        rec[pol] = out
    rel = lambda a, b: float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))  # noqa: E731
    dense = strip_border(prob)
    if n + m <= DENSE_LIMIT:  # the device-resident step on the dense route
        dn = pgf.DeviceNewton(dense, "Full", x0, y0, 1.0, 1.0)
        assert not dn.sparse

        def one_dense():
            dn.set_point(x0, y0)
            dn.step()

        dn.step()  # the two routes against each other: one Full step from zero
        xd, yd = dn.point()
        rec["dense_route"] = "DeviceNewton"
        rec["dense_Full_step_ms"] = spread_ms(one_dense, dense_reps, 1)
        dn.close()
        ours = rec["Full"]["step_ms"]["median"]
    else:
        # above DENSE_LIMIT DeviceNewton refuses a pattern without a band; what took such a problem
        # before is the plug-in step solver, which leaves the banded path for the dense one -- timed
        # against the large border through the same front end
        def plugin(p):
            params = pgf.Params(newton_type="Full", step_solver=pgf.HipStepSolver)
            curr = pgf.Iterate(p, params, x0, y0)
            method = pgf.newton_method(p, params, pgf.Iterate(p, params, x0, y0), 1.0, 1.0)
            step = method.step(curr)
            # a Full step repeated from one point keeps its factorisation (same mask, same
            # derivatives): the timed steps alternate between two points whose active sets differ,
            # so that every one of them factorises
            pts = [curr, step.iterate]
            changes = not np.array_equal(step.active_set, method.step(pts[1]).active_set)
            turn = [0]

            def one():
                method.step(pts[turn[0] % 2])
                turn[0] += 1

            ms = spread_ms(one, 2 * dense_reps, 2)
            ms["mask_changes_between_the_two_points"] = bool(changes)
            return step.iterate.x, step.iterate.y, ms, bool(method.step_solver.sparse)

        xd, yd, rec["dense_Full_step_ms"], was_sparse = plugin(dense)
        assert not was_sparse
        _, _, rec["plugin_Full_step_ms"], was_sparse = plugin(prob)
        assert was_sparse
        rec["dense_route"] = "HipStepSolver (plug-in step; the large border through it: plugin_Full_step_ms)"
        ours = rec["plugin_Full_step_ms"]["median"]
    rec["agreement_with_dense_route"] = {"x_rel": rel(first[0], xd), "y_rel": rel(first[1], yd)}
    rec["dense_over_large_border_full"] = rec["dense_Full_step_ms"]["median"] / ours
    print(json.dumps(rec), flush=True)
    return rec


def gram_kp64_row(reps):
    """The MFMA Gram kernel against k_border_gram on the same C and Y at kp = 64 (a small border
    of 64 nodes on block 16: production runs the FMA kernel there)."""
    from tests.band_util import bordered_lq

    prob = bordered_lq(20000, 12, 0, 21, 43, 1, block=16)
    n, m = prob.num_vars, prob.num_cons
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    dn.step()
    plan = dn._hd.plan
    mfma, fma = gram_time(dn)
    dn.close()
    flops = 2.0 * plan.Nb * plan.kp * plan.kp / 2.0
    rec = {"workload": "gram kernels at kp=64, bordered_lq(20000,bw=12,k=64,B=16)", "Nb": plan.Nb, "kp": plan.kp,
           "mfma_ms": mfma, "fma_ms": fma, "mfma_TF_useful": flops / (mfma["median"] * 1e-3) / 1e12,
           "fma_TF_useful": flops / (fma["median"] * 1e-3) / 1e12, "mfma_faster": mfma["median"] < fma["median"],
           "operand_bytes": 16.0 * plan.Nb * plan.kp, "cache": "warm (same C, Y every launch)"}
    print(json.dumps(rec), flush=True)
    return rec


LARGE_WORKLOADS = ("gram64", "multistate", "k128", "k512", "k1024")


def main_large(args):
    """--only NAME runs one workload and APPENDS its line (one process, one time limit per workload:
    the host work -- the problem, its plan, the dense matrix of the comparison -- grows with k)."""
    from tests.band_util import bordered_lq

    out = args.out if args.out_given else os.path.join(REPO, "profiles", "border_large_timing.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not args.only:
        open(out, "w").close()

    def keep(rec):  # (a line per workload as it finishes)
        with open(out, "a") as f:
            f.write(json.dumps(rec, sort_keys=True) + "\n")

    for name in ([args.only] if args.only else LARGE_WORKLOADS):
        if name == "gram64":
            keep(gram_kp64_row(args.reps))
        elif name == "multistate":
            prob = problems.multistate_ocp(300, 24, 8)
            prob.pgf_border = "auto"
            keep(large_workload("multistate_ocp(300,24,8) auto", prob, args.reps, args.warmup, args.dense_reps,
                                not args.no_check))
        else:
            k = int(name[1:])
            kv = k // 3
            prob = bordered_lq(20000, 12, 0, kv, k - kv, 1, block=16)
            # (the CPU reference step is checked where it takes seconds; every workload is compared
            # with the dense route on the device)
            keep(large_workload(f"bordered_lq(20000,bw=12,k={k},B=16)", prob, args.reps, args.warmup,
                                args.dense_reps, not args.no_check and k <= 128))
    print(json.dumps({"written": out}))


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
    ap.add_argument("--large", action="store_true", help="the large border's workloads (see above)")
    ap.add_argument("--only", choices=LARGE_WORKLOADS, default=None,
                    help="with --large: one workload, its line appended to --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out_given = args.out is not None
    if not args.out_given:
        args.out = os.path.join(REPO, "profiles", "border_band_timing.jsonl")
    _lib.require_gpu()
    if args.large:
        return main_large(args)
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
