"""Banded path with wide blocks (B = 16, 32, 64; csrc/pgf_band_wide.hip): Full steps/s and the
Simplified back-solve step of DeviceNewton, the dense path on the same problem where it fits
(H and J handed over as dense arrays), and the CPU oracle's time per step beside each.

    python tools/time_wide_band.py [--steps K] [--quick] [--narrow] [--split 0|1]

--narrow: the bw 9 .. 10 problems instead (automatic block size: B = 16).
--split:  the factor / solve split of the wide reduction off / on (``problem.pgf_band_split``;
          not given: the library's default, on unless PGF_BW_SPLIT=0); recorded in every row.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import newton_oracle as O  # noqa: E402
from pygradflow_amd import problems  # noqa: E402
from pygradflow_amd.newton import DeviceNewton  # noqa: E402
from pygradflow_amd.sparse import BandPlan  # noqa: E402


def device_times(prob, steps):
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    out = {}
    for pol in ("Full", "Simplified"):
        dn = DeviceNewton(prob, pol, x0, y0, 1.0, 1.0)
        dn.step()  # warm-up (Simplified: the step that factors)
        t0 = time.perf_counter()
        for _ in range(steps):
            dn.step()
        out[pol] = (time.perf_counter() - t0) / steps
        out["sparse"] = dn.sparse
        dn.close()
    return out


def oracle_time(prob, steps=2):
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    t0 = time.perf_counter()
    O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, steps)
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="skip the oracle and the dense comparison")
    ap.add_argument("--narrow", action="store_true", help="the bw 9 .. 10 cases (implies --quick)")
    ap.add_argument("--split", type=int, choices=(0, 1), default=None,
                    help="factor / solve split of the wide reduction (default: the library's)")
    a = ap.parse_args()
    cases = [
        ("grid_box_qp(9, 320)", problems.grid_box_qp(9, 320), False),
        ("multistate_ocp(400, 4, 2)", problems.multistate_ocp(400, 4, 2), False),
        ("grid_box_qp(9, 11000)", problems.grid_box_qp(9, 11000), False),
        ("grid_box_qp(10, 10000)", problems.grid_box_qp(10, 10000), False),  # bw 11: B = 16 either way
    ] if a.narrow else [
        ("multistate_ocp(1000, 12, 4)", problems.multistate_ocp(1000, 12, 4), True),
        ("multistate_ocp(5000, 8, 4)", problems.multistate_ocp(5000, 8, 4), False),
        ("multistate_ocp(7500, 8, 4)", problems.multistate_ocp(7500, 8, 4), False),
        ("grid_box_qp(40, 2000)", problems.grid_box_qp(40, 2000), False),
    ]
    for name, prob, with_dense in cases:
        prob.pgf_force_band = True
        if a.split is not None:
            prob.pgf_band_split = bool(a.split)
        n, m = prob.num_vars, prob.num_cons
        plan = BandPlan(prob.hess_sparse(), prob.jac_sparse(), n, m)
        row = {"case": name, "N": n + m, "bw": plan.bw, "B": plan.block_size}
        if a.split is not None:
            row["split"] = a.split
        if a.narrow:
            a.quick = True
            row["route"] = f"bcr{plan.block_size}"
        t = device_times(prob, a.steps)
        row["wide_full_ms"] = 1e3 * t["Full"]
        row["wide_full_steps_per_s"] = 1.0 / t["Full"]
        row["wide_simplified_ms"] = 1e3 * t["Simplified"]
        if with_dense and not a.quick:
            dense = problems.LinearQuadraticProblem(prob.hess_sparse().toarray(), prob.q,
                                                    prob.jac_sparse().toarray(), prob.b, prob.var_lb,
                                                    prob.var_ub)
            td = device_times(dense, max(2, a.steps // 5))
            assert not td["sparse"]
            row["dense_full_ms"] = 1e3 * td["Full"]
            row["dense_simplified_ms"] = 1e3 * td["Simplified"]
        if not a.quick:
            row["oracle_full_ms"] = 1e3 * oracle_time(prob)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
