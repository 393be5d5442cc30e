#!/usr/bin/env python3
"""The step's head beside the first diagonal chain (``k_chain_head``, csrc/pgf_factor2.hip)
against the CPU oracle (GPU).  Run under PGF_CONDENSED=2 with PGF_HEAD_FUSED unset or 0, and with
PGF_CHAIN_HELP=0 (a grid of 1 + workers); the switches are read once per process.  Used by
tests/test_head_fused_gpu.py.

  * boxed dense QPs (idxI is not the identity) whose reduced sizes land on 200, 256, 257, 300 and
    519 at a step from the second on: m = 70 in the condensed order (panel padded to 96 columns),
    m = 24 with rho = 200, where the condensed order's error bound refuses it (natural order: the
    J rows belong to the workers); Full and ActiveSet, four steps with an outer advance after the
    second: masks bit for bit, iterates to 1e-10, inertia m;
  * the sizes change between the steps, so speculative steps are discarded and enqueued again
    (``pgf_debug_step_stats``);
  * which factorisations ran their head beside the chain (``pgf_debug_head_stats``): the first
    condensed one takes the virtual blocks (plain), the ones with the Gram matrix and the natural
    order are fused above 256 rows; none with PGF_HEAD_FUSED=0;
  * the linear-solver view (``pgf_factor``, ``pgf_linear_solve``) after a fused factorisation
    against numpy.linalg.solve.

argv[1]: an .npz path; x, y and the mask after every step are dumped there (the test compares the
dumps of the two switch settings bit for bit).
"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import newton_oracle as O  # noqa: E402  (checker)
from pygradflow_amd import _lib, problems  # noqa: E402
from pygradflow_amd.newton import DeviceNewton  # noqa: E402

FUSED = os.environ.get("PGF_HEAD_FUSED", "1") != "0"
assert os.environ.get("PGF_CONDENSED") == "2", "run with PGF_CONDENSED=2"
TOL = 1e-10
COND = [(1.0, 1.0), (2.0, 1.0)]      # (dt, rho) of the outer steps: two Newton steps each
NAT = [(1.0, 200.0), (2.0, 200.0)]   # delta ~ 0.005: the condensed order is refused
CASES = [
    # n, m, seed, policy, outer steps, the reduced size that a step from the second on must have
    (284, 70, 1, "Full", COND, 200),
    (364, 70, 1, "Full", COND, 256),
    (366, 70, 1, "ActiveSet", COND, 257),
    (427, 70, 2, "Full", COND, 300),
    (735, 70, 1, "ActiveSet", COND, 519),
    (327, 24, 1, "Full", NAT, 256),
    (331, 24, 1, "Full", NAT, 257),
    (391, 24, 1, "ActiveSet", NAT, 300),
    (704, 24, 1, "Full", NAT, 519),
]


def rel(a, ref):
    return float(np.max(np.abs(a - ref)) / max(1.0, np.max(np.abs(ref)))) if ref.size else 0.0


def step_stats(dn):
    a, b = C.c_int(0), C.c_int(0)
    assert dn._lib.pgf_debug_step_stats(dn._hd.h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


dump = {}
worst = 0.0
tot_fused = tot_plain = tot_redone = redone_fused = 0
for ci, (n, m, seed, kind, outer, target) in enumerate(CASES):
    natural = outer is NAT
    prob = problems.dense_qp(n, m, seed=seed, boxed_frac=0.3)
    x, y = np.zeros(n), np.zeros(m)
    recs = []
    for dt, rho in outer:
        part = O.NewtonOracle(prob, kind, x, y, dt, rho).run(x, y, 2)
        recs.extend(part)
        x, y = part[-1]["xn"], part[-1]["yn"]
    sizes = [int(n - r["mask"].sum()) + (m if natural else 0) for r in recs]
    assert target in sizes[1:] and len(set(sizes)) > 1, (n, m, kind, sizes)
    assert not all(r["mask"].sum() == 0 for r in recs)
    dn = DeviceNewton(prob, kind, np.zeros(n), np.zeros(m), *outer[0])
    f0, p0 = dn.head_stats()
    r0 = step_stats(dn)[1]
    kinds, heads = [], []
    for k, rec in enumerate(recs):
        if k == 2:
            dn.advance_outer(*outer[1])
        diff, n_neg = dn.step()
        xd, yd = dn.point()
        mk = dn.mask()
        assert np.array_equal(mk, rec["mask"]), (n, m, kind, k, "mask")
        ex, ey = rel(xd, rec["xn"]), rel(yd, rec["yn"])
        worst = max(worst, ex, ey)
        assert ex <= TOL and ey <= TOL, (n, m, kind, k, ex, ey)
        assert n_neg == m, (n, m, kind, k, n_neg)
        kinds.append(dn.factor_kind())
        heads.append(dn.head_stats())
        dump[f"c{ci}_x{k}"], dump[f"c{ci}_y{k}"], dump[f"c{ci}_m{k}"] = xd, yd, mk
    assert all(kd == (1 if natural else 2) for kd in kinds), (n, m, kind, kinds)
    assert dn.refinement_stats()[1] == 0
    fused, plain = heads[-1][0] - f0, heads[-1][1] - p0
    redone = step_stats(dn)[1] - r0
    if kind == "Full":
        # one factorisation per step: the first condensed one applies the panel as virtual blocks
        want = [s > 256 and (natural or k >= 1) for k, s in enumerate(sizes)]
        got = [heads[k][0] - (heads[k - 1][0] if k else f0) for k in range(len(recs))]
        assert got == [int(w and FUSED) for w in want], (n, m, kind, sizes, got)
        assert fused + plain == len(recs), (fused, plain)
        # the linear-solver view: factorise without a right-hand side row, solve with any vector
        h, lib = dn._hd.h, dn._lib
        nI, N = C.c_int(0), C.c_int(0)
        assert lib.pgf_reduced_dims(h, C.byref(nI), C.byref(N)) == 0
        N = N.value
        K = np.zeros((N, N))
        _lib.check(lib.pgf_get_kkt(h, _lib.dptr(K), N), h, "pgf_get_kkt")
        K = np.tril(K) + np.tril(K, -1).T
        nn = C.c_int(-1)
        _lib.check(lib.pgf_factor(h, C.byref(nn)), h, "pgf_factor")
        assert nn.value == m, (nn.value, m)
        assert dn.head_stats()[0] - f0 - fused == int(want[-1] and FUSED), (n, m, sizes)
        rhs = np.random.default_rng(n).standard_normal(N)
        sol = np.empty(N)
        _lib.check(lib.pgf_linear_solve(h, _lib.dptr(rhs), 0, _lib.dptr(sol)), h, "pgf_linear_solve")
        ref = np.linalg.solve(K, rhs)
        err = float(np.max(np.abs(sol - ref)) / np.max(np.abs(ref)))
        dump[f"c{ci}_ls"] = sol
        assert err <= TOL, (n, m, err)
    if not FUSED:
        assert fused == 0, (n, m, kind, fused)
    tot_fused += fused
    tot_plain += plain
    tot_redone += redone
    redone_fused += redone if fused else 0
    dn.close()
    print(f"n={n} m={m} {kind}: sizes {sizes} kinds {kinds} fused {fused} plain {plain} redone {redone}",
          flush=True)
assert tot_redone >= 1, "no speculative step was discarded: the sizes never changed on the device"
assert tot_plain >= 1
if FUSED:
    assert tot_fused >= 1 and redone_fused >= 1, (tot_fused, redone_fused)
else:
    assert tot_fused == 0
if len(sys.argv) > 1:
    np.savez(sys.argv[1], **dump)
print(f"head ok, fused {tot_fused} plain {tot_plain} redone {tot_redone} worst {worst:.2e}", flush=True)
