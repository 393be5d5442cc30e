#!/usr/bin/env python3
"""The launches in front of and behind the dense factorisation of a qp step (PGF_STEP_FUSED,
DESIGN.md 4d) against the CPU oracle (GPU): s_y formed by the step update, the row passes over J
and H in one launch, the sums + the H pass's epilogue + the residual in one combine launch, the
residual and the reduced rhs in the mask compaction's launch, pgf_qp_advance_outer in one launch.
Run under PGF_CONDENSED=2 (the condensed order and its s_y at small sizes), alone or with
PGF_STEP_FUSED=0, PGF_CONDENSED=0 or PGF_EVAL_AHEAD=0; the switches are read once per process.
Used by tests/test_step_tail_gpu.py.

Every case runs four steps with an outer advance after the second: masks bit for bit, iterates to
1e-10, inertia m, no LU fallback.
  * boxed_frac = 0.3 (|A| > 0, idxI is not the identity, the sizes change: speculative steps are
    discarded and redone): (n, m) = (284, 70), (366, 65), (427, 63) -- m over, just over and under
    k_cond_y's 64 columns per workgroup, chunks of one row, nothing a multiple of 4 or 256;
  * boxed_frac = 0 (|A| = 0 throughout: the fused front): (300, 64), (700, 300) -- chunks of several
    rows, fewer of them than the scratch holds, n across a 256-column workgroup edge --, (260, 1);
  * m = 0: box_qp(300, dense=True), the combine launch's branch without partial sums;
  * Full everywhere, ActiveSet and Simplified on two cases each (the back-solve steps of Simplified
    take the separate residual launches beside the fused ones);
  * which sequence ran (``pgf_debug_tail_stats``), at least one step redone
    (``pgf_debug_step_stats``) behind a step with a non-empty active set;
  * one solve through the linear-solver view after a Full step against numpy.linalg.solve;
  * after the run a second user of the pooled handle steps correctly (tickets left at zero).

argv[1]: an .npz path; x, y and the mask after every step and the linear solves are dumped there
(the test compares the dumps of the two switch settings bit for bit).
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

FUSED = os.environ.get("PGF_STEP_FUSED", "1") != "0"
AHEAD = os.environ.get("PGF_EVAL_AHEAD", "1") != "0"
COND = os.environ.get("PGF_CONDENSED")
assert COND in ("0", "2"), "run with PGF_CONDENSED=2 (or 0: the natural order)"
TOL = 1e-10
OUTER = [(1.0, 1.0), (2.0, 1.0)]  # (dt, rho) of the outer steps: two Newton steps each
CASES = [
    # n, m, seed, boxed_frac, policy
    (284, 70, 1, 0.3, "Full"),
    (366, 65, 1, 0.3, "Full"),
    (427, 63, 2, 0.3, "Full"),
    (284, 70, 1, 0.3, "ActiveSet"),
    (427, 63, 2, 0.3, "Simplified"),
    (300, 64, 1, 0.0, "Full"),
    (700, 300, 1, 0.0, "Full"),
    (260, 1, 1, 0.0, "Full"),
    (300, 64, 1, 0.0, "ActiveSet"),
    (700, 300, 1, 0.0, "Simplified"),
    (300, 0, 0, None, "Full"),  # box_qp(300, dense=True)
]


def rel(a, ref):
    return float(np.max(np.abs(a - ref)) / max(1.0, np.max(np.abs(ref)))) if ref.size else 0.0


def step_stats(dn):
    a, b = C.c_int(0), C.c_int(0)
    assert dn._lib.pgf_debug_step_stats(dn._hd.h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def oracle_records(prob, kind, n, m):
    x, y = np.zeros(n), np.zeros(m)
    recs = []
    for dt, rho in OUTER:
        part = O.NewtonOracle(prob, kind, x, y, dt, rho).run(x, y, 2)
        recs.extend(part)
        x, y = part[-1]["xn"], part[-1]["yn"]
    return recs


def run_case(prob, kind, n, m, recs, tag, dump):
    """Four steps on a handle from the pool against recs; returns (worst error, redone steps)."""
    worst = 0.0
    dn = DeviceNewton(prob, kind, np.zeros(n), np.zeros(m), *OUTER[0])
    t0, r0 = dn.tail_stats(), step_stats(dn)[1]
    for k, rec in enumerate(recs):
        if k == 2:
            dn.advance_outer(*OUTER[1])
        diff, n_neg = dn.step()
        xd, yd = dn.point()
        mk = dn.mask()
        assert np.array_equal(mk, rec["mask"]), (n, m, kind, k, "mask")
        ex, ey = rel(xd, rec["xn"]), rel(yd, rec["yn"])
        worst = max(worst, ex, ey)
        assert ex <= TOL and ey <= TOL, (n, m, kind, k, ex, ey)
        assert n_neg == m, (n, m, kind, k, n_neg)
        if dump is not None:
            dump[f"{tag}_x{k}"], dump[f"{tag}_y{k}"], dump[f"{tag}_m{k}"] = xd, yd, mk
    if m and n > m:
        assert dn.factor_kind() == (2 if COND == "2" else 1), (n, m, kind, dn.factor_kind())
    assert dn.refinement_stats()[1] == 0, (n, m, kind, "LU fallback")
    fused, plain = (a - b for a, b in zip(dn.tail_stats(), t0))
    redone = step_stats(dn)[1] - r0
    if not (FUSED and AHEAD):
        assert fused == 0, (n, m, kind, fused)
    if not AHEAD:
        assert plain == 0, (n, m, kind, plain)
    elif kind == "Full":  # every step factorises and is checked: one sequence or the other
        assert (fused if FUSED else plain) == len(recs) + redone, (n, m, kind, fused, plain, redone)
        assert (plain if FUSED else fused) == 0, (n, m, kind, fused, plain)
    if kind == "Full" and dump is not None:
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
        rhs = np.random.default_rng(n).standard_normal(N)
        sol = np.empty(N)
        _lib.check(lib.pgf_linear_solve(h, _lib.dptr(rhs), 0, _lib.dptr(sol)), h, "pgf_linear_solve")
        ref = np.linalg.solve(K, rhs)
        err = float(np.max(np.abs(sol - ref)) / np.max(np.abs(ref)))
        dump[f"{tag}_ls"] = sol
        assert err <= TOL, (n, m, err)
    dn.close()
    return worst, redone, fused, plain


dump = {}
worst = 0.0
tot_redone = tot_fused = tot_plain = 0
transition = False
for ci, (n, m, seed, boxed, kind) in enumerate(CASES):
    prob = problems.box_qp(n, dense=True) if boxed is None else problems.dense_qp(n, m, seed=seed, boxed_frac=boxed)
    recs = oracle_records(prob, kind, n, m)
    active = [int(r["mask"].sum()) for r in recs]
    if boxed == 0.0:
        assert not any(active), (n, m, kind, active)
    else:
        assert any(active) and len(set(active)) > 1, (n, m, kind, active)
    w, redone, fused, plain = run_case(prob, kind, n, m, recs, f"c{ci}", dump)
    # a step with a non-empty active set followed by one enqueued with stale sizes and redone
    transition = transition or (kind == "Full" and boxed == 0.3 and redone >= 1)
    worst = max(worst, w)
    tot_redone += redone
    tot_fused += fused
    tot_plain += plain
    print(f"n={n} m={m} {kind}: |A| {active} fused {fused} plain {plain} redone {redone}", flush=True)
    if ci == 2:
        # the pooled handle again (same n, m): tickets and counters were left as a fresh handle's
        w2 = run_case(prob, kind, n, m, recs, "again", None)[0]
        worst = max(worst, w2)
assert tot_redone >= 1 and transition, "no speculative step was discarded: the sizes never changed on the device"
if FUSED and AHEAD:
    assert tot_fused >= 1
elif AHEAD:
    assert tot_plain >= 1 and tot_fused == 0
if len(sys.argv) > 1:
    np.savez(sys.argv[1], **dump)
print(f"step tail ok, fused {tot_fused} plain {tot_plain} redone {tot_redone} worst {worst:.2e}", flush=True)
