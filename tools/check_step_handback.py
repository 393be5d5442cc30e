#!/usr/bin/env python3
"""The hand-back of a dense qp step and the front of a handle without finite bounds (GPU; DESIGN.md
4d: PGF_STEP_HANDBACK, PGF_UNBOUNDED_FRONT) against the CPU oracle, driven the way bench.py drives
its steps: step_async(); residual_norm(device slot); sync(); advance_outer() before every second
step.  The switches are read once per process: tests/test_step_handback_gpu.py runs this file in a
child process per setting and compares the dumps bit for bit.

Cases (n, m), eight steps each, outer steps of two Newton steps with dt = 1, 2, 2, 0.5:
  * boxed_frac 0.3: (96, 24), (200, 56) -- |A| > 0, the sizes change, steps are redone;
  * no finite bound: (96, 24), (300, 21), (519, 1) -- n + m no multiple of 256 or 64, more than one
    256-entry block of the norm, the head launch on and off around N = 256;
  * no constraints: (64, 0), (300, 0) without bounds; box_qp(64, dense=True): m = 0 with bounds;
  * one finite bound far from active on (96, 24): the general path, same bits as without it.
Full everywhere, ActiveSet and Simplified on a boxed and an unbounded case.  Per step: mask equal to
the oracle's, iterates within 1e-10, the returned norm equal to the device slot read from another
stream, and within NORM_ATOL of the norm numpy gives at the point read back (so never that of an
earlier point, outer point or dt); per case: one host synchronisation per step that was not redone,
every wait satisfied by the sequence word (or, with CHECK_SPIN_ZERO=1, none), no compaction on a
handle without finite bounds.  Then the same steps as step() + residual_norm() without a slot (same
bits), the norm after set_point, advance_outer with a new dt and set_outer, steps the guard
refines (illcond_qp(200, 56) at dt = 1e5), and a pooled handle that goes unbounded -> boxed ->
unbounded.

argv[1]: an .npz path for x, y, mask and norm of every step.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import newton_oracle as O  # noqa: E402  (checker)
from pygradflow_amd import problems  # noqa: E402
from pygradflow_amd.newton import DeviceNewton  # noqa: E402

HANDBACK = os.environ.get("PGF_STEP_HANDBACK", "1") != "0"
UNB_FRONT = os.environ.get("PGF_UNBOUNDED_FRONT", "1") != "0"
SPIN_ZERO = os.environ.get("CHECK_SPIN_ZERO") == "1"
TOL = 1e-10
# The norm is a sum of (n + m) squares of O(1) terms formed from dot products of length <= n in
# another order than numpy's: absolute error <= ~ n * eps * |terms| per entry; 1e-9 per unit of the
# point's and the data's size is two orders above that at n <= 519 and far below the change of the
# norm from one of the early Newton steps, outer points or dt to the next.
NORM_ATOL = 1e-9
DTS = [1.0, 2.0, 2.0, 0.5]
RHO = 1.0
CASES = [
    # name, n, m, seed, variant, policy
    ("boxed96", 96, 24, 1, "boxed", "Full"),
    ("boxed200", 200, 56, 1, "boxed", "Full"),
    ("boxed96_as", 96, 24, 1, "boxed", "ActiveSet"),
    ("boxed200_simp", 200, 56, 1, "boxed", "Simplified"),
    ("unb96", 96, 24, 1, "unbounded", "Full"),
    ("unb300", 300, 21, 1, "unbounded", "Full"),
    ("unb519", 519, 1, 1, "unbounded", "Full"),
    ("unb300_as", 300, 21, 1, "unbounded", "ActiveSet"),
    ("unb96_simp", 96, 24, 1, "unbounded", "Simplified"),
    ("nocons64", 64, 0, 2, "unbounded", "Full"),
    ("nocons300", 300, 0, 2, "unbounded", "Full"),
    ("box64", 64, 0, 0, "box", "Full"),
    ("onebound96", 96, 24, 1, "onebound", "Full"),
]


def make_problem(n, m, seed, variant):
    if variant == "box":
        return problems.box_qp(n, dense=True)
    prob = problems.dense_qp(n, m, seed=seed, boxed_frac=0.3 if variant == "boxed" else 0.0)
    if variant == "onebound":
        prob.var_ub[n // 2] = 1e6  # finite, never active
    return prob


def rel(a, ref):
    return float(np.max(np.abs(a - ref)) / max(1.0, np.max(np.abs(ref)))) if ref.size else 0.0


def ints(fn, dn):
    a, b = C.c_int(0), C.c_int(0)
    assert fn(dn._hd.h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def qp_data(prob):
    x0 = np.zeros(prob.num_vars)
    H = np.asarray(prob.lag_hess(x0, np.zeros(prob.num_cons)).todense())
    A = np.asarray(prob.cons_jac(x0).todense()).reshape(prob.num_cons, prob.num_vars)
    q = np.asarray(prob.obj_grad(x0))
    b = -np.asarray(prob.cons(x0))
    return H, A, q, b


def ref_norm(data, lb, ub, x, y, xh, yh, dt, rho):
    """ImplicitFunc.value_at (unscaled) at (x, y) for the outer point (xh, yh)."""
    H, A, q, b = data
    c = A @ x - b
    g = H @ x + (q + A.T @ (rho * c + y))
    p = xh - dt * g
    act = (p < lb - 1e-8) | (p > ub + 1e-8)
    p = np.where(act, np.clip(p, lb, ub), p)
    return float(np.sqrt(np.sum((x - p) ** 2) + np.sum((y - (yh + dt * c)) ** 2)))


def check_norm(tag, data, prob, val, x, y, xh, yh, dt):
    ref = ref_norm(data, prob.var_lb, prob.var_ub, x, y, xh, yh, dt, RHO)
    scale = 1.0 + np.linalg.norm(np.concatenate([x, y, xh, yh])) * max(1.0, dt)
    assert abs(val - ref) <= NORM_ATOL * scale, (tag, val, ref, scale)


def oracle_records(prob, kind, n, m):
    x, y = np.zeros(n), np.zeros(m)
    recs = []
    for dt in DTS:
        part = O.NewtonOracle(prob, kind, x, y, dt, RHO).run(x, y, 2)
        recs.extend(part)
        x, y = part[-1]["xn"], part[-1]["yn"]
    return recs


side = torch.cuda.Stream()


def run_bench_pattern(name, prob, kind, n, m, recs, data, dump):
    """bench.py's pattern against recs; returns the per-step (x, y, mask, norm)."""
    dn = DeviceNewton(prob, kind, np.zeros(n), np.zeros(m), DTS[0], RHO)
    if SPIN_ZERO:
        assert dn._lib.pgf_debug_handback_spin_bound(dn._hd.h, 0.0) == 0
    slot = torch.zeros(1, dtype=torch.float64, device="cuda")
    out = []
    s0, r0 = dn.step_stats()
    w0, f0 = ints(dn._lib.pgf_debug_handback_stats, dn)
    g0, u0 = ints(dn._lib.pgf_debug_front_stats, dn)
    ref0 = dn.refinement_stats()[0]
    xh, yh, dt = np.zeros(n), np.zeros(m), DTS[0]
    for k, rec in enumerate(recs):
        if k % 2 == 0 and k > 0:
            xh, yh = dn.point()
            dt = DTS[k // 2]
            dn.advance_outer(dt, RHO)
        sa, ra = dn.step_stats()
        dn.step_async()
        norm = dn.residual_norm(slot.data_ptr())
        with torch.cuda.stream(side):  # (not the solver's stream, no wait for it)
            seen = float(slot.cpu()[0])
        assert seen == norm, (name, k, seen, norm)
        dn.sync()
        sb, rb = dn.step_stats()
        x, y = dn.point()
        mk = dn.mask()
        assert np.array_equal(mk, rec["mask"]), (name, k, "mask")
        ex, ey = rel(x, rec["xn"]), rel(y, rec["yn"])
        assert ex <= TOL and ey <= TOL, (name, k, ex, ey)
        check_norm((name, k), data, prob, norm, x, y, xh, yh, dt)
        if kind == "Full" and k > 0 and rb == ra:
            assert sb - sa == 1, (name, k, sb - sa)  # one host synchronisation per step not redone
        out.append((x, y, mk, norm))
        dump[f"{name}_x{k}"], dump[f"{name}_y{k}"], dump[f"{name}_m{k}"] = x, y, mk
        dump[f"{name}_n{k}"] = np.array([norm, seen])
    assert dn.refinement_stats()[0] == ref0, (name, "refined")  # (the norm above is the kept point's)
    redone = dn.step_stats()[1] - r0
    by_word, fell = (a - b for a, b in zip(ints(dn._lib.pgf_debug_handback_stats, dn), (w0, f0)))
    general, unb = (a - b for a, b in zip(ints(dn._lib.pgf_debug_front_stats, dn), (g0, u0)))
    fused = kind == "Full"  # every Full step factorises, is checked and takes the fused tail
    if not HANDBACK:
        assert by_word == 0 and fell == 0, (name, by_word, fell)
    elif fused:
        assert by_word + fell == len(recs) + redone, (name, by_word, fell, redone)
        assert (by_word if not SPIN_ZERO else fell) == len(recs) + redone, (name, by_word, fell)
    else:
        assert (fell if not SPIN_ZERO else by_word) == 0, (name, by_word, fell)
    bounded = bool(np.any(np.isfinite(prob.var_lb)) or np.any(np.isfinite(prob.var_ub)))
    if bounded or not UNB_FRONT:
        assert unb == 0 and general > 0, (name, general, unb)
    else:
        assert general == 0 and unb > 0 and redone == 0, (name, general, unb, redone)
        assert not dn.mask().any()
        nI, N = C.c_int(0), C.c_int(0)
        assert dn._lib.pgf_reduced_dims(dn._hd.h, C.byref(nI), C.byref(N)) == 0
        assert (nI.value, N.value) == (n, n + m), (name, nI.value, N.value)
        if kind == "ActiveSet":  # no wait for a mask difference: the step's own wait only
            assert dn.step_stats()[0] - s0 == len(recs), (name, dn.step_stats()[0] - s0)
    dn.close()
    return out, redone


def run_plain_pattern(name, prob, kind, n, m, kept):
    """step() followed by a stand-alone residual_norm(): the same bits."""
    dn = DeviceNewton(prob, kind, np.zeros(n), np.zeros(m), DTS[0], RHO)
    for k, (x0, y0, mk0, norm0) in enumerate(kept):
        if k % 2 == 0 and k > 0:
            dn.advance_outer(DTS[k // 2], RHO)
        dn.step()
        norm = dn.residual_norm()
        x, y = dn.point()
        assert np.array_equal(x, x0) and np.array_equal(y, y0) and np.array_equal(dn.mask(), mk0), (name, k)
        assert norm == norm0, (name, k, norm, norm0)
    dn.close()


def staleness(prob, n, m, data, dump):
    """The norm after whatever moves the point or the outer point is taken again."""
    dn = DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, RHO)
    xh, yh, dt = np.zeros(n), np.zeros(m), 1.0
    vals = []
    dn.step()
    x, y = dn.point()
    vals.append(dn.residual_norm())
    check_norm("after step", data, prob, vals[-1], x, y, xh, yh, dt)
    dn.set_point(0.5 * x, 2.0 * y)
    vals.append(dn.residual_norm())
    check_norm("set_point", data, prob, vals[-1], 0.5 * x, 2.0 * y, xh, yh, dt)
    dn.step()
    x, y = dn.point()
    dn.advance_outer(3.0, RHO)  # a new outer point and a new dt: g, c stay valid, the norm does not
    xh, yh, dt = x, y, 3.0
    vals.append(dn.residual_norm())
    check_norm("advance_outer", data, prob, vals[-1], x, y, xh, yh, dt)
    assert vals[-1] != vals[-2]
    dn.step()
    xh, yh, dt = 0.1 * np.ones(n), np.zeros(m), 0.7
    dn.set_outer(xh, yh, dt, RHO)
    vals.append(dn.residual_norm())
    check_norm("set_outer", data, prob, vals[-1], xh, yh, xh, yh, dt)
    dn.close()
    dump["stale_norms"] = np.array(vals)


def refined_step(dump):
    """Steps the guard refines inside sync() (hard_illcond_n200_m56_dt1e5's problem, the guard's
    tolerance below roundoff so that every checked step takes a refinement round): the norm taken
    afterwards is the refined point's, not the one the tail left for the point before."""
    n, m, dt = 200, 56, 1e5
    prob = problems.illcond_qp(n, m, seed=4, lo=-4.0, hi=4.0)
    data = qp_data(prob)
    dn = DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), dt, RHO)
    r0 = dn.refinement_stats()[0]
    assert dn._lib.pgf_set_refinement(dn._hd.h, 1, 1e-30, 0.0) == 0
    slot = torch.zeros(1, dtype=torch.float64, device="cuda")
    vals = []
    try:
        for k in range(2):
            dn.step_async()
            vals.append(dn.residual_norm(slot.data_ptr()))
            dn.sync()
            x, y = dn.point()
            vals.append(dn.residual_norm())
            check_norm(("refined", k), data, prob, vals[-1], x, y, np.zeros(n), np.zeros(m), dt)
            dump[f"refined_x{k}"] = x
        assert dn.refinement_stats()[0] - r0 >= 2, "no step was refined"
    finally:
        assert dn._lib.pgf_set_refinement(dn._hd.h, 1, 1e-11, 0.0) == 0  # (the handle is pooled)
        dn.close()
    dump["refined_norms"] = np.array(vals)


dump = {}
tot_redone = 0
kept_all = {}
for name, n, m, seed, variant, kind in CASES:
    prob = make_problem(n, m, seed, variant)
    recs = oracle_records(prob, kind, n, m)
    data = qp_data(prob)
    kept, redone = run_bench_pattern(name, prob, kind, n, m, recs, data, dump)
    if variant == "boxed" and kind == "Full":
        assert redone > 0, (name, "no step was redone")
    tot_redone += redone
    run_plain_pattern(name, prob, kind, n, m, kept)
    kept_all[name] = kept
    print(f"{name} {kind}: redone {redone}", flush=True)
# one finite bound far from active: the general path, the bits of the handle without it
for k, (a, b) in enumerate(zip(kept_all["onebound96"], kept_all["unb96"])):
    assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])) and a[3] == b[3], ("onebound", k)
# a pooled handle (96, 24): unbounded -> boxed -> unbounded
for variant in ("boxed", "unbounded"):
    name = {"boxed": "boxed96", "unbounded": "unb96"}[variant]
    prob = make_problem(96, 24, 1, variant)
    kept, _ = run_bench_pattern(name + "_again", prob, "Full", 96, 24, oracle_records(prob, "Full", 96, 24),
                                qp_data(prob), {})
    for k, (a, b) in enumerate(zip(kept, kept_all[name])):
        assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])) and a[3] == b[3], (name, "pooled", k)
prob = make_problem(200, 56, 1, "boxed")
staleness(prob, 200, 56, qp_data(prob), dump)
refined_step(dump)
if len(sys.argv) > 1:
    np.savez(sys.argv[1], **dump)
print(f"step handback ok, redone {tot_redone}", flush=True)
