"""The Globalized policy in the device batch (GPU): ``BatchedDeviceNewton(..., "Globalized",
line_search=True)`` against the reference's own steps (tests/golden/globalized/glob_*.npz), per
instance and with the assertions of tests/test_line_search_gpu.py::test_steps_match_reference -- on a
dense batch, a narrow band batch with per-instance dt, several workgroups per instance, the wide
route, failed searches beside accepted ones -- and the counts: one host wait per step and a number
of launches that depends neither on the batch size nor on the trial counts."""

import math

import numpy as np
import pytest

from tests import line_search_ref as R
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu

TOL = R.TOL
_runs = {}


def _batch(problems, dt, rho=1.0, **kw):
    from pygradflow_amd.batched import BatchedDeviceNewton

    kw.setdefault("line_search", True)
    return BatchedDeviceNewton(lambda i: problems[i], len(problems), "Globalized", dt, rho, **kw)


def _step(bn):
    """One step of every instance: what test_steps_match_reference looks at, per instance."""
    before = bn.points()
    status, _, diff = bn.step_local()
    rec = dict(before=before, after=bn.points(), mask=bn.masks(), status=status.copy(), diff=diff.copy(),
               ls=bn.line_search(), direction=[s.direction() for s in bn.solvers])
    if bn._b is not None:
        rec["launches"], rec["waits"] = bn.line_search_stats()
    return rec


def _check(case, k, rec, i, xhat, yhat):
    """Instance i of the recorded step against step k of its fixture."""
    import pygradflow_amd._lib as L

    pre = f"{k}/"
    merit0 = float(case[pre + "merit0"])
    scale = 1e-10 * max(1.0, merit0)
    failed, trials = bool(case[pre + "failed"]), int(case[pre + "trials"])
    ls = {key: val[i] for key, val in rec["ls"].items()}
    ref_merits = case[pre + "merits"]
    err_m = float(np.max(np.abs(ls["trial_merits"][:trials] - ref_merits))) if trials else 0.0
    dx, dy = rec["direction"][i]
    print("instance", i, "step", k, "trials", ls["trials"], "alpha", ls["alpha"], "merit0 err",
          abs(ls["merit0"] - merit0), "merit err", err_m, "dx err", rel_err(dx, case[pre + "dx"]), "status",
          rec["status"][i])
    bx, by = rec["before"][0][i], rec["before"][1][i]
    ax, ay = rec["after"][0][i], rec["after"][1][i]
    assert rel_err(bx, case[pre + "x"]) <= TOL
    assert rel_err(by, case[pre + "y"]) <= TOL
    assert np.array_equal(rec["mask"][i], case[pre + "mask"])
    assert rel_err(dx, case[pre + "dx"]) <= TOL
    assert rel_err(dy, case[pre + "dy"]) <= TOL
    assert (rec["status"][i] == L.PGF_LINE_SEARCH) == failed
    assert rec["status"][i] in (L.PGF_OK, L.PGF_LINE_SEARCH)
    assert ls["trials"] == trials
    assert abs(ls["merit0"] - merit0) <= scale
    if trials:
        assert abs(ls["slope"] - float(case[pre + "slope"])) <= scale
        assert err_m <= scale
    if failed:
        assert trials == 30
        assert ax.tobytes() == bx.tobytes() and ay.tobytes() == by.tobytes()  # not moved, bit for bit
        assert rec["diff"][i] == 0.0
        return
    assert ls["alpha"] == float(case[pre + "alpha"])
    assert rel_err(ax, case[pre + "xn"]) <= TOL
    assert rel_err(ay, case[pre + "yn"]) <= TOL
    want = float(np.sqrt(np.sum((xhat - case[pre + "xn"]) ** 2) + np.sum((yhat - case[pre + "yn"]) ** 2)))
    assert abs(rec["diff"][i] - want) <= TOL * max(1.0, want)


def _dense_pair():
    """Test 1's run, once: B = 2 dense, dense_qp(250, 9) seeds 2 and 3, every step of the fixtures."""
    if "pair" in _runs:
        return _runs["pair"]
    cases = [R.load_case("dense_qp_n250_m9_s2"), R.load_case("dense_qp_n250_m9_s3")]
    bn = _batch([R.build_problem(c) for c in cases], float(cases[0]["dt"]), float(cases[0]["rho"]),
                newton_tol=float(cases[0]["newton_tol"]))
    try:
        assert not bn.band
        steps = [_step(bn) for _ in range(int(cases[0]["steps"]))]
    finally:
        bn.close()
    _runs["pair"] = (cases, steps)
    return _runs["pair"]


def test_dense_two_instances_with_different_trial_counts():
    """n + m = 259: two ladder workgroups per instance, the second with three y entries only; trials
    [1, 4, 1, 5] beside [1, 10, 1, 10] in the same launches."""
    cases, steps = _dense_pair()
    for k, rec in enumerate(steps):
        for i, case in enumerate(cases):
            _check(case, k, rec, i, case["x0"], case["y0"])
    assert [int(r["ls"]["trials"][0]) for r in steps] == [1, 4, 1, 5]
    assert [int(r["ls"]["trials"][1]) for r in steps] == [1, 10, 1, 10]


def test_narrow_band_with_per_instance_dt():
    """box_qp(64) twice on the narrow band route, dt = 1 and 100: each against its own fixture, and
    bit for bit what the same two handles give one after the other."""
    cases = [R.load_case("box_qp_n64_dt1"), R.load_case("box_qp_n64_dt100")]
    dts = np.array([float(c["dt"]) for c in cases])
    out = {}
    for seq in (False, True):
        bn = _batch([R.build_problem(c, pgf_force_band=True) for c in cases], 1.0, sequential=seq)
        try:
            if not seq:
                assert bn.band and bn.band_block == 8 and bn.band_border == 0
            bn.advance_outer_each(dts, np.ones(2))
            out[seq] = [_step(bn) for _ in range(5)]
        finally:
            bn.close()
    for k in range(5):
        dev, one = out[False][k], out[True][k]
        for i, case in enumerate(cases):
            _check(case, k, dev, i, case["x0"], case["y0"])
            _check(case, k, one, i, case["x0"], case["y0"])
        assert dev["after"][0].tobytes() == one["after"][0].tobytes()
        assert dev["after"][1].tobytes() == one["after"][1].tobytes()
        assert dev["ls"]["alpha"].tobytes() == one["ls"]["alpha"].tobytes()
        assert np.array_equal(dev["ls"]["trials"], one["ls"]["trials"])
        assert dev["ls"]["trial_merits"].tobytes() == one["ls"]["trial_merits"].tobytes()
        assert np.array_equal(dev["status"], one["status"])


def test_several_workgroups_per_instance_and_a_frozen_one():
    """box_qp(513) three times on the band route (513 = 2 * 256 + 1: three ladder workgroups, the
    last with one entry); instance 1 sits the last step out."""
    import pygradflow_amd._lib as L

    case = R.load_case("box_qp_n513_dt1")
    nsteps = int(case["steps"])
    bn = _batch([R.build_problem(case, pgf_force_band=True) for _ in range(3)], float(case["dt"]))
    try:
        assert bn.band
        steps = []
        for k in range(nsteps):
            if k == nsteps - 1:
                bn.set_frozen([False, True, False])
            steps.append(_step(bn))
    finally:
        bn.close()
    for k, rec in enumerate(steps):
        last = k == nsteps - 1
        for i in range(3):
            if last and i == 1:
                continue
            _check(case, k, rec, i, case["x0"], case["y0"])
        for key in ("alpha", "trials", "merit0", "slope", "trial_merits"):
            assert rec["ls"][key][0].tobytes() == rec["ls"][key][2].tobytes()
            if not last:
                assert rec["ls"][key][0].tobytes() == rec["ls"][key][1].tobytes()
        for part in (0, 1):
            assert rec["after"][part][0].tobytes() == rec["after"][part][2].tobytes()
            if not last:
                assert rec["after"][part][0].tobytes() == rec["after"][part][1].tobytes()
    prev, rec = steps[-2], steps[-1]
    assert rec["status"][1] == L.PGF_OK and rec["diff"][1] == 0.0
    for part in (0, 1):
        assert rec["after"][part][1].tobytes() == prev["after"][part][1].tobytes()
    for key in ("alpha", "trials", "merit0", "slope", "trial_merits"):
        assert rec["ls"][key][1].tobytes() == prev["ls"][key][1].tobytes()


def test_wide_route_and_failure_then_a_full_step():
    import pygradflow_amd._lib as L
    from pygradflow_amd.newton import _POLICY_BITS

    case = R.load_case("multistate_ocp_fail")
    bn = _batch([R.build_problem(case, pgf_force_band=True) for _ in range(2)], float(case["dt"]),
                float(case["rho"]), wide_band=True)
    try:
        assert bn.band and bn.band_block >= 16
        steps = [_step(bn) for _ in range(2)]
        bn.policy = _POLICY_BITS["Full"]  # the same batch, the same outer step
        status, _, _ = bn.step_local()
        full = bn.points()
    finally:
        bn.close()
    for k, rec in enumerate(steps):
        for i in range(2):
            _check(case, k, rec, i, case["x0"], case["y0"])
    assert list(steps[0]["status"]) == [L.PGF_OK, L.PGF_OK]
    assert list(steps[1]["status"]) == [L.PGF_LINE_SEARCH, L.PGF_LINE_SEARCH]
    assert list(steps[1]["ls"]["trials"]) == [30, 30]
    assert list(status) == [L.PGF_OK, L.PGF_OK]
    for i in range(2):
        assert rel_err(full[0][i], case["full/xn"]) <= TOL
        assert rel_err(full[1][i], case["full/yn"]) <= TOL


def _mixed():
    """Test 5's runs, once: the failing dense_qp(40, 10), a neighbour that does not fail, the failing
    one again -- through the handles one after the other, then as a device batch."""
    if "mixed" in _runs:
        return _runs["mixed"]
    from pygradflow_amd import problems as P

    case = R.load_case("dense_qp_n40_m10_fail")
    # (seed 4: the reference accepts every one of its first six steps from x0 = y0 = 0 at dt = 1)
    other = P.dense_qp(40, 10, seed=4, boxed_frac=1.0, box=0.1)
    out = {}
    for seq in (True, False):
        probs = [R.build_problem(case), other, R.build_problem(case)]
        bn = _batch(probs, float(case["dt"]), float(case["rho"]), sequential=seq)
        try:
            out[seq] = [_step(bn) for _ in range(5)]
        finally:
            bn.close()
    _runs["mixed"] = (case, other, out[True], out[False])
    return _runs["mixed"]


def test_mixed_outcome_in_one_step():
    import pygradflow_amd._lib as L

    case, other, seq, dev = _mixed()
    fail_ok_fail = [L.PGF_LINE_SEARCH, L.PGF_OK, L.PGF_LINE_SEARCH]
    assert list(seq[3]["status"]) == fail_ok_fail  # the precondition, on the handles
    assert all(list(seq[k]["status"]) == [L.PGF_OK] * 3 for k in range(3))
    assert list(dev[3]["status"]) == fail_ok_fail
    dt, rho, tol = float(case["dt"]), float(case["rho"]), float(case["newton_tol"])
    xhat, yhat = np.zeros(40), np.zeros(10)
    for k in range(4):
        for i in (0, 2):
            _check(case, k, dev[k], i, case["x0"], case["y0"])
        # the neighbour: against the handles' run, and its search against the numpy form fed with
        # the device's own direction
        d, s = dev[k], seq[k]
        for part in (0, 1):
            assert rel_err(d["after"][part][1], s["after"][part][1]) <= TOL
        assert np.array_equal(d["mask"][1], s["mask"][1])
        dx, dy = d["direction"][1]
        ref = R.line_search(other, dt, rho, tol, xhat, yhat, d["before"][0][1], d["before"][1][1], dx, dy)
        scale = 1e-10 * max(1.0, ref["merit0"])
        assert not ref["failed"] and d["status"][1] == L.PGF_OK
        assert d["ls"]["trials"][1] == ref["trials"] == s["ls"]["trials"][1]
        assert d["ls"]["alpha"][1] == ref["alpha"]
        assert abs(d["ls"]["merit0"][1] - ref["merit0"]) <= scale
        assert abs(d["ls"]["slope"][1] - ref["slope"]) <= scale
        assert np.max(np.abs(d["ls"]["trial_merits"][1] - ref["merits"])) <= scale
        assert rel_err(d["after"][0][1], ref["xn"]) <= TOL and rel_err(d["after"][1][1], ref["yn"]) <= TOL
        assert abs(d["diff"][1] - ref["diff"]) <= TOL * max(1.0, ref["diff"])
    # one instance's failure does not touch another, and the batch serves the next step
    d, s = dev[4], seq[4]
    assert np.array_equal(d["status"], s["status"])
    assert d["status"][1] == L.PGF_OK and d["diff"][1] > 0.0
    for part in (0, 1):
        assert rel_err(d["after"][part], s["after"][part]) <= TOL
        for i in (0, 2):  # failed again from the same point: still not moved
            assert d["after"][part][i].tobytes() == dev[3]["before"][part][i].tobytes()


def test_one_wait_and_launch_counts_independent_of_trials_and_batch_size():
    _, pair = _dense_pair()
    assert [int(r["ls"]["trials"][1]) for r in pair] == [1, 10, 1, 10]
    print("B = 2: waits", [r["waits"] for r in pair], "stage launches", [r["launches"] for r in pair])
    assert all(r["waits"] == 1 for r in pair)
    assert len({r["launches"] for r in pair}) == 1 and pair[0]["launches"] > 0
    _, _, _, dev = _mixed()
    print("B = 3: waits", [r["waits"] for r in dev], "stage launches", [r["launches"] for r in dev])
    assert all(r["waits"] == 1 for r in dev)
    assert {r["launches"] for r in dev} == {pair[0]["launches"]}


@pytest.mark.parametrize("name,wide", [("box_qp_n64_dt1", False), ("multistate_ocp_fail", True)])
def test_instance_repaired_on_its_handle_searches_there(name, wide):
    """Instance 1's handle gets a refine_tol no solve can meet (1e-300; refine_fail stays 1e-7): every
    step the stage sits it out on the device, the guard refines it on its handle -- the step update
    from the outer point -- and the handle's own line search follows.  Both instances still match
    the fixture, the failed search of the wide case included; instance 0 never leaves the device."""
    import pygradflow_amd._lib as L

    case = R.load_case(name)
    nsteps = int(case["steps"])
    bn = _batch([R.build_problem(case, pgf_force_band=True) for _ in range(2)], float(case["dt"]),
                float(case["rho"]), wide_band=wide)
    lib, h1 = L.load(), bn.solvers[1]._hd.h
    try:
        assert bn.band and (bn.band_block >= 16) == wide
        L.check(lib.pgf_set_refinement(h1, 1, 1e-300, 1e-7), h1)
        steps = [_step(bn) for _ in range(nsteps)]
        repaired = bn.repaired()
    finally:
        lib.pgf_set_refinement(h1, 1, 1e-11, 1e-7)  # (the defaults: the handle goes back to the pool)
        bn.close()
    for k, rec in enumerate(steps):
        for i in range(2):
            _check(case, k, rec, i, case["x0"], case["y0"])
    print("repaired", repaired, "waits", [r["waits"] for r in steps], "launches", [r["launches"] for r in steps])
    assert repaired == nsteps
    assert all(r["waits"] > 1 for r in steps)  # (the repair and the handle's search wait on their own)
    assert len({r["launches"] for r in steps}) == 1


def test_refusals_leave_batches_that_step():
    import ctypes as C

    import pygradflow_amd as pgf
    from pygradflow_amd import _lib as L
    from pygradflow_amd.batched import BatchedDeviceNewton
    from pygradflow_amd.newton import _POLICY_BITS

    case = R.load_case("dense_qp_n24_m6")
    prob = R.build_problem(case)
    dt, rho = float(case["dt"]), float(case["rho"])
    lib = L.load()
    glob = _POLICY_BITS["Globalized"]
    ip = C.POINTER(C.c_int)

    def steps_ok(bn, want_trials):
        status, _, diff = bn.step_local()
        assert list(status) == [L.PGF_OK] * bn.count and np.all(diff > 0.0)
        assert list(bn.line_search()["trials"]) == [want_trials] * bn.count

    # the keyword: raised before any handle is built
    with pytest.raises(ValueError, match="Globalized"):
        BatchedDeviceNewton(lambda i: prob, 2, "Full", dt, rho, line_search=True)
    for kw in ("border", "wide_border", "band_ctl", "border_ctl", "ctl_refine"):
        with pytest.raises(ValueError, match=kw):
            BatchedDeviceNewton(lambda i: prob, 2, "Globalized", dt, rho, line_search=True, **{kw: True})
    with pytest.raises(ValueError, match="newton_tol"):
        BatchedDeviceNewton(lambda i: prob, 2, "Globalized", dt, rho, line_search=True, newton_tol=-1.0)
    with pytest.raises(NotImplementedError, match="Globalized"):
        BatchedDeviceNewton(lambda i: prob, 2, "Globalized", dt, rho)

    # the flag with every flag it does not go with, and for an unsymmetric formulation
    x0, y0 = case["x0"], case["y0"]
    sym = [pgf.DeviceNewton(prob, "Globalized", x0, y0, dt, rho) for _ in range(2)]
    uns = pgf.DeviceNewton(prob, "Globalized", x0, y0, dt, rho, step_solver_type="Standard")
    try:
        arr = (C.c_void_p * 2)(*[s._hd.h for s in sym])
        b = C.c_void_p()
        for extra in (L.BATCH_BORDER, L.BATCH_WIDE_BORDER | L.BATCH_BORDER | L.BATCH_WIDE_BAND, L.BATCH_BAND_CTL,
                      L.BATCH_BORDER_CTL | L.BATCH_BORDER | L.BATCH_BAND_CTL, L.BATCH_CTL_REFINE | L.BATCH_BAND_CTL,
                      L.BATCH_BORDER_CTL, L.BATCH_CTL_REFINE, L.BATCH_WIDE_BORDER):
            assert lib.pgf_batch_create_ex(arr, 2, L.BATCH_LINE_SEARCH | extra, C.byref(b)) == L.PGF_INVALID
        assert b"PGF_BATCH_LINE_SEARCH" in lib.pgf_last_error(sym[0]._hd.h)
        mixed = (C.c_void_p * 2)(sym[0]._hd.h, uns._hd.h)
        assert lib.pgf_batch_create_ex(mixed, 2, L.BATCH_LINE_SEARCH, C.byref(b)) == L.PGF_INVALID
        assert b"Symmetric" in lib.pgf_last_error(uns._hd.h)
        # the handles are still their own: a batch over them steps
        assert lib.pgf_batch_create_ex(arr, 2, L.BATCH_LINE_SEARCH | L.BATCH_WIDE_BAND, C.byref(b)) == L.PGF_OK
        try:
            assert lib.pgf_batch_advance_outer(b, dt, rho) == L.PGF_OK
            assert lib.pgf_batch_step_async(b, glob, math.nan) == L.PGF_OK
            st = np.zeros(2, dtype=np.int32)
            assert lib.pgf_batch_sync(b, st.ctypes.data_as(ip), None, None) == L.PGF_OK
            assert list(st) == [L.PGF_OK, L.PGF_OK]
        finally:
            lib.pgf_batch_destroy(b)
    finally:
        for s in sym + [uns]:
            s.close()

    # a batch without the flag: today's refusal, unchanged, and no line-search entry point
    plain = BatchedDeviceNewton(lambda i: prob, 2, "Full", dt, rho)
    try:
        assert lib.pgf_batch_step_async(plain._b, glob, math.nan) == L.PGF_INVALID
        assert b"PGF_STEP_LINE_SEARCH is served by single handles only" in lib.pgf_batch_last_error(plain._b)
        assert lib.pgf_batch_set_line_search(plain._b, 1e-8) == L.PGF_INVALID
        assert lib.pgf_batch_line_search_stats(plain._b, None, None, None, None, None) == L.PGF_INVALID
        status, _, diff = plain.step_local()
        assert list(status) == [L.PGF_OK, L.PGF_OK] and np.all(diff > 0.0)
    finally:
        plain.close()

    bn = _batch([prob, prob], dt, rho)
    try:
        b = bn._b
        assert lib.pgf_batch_line_search_stats(b, None, None, None, None, None) == L.PGF_NOT_READY
        lw = C.c_int(-1), C.c_int(-1)
        assert lib.pgf_batch_debug_line_search_stats(b, C.byref(lw[0]), C.byref(lw[1])) == L.PGF_OK
        assert (lw[0].value, lw[1].value) == (0, 0)
        for tol in (-1e-8, math.nan):
            assert lib.pgf_batch_set_line_search(b, tol) == L.PGF_INVALID
        assert lib.pgf_batch_set_line_search(None, 1e-8) == L.PGF_INVALID
        # the bit without both companions, as on the single handle
        for bits in (L.STEP_LINE_SEARCH, L.STEP_LINE_SEARCH | L.STEP_RECOMPUTE_MASK,
                     L.STEP_LINE_SEARCH | L.STEP_RECOMPUTE_MASK | L.STEP_REFACTOR_ON_CHANGE):
            assert lib.pgf_batch_step_async(b, bits, math.nan) == L.PGF_INVALID
        # not in the device-resident controller's loop
        assert lib.pgf_batch_ctl_iterate(b, glob, math.nan, 1) == L.PGF_INVALID
        steps_ok(bn, int(case["0/trials"]))
        # such a batch still takes the other policies, and the Globalized one again behind them
        bn.policy = _POLICY_BITS["Full"]
        status, _, diff = bn.step_local()
        assert list(status) == [L.PGF_OK, L.PGF_OK]
        assert lib.pgf_batch_line_search_stats(b, None, None, None, None, None) == L.PGF_OK  # any pointer null
        bn.policy = glob
        status, _, _ = bn.step_local()
        assert set(status) <= {L.PGF_OK, L.PGF_LINE_SEARCH}
    finally:
        bn.close()
