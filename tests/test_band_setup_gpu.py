"""Configuration and lifetimes of the banded handle (csrc/pgf_api_band_setup.hip) at the C ABI: what
the pgf_sparse_* setters refuse, and one handle reconfigured in place against fresh ones.

Bars as in test_gpu_parity.py against the oracle (masks bit-identical, x and y within 1e-10
relative); between a reconfigured and a fresh handle everything is compared for equality.  Every problem of
the reconfiguration has n = 251, m = 85, so that one handle takes them all:

  plain_lq(251, 85, 2)                    plan bandwidth 6: block 8 (and 16 when forced)
  plain_lq(251, 85, 6)                    plan bandwidth 11: block 16 by the automatic rule
  case(3, 333, bw=2)                      a small border on the narrow route
  case(65, 271, bw=2, block=16, mloc=41)  the first size of the large border, kp = 128
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from oracle import newton_oracle as O
from tests import golden_util as G
from tests.band_util import TOL, band_problem, case, forced, plan_of

pytestmark = pytest.mark.gpu

N_VARS, N_CONS = 251, 85


def plain_lq(n, m, bw, seed, block=None, split=None):
    """band_problem's H of half-width bw with a diagonal in [1, 2], m local constraints
    x[a] - c x[a + 1] = b spread evenly (bordered_lq's), the box [-0.5, 0.5]; no border; forced."""
    from pygradflow_amd import problems

    rng = np.random.default_rng(seed)
    base = band_problem(n, rng.uniform(1.0, 2.0, n), seed, bw)
    a = (np.arange(m) * (n - 1)) // max(m, 1)
    A = sps.csr_matrix((np.concatenate([np.ones(m), -rng.uniform(0.5, 1.0, m)]),
                        (np.concatenate([np.arange(m)] * 2), np.concatenate([a, a + 1]))), shape=(m, n))
    prob = problems.LinearQuadraticProblem(base.hess_sparse(), base.q, A, 0.1 * rng.standard_normal(m),
                                           np.full(n, -0.5), np.full(n, 0.5))
    return forced(prob, block, split)


def narrow(block=None, split=None):
    return plain_lq(N_VARS, N_CONS, 2, 5, block, split)


def wide():
    return plain_lq(N_VARS, N_CONS, 6, 5)


def border3():
    return case(3, 333, bw=2)


def border65():
    prob = case(65, 271, bw=2, block=16, mloc=41)
    prob.pgf_border_limit = 1024
    return prob


def oracle_run(prob, steps):
    x0, y0 = np.zeros(prob.num_vars), np.zeros(prob.num_cons)
    return O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, steps)


def newton(pgf, prob):
    return pgf.DeviceNewton(prob, "Full", np.zeros(prob.num_vars), np.zeros(prob.num_cons), 1.0, 1.0)


def step_matches(dn, rec):
    dn.step()
    x, y = dn.point()
    assert np.array_equal(dn.mask(), rec["mask"])
    assert G.rel_err(x, rec["xn"]) <= TOL and G.rel_err(y, rec["yn"]) <= TOL


def raw_sparse_handle(lib, n, m):
    from pygradflow_amd import _lib

    h = C.c_void_p()
    _lib.check(lib.pgf_create(n, m, 0, _lib.CREATE_SPARSE, C.byref(h)), None, "pgf_create")
    return h


# ------------------------------------------------------------------ a: refusals
def test_what_the_setters_refuse(pgf):
    from pygradflow_amd import _lib, problems

    lib = _lib.load()
    INVALID, NOT_READY = _lib.PGF_INVALID, _lib.PGF_NOT_READY
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731

    def refused(rc, h, code, text):
        assert rc == code and lib.pgf_last_error(h) == text, (rc, lib.pgf_last_error(h))

    def set_pattern(h, plan, bw=None, pos=True):
        return lib.pgf_sparse_set_pattern(
            h, plan.bw if bw is None else bw, ip(plan.pos) if pos else None, plan.nnzH, ip(plan.Hptr),
            ip(plan.Hrow), ip(plan.Hcol), ip(plan.Hslot), plan.nnzJ, ip(plan.Jptr), ip(plan.Jcol),
            ip(plan.Jslot), ip(plan.JTptr), ip(plan.JTrow), ip(plan.JTmap))

    recs = oracle_run(border3(), 5)
    bordered = newton(pgf, border3())  # narrow route, k = 3: every group leaves it as it was
    dense = newton(pgf, problems.dense_qp(8, 2, seed=0))
    tiny_prob = plain_lq(8, 2, 2, 7)
    tiny, wide_dn = newton(pgf, tiny_prob), newton(pgf, wide())
    assert wide_dn._hd.plan.bw > 8 and wide_dn._hd.plan.block_size == 16
    bare = raw_sparse_handle(lib, 5, 0)  # a banded handle that has seen no pattern
    hb, hd = bordered._hd.h, dense._hd.h
    plan = bordered._hd.plan
    only_band = b"pgf_sparse_set_pattern first"

    # pgf_sparse_set_pattern
    refused(set_pattern(hd, plan), hd, NOT_READY, b"handle was not created with PGF_CREATE_SPARSE")
    for bw in (-1, 65):
        refused(set_pattern(hb, plan, bw=bw), hb, INVALID, b"bandwidth must be 0..64 in this version")
    refused(set_pattern(hb, plan, pos=False), hb, INVALID, b"null pattern")
    assert bordered.border_stats()[0] == 3
    step_matches(bordered, recs[0])

    # pgf_sparse_set_border
    refused(lib.pgf_sparse_set_border(hd, 1), hd, INVALID, b"pgf_sparse_set_border: banded handles only")
    refused(lib.pgf_sparse_set_border(hb, -1), hb, INVALID, b"border size must be 0..64")
    refused(lib.pgf_sparse_set_border(hb, 65), hb, INVALID, b"border size must be 0..64")
    for k in (10, 11):  # n + m = 10
        refused(lib.pgf_sparse_set_border(tiny._hd.h, k), tiny._hd.h, INVALID,
                b"the border must leave at least one band row")
    refused(lib.pgf_sparse_set_border(bare, 1), bare, NOT_READY, only_band)
    assert bordered.border_stats()[0] == 3 and tiny.border_stats()[0] == 0
    step_matches(bordered, recs[1])
    step_matches(tiny, oracle_run(tiny_prob, 1)[0])

    # pgf_sparse_set_block_size
    refused(lib.pgf_sparse_set_block_size(hb, 7), hb, INVALID,
            b"block size must be 0 (automatic), 8, 16, 32 or 64")
    refused(lib.pgf_sparse_set_block_size(wide_dn._hd.h, 8), wide_dn._hd.h, INVALID,
            b"block size is smaller than the half-bandwidth")
    refused(lib.pgf_sparse_set_block_size(bare, 8), bare, NOT_READY, only_band)
    step_matches(bordered, recs[2])
    step_matches(wide_dn, oracle_run(wide(), 1)[0])

    # pgf_sparse_set_values
    hv, jv = plan.values(bordered.problem.hess_sparse(), bordered.problem.jac_sparse())
    assert plan.nnzH > 0 and plan.nnzJ > 0
    refused(lib.pgf_sparse_set_values(hb, None, _lib.dptr(jv)), hb, INVALID, b"null values")
    refused(lib.pgf_sparse_set_values(hb, _lib.dptr(hv), None), hb, INVALID, b"null values")
    refused(lib.pgf_sparse_set_values(bare, _lib.dptr(hv), _lib.dptr(jv)), bare, NOT_READY, only_band)
    step_matches(bordered, recs[3])

    # pgf_sparse_set_factor_split
    refused(lib.pgf_sparse_set_factor_split(hd, 0), hd, INVALID,
            b"pgf_sparse_set_factor_split: banded handles only")
    step_matches(bordered, recs[4])

    assert lib.pgf_destroy(bare) == _lib.PGF_OK
    for dn in (bordered, dense, tiny, wide_dn):
        dn.close()


# ------------------------------------------------------------------ b: reconfiguration
def run_state(lib, dn, rhs):
    """Two Full steps from zero and one pgf_linear_solve on the handle as it is configured: the
    points, the inertias, the guard's measure after each, the solution, and the counters (the
    border's as they stand: a declaration starts them again; the others as increments)."""
    from pygradflow_amd import _lib

    band0, refined0 = dn.band_stats(), dn.refinement_stats()[0]
    dn.set_outer(np.zeros(dn.n), np.zeros(dn.m), 1.0, 1.0)
    arrays, scalars = [], []
    for _ in range(2):
        _, n_neg = dn.step()
        arrays.extend(dn.point())
        scalars += [n_neg, dn.refinement_stats()[2]]
    sol = np.empty(dn.n + dn.m)
    _lib.check(lib.pgf_linear_solve(dn._hd.h, _lib.dptr(rhs), 0, _lib.dptr(sol)), dn._hd.h, "pgf_linear_solve")
    arrays.append(sol)
    scalars.append(dn.refinement_stats()[2])
    scalars.append(dn.refinement_stats()[0] - refined0)
    scalars += [a - b for a, b in zip(dn.band_stats(), band0)]
    scalars += list(dn.border_stats())
    return arrays, scalars


def test_a_reconfigured_handle_is_a_fresh_one(pgf):
    from pygradflow_amd import _lib
    from pygradflow_amd.step_solver import POOL, _Handle

    lib = _lib.load()
    key = (N_VARS, N_CONS, 0)

    def new_handle():  # (not from the pool: it may hold handles of this size that other tests left)
        return _Handle(raw_sparse_handle(lib, N_VARS, N_CONS), *key, True)

    ok = lambda rc: _lib.check(rc, one.h, "reconfiguration")  # noqa: E731
    rhs = np.random.default_rng(11).standard_normal(N_VARS + N_CONS)
    one = new_handle()  # the handle that goes through every state

    def on(hd, prob):
        """A DeviceNewton for prob on the handle hd (the pool hands out what came back last)."""
        POOL.release(hd)
        dn = newton(pgf, prob)
        assert dn._hd is hd and dn.sparse
        return dn

    def take_back(dn, hd):
        dn.close()
        assert POOL.acquire(*key, sparse=True) is hd

    # (state, border k, oracle's problem, problem of a fresh handle, how the one handle gets there: ABI calls on it
    # as it stands, then the problem uploaded through a DeviceNewton unless it stays as it is)
    states = [
        ("plain narrow band", 0, narrow, narrow, [], narrow),
        ("border of 3", 3, border3, border3, [], border3),
        ("border removed", 0, narrow, narrow, [lambda h: lib.pgf_sparse_set_border(h, 0)], narrow),
        ("block size 16", 0, narrow, lambda: narrow(block=16),
         [lambda h: lib.pgf_sparse_set_block_size(h, 16)], None),
        ("split off", 0, narrow, lambda: narrow(block=16, split=False),
         [lambda h: lib.pgf_sparse_set_factor_split(h, 0)], None),
        ("split on", 0, narrow, lambda: narrow(block=16, split=True),
         [lambda h: lib.pgf_sparse_set_factor_split(h, 1)], None),
        ("large border of 65", 65, border65, border65, [], border65),
        ("large border removed", 0, narrow, narrow, [lambda h: lib.pgf_sparse_set_border(h, 0)], narrow),
        ("another bandwidth", 0, wide, wide, [], wide),
    ]
    oracle = {f: oracle_run(f(), 2) for f in (narrow, border3, border65, wide)}  # computed once
    dn = None
    for name, k, base, fresh_prob, calls, upload in states:
        for call in calls:
            ok(call(one.h))
        if upload is not None:
            if dn is not None:
                take_back(dn, one)
            dn = on(one, upload())
        got = run_state(lib, dn, rhs)
        fresh_hd = new_handle()
        fdn = on(fresh_hd, fresh_prob())
        want = run_state(lib, fdn, rhs)
        block = fdn._hd.plan.block_size
        take_back(fdn, fresh_hd)
        assert lib.pgf_destroy(fresh_hd.h) == _lib.PGF_OK
        print(name, "block", block, "scalars", want[1], "reconfigured", got[1])
        assert want[1][-3] == k  # pgf_debug_border_stats reports the state's border
        assert got[1] == want[1], name
        assert len(got[0]) == len(want[0]) == 5
        for a, b in zip(got[0], want[0]):
            assert np.array_equal(a, b), name
        # the fresh handle itself against the oracle
        for j, rec in enumerate(oracle[base]):
            assert G.rel_err(want[0][2 * j], rec["xn"]) <= TOL and G.rel_err(want[0][2 * j + 1], rec["yn"]) <= TOL, name
            assert want[1][2 * j] == N_CONS, name
        # the wide route ran, with solve phases exactly where the split is on
        reductions, solve_phases = want[1][-6], want[1][-5]
        if block > 8 and k == 0:
            assert reductions > 0 and (solve_phases > 0) == (name != "split off"), name
    assert plan_of(narrow()).block_size == 8 and plan_of(wide()).block_size == 16
    take_back(dn, one)
    assert lib.pgf_destroy(one.h) == _lib.PGF_OK
