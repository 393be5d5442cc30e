"""The pivoted LU on the GPU: every panel kernel (k_lu_panel_reg<1..5> and the streaming
k_lu_panel), the pivot rule (max |a|, smallest row on ties, a NaN is reported), exact zero pivots
in every position, the row permutation, and both solves on both sides of their block boundaries.

tests/check_lu.py does the work in a child process (PGF_LU_PANEL is read once per process), in
groups so that no single test runs long; inputs and bounds are tests/lu_util.py's, proven on the
CPU by tests/test_lu_cases.py.  The parent reads the panel counts the child printed: a variant
cannot quietly run the other kernel.  One more pass goes through the solver handle, whose LU is
allocated and filled by another route (pgf_set_formulation, device assembly)."""

import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lu_util as LU

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = {"default": {}, "streaming_panels": {"PGF_LU_PANEL": "1"}}
# the large sizes only in the default process: the smallest that instantiate k_lu_panel_reg<2..5>
# and pass from the streaming kernel to the register kernel by themselves
GROUPS = [("default", g) for g in ("small", "exact", "edge", "large0", "large1", "large2", "large_exact")]
GROUPS += [("streaming_panels", g) for g in ("small", "exact", "edge")]


def _panels(stdout):
    """[(N, reg, streamed)] from check_lu.py's "panels <N> <reg> <streamed>" lines."""
    return [tuple(int(w) for w in ln.split()[1:4]) for ln in stdout.splitlines() if ln.startswith("panels ")]


@pytest.mark.parametrize("variant,group", GROUPS, ids=[f"{v}-{g}" for v, g in GROUPS])
def test_lu_group_under_panel_variant(gpu_available, variant, group):
    if not gpu_available:
        pytest.skip("needs a GPU")
    env = dict(os.environ)
    env.pop("PGF_LU_PANEL", None)
    env.update(VARIANTS[variant])
    out = subprocess.run([sys.executable, os.path.join(REPO, "tests", "check_lu.py"), group], env=env,
                         cwd=REPO, capture_output=True, text=True, timeout=600)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "lu ok" in out.stdout
    panels = _panels(out.stdout)
    assert panels
    for N, reg, streamed in panels:
        assert reg + streamed == -(-N // 32), (N, reg, streamed)
        if variant == "streaming_panels":
            assert reg == 0, (N, reg, streamed)
        else:
            assert streamed == sum(1 for c0 in range(0, N, 32) if N - c0 > 5120), (N, reg, streamed)
    sizes = {N for N, _, _ in panels}
    if group == "small":
        assert sizes >= set(LU.GAUSS_SMALL)
    if group == "large2":
        assert {p for p in panels if p[0] > 5120} == {(5121, 160, 1), (5153, 160, 2)}


def test_lu_behind_the_solver_handle(pgf):
    """Standard formulation on a bare handle with n + m = 1057: the Newton matrix the device
    assembled, and pgf_linear_solve with it and with its transpose, under the solve bounds of
    lu_util (|L||U| from LAPACK's factors of the same matrix)."""
    from pygradflow_amd import _lib
    from tests import golden_util as G
    from tests import unsym_ref as R
    from tests.test_unsym_device_gpu import _Raw

    n, m = 800, 257
    rng = np.random.default_rng(1057)
    S = rng.standard_normal((n, n))
    H = S + S.T
    J = rng.standard_normal((m, n))
    mask = np.zeros(n, dtype=bool)
    mask[rng.permutation(n)[: n // 3]] = True
    dt, rho = 0.7, 1.3
    inf = np.full(n, np.inf)
    raw = _Raw(n, m, -inf, inf, np.zeros(n), np.zeros(m), dt, rho, _lib.FORM_STANDARD)
    try:
        raw.derivs(H, J)
        raw.mask(mask)
        M = raw.matrix()
        assert G.rel_err(M, R.newton_matrix("Standard", H, J, mask, dt, rho)) <= 1e-14

        def solve(b, trans):
            sol = np.empty(n + m)
            raw.ck(raw.lib.pgf_linear_solve(raw.h, _lib.dptr(_lib.as_f64(b)), int(trans), _lib.dptr(sol)))
            return sol

        ratios = LU.check_solves_with_reference_factor(M, LU.rhs_set(n + m), solve)
        print(f"handle n+m={n + m}: error / bound {ratios}")
        assert set(ratios) == {"solve", "solve_trans"}
    finally:
        raw.close()
