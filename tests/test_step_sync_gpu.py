"""Speculative index-set sizes of the dense qp step (GPU).

A step is enqueued with the last known |I|, |A| and redone by pgf_qp_sync when the compaction
finds other sizes.  Each sequence runs in a child process (the switches are read once per
process) with PGF_STEP_SPEC=1 and =0; the iterates, masks and step lengths must agree bit for bit,
a step must be redone exactly when |I| changed, and every other step must cost one host
synchronisation."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import pygradflow_amd as pgf
from pygradflow_amd import problems
cfg = json.loads(sys.argv[2])
n, m, kind = cfg["n"], cfg["m"], cfg["kind"]
prob = problems.dense_qp(n, m, seed=cfg.get("seed", 0), boxed_frac=cfg.get("boxed", 0.5))
dn = pgf.DeviceNewton(prob, kind, np.zeros(n), np.zeros(m), cfg.get("dt", 1.0), 1.0)
h, lib = dn._hd.h, dn._lib
def stats():
    a, b = C.c_int(0), C.c_int(0)
    assert lib.pgf_debug_step_stats(h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value
def nI():
    a, b = C.c_int(0), C.c_int(0)
    assert lib.pgf_reduced_dims(h, C.byref(a), C.byref(b)) == 0
    return a.value
rec = []
for i in range(cfg["steps"]):
    if i > 0 and i % cfg.get("outer", 2) == 0:
        dn.advance_outer(cfg.get("dt", 1.0) * (1.5 if i % 4 == 0 else 1.0), 1.0)
    if i == cfg.get("fail_helper_at", -1):
        lib.pgf_debug_fail_next_helper(h)
    if i == cfg.get("set_mask_at", -1):
        # a host mask with more active entries than the step will compute: its size is wrong
        mk = np.ascontiguousarray(dn.mask().astype(np.uint8))
        mk[::7] = 1
        assert lib.pgf_set_active_set(h, mk.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
    s0 = stats()
    norm = 0.0
    if cfg.get("async"):
        # bench.py's pattern: the norm is taken while the step is in flight
        dn.step_async()
        norm = dn.residual_norm()
        diff, _ = dn.sync()
    else:
        diff, _ = dn.step()
    s1 = stats()
    x, y = dn.point()
    rec.append(dict(x=x.tobytes().hex(), y=y.tobytes().hex(), mask=dn.mask().tobytes().hex(),
                    diff=float(diff).hex(), norm=float(norm).hex(), nI=nI(), syncs=s1[0] - s0[0],
                    redone=s1[1] - s0[1]))
print("REC" + json.dumps(rec))
"""


def _run(cfg, **env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", CHILD, REPO, json.dumps(cfg)], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("REC")][-1]
    return json.loads(line[3:])


def _same_results(a, b):
    assert len(a) == len(b)
    for k, (ra, rb) in enumerate(zip(a, b)):
        for key in ("x", "y", "mask", "diff", "norm", "nI"):
            assert ra[key] == rb[key], f"step {k}: {key} differs"


CASES = {
    "full_1024": dict(n=1024, m=256, kind="Full", steps=10),
    "full_4096": dict(n=4096, m=1024, kind="Full", steps=6),
    "full_async_norms": dict(n=1024, m=256, kind="Full", steps=10, **{"async": True}),
    "active_set": dict(n=1024, m=256, kind="ActiveSet", steps=10),
    "simplified": dict(n=1024, m=256, kind="Simplified", steps=10),
    "mismatch_with_helper_failure": dict(n=1024, m=256, kind="Full", steps=8, fail_helper_at=3,
                                         set_mask_at=3),
    "set_active_set": dict(n=1024, m=256, kind="Full", steps=6, set_mask_at=3),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_speculative_counts_match_synchronous_counts(gpu_available, name):
    if not gpu_available:
        pytest.skip("needs a GPU")
    cfg = CASES[name]
    spec = _run(cfg, PGF_STEP_SPEC="1")
    sync = _run(cfg, PGF_STEP_SPEC="0")
    _same_results(spec, sync)
    assert all(r["redone"] == 0 for r in sync)
    if cfg["kind"] == "Full":
        prev = None
        for k, r in enumerate(spec):
            changed = prev is not None and r["nI"] != prev
            if k == 0:
                assert r["redone"] == 0  # the first step of a handle waits for its counts
            elif cfg.get("set_mask_at") == k:
                # guessed from the host-counted mask pgf_set_active_set was given: too many active
                assert r["redone"] == 1, (k, r["redone"])
            else:
                assert r["redone"] == (1 if changed else 0), (k, r["nI"], prev, r["redone"])
            if k > 0 and not changed and k not in (cfg.get("fail_helper_at"), cfg.get("set_mask_at")):
                assert r["syncs"] == 1, (k, r["syncs"])
            prev = r["nI"]
        assert any(r["redone"] for r in spec)  # the redo path ran


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["0", "2"])
def test_speculative_counts_in_both_pivot_orders(gpu_available, order):
    if not gpu_available:
        pytest.skip("needs a GPU")
    cfg = dict(n=1024, m=256, kind="Full", steps=8)
    spec = _run(cfg, PGF_STEP_SPEC="1", PGF_CONDENSED=order)
    sync = _run(cfg, PGF_STEP_SPEC="0", PGF_CONDENSED=order)
    _same_results(spec, sync)


@pytest.mark.gpu
def test_redone_steps_match_the_oracle(gpu_available):
    """Full steps on a boxed QP whose |I| changes, taken as bench.py takes them (step_async,
    residual_norm, sync), against the CPU oracle: masks exact, iterates within 1e-10."""
    if not gpu_available:
        pytest.skip("needs a GPU")
    import ctypes as C

    import numpy as np

    from oracle import newton_oracle as O
    from pygradflow_amd import problems
    from pygradflow_amd.newton import DeviceNewton

    n, m = 256, 64
    prob = problems.dense_qp(n, m, seed=3, boxed_frac=0.5)
    x0, y0 = np.zeros(n), np.zeros(m)
    recs = O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, 8)
    dn = DeviceNewton(prob, "Full", x0, y0, 1.0, 1.0)
    try:
        for k, rec in enumerate(recs):
            dn.step_async()
            dn.residual_norm()
            dn.sync()
            x, y = dn.point()
            assert np.array_equal(dn.mask(), rec["mask"]), f"mask mismatch at step {k}"
            ex = np.max(np.abs(x - rec["xn"])) / max(1.0, np.max(np.abs(rec["xn"])))
            ey = np.max(np.abs(y - rec["yn"])) / max(1.0, np.max(np.abs(rec["yn"])))
            assert ex <= 1e-10 and ey <= 1e-10, (k, ex, ey)
        sizes = {int(r["mask"].sum()) for r in recs[1:]}
        redone = C.c_int(0)
        assert dn._lib.pgf_debug_step_stats(dn._hd.h, None, C.byref(redone)) == 0
        if len(sizes) > 1:
            assert redone.value >= 1
    finally:
        dn.close()
