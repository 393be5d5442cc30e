"""The hand-back of a dense qp step and the front of a handle without finite bounds (GPU; DESIGN.md
4d: PGF_STEP_HANDBACK, PGF_UNBOUNDED_FRONT).

With the hand-back the tail's last launch leaves the new point's residual norm in the status block
and the block in host memory, and the step's one wait spins on a sequence word; a handle whose
bounds are all infinite keeps an empty mask and identity index lists and launches no compaction.
Neither changes a value.  The switches are read once per process, so every setting runs
tools/check_step_handback.py in a child process (its docstring lists the cases: boxed, unbounded,
m = 0 and box QPs at sizes around the 256-entry blocks, Full / ActiveSet / Simplified, eight steps
in bench.py's pattern; masks equal to the oracle's, iterates within 1e-10, the norm against numpy
and against the device slot read from another stream, the counters of waits, host synchronisations
and compactions, redone and refined steps, a pooled handle).  The dumps of all settings must be
bit-identical: the norm of the fused tail is the stand-alone kernel's, after every event that moves
the point or the outer point too."""

import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = {
    "default": {},
    "handback_off": {"PGF_STEP_HANDBACK": "0"},
    "unbounded_front_off": {"PGF_UNBOUNDED_FRONT": "0"},
    "spin_bound_zero": {"CHECK_SPIN_ZERO": "1"},  # every wait falls back to the runtime's
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every mode once; name -> (completed process, dump path)."""
    out = {}
    d = tmp_path_factory.mktemp("step_handback")
    for name, extra in MODES.items():
        env = dict(os.environ)
        for k in ("PGF_STEP_HANDBACK", "PGF_UNBOUNDED_FRONT", "PGF_STEP_FUSED", "PGF_EVAL_AHEAD", "PGF_STEP_SPEC",
                  "CHECK_SPIN_ZERO"):
            env.pop(k, None)
        env.update(extra)
        path = str(d / f"{name}.npz")
        res = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_step_handback.py"), path], env=env,
                             cwd=REPO, capture_output=True, text=True, timeout=600)
        out[name] = (res, path)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MODES))
def test_step_handback_matches_oracle(gpu_available, name, request):
    if not gpu_available:
        pytest.skip("needs a GPU")
    res, _ = request.getfixturevalue("runs")[name]
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "step handback ok" in res.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(set(MODES) - {"default"}))
def test_switch_settings_are_bit_identical(gpu_available, name, request):
    if not gpu_available:
        pytest.skip("needs a GPU")
    runs = request.getfixturevalue("runs")
    for key in ("default", name):
        assert runs[key][0].returncode == 0, runs[key][0].stdout[-2000:] + runs[key][0].stderr[-2000:]
    a, b = np.load(runs["default"][1]), np.load(runs[name][1])
    assert sorted(a.files) == sorted(b.files) and len(a.files) > 0
    for key in a.files:
        assert a[key].tobytes() == b[key].tobytes(), key
