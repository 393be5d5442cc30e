"""The launches in front of and behind the dense factorisation of a qp step in fewer launches
(PGF_STEP_FUSED; GPU): s_y in the step update, the row passes over J and H in one
launch, one combine launch for the partial sums, the H pass's epilogue and the residual, the
residual and the reduced rhs in the mask compaction's launch, the outer advance in one launch.

PGF_STEP_FUSED, PGF_CONDENSED and PGF_EVAL_AHEAD are read once per process, so every mode runs
tools/check_step_tail.py in a child process (its docstring lists the cases: boxed and unboxed
dense QPs with m around k_cond_y's 64 columns, ragged chunks, m = 1 and m = 0; Full, ActiveSet and
Simplified; four steps with an outer advance; masks equal to the oracle's, iterates within 1e-10,
inertia m, no LU fallback, a redone speculative step, a second user of the pooled handle).  The
fusion changes the launch a value is computed in, not how it is computed: the dumps of the two
switch settings must be bit-identical."""

import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = {
    "default": {},
    "switch_off": {"PGF_STEP_FUSED": "0"},
    "natural_order": {"PGF_CONDENSED": "0"},  # no k_cond_y; the J rows are in K
    "no_eval_ahead": {"PGF_EVAL_AHEAD": "0"},  # the fused tail must not engage
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every mode once; name -> (completed process, dump path)."""
    out = {}
    d = tmp_path_factory.mktemp("step_tail")
    for name, extra in MODES.items():
        env = dict(os.environ)
        for k in ("PGF_STEP_FUSED", "PGF_EVAL_AHEAD", "PGF_HEAD_FUSED", "PGF_STEP_SPEC"):
            env.pop(k, None)
        env["PGF_CONDENSED"] = "2"
        env.update(extra)
        path = str(d / f"{name}.npz")
        res = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_step_tail.py"), path], env=env,
                             cwd=REPO, capture_output=True, text=True, timeout=600)
        out[name] = (res, path)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MODES))
def test_step_tail_matches_oracle(gpu_available, name, request):
    if not gpu_available:
        pytest.skip("needs a GPU")
    res, _ = request.getfixturevalue("runs")[name]
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "step tail ok" in res.stdout


@pytest.mark.gpu
def test_switch_settings_are_bit_identical(gpu_available, request):
    if not gpu_available:
        pytest.skip("needs a GPU")
    runs = request.getfixturevalue("runs")
    for name in ("default", "switch_off"):
        assert runs[name][0].returncode == 0, runs[name][0].stdout[-2000:] + runs[name][0].stderr[-2000:]
    a, b = np.load(runs["default"][1]), np.load(runs["switch_off"][1])
    assert sorted(a.files) == sorted(b.files) and len(a.files) > 0
    for key in a.files:
        assert a[key].tobytes() == b[key].tobytes(), key
