"""The step's head -- K's assembly and the condensed system's panel -- beside the first diagonal
chain of the dense factorisation (``k_chain_head``, GPU).

PGF_HEAD_FUSED, PGF_CHAIN_HELP and PGF_CONDENSED are read once per process, so every mode runs
tools/check_head.py in a child process: boxed dense QPs whose reduced sizes land on 200, 256,
257, 300 and 519 (m = 70 condensed with the panel padded to 96 columns, m = 24 in the natural
order), Full and ActiveSet with an outer advance between the steps -- masks equal to the
oracle's, iterates within 1e-10, inertia m, at least one speculative step redone
(``pgf_debug_step_stats``), fused and plain heads where they belong (``pgf_debug_head_stats``;
none fused with the switch off) and a solve through the linear-solver view after a fused
factorisation.  The fusion changes where an entry of K and V is written, not how it is computed:
the dumps of the two switch settings must be bit-identical."""

import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = {
    "fused": {},
    "switch_off": {"PGF_HEAD_FUSED": "0"},
    "no_helpers": {"PGF_CHAIN_HELP": "0"},  # a grid of 1 + workers
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every mode once; name -> (completed process, dump path)."""
    out = {}
    d = tmp_path_factory.mktemp("head")
    for name, extra in MODES.items():
        env = dict(os.environ)
        env.pop("PGF_HEAD_FUSED", None)
        env["PGF_CONDENSED"] = "2"
        env.update(extra)
        path = str(d / f"{name}.npz")
        res = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_head.py"), path], env=env,
                             cwd=REPO, capture_output=True, text=True, timeout=600)
        out[name] = (res, path)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MODES))
def test_head_matches_oracle(gpu_available, name, request):
    if not gpu_available:
        pytest.skip("needs a GPU")
    res, _ = request.getfixturevalue("runs")[name]
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "head ok" in res.stdout


@pytest.mark.gpu
def test_switch_settings_are_bit_identical(gpu_available, request):
    if not gpu_available:
        pytest.skip("needs a GPU")
    runs = request.getfixturevalue("runs")
    for name in ("fused", "switch_off"):
        assert runs[name][0].returncode == 0, runs[name][0].stdout[-2000:] + runs[name][0].stderr[-2000:]
    a, b = np.load(runs["fused"][1]), np.load(runs["switch_off"][1])
    assert sorted(a.files) == sorted(b.files) and len(a.files) > 0
    for key in a.files:
        assert a[key].tobytes() == b[key].tobytes(), key
