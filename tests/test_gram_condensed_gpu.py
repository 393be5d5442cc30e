"""The condensed factorisation with the resident Gram matrix G = J^T J (GPU).

PGF_CONDENSED and PGF_CONDENSED_GRAM are read once per process, so every mode runs
tools/check_gram.py in a child process: boxed dense QPs (n 600 ... 1100, ragged m) under Full,
Simplified and ActiveSet with outer advances between the steps -- masks equal to the oracle's,
iterates within 1e-10, inertia m --, which factorisations took their rank-m term from G
(``pgf_debug_gram_stats``: none / from the second one after an upload / all), the linear-solver
view after such a factorisation, a new J through ``pgf_set_derivs_dense`` (G rebuilt; never built
when derivatives arrive before every step under the default rule) and the exact zero pivot of the
condensed order, which must still be repeated in the natural order inside the call."""

import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRAM_MODES = {
    "virtual_blocks": "0",   # never build G: the rank-m term as virtual column blocks
    "default_rule": "1",     # G from the second condensed factorisation after an upload
    "gram_at_once": "2",     # G at the first one
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GRAM_MODES))
def test_gram_condensed_matches_oracle(gpu_available, name):
    if not gpu_available:
        pytest.skip("needs a GPU")
    env = dict(os.environ)
    env["PGF_CONDENSED"] = "2"
    env["PGF_CONDENSED_GRAM"] = GRAM_MODES[name]
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_gram.py")], env=env,
                         cwd=REPO, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "gram ok" in out.stdout
