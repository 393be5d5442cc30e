"""Random operation sequences on one handle against the CPU oracle (GPU; tests/seq_util.py has the
model, the generator, the adapters and the bars; tests/test_seq_model_host.py shows that the committed
seeds have teeth).

One test per (adapter, problem, policy, seed):
  * dense: DeviceNewton on twelve dense_qp shapes, in this process and -- the pivot order's switch is
    read once per process -- in one child process each under PGF_CONDENSED=0 and PGF_CONDENSED=2 (this
    file with a command, the outcomes in an .npz);
  * band: narrow, wide (factor / solve split on and off) and bordered problems, every policy;
  * dense_batch, band_batch: BatchedDeviceNewton as a device batch, two sequences per policy and
    problem set, every instance against its own model.
A failure names the adapter, the seed, the operations, the first failing one and the quantity;
``python tests/seq_util.py replay <adapter> <seed>`` shows every operation's errors.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import seq_util as S  # noqa: E402

CASES = {a: S.committed(a) for a in S.ADAPTERS}
CONDENSED = ("0", "2")


def _run(case):
    worst = S.run_sequence(case, S.DeviceBackend())
    print(f"SEQ {case.adapter} {case.id} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(worst.items())))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES["dense"], ids=lambda c: c.id)
def test_dense_sequence(pgf, case):
    _run(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES["band"], ids=lambda c: c.id)
def test_band_sequence(pgf, case):
    _run(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES["dense_batch"], ids=lambda c: c.id)
def test_dense_batch_sequence(pgf, case):
    _run(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES["band_batch"], ids=lambda c: c.id)
def test_band_batch_sequence(pgf, case):
    _run(case)


# ------------------------------------------------------------------ child process: PGF_CONDENSED
def child_dense(out):
    """Every committed dense sequence in this process; per case the failure's message (empty: passed)
    and the worst errors on x and y."""
    res = {}
    for case in S.committed("dense"):
        try:
            worst = S.run_sequence(case, S.DeviceBackend())
            res[case.id + "/msg"] = np.array("")
            res[case.id + "/err"] = np.array([worst.get("x", 0.0), worst.get("y", 0.0)])
        except S.SequenceFailure as e:
            res[case.id + "/msg"] = np.array(str(e))
            res[case.id + "/err"] = np.array([np.nan, np.nan])
    np.savez(out, **res)
    print("sequence child ok", flush=True)


@pytest.fixture(scope="module")
def condensed_results(tmp_path_factory):
    """PGF_CONDENSED value -> the child's outcomes, one child per value, run on first use"""
    cache = {}
    d = tmp_path_factory.mktemp("sequences")

    def get(value):
        if value not in cache:
            out = str(d / f"condensed{value}.npz")
            env = dict(os.environ)
            env["PGF_CONDENSED"] = value
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "dense", out], env=env, cwd=REPO,
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert "sequence child ok" in r.stdout
            with np.load(out) as z:
                cache[value] = {k: z[k] for k in z.files}
        return cache[value]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES["dense"], ids=lambda c: c.id)
@pytest.mark.parametrize("value", CONDENSED)
def test_dense_sequence_under_pgf_condensed(pgf, condensed_results, value, case):
    got = condensed_results(value)
    msg = str(got[case.id + "/msg"])
    print(f"SEQ dense_condensed{value} {case.id} x={got[case.id + '/err'][0]:.2e} y={got[case.id + '/err'][1]:.2e}")
    assert msg == "", f"PGF_CONDENSED={value}: {msg}"


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dense":
        child_dense(sys.argv[2])
    else:
        sys.exit(2)
