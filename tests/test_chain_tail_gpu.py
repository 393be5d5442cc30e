"""The chain's own inverse of its block's last diagonal tile (PGF_CHAIN_TAIL, GPU).

With helper workgroups the diagonal chain of the dense LDL^T inverts the last full 64 x 64 tile
of its 256-column block itself, from its LDS, instead of handing it to helper I; a ragged last
tile stays with the helper, and the path without helpers is untouched.  The switches are read
once per process, so every variant runs in a child process (this file with a command): it drives
HipLinearSolver on the seeded quasi-definite matrices of tools/check_factor.py at the smallest
sizes that reach each case and leaves solutions and inertias in a file.  Checked here:
  * every variant against numpy.linalg.solve and numpy's inertia, with check_factor.py's bars;
  * PGF_CHAIN_TAIL=1 against PGF_CHAIN_TAIL=0 bit for bit (the inverse is the same arithmetic),
    with the chain inside the fused launches and as a launch of its own (PGF_FUSED=0);
  * a device batch of three instances with reduced size 320 against the same one by one.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N -> (n1, n2) of check_factor.py's sqd(): positive definite n1 x n1, -0.5 I of n2
#   64 .. 256  one block of 1 .. 4 sub-panels, the last tile full
#   257        the second block is a single column: ragged, helper I's
#   100, 300   ragged last tiles (36 and 44 columns)
#   320        256 + 64: the chain's inverse of block 0's tile 3 feeds T(0) and block 1's own
#   576        256 + 256 + 64
#   833        four blocks, the last one ragged
SIZES = {64: (48, 16), 128: (96, 32), 192: (150, 42), 256: (200, 56), 257: (200, 57), 100: (70, 30),
         300: (213, 87), 320: (250, 70), 576: (450, 126), 833: (650, 183)}
ERR_BAR = 1e-11  # tools/check_factor.py: max |sol - ref| / max(1, max |ref|) < 1e-11

VARIANTS = {
    "chain_tail": {"PGF_CHAIN_TAIL": "1"},
    "helper_tail": {"PGF_CHAIN_TAIL": "0"},
    "chain_tail_unfused": {"PGF_CHAIN_TAIL": "1", "PGF_FUSED": "0"},
    "helper_tail_unfused": {"PGF_CHAIN_TAIL": "0", "PGF_FUSED": "0"},
    "no_helpers": {"PGF_CHAIN_HELP": "0"},
}


def sqd(rng, n1, n2):  # tools/check_factor.py
    G1 = rng.standard_normal((n1, n1)) / np.sqrt(max(n1, 1))
    A = G1 @ G1.T + np.eye(n1)
    B = rng.standard_normal((n2, n1)) / np.sqrt(max(n1, 1))
    return np.block([[A, B.T], [B, -0.5 * np.eye(n2)]])


def system(N):
    n1, n2 = SIZES[N]
    rng = np.random.default_rng(n1 * 1000 + n2)
    K = sqd(rng, n1, n2)
    return K, rng.standard_normal(n1 + n2)


# ------------------------------------------------------------------ child process
def child_solver(out):
    sys.path.insert(0, REPO)
    import pygradflow_amd as pgf

    res = {}
    for N in SIZES:
        K, rhs = system(N)
        sv = pgf.HipLinearSolver(K, symmetric=True)
        res[f"sol{N}"] = np.asarray(sv.solve(rhs), dtype=np.float64)
        res[f"neg{N}"] = np.int64(sv.num_neg_eigvals())
        sv.close()
    np.savez(out, **res)
    print("chain tail child ok", flush=True)


def child_batch():
    sys.path.insert(0, REPO)
    from pygradflow_amd import problems
    from pygradflow_amd.batched import BatchedDeviceNewton

    def make(i):  # unbounded, m = 0: the reduced matrix is H + lambda I of size 320 = 256 + 64
        return problems.dense_qp(320, 0, seed=300 + i)

    a = BatchedDeviceNewton(make, 3, "Full", 1.0, 1.0)
    b = BatchedDeviceNewton(make, 3, "Full", 1.0, 1.0, sequential=True)
    for k in range(2):
        ra, rb = a.step().cpu().numpy(), b.step().cpu().numpy()
        assert np.allclose(ra, rb, rtol=1e-9, atol=1e-12), k
    xa, _ = a.points()
    xb, _ = b.points()
    err = np.max(np.abs(xa - xb)) / max(1.0, np.max(np.abs(xb)))
    print(f"batch vs one-by-one {err:.2e}", flush=True)
    assert err <= 1e-11, err  # tools/check_batch.py's bar
    a.close()
    b.close()
    print("chain tail batch ok", flush=True)


# ------------------------------------------------------------------ tests
def _child(args, extra_env):
    env = dict(os.environ)
    for k in ("PGF_CHAIN_TAIL", "PGF_CHAIN_HELP", "PGF_FUSED"):
        env.pop(k, None)
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, cwd=REPO,
                          capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def variant_results(tmp_path_factory):
    """name -> {sol<N>, neg<N>} of one child process per variant, run on first use"""
    cache = {}
    d = tmp_path_factory.mktemp("chain_tail")

    def get(name):
        if name not in cache:
            out = str(d / f"{name}.npz")
            r = _child(["solver", out], VARIANTS[name])
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert "chain tail child ok" in r.stdout
            with np.load(out) as z:
                cache[name] = {k: z[k] for k in z.files}
        return cache[name]

    return get


@pytest.fixture(scope="module")
def references():
    """N -> (numpy's solution, numpy's count of negative eigenvalues), computed once"""
    ref = {}
    for N in SIZES:
        K, rhs = system(N)
        ref[N] = (np.linalg.solve(K, rhs), int(np.sum(np.linalg.eigvalsh(K) < 0.0)))
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("N", sorted(SIZES))
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variant_agrees_with_numpy(gpu_available, variant_results, references, name, N):
    if not gpu_available:
        pytest.skip("needs a GPU")
    got = variant_results(name)
    ref, neg = references[N]
    assert neg == SIZES[N][1]
    err = np.max(np.abs(got[f"sol{N}"] - ref)) / max(1.0, np.max(np.abs(ref)))
    print(f"{name} N={N}: err={err:.2e} n_neg={int(got[f'neg{N}'])} (numpy {neg})")
    assert int(got[f"neg{N}"]) == neg
    assert err < ERR_BAR, (name, N, err)


@pytest.mark.gpu
@pytest.mark.parametrize("N", sorted(SIZES))
@pytest.mark.parametrize("pair", [("chain_tail", "helper_tail"), ("chain_tail_unfused", "helper_tail_unfused")],
                         ids=["fused", "unfused"])
def test_chain_tail_is_bit_identical_to_the_helper(gpu_available, variant_results, pair, N):
    if not gpu_available:
        pytest.skip("needs a GPU")
    a, b = variant_results(pair[0]), variant_results(pair[1])
    assert int(a[f"neg{N}"]) == int(b[f"neg{N}"])
    sa, sb = a[f"sol{N}"], b[f"sol{N}"]
    assert sa.shape == sb.shape and sa.tobytes() == sb.tobytes(), (N, np.max(np.abs(sa - sb)))


@pytest.mark.gpu
def test_batch_of_reduced_size_320_matches_one_by_one(gpu_available):
    if not gpu_available:
        pytest.skip("needs a GPU")
    r = _child(["batch"], {})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "chain tail batch ok" in r.stdout


if __name__ == "__main__":
    if sys.argv[1] == "solver":
        child_solver(sys.argv[2])
    elif sys.argv[1] == "batch":
        child_batch()
    else:
        sys.exit(2)
