"""
What the library computes does not depend on the environment variables it no longer reads.  This process computes the
cases of tests/env_retired_cases.py with a clean environment; one child process computes them with every retired
variable set to the value that used to change the most (NEGF_GJ_DEBUG=32 and NEGF_GJ_STRIP_DBG=15: wrong-result
ablations; other window kernels, the vector-unit products, the element form of the permuted accumulate, the eager
gather, the blocking wait, no round robin).  Outputs and info are compared with np.array_equal; the launch masks show
that each case ran the kernel it is there for, in both processes:
  * n = 40, negf_set_inverse_algo(2): the single-workgroup blocked kernel, through gr_batch;
  * n = 72, negf_set_inverse_algo(3): the strip kernel over two windows -- gr_batch (the gather), gr_int (the deferred
    gather and the permuted accumulate), gless_int (the products);
  * n = 300, the automatic rule: the look-ahead window kernel, through gr_int.
A constant-Sigma provider with two contacts, six energies, one of them complex.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import env_retired_cases as rc

pytestmark = pytest.mark.gpu

CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "env_retired_cases.py")


@pytest.fixture(scope="module")
def clean(engine):
    assert not any(k in os.environ for k in rc.RETIRED)
    return rc.run_gpu(engine)


@pytest.fixture(scope="module")
def with_retired(tmp_path_factory):
    """the same by a fresh process with every retired variable set"""
    out = str(tmp_path_factory.mktemp("env_retired") / "gpu.npz")
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), CASES, "gpu", out]
    r = subprocess.run(cmd, env={**os.environ, **rc.RETIRED}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with np.load(out, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("n,algo,calls,bit", rc.GPU_CASES, ids=[f"n{c[0]}" for c in rc.GPU_CASES])
def test_retired_variables_change_nothing(clean, with_retired, n, algo, calls, bit):
    for call in calls:
        k = f"{call}_{n}"
        a, b = clean[k], with_retired[k]
        assert np.all(np.isfinite(a.view(np.float64))) and np.any(a != 0), k
        assert np.all(clean[k + "_info"] == 0), k
        for side in (clean, with_retired):
            masks = side[k + "_masks"]
            assert masks.size >= 1 and all(int(m) >> bit & 1 for m in masks), (k, masks.tolist())
        assert np.array_equal(clean[k + "_masks"], with_retired[k + "_masks"]), k
        assert np.array_equal(clean[k + "_info"], with_retired[k + "_info"]), k
        assert a.shape == b.shape and np.array_equal(a, b), f"{k}: max |difference| {np.max(np.abs(a - b)):.3e}"
