"""
The renormalisation-decimation kernel (k_chain1d_rd.hip) shares the small inverse of the fixed-point kernel
(chain_rs_inverse.h: rs_inverse, rs_factor, the update tiles), so a restructuring of that header must leave what it
computes as it was: tests/golden/chain_rd_parent.npz, recorded on the GPU by scripts/gen_chain_rd_parent_fixture.py from a
build of the commit before the header's settled build switches were retired.  Sigma (through the SHA-256 digests of its
blocks, chain_phases_cases.digests), the step counts and the convergence flags are compared bit for bit:
  * n_c = 9, 16, 19, 32, 35, 50, 64 -- both sides of every pitch class of the kernel (17, 33, 49, 65) -- and the unequal
    pair (50, 40);
  * the four energies of chain_lazy_stop_cases.ES (two of them on the real axis), free running, default tolerance.
"""
import os

import numpy as np
import pytest

import chain_lazy_stop_cases as lz
import chain_phases_cases as cs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_rd_parent.npz")
SIZES = [(9, 9), (16, 16), (19, 19), (32, 32), (35, 35), (50, 50), (64, 64), (50, 40)]


def key(ncL, ncR):
    return f"rd_{ncL}_{ncR}"


def run(ncL, ncR):
    """(blocks [energy][contact], step counts, flags) of a fresh provider with the doubling solver"""
    g, inds = cs.provider(ncL, ncR, lz.seed_of(ncL, ncR), leads=lz.leads(ncL, ncR))
    g.solver = "doubling"
    sig, its, cv = g.sigma_batch(lz.ES)
    return cs.blocks(sig, inds), its, cv


@pytest.fixture(scope="module")
def parent():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture
def cold(engine):
    engine.set_chain_cache(0)                      # every evaluation runs its decimation steps
    yield engine
    engine.set_chain_cache(512)


@pytest.mark.parametrize("ncL,ncR", SIZES)
def test_rd_equals_parent(cold, parent, ncL, ncR):
    blk, its, cv = run(ncL, ncR)
    k = key(ncL, ncR)
    print(k, "steps", its.ravel().tolist(), "flags", cv.ravel().tolist())
    assert np.array_equal(its, parent[k + "_it"]) and np.array_equal(cv, parent[k + "_cv"]), k
    assert np.array_equal(cs.digests(blk), parent[k + "_sha"]), k
