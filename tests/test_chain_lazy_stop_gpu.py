"""
The stopping test of the chain fixed-point kernel (k_chain1d_rs.hip, gather_mix) run by wave -- slot 0 of every
lane first, the other slots only when no lane of the wave is over on it -- and the pinned arithmetic of the mixing step
and of the stage schedule's factoring, against what the commit before them computed:
tests/golden/chain_lazy_stop_parent.npz, recorded on the GPU by scripts/gen_chain_lazy_stop_fixture.py from a build of
that commit.  No operation on any element changes, so Sigma (through the SHA-256 digests of its blocks), the sweep
counts and the convergence flags are compared bit for bit:
  * n_c = 9 (one slot per lane), 19, 25, 35, 50, 51, 64 and the unequal pair (50, 40); four energies, two of them real;
    conv = 1e-1, 1e-2, 1e-5 -- fixed points that stop on the test after tens or hundreds of sweeps, and some at the cap;
  * the same through the round robin (5 slots, quantum 7: every job set aside and resumed) and through the g(E)
    cache (fill, then hit).
The generator asserts on the numpy oracle's iterates that the cases hold a sweep in which one wave passes on slot 0
while another element of the workgroup fails, and that a unit of every size class stops on the test below the cap.
"""
import os

import numpy as np
import pytest

import chain_lazy_stop_cases as lz
import chain_phases_cases as cs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_lazy_stop_parent.npz")


@pytest.fixture(scope="module")
def parent():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture
def cold(engine):
    engine.set_chain_cache(0)                      # every evaluation runs its fixed points
    engine.set_chain_round_robin(-1, 0)
    yield engine
    engine.set_chain_round_robin(-1, 0)
    engine.set_chain_cache(512)


def _check(parent, ncL, ncR, ci, what):
    blk, its, cv = lz.run(ncL, ncR, ci)
    k = lz.key(ncL, ncR, ci)
    print(what, k, "sweeps", its.ravel().tolist(), "flags", cv.ravel().tolist())
    assert np.array_equal(its, parent[k + "_it"]) and np.array_equal(cv, parent[k + "_cv"]), (what, k)
    assert np.array_equal(cs.digests(blk), parent[k + "_sha"]), (what, k)


def test_record_holds_units_that_stop_on_the_test(parent):
    for ncL, ncR in lz.SIZES:
        assert any(((parent[lz.key(ncL, ncR, ci) + "_cv"] == 1) & (parent[lz.key(ncL, ncR, ci) + "_it"] < lz.MAX_ITER)).any()
                   for ci in range(len(lz.CONVS))), (ncL, ncR)


@pytest.mark.parametrize("ncL,ncR,ci", lz.cases())
def test_plain_launch_equals_parent(cold, parent, ncL, ncR, ci):
    _check(parent, ncL, ncR, ci, "plain")


@pytest.mark.parametrize("ncL,ncR,ci", lz.cases())
def test_round_robin_equals_parent(cold, parent, ncL, ncR, ci):
    cold.set_chain_round_robin(7, 5)
    _check(parent, ncL, ncR, ci, "round robin")


@pytest.mark.parametrize("ncL,ncR,ci", lz.cases())
def test_cache_fill_and_hit_equal_parent(cold, parent, ncL, ncR, ci):
    cold.set_chain_cache(512)
    cold.chain_cache_clear()
    _check(parent, ncL, ncR, ci, "fill")
    _check(parent, ncL, ncR, ci, "hit")
    assert cold.chain_cache_stats()["hits"] >= 1
