"""
The three phases around the inverse in the chain fixed-point kernel (k_chain1d_rs.hip: the streamed B operand of both
products, the M = A - T B^H stores, the mixing step) against what the commit before they were reworked computed:
tests/golden/chain_phases_parent.npz, recorded on the GPU by scripts/gen_chain_phases_fixture.py from a build of that
commit.  The rework keeps the arithmetic of every element, so Sigma, the sweep counts and the convergence flags are
compared bit for bit (the Sigma blocks through their SHA-256 digests, and in full where the record keeps them):
  * equal contacts at every pitch class and on both sides of every class boundary, contacts of unequal size (the
    guarded class, n differing per job of one launch), two energies (one complex), 0 / 1 / 3 forced sweeps;
  * n_c = 50, eta = 1e-4 free-running on 8 energies: units that stop on the test and units that reach the cap;
  * within this build: the same grid with every job set aside and resumed (round robin, 5 slots, quantum 7) and
    through the g(E) cache (fill, then hit) equals the plain cold launch;
  * a NaN lead at (50, 50) is reported and contained (the property of test_chain_halftile_gpu.py).
"""
import os

import numpy as np
import pytest

import chain_phases_cases as cs
from helpers import chain_lead

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_phases_parent.npz")


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


@pytest.fixture(scope="module")
def free_plain(engine):
    """The free-running grid by the plain cold launch of this build, computed once."""
    engine.set_chain_cache(0); engine.set_chain_round_robin(0, 0)
    try:
        return cs.run_free()
    finally:
        engine.set_chain_round_robin(-1, 0); engine.set_chain_cache(512)


def _same(blk, blk0):
    return all(np.array_equal(b, b0) for row, row0 in zip(blk, blk0) for b, b0 in zip(row, row0))


@pytest.mark.parametrize("force_iters", cs.FORCE)
@pytest.mark.parametrize("ncL,ncR", cs.sizes())
def test_fixed_sweeps_equal_parent(cold, parent, ncL, ncR, force_iters):
    blk, its, cv = cs.run_fixed(ncL, ncR, force_iters)
    k = cs.key_fixed(ncL, ncR, force_iters)
    assert np.array_equal(its, parent[k + "_it"]) and np.array_equal(cv, parent[k + "_cv"])
    assert np.all(its == force_iters)
    assert np.array_equal(cs.digests(blk), parent[k + "_sha"]), k
    if (ncL, ncR, force_iters) in cs.FULL_FIXED:
        for m, row in enumerate(blk):
            for c, b in enumerate(row):
                assert np.array_equal(b, parent[f"{k}_blk_{m}_{c}"]), (k, m, c)


def test_free_running_equal_parent(free_plain, parent):
    blk, its, cv = free_plain
    pit, pcv = parent["free_it"], parent["free_cv"]
    assert (pcv == 1).any() and ((pcv == 0) & (pit == pit.max())).any()     # both kinds of unit are in the record
    assert np.array_equal(its, pit) and np.array_equal(cv, pcv)
    assert np.array_equal(cs.digests(blk), parent["free_sha"])
    for m in parent["free_full"]:
        for c in (0, 1):
            assert np.array_equal(blk[m][c], parent[f"free_blk_{m}_{c}"]), (m, c)


def test_resumed_jobs_equal_plain_launch(cold, free_plain):
    """Round robin on 5 slots with a quantum of 7 sweeps: every job is set aside and resumed, its old iterate rebuilt
    from the work matrix."""
    cold.set_chain_round_robin(7, 5)
    blk, its, cv = cs.run_free()
    assert np.array_equal(its, free_plain[1]) and np.array_equal(cv, free_plain[2])
    assert _same(blk, free_plain[0])


def test_cache_fill_and_hit_equal_cold(cold, free_plain):
    cold.set_chain_cache(512)
    cold.chain_cache_clear()
    for what in ("fill", "hit"):
        blk, its, cv = cs.run_free()
        assert np.array_equal(its, free_plain[1]) and np.array_equal(cv, free_plain[2]), what
        assert _same(blk, free_plain[0]), what
    assert cold.chain_cache_stats()["hits"] >= 1


def _nonfinite(x):
    return ~(np.isfinite(x.real) & np.isfinite(x.imag))


def test_nan_lead_is_reported_and_contained(cold):
    nc = 50
    good = (chain_lead(nc, 801), chain_lead(nc, 802))
    alpha = good[1][0].copy(); alpha[1, 2] = np.nan
    bad = (good[0], (alpha, good[1][1], good[1][2], good[1][3]))
    E = np.array([-0.8, 0.3, 0.1 + 0.2j, 1.1])
    g_bad, inds = cs.provider(nc, nc, 800, leads=bad)
    s_bad, it_bad, cv_bad = g_bad.sigma_batch(E)
    g_good, _ = cs.provider(nc, nc, 800, leads=good)
    s_good, it_good, cv_good = g_good.sigma_batch(E)
    i0, i1 = np.ix_(inds[0], inds[0]), np.ix_(inds[1], inds[1])
    for m in range(E.size):
        assert int(cv_bad[m, 1]) == 0 and np.all(_nonfinite(s_bad[m][i1])), m
        assert np.array_equal(s_bad[m][i0], s_good[m][i0]), m
        assert np.all(np.isfinite(s_good[m]))
    assert np.array_equal(it_bad[:, 0], it_good[:, 0]) and np.array_equal(cv_bad[:, 0], cv_good[:, 0])
