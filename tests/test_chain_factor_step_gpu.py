"""
The column step of the chain kernel's panel factoring (rs_factor, chain_rs_inverse.h) against what the commit before
it was made leaner computed: tests/golden/chain_factor_step_parent.npz, recorded on the GPU by
scripts/gen_chain_factor_step_fixture.py from a build of that commit.  The leaner step keeps every FP64 operation and
the pivot choice, so Sigma, the sweep counts and the flags are compared bit for bit, NaN positions included, on the
cases the other records do not force (tests/chain_factor_step_cases.py): pivot ties within the high word of the key, a
column that is zero in every available row, a NaN and an Inf in a pivot row, leads scaled by 2^64 and 2^-64 -- at
n_c = 50, 35, 19 and (19, 9), 3 to 5 forced sweeps.  (The Sigma entry point returns sweep counts and flags; it has no
further info word.)
"""
import os

import numpy as np
import pytest

import chain_factor_step_cases as cs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_factor_step_parent.npz")


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


@pytest.mark.parametrize("ncL,ncR,force_iters,kind", cs.cases())
def test_factor_step_equals_parent(cold, parent, ncL, ncR, force_iters, kind):
    blk, its, cv = cs.run(ncL, ncR, force_iters, kind)
    k = cs.key(ncL, ncR, kind)
    assert np.array_equal(its, parent[k + "_it"]) and np.array_equal(cv, parent[k + "_cv"]), k
    assert np.all(its == force_iters)
    assert np.array_equal(cs.digests(blk), parent[k + "_sha"]), k
    if (ncL, ncR) in cs.FULL:
        for m, row in enumerate(blk):
            for c, b in enumerate(row):
                assert np.array_equal(b, parent[f"{k}_blk_{m}_{c}"], equal_nan=True), (k, m, c)


def test_the_record_holds_what_it_is_for(parent):
    """The forced cases did what they were written for when the record was taken: the singular and the non-finite
    ones are reported (flag 0) with non-finite values, the tie and the scaled ones stay finite."""
    for ncL, ncR in cs.FULL:
        for kind in cs.KINDS:
            k = cs.key(ncL, ncR, kind)
            vals = np.concatenate([parent[f"{k}_blk_{m}_{c}"].view(np.float64).ravel() for m in range(cs.ES.size) for c in (0, 1)])
            if kind in ("zerocol", "nan", "inf"):
                assert not np.all(np.isfinite(vals)), k
            else:
                assert np.all(np.isfinite(vals)), k
