"""
The panel overhead of the chain kernel's factoring (rs_factor, chain_rs_inverse.h) against what the commit before it was
cut computed: tests/golden/chain_panel_overhead_parent.npz, recorded on the GPU by
scripts/gen_chain_panel_overhead_fixture.py from a build of that commit.  The panel is now loaded without a test on the
row (the lanes behind row n carry whatever the work matrix holds there), the stage schedule carries the mask of available
rows from panel to panel instead of reading colof, and the pivot tables are stored once per panel; no FP64 operation and
no pivot choice changed, so Sigma, the sweep counts and the flags are compared bit for bit, NaN positions included, on
the cases of tests/chain_panel_overhead_cases.py: non-finite spare rows beside a finite contact, a singular column in the
first, a middle and the last panel, narrow last panels and one-panel systems, plain and round robin (every fixed point set
aside and resumed), at n_c = 50, 35, 19, 20, (19, 9), (50, 40), 64, 8 and (8, 5), 3 to 5 forced sweeps.

A panel with no available row is not among them because no call can reach it: an inverse of n rows runs n column steps,
every step with an available row takes exactly one out of the mask, so step k finds n - k >= 1 rows available.  (A step
without a pivot lane stores nothing in either table, before and after: the late stores are under "a row was recorded".)
"""
import os

import numpy as np
import pytest

import chain_panel_overhead_cases as cs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_panel_overhead_parent.npz")


@pytest.fixture(scope="module")
def parent():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture
def cold(engine):
    engine.set_chain_cache(0)                      # every evaluation runs its fixed points
    yield engine
    engine.set_chain_round_robin(-1, 0)
    engine.set_chain_cache(512)


@pytest.mark.parametrize("ncL,ncR,force_iters,kind,mode", cs.cases())
def test_panel_overhead_equals_parent(cold, parent, ncL, ncR, force_iters, kind, mode):
    blk, its, cv = cs.run(cold, ncL, ncR, force_iters, kind, mode)
    k = cs.key(ncL, ncR, kind, mode)
    assert np.array_equal(its, parent[k + "_it"]) and np.array_equal(cv, parent[k + "_cv"]), k
    assert np.all(its == force_iters)
    assert np.array_equal(cs.finite(blk), parent[k + "_fin"]), k
    assert np.array_equal(cs.digests(blk), parent[k + "_sha"]), k


def test_the_record_holds_what_it_is_for(parent):
    """The forced cases did what they were written for when the record was taken: the overflowing lead is non-finite at
    every energy while the other contact of the same launch stays finite, the singular columns are reported with
    non-finite values, the plain and the scaled ones stay finite; and the round robin computed what the plain launch did."""
    for ncL, ncR, _ in cs.SIZES:
        for kind in cs.KINDS:
            fin = parent[cs.key(ncL, ncR, kind, "plain") + "_fin"]
            if kind == "spill":
                assert not fin[:, 0].any() and fin[:, 1].all(), (ncL, ncR)
            elif kind in ("plain", "tiny"):
                assert fin.all(), (ncL, ncR, kind)
            else:
                assert not fin.all(), (ncL, ncR, kind)
            for s in ("_sha", "_it", "_cv"):
                assert np.array_equal(parent[cs.key(ncL, ncR, kind, "rr") + s], parent[cs.key(ncL, ncR, kind, "plain") + s])
