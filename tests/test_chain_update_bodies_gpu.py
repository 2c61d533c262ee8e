"""
The update bodies of the chain kernel's stage schedule (chain_rs_inverse.h: rs_job_whole, rs_job_half, rs_job_strip, the row
strip and the look-ahead) against what the commit before they were cut computed: tests/golden/chain_update_bodies_parent.npz,
recorded on the GPU by scripts/gen_chain_update_bodies_fixture.py from a build of that commit.  The bodies now read the
pivot rows as element offsets from a second table the factoring wave stores beside the row numbers, and take their lane
bases from one set made at the top of every inverse; no FP64 operation, operand or order changed, so Sigma, the sweep counts
and the flags are compared bit for bit, NaN positions included, on the cases of tests/chain_update_bodies_cases.py: a zero
column in the first, a middle and the last panel, a pivot permutation that is not the identity in any panel, leads scaled by
2^+-64, plain and round robin (every fixed point set aside and resumed), at n_c = 50, 35, 19, (19, 9), (50, 40), 64 and 20,
3 to 5 forced sweeps.
"""
import os

import numpy as np
import pytest

import chain_update_bodies_cases as cs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_update_bodies_parent.npz")


@pytest.fixture(scope="module")
def parent():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture
def cold(engine):
    engine.set_chain_cache(0)                      # every evaluation runs its fixed points
    yield engine
    engine.set_chain_round_robin(-1, 0)
    engine.set_chain_cache(512)


@pytest.mark.gpu
@pytest.mark.parametrize("ncL,ncR,force_iters,kind,mode", cs.cases())
def test_update_bodies_equal_parent(cold, parent, ncL, ncR, force_iters, kind, mode):
    blk, its, cv = cs.run(cold, ncL, ncR, force_iters, kind, mode)
    k = cs.key(ncL, ncR, kind, mode)
    assert np.array_equal(its, parent[k + "_it"]) and np.array_equal(cv, parent[k + "_cv"]), k
    assert np.all(its == force_iters)
    assert np.array_equal(cs.finite(blk), parent[k + "_fin"]), k
    assert np.array_equal(cs.digests(blk), parent[k + "_sha"]), k


def test_the_permuted_lead_pivots_outside_every_panel():
    """The construction of the `perm` kind: in every column j of A = z S - alpha the entry in row (j + 11) mod n outweighs
    the rest of the column together, so the first inverse takes that row for column j -- for every size used here a row
    outside the panel of column j (or, in the 9-row contact, not row j)."""
    for ncL, ncR, _ in cs.SIZES:
        _, sL, sR = cs.seeds(ncL, ncR)
        for nc, seed in ((ncL, sL), (ncR, sR)):
            assert cs.dominance(nc, seed) > 2.0, (nc, seed)
            s = cs.SHIFT % nc
            assert s != 0 and (nc < 16 or (s >= 8 and nc - s >= 8)), nc


def test_the_record_holds_what_it_is_for(parent):
    """The forced cases did what they were written for when the record was taken: the singular columns are reported with
    non-finite values, every other kind stays finite; and the round robin computed what the plain launch did."""
    for ncL, ncR, _ in cs.SIZES:
        for kind in cs.KINDS:
            fin = parent[cs.key(ncL, ncR, kind, "plain") + "_fin"]
            if kind in ("zc0", "zcm", "zcl"):
                assert not fin.all(), (ncL, ncR, kind)
            else:
                assert fin.all(), (ncL, ncR, kind)
            for s in ("_sha", "_it", "_cv"):
                assert np.array_equal(parent[cs.key(ncL, ncR, kind, "rr") + s], parent[cs.key(ncL, ncR, kind, "plain") + s])
