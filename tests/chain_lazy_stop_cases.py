"""
The cases of tests/test_chain_lazy_stop_gpu.py, shared with scripts/gen_chain_lazy_stop_fixture.py (which records what
a build of the PARENT commit computes for them): free-running fixed points of the 1-D chain kernel that STOP ON THE
TEST -- the stopping test of the mixing step decides their sweep counts and flags, and through them every bit of Sigma.

Per case (a pair of contact sizes and a tolerance) one launch of four energies x two contacts; the record holds the
sweep counts, the flags and the SHA-256 digest of every Sigma block's bytes (chain_phases_cases.digests).
"""
import numpy as np

import chain_phases_cases as cs

# one slot per lane (9: the test by wave is trivially the full one), every pitch class with a remainder strip and their
# neighbours, the 2-per-CU class, and contacts of unequal size (the guarded class, n differing per job of one launch)
SIZES = [(9, 9), (19, 19), (25, 25), (35, 35), (50, 50), (51, 51), (64, 64), (50, 40)]
ES = np.concatenate([cs.ES, [-1.2, 0.7]])           # the two of chain_phases_cases and two on the real axis
CONVS = [1e-1, 1e-2, 1e-5]                          # units stop after a few, tens, a hundred and more sweeps (or reach the cap)
MAX_ITER = 2000


def cases():
    return [(ncL, ncR, ci) for ncL, ncR in SIZES for ci in range(len(CONVS))]


def key(ncL, ncR, ci):
    return f"lz_{ncL}_{ncR}_{ci}"


def seed_of(ncL, ncR):
    return 9100 + 64 * ncL + ncR


def leads(ncL, ncR):
    from helpers import chain_lead
    s = seed_of(ncL, ncR)
    return chain_lead(ncL, s + 1), chain_lead(ncR, s + 2)


def run(ncL, ncR, ci):
    """(blocks [energy][contact], sweep counts, flags) of a fresh provider"""
    g, inds = cs.provider(ncL, ncR, seed_of(ncL, ncR), leads=leads(ncL, ncR))
    sig, its, cv = g.sigma_batch(ES, conv=CONVS[ci])
    return cs.blocks(sig, inds), its, cv
