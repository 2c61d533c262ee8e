"""
The cases of tests/test_chain_phases_gpu.py, shared with scripts/gen_chain_phases_fixture.py (which records what a
build of the PARENT commit computes for them): Sigma blocks of both contacts, sweep counts and convergence flags of the
1-D chain fixed-point kernel, to be reproduced bit for bit.

A record holds, per case, the sweep counts, the flags and the SHA-256 digest of every Sigma block's bytes (equal
digests <=> equal bits; the blocks of all cases together are 4.5 MB, the digests a few KB); the blocks themselves are
kept for the cases listed in FULL_FIXED and for one energy of the free-running grid.
"""
import hashlib

import numpy as np

from helpers import chain_lead, random_system

ETA = 1e-4
EQUAL = [9, 16, 17, 19, 25, 33, 35, 41, 48, 49, 50, 51, 57, 64]     # every pitch class, both sides of every boundary
UNEQUAL = [(50, 40), (35, 20), (19, 9)]                              # the guarded class; n differs per job in one launch
FORCE = [0, 1, 3]
ES = np.array([0.3, 0.1 + 0.2j])
FREE_NC = 50
FREE_E = np.linspace(-1.9, 1.9, 8)
FULL_FIXED = [(19, 19, 3), (50, 50, 3)]                              # (ncL, ncR, force_iters) whose blocks are kept in full


def sizes():
    return [(n, n) for n in EQUAL] + UNEQUAL


def provider(ncL, ncR, seed, leads=None, eta=ETA):
    """(a fresh chain provider, the two contacts' index lists)"""
    from gaunegf_amd.surfG1D import surfG
    N = ncL + ncR + 7
    F, S = random_system(N, seed)
    inds = [list(range(ncL)), list(range(N - ncR, N))]
    aL, aR = leads or (chain_lead(ncL, seed + 1), chain_lead(ncR, seed + 2))
    kw = dict(taus=[aL[2].copy(), aR[2].copy()], staus=[aL[3].copy(), aR[3].copy()], alphas=[aL[0], aR[0]],
              aOverlaps=[aL[1], aR[1]], betas=[aL[2], aR[2]], bOverlaps=[aL[3], aR[3]], eta=eta)
    return surfG(F, S, inds, **kw), inds


def blocks(sig, inds):
    """[energy][contact] -> the contact's Sigma block, C-contiguous"""
    return [[np.ascontiguousarray(s[np.ix_(i, i)]) for i in inds] for s in sig]


def digests(blk):
    """uint8 [energies, contacts, 32]"""
    return np.array([[np.frombuffer(hashlib.sha256(b.tobytes()).digest(), np.uint8) for b in row] for row in blk])


def seed_of(ncL, ncR):
    return 700 + 64 * ncL + ncR


def run_fixed(ncL, ncR, force_iters):
    g, inds = provider(ncL, ncR, seed_of(ncL, ncR))
    g.force_iters = force_iters
    sig, its, cv = g.sigma_batch(ES)
    return blocks(sig, inds), its, cv


def run_free():
    g, inds = provider(FREE_NC, FREE_NC, 55)
    sig, its, cv = g.sigma_batch(FREE_E)
    return blocks(sig, inds), its, cv


def key_fixed(ncL, ncR, force_iters):
    return f"fx_{ncL}_{ncR}_{force_iters}"
