"""
The cases of tests/test_chain_factor_step_gpu.py, shared with scripts/gen_chain_factor_step_fixture.py (which records
what a build of the PARENT commit computes for them).  They force what the column step of the chain kernel's panel
factoring (rs_factor, chain_rs_inverse.h) decides and the other records leave to chance.  The first sweep inverts
A = (E + i eta) S_alpha - alpha, so the lead blocks are written such that A has

  tie      in column 0 two rows whose |re| + |im| agree in the high word and differ below it, the LARGER in the higher
           row, far apart in the wave (the search takes the lower row), every other entry of the column small;
  tie3     the same with three rows, two of them exactly equal;
  zerocol  a column that is zero in every row: when its step comes no row has a usable key and the step takes the
           lowest row that is still available (the inverse is singular from there on: non-finite values, reported);
  nan/inf  a NaN / an Inf entry in the row that becomes the pivot of column 0, in a column of the second panel (of the
           first one for the 9-row contact);
  up/down  all four lead blocks scaled by 2^64 / 2^-64.

Every kind runs at n_c = 50 and 35 (the stage schedule), 19 (the generic loop with a remainder strip) and (19, 9)
(contacts of unequal size), with 3 to 5 forced sweeps, at one real and one complex energy.

A record holds per case the sweep counts, the flags and the SHA-256 digest of every Sigma block; the blocks of the two
small sizes are kept in full.  NaNs are brought to one bit pattern first (which operand's payload a fused multiply-add
hands on is the compiler's operand order, not arithmetic), so equal digests <=> array_equal with the NaN positions.
"""
import hashlib

import numpy as np

from helpers import chain_lead, random_system

ETA = 1e-4
ES = np.array([0.3, 0.1 + 0.2j])
KINDS = ["tie", "tie3", "zerocol", "nan", "inf", "up", "down"]
SIZES = [(50, 50, 4), (35, 35, 3), (19, 19, 5), (19, 9, 4)]         # (ncL, ncR, forced sweeps)
FULL = [(19, 19), (19, 9)]                                           # sizes whose blocks are kept in full


def cases():
    return [(ncL, ncR, fi, kind) for ncL, ncR, fi in SIZES for kind in KINDS]


def key(ncL, ncR, kind):
    return f"fs_{ncL}_{ncR}_{kind}"


def lead(nc, seed, kind):
    alpha, Salpha, beta, Sbeta = (x.copy() for x in chain_lead(nc, seed))
    lo, hi = 2, nc - 3                              # two rows far apart in the wave
    late = 11 if nc > 16 else 5                     # a column of the second panel (nc = 9: of the first)
    if kind in ("tie", "tie3"):
        alpha[:, 0] *= 2.0 ** -6; Salpha[:, 0] = 0.0
        alpha[lo, 0] = 4.0; alpha[hi, 0] = 4.0 * (1.0 + 2.0 ** -30)
        if kind == "tie3":
            alpha[nc // 2, 0] = 4.0
    elif kind == "zerocol":
        alpha[:, late] = 0.0; Salpha[:, late] = 0.0
    elif kind in ("nan", "inf"):
        alpha[4, 0] = 6.0                            # row 4 becomes the pivot of column 0
        alpha[4, late] = np.nan if kind == "nan" else np.inf
    elif kind in ("up", "down"):
        f = 2.0 ** 64 if kind == "up" else 2.0 ** -64
        alpha, Salpha, beta, Sbeta = alpha * f, Salpha * f, beta * f, Sbeta * f
    else:
        raise ValueError(kind)
    return alpha, Salpha, beta, Sbeta


def provider(ncL, ncR, kind):
    from gaunegf_amd.surfG1D import surfG
    seed = 900 + 64 * ncL + ncR
    N = ncL + ncR + 7
    F, S = random_system(N, seed)
    inds = [list(range(ncL)), list(range(N - ncR, N))]
    aL, aR = lead(ncL, seed + 1, kind), lead(ncR, seed + 2, kind)
    kw = dict(taus=[aL[2].copy(), aR[2].copy()], staus=[aL[3].copy(), aR[3].copy()], alphas=[aL[0], aR[0]],
              aOverlaps=[aL[1], aR[1]], betas=[aL[2], aR[2]], bOverlaps=[aL[3], aR[3]], eta=ETA)
    return surfG(F, S, inds, **kw), inds


def canonical(b):
    """The block with every NaN brought to one bit pattern (real and imaginary parts on their own)."""
    v = np.ascontiguousarray(b).view(np.float64).copy()
    v[np.isnan(v)] = np.nan
    return v.view(np.complex128)


def run(ncL, ncR, force_iters, kind):
    """([energy][contact] Sigma blocks, NaNs canonical; sweep counts; flags)"""
    g, inds = provider(ncL, ncR, kind)
    g.force_iters = force_iters
    sig, its, cv = g.sigma_batch(ES)
    return [[canonical(s[np.ix_(i, i)]) for i in inds] for s in sig], its, cv


def digests(blk):
    """uint8 [energies, contacts, 32]"""
    return np.array([[np.frombuffer(hashlib.sha256(b.tobytes()).digest(), np.uint8) for b in row] for row in blk])
