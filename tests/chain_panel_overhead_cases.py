"""
The cases of tests/test_chain_panel_overhead_gpu.py, shared with scripts/gen_chain_panel_overhead_fixture.py (which
records what a build of the PARENT commit computes for them).  They force what the panel overhead of the chain kernel's
factoring (rs_factor, chain_rs_inverse.h: the panel loads without a test on the row, the mask of available rows carried
from panel to panel, the pivot tables stored once per panel) could get wrong and the other records leave to chance:

  plain    a random lead: the narrow last panel (n_c = 50: 2 columns, 35: 3, 19: 3, 20: 4) and the one-panel systems
           (n_c = 8 and (8, 5)) store their tables under a lane mask that is new for both;
  spill    the LEFT lead's coupling blocks scaled by 2^520: its first inverse is finite, its first sweep overflows and the
           iterate is Inf / NaN from there on, so the rows of the work matrix behind row n -- the old iterate's slots
           where three workgroups share a compute unit -- feed non-finite values into the lanes the panel loads no longer
           zero.  The right lead of the same launch is untouched and stays finite;
  tiny     the left lead scaled by 2^-400: finite results of the order 2^400, the spare lanes overflow on their own;
  zc0/zcm/zcl  a column that is zero in every row (no usable key: the step takes the lowest available row), in the first,
           a middle and the last panel: the pivot tables written late must come out as the parent's.

Every kind runs at n_c = 50 and 35 (the stage schedule), 19 (the generic loop with a remainder strip), 20 (a generic class
with fewer than 64 rows), (19, 9) and (50, 40) (contacts of unequal size), 64 (no spare row), 8 and (8, 5) (one panel),
3 to 5 forced sweeps, three energies -- in the plain launch and, with 4 slots for the 6 fixed points and a quantum of 2
sweeps, in the round-robin instantiation, where every fixed point is set aside and resumed (the carried mask starts
afresh with every inverse).

A record holds per case the sweep counts, the flags and the SHA-256 digest of every Sigma block.  NaNs are brought to one
bit pattern first (which operand's payload a fused multiply-add hands on is the compiler's operand order, not
arithmetic), so equal digests <=> array_equal with the NaN positions.
"""
import hashlib

import numpy as np

from helpers import chain_lead, random_system

ETA = 1e-4
ES = np.array([0.3, 0.1 + 0.2j, -0.7])
KINDS = ["plain", "spill", "tiny", "zc0", "zcm", "zcl"]
SIZES = [(50, 50, 4), (35, 35, 3), (19, 19, 5), (20, 20, 4), (19, 9, 4), (50, 40, 3), (64, 64, 3), (8, 8, 5), (8, 5, 4)]
MODES = {"plain": (0, 0), "rr": (2, 4)}             # set_chain_round_robin(quantum, slots)


def cases():
    return [(ncL, ncR, fi, kind, mode) for ncL, ncR, fi in SIZES for kind in KINDS for mode in MODES]


def key(ncL, ncR, kind, mode):
    return f"po_{ncL}_{ncR}_{kind}_{mode}"


def lead(nc, seed, kind, left):
    alpha, Salpha, beta, Sbeta = (x.copy() for x in chain_lead(nc, seed))
    if kind == "spill" and left:
        beta, Sbeta = beta * 2.0 ** 520, Sbeta * 2.0 ** 520
    elif kind == "tiny" and left:
        f = 2.0 ** -400
        alpha, Salpha, beta, Sbeta = alpha * f, Salpha * f, beta * f, Sbeta * f
    elif kind in ("zc0", "zcm", "zcl"):
        npan = (nc + 7) // 8
        c = {"zc0": min(3, nc - 1), "zcm": min(8 * (npan // 2) + 3, nc - 1), "zcl": nc - 1}[kind]
        alpha[:, c] = 0.0; Salpha[:, c] = 0.0
    return alpha, Salpha, beta, Sbeta


def provider(ncL, ncR, kind):
    from gaunegf_amd.surfG1D import surfG
    seed = 1700 + 64 * ncL + ncR
    N = ncL + ncR + 7
    F, S = random_system(N, seed)
    inds = [list(range(ncL)), list(range(N - ncR, N))]
    aL, aR = lead(ncL, seed + 1, kind, True), lead(ncR, seed + 2, kind, False)
    kw = dict(taus=[aL[2].copy(), aR[2].copy()], staus=[aL[3].copy(), aR[3].copy()], alphas=[aL[0], aR[0]],
              aOverlaps=[aL[1], aR[1]], betas=[aL[2], aR[2]], bOverlaps=[aL[3], aR[3]], eta=ETA)
    return surfG(F, S, inds, **kw), inds


def canonical(b):
    """The block with every NaN brought to one bit pattern (real and imaginary parts on their own)."""
    v = np.ascontiguousarray(b).view(np.float64).copy()
    v[np.isnan(v)] = np.nan
    return v.view(np.complex128)


def run(engine, ncL, ncR, force_iters, kind, mode):
    """([energy][contact] Sigma blocks, NaNs canonical; sweep counts; flags), every evaluation running its fixed points"""
    engine.set_chain_round_robin(*MODES[mode])
    g, inds = provider(ncL, ncR, kind)
    g.force_iters = force_iters
    sig, its, cv = g.sigma_batch(ES)
    return [[canonical(s[np.ix_(i, i)]) for i in inds] for s in sig], its, cv


def digests(blk):
    """uint8 [energies, contacts, 32]"""
    return np.array([[np.frombuffer(hashlib.sha256(b.tobytes()).digest(), np.uint8) for b in row] for row in blk])


def finite(blk):
    """bool [energies, contacts]: the block holds finite values only"""
    return np.array([[bool(np.all(np.isfinite(b.view(np.float64)))) for b in row] for row in blk])
