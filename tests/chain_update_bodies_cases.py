"""
The cases of tests/test_chain_update_bodies_gpu.py, shared with scripts/gen_chain_update_bodies_fixture.py (which records
what a build of the PARENT commit computes for them).  They force what the update bodies of the chain kernel's stage
schedule (chain_rs_inverse.h: the pivot table read as element offsets, the lane bases made once per inverse) could get
wrong and the other records leave to chance:

  plain    a random lead;
  zc0/zcm/zcl  a column that is zero in every row, in the first, a middle and the last panel: that step takes the lowest
           available row, and the offset table must hold it like the row table does;
  perm     alpha = 4 C + a small random part, C the cyclic shift by 11 rows: column j of A = z S - alpha is dominated by its
           entry in row (j + 11) mod n, which lies outside the panel of column j for every n used here, so the pivot
           permutation is not the identity in ANY panel and every Q fragment gathers rows scattered over the matrix
           (dominance() checks the construction on the host);
  up64/dn64  both leads scaled by 2^+64 / 2^-64.

Every kind runs at n_c = 50 and 35 (the stage schedule), 19 and 20 (the generic loop, with and without a remainder strip),
(19, 9) and (50, 40) (contacts of unequal size), 64 (no spare row), 3 to 5 forced sweeps, three energies -- in the plain
launch and, with 4 slots for the 6 fixed points and a quantum of 2 sweeps, in the round-robin instantiation, where every
fixed point is set aside and resumed.

A record holds per case the sweep counts, the flags and the SHA-256 digest of every Sigma block, NaNs brought to one bit
pattern first (chain_panel_overhead_cases.canonical), so equal digests <=> array_equal with the NaN positions.
"""
import numpy as np

from chain_panel_overhead_cases import ES, ETA, MODES, canonical, digests, finite  # noqa: F401
from helpers import chain_lead, random_system

KINDS = ["plain", "zc0", "zcm", "zcl", "perm", "up64", "dn64"]
SIZES = [(50, 50, 4), (35, 35, 3), (19, 19, 5), (19, 9, 4), (50, 40, 3), (64, 64, 3), (20, 20, 4)]
SHIFT = 11


def cases():
    return [(ncL, ncR, fi, kind, mode) for ncL, ncR, fi in SIZES for kind in KINDS for mode in MODES]


def key(ncL, ncR, kind, mode):
    return f"ub_{ncL}_{ncR}_{kind}_{mode}"


def lead(nc, seed, kind):
    alpha, Salpha, beta, Sbeta = (x.copy() for x in chain_lead(nc, seed))
    if kind in ("zc0", "zcm", "zcl"):
        npan = (nc + 7) // 8
        c = {"zc0": min(3, nc - 1), "zcm": min(8 * (npan // 2) + 3, nc - 1), "zcl": nc - 1}[kind]
        alpha[:, c] = 0.0; Salpha[:, c] = 0.0
    elif kind == "perm":
        alpha = 0.01 * alpha + 4.0 * np.roll(np.eye(nc), SHIFT % nc, axis=0)
    elif kind in ("up64", "dn64"):
        f = 2.0 ** (64 if kind == "up64" else -64)
        alpha, Salpha, beta, Sbeta = alpha * f, Salpha * f, beta * f, Sbeta * f
    return alpha, Salpha, beta, Sbeta


def dominance(nc, seed):
    """min over the energies and columns j of |A[(j + SHIFT) mod n, j]| / (sum of the column's other |entries|), A = z S - alpha"""
    alpha, Salpha, _, _ = lead(nc, seed, "perm")
    worst = np.inf
    for e in ES:
        A = np.abs((e + 1j * ETA) * Salpha - alpha)
        j = np.arange(nc)
        big = A[(j + SHIFT) % nc, j]
        worst = min(worst, float(np.min(big / (A.sum(axis=0) - big))))
    return worst


def seeds(ncL, ncR):
    seed = 2900 + 64 * ncL + ncR
    return seed, seed + 1, seed + 2


def provider(ncL, ncR, kind):
    from gaunegf_amd.surfG1D import surfG
    seed, sL, sR = seeds(ncL, ncR)
    N = ncL + ncR + 7
    F, S = random_system(N, seed)
    inds = [list(range(ncL)), list(range(N - ncR, N))]
    aL, aR = lead(ncL, sL, kind), lead(ncR, sR, kind)
    kw = dict(taus=[aL[2].copy(), aR[2].copy()], staus=[aL[3].copy(), aR[3].copy()], alphas=[aL[0], aR[0]],
              aOverlaps=[aL[1], aR[1]], betas=[aL[2], aR[2]], bOverlaps=[aL[3], aR[3]], eta=ETA)
    return surfG(F, S, inds, **kw), inds


def run(engine, ncL, ncR, force_iters, kind, mode):
    """([energy][contact] Sigma blocks, NaNs canonical; sweep counts; flags), every evaluation running its fixed points"""
    engine.set_chain_round_robin(*MODES[mode])
    g, inds = provider(ncL, ncR, kind)
    g.force_iters = force_iters
    sig, its, cv = g.sigma_batch(ES)
    return [[canonical(s[np.ix_(i, i)]) for i in inds] for s in sig], its, cv
