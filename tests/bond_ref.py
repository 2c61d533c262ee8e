"""numpy restatement, extended-precision truth and seeded inputs for the local (bond) transmission
(test_bond_host.py on the CPU, test_bond_gpu.py on the MI355X).

    K(E) = E S - F                     (no self-energies)
    A_c  = G Gamma_c G^H               G = (E S - F - sum Sigma)^-1,  Gamma_c = i (Sigma_c - Sigma_c^H)
    flow[i, j] = 2 Im[K_ij A_c,ji]     transmission flowing from orbital i to orbital j

Two float64 forms (flow: inv and two products; flow_alt: two LU solves, no explicit inverse) and a clongdouble truth
on xprec.refine's inverse.  C_BOND is the accuracy constant of the calibrated bar (test_bond_host.test_calibration):
a result passes when its relative Frobenius error against the truth is at most C_BOND times the larger error of the two
float64 forms on that input.
"""
import numpy as np
import scipy.linalg as sla

import xprec
from helpers import random_system

LD = np.clongdouble
C_BOND = 4.0          # smallest power of two >= 2 R, R = worst error ratio between the two float64 forms (test_calibration)
PROJECT_BAR = 1e-8    # relative Frobenius bar of G(E)-derived quantities


def gamma(sig):
    return 1j * (sig - sig.conj().T)


def flow(F, S, sigmas, E, c=0):
    """float64 restatement: inv, (G Gamma) G^H."""
    A = E * S - F - sum(sigmas)
    G = np.linalg.inv(A)
    Ac = (G @ gamma(sigmas[c])) @ G.conj().T
    return 2.0 * np.imag((E * S - F) * Ac.T)


def flow_alt(F, S, sigmas, E, c=0):
    """second float64 form, no explicit inverse: Y = A^-1 Gamma, A_c = (A^-1 Y^H)^H (two LU solves)."""
    A = E * S - F - sum(sigmas)
    Y = np.linalg.solve(A, gamma(sigmas[c]))
    Ac = np.linalg.solve(A, Y.conj().T).conj().T
    return 2.0 * np.imag((E * S - F) * Ac.T)


def flow_truth(F, S, sigmas, E, c=0):
    """The same in clongdouble on a refined inverse; returned as longdouble [n, n]."""
    xprec.require_extended()
    n = F.shape[0]
    Sl, Fl = np.asarray(S).astype(LD), np.asarray(F).astype(LD)
    K = LD(E) * Sl - Fl
    A = K - sum(np.asarray(s).astype(LD) for s in sigmas)
    (G, _), = xprec.refine([(A, np.arange(n))], [2.0 ** -55])
    gam = LD(1j) * (np.asarray(sigmas[c]).astype(LD) - np.asarray(sigmas[c]).astype(LD).conj().T)
    Ac = _matmul_ld(_matmul_ld(G, gam), G.conj().T)
    return 2 * (K * Ac.T).imag


def _matmul_ld(A, B):
    """clongdouble product through four longdouble ones (those run in numpy's fast loops)."""
    Ar, Ai, Br, Bi = (np.ascontiguousarray(x) for x in (A.real, A.imag, B.real, B.imag))
    out = np.empty((A.shape[0], B.shape[1]), dtype=LD)
    out.real = Ar @ Br - Ai @ Bi
    out.imag = Ar @ Bi + Ai @ Br
    return out


def rel_err(x, truth):
    """relative Frobenius error of a float64 table against a longdouble truth."""
    d = np.asarray(x).astype(np.longdouble) - truth
    return float(np.sqrt((d * d).sum()) / np.sqrt((truth * truth).sum()))


def group_table(fl, groups, n_groups=None):
    """flowG[a, b] = sum_{i in a, j in b} flow[i, j]."""
    g = np.asarray(groups)
    ng = int(g.max()) + 1 if n_groups is None else n_groups
    M = np.zeros((g.size, ng))
    M[np.arange(g.size), g] = 1.0
    return M.T @ fl @ M


def transmission(F, S, sigmas, E, c=0):
    """total transmission out of contact c: sum over the other contacts of Re Tr[Gamma_c G Gamma_o G^H]."""
    G = np.linalg.inv(E * S - F - sum(sigmas))
    go = sum(gamma(s) for k, s in enumerate(sigmas) if k != c)
    return float(np.real(np.trace(gamma(sigmas[c]) @ G @ go @ G.conj().T)))


def cut_defect(fl, T, in_P):
    """(|sum_{i in P, j in Q} flow - T|, max(|T|, sum_cut |flow|)) for the split P = in_P, Q = the rest."""
    P = np.asarray(in_P, dtype=bool)
    blockPQ = fl[np.ix_(P, ~P)]
    return abs(blockPQ.sum() - T), max(abs(T), np.abs(blockPQ).sum())


# --------------------------------------------------------------------------- seeded inputs
class BondCase:
    """A junction with two CONST contacts confined to their orbital lists."""

    def __init__(self, n, nc, seed, hermitian_complex=False, overlap=0.02):
        self.n, self.nc, self.seed = n, nc, seed
        rng = np.random.default_rng(9100 + seed)
        F, _ = random_system(n, 9200 + seed)
        B = rng.standard_normal((n, n))
        S = np.eye(n) + overlap * (B + B.T) / 2
        if hermitian_complex:
            X = rng.standard_normal((n, n)); Y = rng.standard_normal((n, n))
            F = F + 0.3j * (X - X.T) / np.sqrt(2 * n)
            S = S + 0.5j * overlap * (Y - Y.T) / 2
        self.F, self.S = np.asarray(F, dtype=complex), np.asarray(S, dtype=complex)
        self.inds = [np.arange(nc[0]), np.arange(n - nc[1], n)]
        self.sigmas = [self._sigma(ix, rng) for ix in self.inds]
        # a real grid with one point 5e-4 above an eigenvalue of (F, S)
        ev = sla.eigh(self.F, self.S, eigvals_only=True)
        near = float(ev[np.argmin(np.abs(ev - 0.6))]) + 5e-4
        self.energies = np.array([-1.0, 0.3, near, 2.0])

    def _sigma(self, idx, rng):
        """-i Gamma / 2 + a Hermitian shift on the contact orbitals, |Gamma| ~ 0.1 ... 1."""
        k = len(idx)
        A = rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k))
        gam = 0.3 * np.eye(k) + 0.4 * (A @ A.conj().T) / (2 * k)
        Bm = rng.standard_normal((k, k))
        s = np.zeros((self.n, self.n), complex)
        s[np.ix_(idx, idx)] = 0.05 * (Bm + Bm.T) - 0.5j * gam
        return s

    def atom_groups(self, per=None):
        """orbital -> group ("atoms"): consecutive runs of at most `per` orbitals that never straddle the edge of a
        contact, so that every group boundary between the contacts is a valid cut."""
        return aligned_groups(self.n, self.nc, per)

    def group_cuts(self, groups, rng=None):
        """Splits of the GROUPS (True = the side of contact 0): every group boundary from the end of contact 0 to the
        start of contact 1, and one random assignment of the groups in between."""
        groups = np.asarray(groups)
        ng = int(groups.max()) + 1
        g_lo, g_hi = int(groups[self.nc[0] - 1]) + 1, int(groups[self.n - self.nc[1]])     # interior groups [g_lo, g_hi)
        out = [np.arange(ng) < b for b in range(g_lo, g_hi + 1)]
        rng = rng or np.random.default_rng(self.seed + 50)
        P = np.arange(ng) < g_lo
        P[g_lo:g_hi] = rng.random(g_hi - g_lo) < 0.5
        out.append(P)
        return out

    def cuts(self, rng=None):
        """Splits P (True) | Q of the ORBITALS with contact 0 in P and contact 1 in Q: every boundary between the
        contacts at a stride, and one random assignment of the interior."""
        lo, hi = self.nc[0], self.n - self.nc[1]
        out = []
        for b in sorted(set(np.linspace(lo, hi, 5).astype(int))):
            out.append(np.arange(self.n) < b)
        rng = rng or np.random.default_rng(self.seed)
        P = np.zeros(self.n, dtype=bool)
        P[:lo] = True
        P[lo:hi] = rng.random(hi - lo) < 0.5
        out.append(P)
        return out


def const_cases():
    """n = 24, 60 (single-kernel path), 130 (blocked inverse); contacts of 4 ... 30 orbitals; one complex Hermitian."""
    return [BondCase(24, (4, 5), 1), BondCase(60, (8, 12), 2, hermitian_complex=True), BondCase(130, (30, 20), 3)]


def aligned_groups(n, nc, per=None):
    """Runs of at most `per` consecutive orbitals, cut at the contacts' edges nc[0] and n - nc[1] as well."""
    per = per or max(2, n // 12)
    edges = sorted(set(range(0, n, per)) | {nc[0], n - nc[1]})
    return np.searchsorted(np.asarray(edges), np.arange(n), side="right") - 1
