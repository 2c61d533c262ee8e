"""numpy restatement, extended-precision truth and seeded inputs for the overlap / Hamilton populations and the projected
DOS (test_population_host.py on the CPU, test_population_gpu.py on the MI355X).

    G = (E S - F - sum Sigma)^-1,  Gamma_c = i (Sigma_c - Sigma_c^H),  A_c = G Gamma_c G^H,  X = S or F
    retarded (c = None):   pop[i, j]   = -(1/pi)  Im[G_ij conj(X_ij)]        p_a   = -(1/pi)  Im[w_a^H G w_a]
    contact c:             pop_c[i, j] = (1/2 pi) Re[A_c,ij conj(X_ij)]      p_c,a = (1/2 pi) Re[w_a^H A_c w_a]
    rows[a] = sum_b table[a, b]

Two float64 forms that really differ (inv and solve(A, I) take the same LAPACK route and do not count as two):
  table / proj           the explicit LU inverse, (G Gamma) G^H, w^H (G w)
  table_alt / proj_alt   retarded table: G = R^-1 Q^H from a QR factorisation; contact table: two LU solves that never form
                         G (Y = A^-1 Gamma, A_c = (A^-1 Y^H)^H); projections: LU solves on the vectors only
                         (y = A^-1 w;  z = A^-H w, p_c = z^H Gamma_c z / 2 pi).
The truth is the same arithmetic in clongdouble on xprec.refine's inverse.

C_POP is the accuracy constant of the calibrated bar (test_population_host.test_calibration): a result passes when its
relative Frobenius error against the truth is at most C_POP times the larger error of the two float64 forms on that input.
Measured on the CPU over bond_ref.const_cases() x {retarded, contact 0, contact 1} x {S, F} tables and the projections on
the complete set of (F, S)'s eigenvectors: R = 6.02 (worst ratio between the two forms' errors, at the n = 24
contact-0 projection) -> C_POP = 16; the float64 errors themselves are 1.5e-16 ... 1.3e-14.
"""
import numpy as np
import scipy.linalg as sla

import bond_ref as br
import xprec

LD = np.clongdouble
C_POP = 16.0          # smallest power of two >= 2 R, R = 6.02 (test_population_host.test_calibration)
PROJECT_BAR = br.PROJECT_BAR
INV_PI = 1.0 / np.pi

FORMS = (None, 0, 1)  # the retarded form and the two contacts
OPS = ("S", "F")


def _x(F, S, op):
    return S if op == "S" else F


def _assembled(F, S, sigmas, E):
    return E * S - F - sum(sigmas)


# --------------------------------------------------------------------------- float64, form 1: the explicit inverse
def spectral(F, S, sigmas, E, c=None):
    """The matrix the population reads: G (c None) or A_c = (G Gamma_c) G^H."""
    G = np.linalg.inv(_assembled(F, S, sigmas, E))
    if c is None:
        return G
    return (G @ br.gamma(sigmas[c])) @ G.conj().T


def table_of(M, X, c):
    """pop table from the matrix M = G or A_c."""
    return -INV_PI * np.imag(M * np.conj(X)) if c is None else 0.5 * INV_PI * np.real(M * np.conj(X))


def table(F, S, sigmas, E, c=None, op="S"):
    return table_of(spectral(F, S, sigmas, E, c), _x(F, S, op), c)


def proj_of(M, W, c):
    """p_a from the matrix M and the vectors W [k, n]."""
    q = np.einsum("ai,ai->a", np.conj(W), (M @ W.T).T)
    return -INV_PI * np.imag(q) if c is None else 0.5 * INV_PI * np.real(q)


def proj(F, S, sigmas, E, W, c=None):
    return proj_of(spectral(F, S, sigmas, E, c), W, c)


# --------------------------------------------------------------------------- float64, form 2: QR / LU solves, no inv
def table_alt(F, S, sigmas, E, c=None, op="S"):
    A = _assembled(F, S, sigmas, E)
    if c is None:
        Q, R = np.linalg.qr(A)
        M = sla.solve_triangular(R, Q.conj().T)
    else:
        Y = np.linalg.solve(A, br.gamma(sigmas[c]))
        M = np.linalg.solve(A, Y.conj().T).conj().T
    return table_of(M, _x(F, S, op), c)


def proj_alt(F, S, sigmas, E, W, c=None):
    A = _assembled(F, S, sigmas, E)
    if c is None:
        Y = np.linalg.solve(A, W.T)                                        # y_a = G w_a
        return -INV_PI * np.imag(np.einsum("ai,ia->a", np.conj(W), Y))
    Z = np.linalg.solve(A.conj().T, W.T)                                   # z_a = G^H w_a
    return 0.5 * INV_PI * np.real(np.einsum("ia,ia->a", np.conj(Z), br.gamma(sigmas[c]) @ Z))


# --------------------------------------------------------------------------- clongdouble truth
def spectral_truth(F, S, sigmas, E, c=None, G=None):
    """G (c None) or A_c in clongdouble; ``G``: the refined inverse of an earlier call on the same input."""
    xprec.require_extended()
    n = F.shape[0]
    if G is None:
        A = LD(E) * np.asarray(S).astype(LD) - np.asarray(F).astype(LD) - sum(np.asarray(s).astype(LD) for s in sigmas)
        (G, _), = xprec.refine([(A, np.arange(n))], [2.0 ** -55])
    if c is None:
        return G
    sc = np.asarray(sigmas[c]).astype(LD)
    return br._matmul_ld(br._matmul_ld(G, LD(1j) * (sc - sc.conj().T)), G.conj().T)


def table_truth_of(M, X, c):
    Xl = np.asarray(X).astype(LD)
    pi = np.longdouble(np.pi) + np.longdouble(1.2246467991473532e-16)     # pi to longdouble precision (double-double tail)
    prod = M * np.conj(Xl)
    return -prod.imag / pi if c is None else prod.real / (2 * pi)


def proj_truth_of(M, W, c):
    Wl = np.asarray(W).astype(LD)
    pi = np.longdouble(np.pi) + np.longdouble(1.2246467991473532e-16)
    q = (np.conj(Wl) * br._matmul_ld(M, np.ascontiguousarray(Wl.T)).T).sum(axis=1)
    return -q.imag / pi if c is None else q.real / (2 * pi)


def rel_err(x, truth):
    """relative Frobenius error of a float64 array against a longdouble truth."""
    d = np.asarray(x).astype(np.longdouble) - truth
    return float(np.sqrt((d * d).sum()) / np.sqrt((truth * truth).sum()))


# --------------------------------------------------------------------------- groups, vectors, inputs
def group_table(tab, groups, n_groups=None):
    return br.group_table(tab, groups, n_groups)


def group_rows(tab, groups, n_groups=None):
    return group_table(tab, groups, n_groups).sum(axis=1)


def complete_set(F, S):
    """(energies, C [n, n]): the eigenvectors of (F, S), a complete S-orthonormal set (C^H S C = 1)."""
    F = np.asarray(F); S = np.asarray(S)
    return sla.eigh((F + F.conj().T) / 2, (S + S.conj().T) / 2)


def vectors(F, S, C):
    """W [k, n] with rows w_a = S c_a for the orbital coefficients in the columns of C."""
    return np.ascontiguousarray((np.asarray(S) @ np.asarray(C)).T).astype(complex)


def const_cases():
    """bond_ref.const_cases(): n = 24, n = 60 complex Hermitian, n = 130; four real energies, one 5e-4 above an eigenvalue."""
    return br.const_cases()


def case_n300():
    """n = 300: a 256-thread workgroup's column loop wraps; the windowed inverse."""
    return br.BondCase(300, (50, 40), 4)
