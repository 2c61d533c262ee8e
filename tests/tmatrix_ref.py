"""numpy restatement, extended-precision truth and seeded inputs for the multi-terminal transmission matrix and the
dephasing probes (test_tmatrix_host.py on the CPU, test_tmatrix_gpu.py on the MI355X).

A junction is (F, S) and a list of terminals [(I_a, Sigma_a)]: orbital list and K_a x K_a complex block -- the contacts
first, then the probes.

    A(E)    = E S - F - sum_a scatter(Sigma_a on I_a x I_a),   G = A^-1
    Gamma_a = i (Sigma_a - Sigma_a^H)
    T[a][b] = Re Tr[Gamma_a G Gamma_b G^H] = Re sum_ij (Gamma_a G_ab Gamma_b)_ij conj(G_ab,ij),   G_ab = G[I_a, I_b]

Two float64 forms that really differ:
  tmatrix       the explicit LU inverse, the n x n coupling matrices and the literal trace Re Tr[Gamma_a (G Gamma_b G^H)]
  tmatrix_alt   LU solves on the terminals' columns only (G[:, I_b] = A^-1 e_{I_b}; G is never formed), then the block form
The truth is the block form in clongdouble on xprec.refine's inverse.

C_TM is the accuracy constant of the calibrated bar (test_tmatrix_host.test_calibration): a result passes when its
relative Frobenius error against the truth is at most C_TM times the larger error of the two float64 forms on that
input.  Measured on the CPU over cases() x their four energies: R = 1.40 (worst ratio between the two forms' errors, at n = 200,
E = -1) -> C_TM = 4; the float64 errors themselves are 6.4e-17 ... 5.9e-16.
"""
import functools

import numpy as np
import scipy.linalg as sla

import bond_ref as br
import xprec

LD = np.clongdouble
C_TM = 4.0            # smallest power of two >= 2 R (test_tmatrix_host.test_calibration)
PROJECT_BAR = br.PROJECT_BAR


def gamma(blk):
    blk = np.asarray(blk)
    return 1j * (blk - blk.conj().T)


def assembled(F, S, terms, E, dtype=complex):
    A = dtype(E) * np.asarray(S).astype(dtype) - np.asarray(F).astype(dtype)
    for idx, blk in terms:
        A[np.ix_(idx, idx)] -= np.asarray(blk).astype(dtype)
    return A


def dense(n, idx, blk):
    out = np.zeros((n, n), complex)
    out[np.ix_(idx, idx)] = blk
    return out


# --------------------------------------------------------------------------- float64, form 1: inverse, literal trace
def tmatrix(F, S, terms, E):
    n = F.shape[0]
    G = np.linalg.inv(assembled(F, S, terms, E))
    gams = [dense(n, idx, gamma(blk)) for idx, blk in terms]
    Ms = [(G @ g) @ G.conj().T for g in gams]
    return np.array([[np.real(np.trace(ga @ Mb)) for Mb in Ms] for ga in gams])


# --------------------------------------------------------------------------- float64, form 2: LU solves on the columns
def tmatrix_alt(F, S, terms, E):
    n = F.shape[0]
    lu = sla.lu_factor(assembled(F, S, terms, E))
    eye = np.eye(n, dtype=complex)
    cols = [sla.lu_solve(lu, eye[:, idx]) for idx, _ in terms]                  # G[:, I_b]
    gams = [gamma(blk) for _, blk in terms]
    C = len(terms)
    T = np.zeros((C, C))
    for a, (ia, _) in enumerate(terms):
        for b in range(C):
            Gab = cols[b][ia]
            T[a, b] = np.real(np.sum((gams[a] @ Gab @ gams[b]) * np.conj(Gab)))
    return T


# --------------------------------------------------------------------------- clongdouble truth
def tmatrix_truth(F, S, terms, E):
    xprec.require_extended()
    n = F.shape[0]
    A = assembled(F, S, terms, E, LD)
    (G, _), = xprec.refine([(A, np.arange(n))], [2.0 ** -55])
    gams = []
    for _, blk in terms:
        b = np.asarray(blk).astype(LD)
        gams.append(LD(1j) * (b - b.conj().T))
    C = len(terms)
    T = np.zeros((C, C), dtype=np.longdouble)
    for a, (ia, _) in enumerate(terms):
        for b, (ib, _) in enumerate(terms):
            Gab = np.ascontiguousarray(G[np.ix_(ia, ib)])
            Y = br._matmul_ld(br._matmul_ld(gams[a], Gab), gams[b])
            T[a, b] = (Y * np.conj(Gab)).real.sum()
    return T


def rel_err(x, truth):
    return br.rel_err(x, truth)


# --------------------------------------------------------------------------- effective transmission
def t_eff(T, n_real, d=None, s=0):
    """T_eff[d][s] of ONE matrix T [C, C] whose terminals n_real .. C - 1 float:
    To = T with zero diagonal, W_pp = sum_{c != p} To[p][c], W_pq = -To[p][q], P' = probes with W_pp > 0,
    T_eff = To[d][s] + To[d][P'] W^-1 To[P'][s]."""
    T = np.asarray(T, dtype=float)
    C = T.shape[0]
    d = n_real - 1 if d is None else d
    To = T - np.diag(np.diag(T))
    P = [p for p in range(n_real, C) if To[p].sum() > 0]
    if not P:
        return To[d, s]
    W = -To[np.ix_(P, P)]
    W[np.arange(len(P)), np.arange(len(P))] = [To[p].sum() for p in P]
    return To[d, s] + To[d, P] @ np.linalg.solve(W, To[P, s])


# --------------------------------------------------------------------------- seeded inputs
def sigma_block(k, rng, real=False, scale=1.0):
    """-i Gamma / 2 + a Hermitian shift, Gamma Hermitian positive definite (real symmetric for ``real``), |Gamma| ~ 0.1 ... 1."""
    A = rng.standard_normal((k, k)) + (0 if real else 1j * rng.standard_normal((k, k)))
    gam = 0.3 * np.eye(k) + 0.4 * (A @ A.conj().T) / (2 * k)
    B = rng.standard_normal((k, k))
    return scale * (0.05 * (B + B.T) - 0.5j * gam)


class TCase:
    """(F, S) of bond_ref.BondCase with ``n_c`` contacts followed by probes; terms = [(sorted indices, block)]."""

    def __init__(self, name, n, seed, lists, n_c, hermitian_complex=False, zero=()):
        base = br.BondCase(n, (2, 2), seed, hermitian_complex=hermitian_complex)
        self.name, self.n, self.n_c = name, n, n_c
        self.F, self.S, self.energies = base.F, base.S, base.energies
        self.real = not hermitian_complex
        rng = np.random.default_rng(4400 + seed)
        self.terms = []
        for t, idx in enumerate(lists):
            idx = np.asarray(sorted(idx), dtype=int)
            blk = sigma_block(idx.size, rng, real=self.real)
            if t in zero:
                blk = np.zeros_like(blk)
            self.terms.append((idx, blk))

    @property
    def contacts(self):
        return self.terms[:self.n_c]

    @property
    def probes(self):
        return self.terms[self.n_c:]

    def contact_sigmas(self, terms=None):
        """dense n x n Sigma of the contacts (of ``terms``), what Engine.sigma_const takes"""
        return [dense(self.n, idx, blk) for idx, blk in (self.contacts if terms is None else terms)]


@functools.lru_cache(maxsize=None)
def cases():
    r = np.arange
    return (
        # four contacts K = (1, 5, 9, 4), no probes; the single-kernel inverse
        TCase("n24", 24, 11, [[0], r(2, 7), r(9, 18), r(20, 24)], 4),
        # contacts (5, 9) + probes K = 1, 1, 3, 9: probe 0 on a lead orbital, probes 2 and 3 overlap, probe 1 has Sigma = 0
        TCase("n40", 40, 12, [r(0, 5), r(31, 40), [2], [17], [10, 12, 14], r(12, 21)], 2, hermitian_complex=True, zero=(3,)),
        # contacts (40, 30) + ten probes of 9; the blocked inverse
        TCase("n130", 130, 13, [r(0, 40), r(100, 130)] + [r(40 + 6 * q, 49 + 6 * q) for q in range(10)], 2),
        # terminals of K = 100, 17 (contacts) and 63, 64, 65 (probes, overlapping): every class of the pair routing
        TCase("n200", 200, 14, [r(0, 100), r(183, 200), r(90, 153), r(100, 164), r(118, 183)], 2, hermitian_complex=True),
    )


@functools.lru_cache(maxsize=None)
def truth_table():
    """[(tag, case, E, truth, err_a, err_b)] over every (case, energy) of cases(): the clongdouble truth and the errors of
    the two float64 forms against it.  Computed once per process and shared by the tests that need it."""
    items = [(c, float(E)) for c in cases() for E in c.energies]

    def make(item):
        c, E = item
        t = tmatrix_truth(c.F, c.S, c.terms, E)
        return (f"{c.name} E={E:.6g}", c, E, t, rel_err(tmatrix(c.F, c.S, c.terms, E), t),
                rel_err(tmatrix_alt(c.F, c.S, c.terms, E), t))
    return xprec.pmap(make, items)
