"""Extended-precision truth for the Green's-function path, conditioning-aware bars and the case table
shared by test_accuracy_host.py (CPU) and test_accuracy_gpu.py (MI355X).

Truth.  A = E S - F - Sigma is formed in np.clongdouble (64-bit mantissa) from the float64 inputs; columns of
A^-1 come from mixed-precision iterative refinement: an fp64 LU (LAPACK) solves for the corrections, the residual
e_j - A x and the iterate x are kept in clongdouble.  The refinement stops when the correction stalls and asserts
that it converged far below the bar.  The limiting accuracy is about kappa * 2^-64 (1e-10 at kappa = 2e9, against
a bar of 1e-6 there); test_accuracy_host.py checks it against mpmath.

Bar.  For every column j:  ||G_hat e_j - G e_j|| / ||G e_j|| <= delta,  delta = C_BAR * sqrt(n) * u * kappa_2(A),
u = 2^-53, kappa_2 from fp64 singular values.  C_BAR = 2 is the smallest power of two at least twice the worst
ratio of LAPACK's solve and a textbook izamax Gauss-Jordan over the case table (test_calibration).
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.linalg as sla

from helpers import random_system

LD = np.clongdouble
U = 2.0 ** -53
C_BAR = 2.0
GAMMA = 0.1                          # contact broadening of the const providers (-i GAMMA on the contact diagonal)
FULL_COLUMNS_UPTO = 256              # n above this: a fixed sample of columns (sample_columns)


def require_extended():
    """The truth needs a long double of at least 64 mantissa bits (x87 extended); a platform where long double
    is plain double cannot check the bars and fails here instead of skipping."""
    eps = np.finfo(np.longdouble).eps
    assert eps <= 2.0 ** -63, f"np.longdouble has eps {eps}: no extended precision for the reference"


def gamma_n(k):
    """Higham's gamma_k = k u / (1 - k u)."""
    return k * U / (1.0 - k * U)


def bar(n, kappa, c=C_BAR):
    return c * np.sqrt(n) * U * kappa


def kappa2(A):
    s = np.linalg.svd(np.asarray(A, dtype=np.complex128), compute_uv=False)
    return float(s[0] / s[-1])


def _threads():
    try:
        k = int(os.environ.get("OMP_NUM_THREADS", "8"))
    except ValueError:
        k = 8
    return max(1, min(k, 16))


def pmap(fn, items):
    """map over a thread pool (for extended-precision products, which release the GIL)."""
    items = list(items)
    if len(items) <= 1:
        return [fn(x) for x in items]
    with ThreadPoolExecutor(min(_threads(), len(items))) as ex:
        return list(ex.map(fn, items))


# --------------------------------------------------------------------------- #
# the case table
# --------------------------------------------------------------------------- #
class Case:
    """One system and its energies.  `sigs` are the two contact self-energies (complex128) exactly as the device
    provider receives them; `factor` maps the truth of `base` onto this case (G3: -i, G5: 2^-k), None for a base."""

    def __init__(self, name, n, F, S, inds, sigs, energies, resonant=None, base=None, factor=None):
        self.name, self.n = name, n
        self.F, self.S, self.inds, self.sigs = F, S, inds, sigs
        self.energies = np.asarray(energies, dtype=np.complex128)
        self.resonant, self.base, self.factor = resonant, base, factor

    @property
    def sig_tot(self):
        return self.sigs[0] + self.sigs[1]

    def A64(self, E):
        return E * self.S - self.F - self.sig_tot

    def A_ld(self, E):
        return LD(E) * self.S.astype(LD) - self.F.astype(LD) - self.sig_tot.astype(LD)

    def contact_columns(self):
        return sorted(set(self.inds[0]) | set(self.inds[1]))

    def gammas(self):
        return [1j * (s - s.conj().T) for s in self.sigs]


def _contacts(n):
    if n < 4:
        return [[0], [0]]
    nc = max(1, min(12, n // 10))
    return [list(range(nc)), list(range(n - nc, n))]


def _sigmas(n, S, inds):
    from oracle import form_sigma
    return [form_sigma(inds[0], -1j * GAMMA, n, S), form_sigma(inds[1], -1j * GAMMA, n, S)]


def ladder(n, seed=0):
    """G1: a random system with one spectator orbital coupled to the rest at 1e-7.  The contacts' -1e-9 i S puts its
    level at Im lambda0 ~ -2e-9; energies Re lambda0 + {1, 1e-2, 1e-5, 1e-8, 0} span kappa_2 ~ 1e1 ... 2e9, plus
    one contour point 0.3 + 2i."""
    F, S = random_system(n, 7000 + n + seed)
    inds = _contacts(n)
    k = n - 1 if n < 4 else n // 2 + 3
    rng = np.random.default_rng(17 + n)
    keep = [i for i in range(n) if i != k]
    if keep:
        ev = np.sort(sla.eigh(F[np.ix_(keep, keep)], S[np.ix_(keep, keep)], eigvals_only=True))
        mids = (ev[1:] + ev[:-1]) / 2 if ev.size > 1 else ev + 0.5
        eps = float(mids[np.argmin(np.abs(mids - 0.1))])
    else:
        eps = 0.1
    v = 1e-7 * rng.standard_normal(n)
    F[k, :] = v; F[:, k] = v; F[k, k] = eps
    S[k, :] = 0.0; S[:, k] = 0.0; S[k, k] = 1.0
    sigs = _sigmas(n, S, inds)
    lam = sla.eig(F + sigs[0] + sigs[1], S, right=False)
    lam0 = lam[np.argmin(np.abs(lam - eps))]
    E = [lam0.real + d for d in (1.0, 1e-2, 1e-5, 1e-8, 0.0)] + [0.3 + 2j]
    return Case("G1", n, F, S, inds, sigs, E, resonant=k)


def bipartite(n, seed=0, confined=False):
    """G2: orthogonal tight binding with random hoppings between even and odd sites only: a zero diagonal, so at
    E = 0 every diagonal entry of A is -Sigma_ii (2e-9 i off the contacts) and Gauss-Jordan must exchange rows.  The
    first contact sits in the middle, so the leading rows are all bare sites.  confined=True ("G2c") drops formSigma's
    -1e-9 i S background (and E = 0 with it), so that Gamma_c lives on the contact orbitals."""
    rng = np.random.default_rng(8000 + n + seed)
    T = rng.standard_normal((n, n))
    H = (T + T.T) / np.sqrt(2 * n) * 2
    idx = np.arange(n)
    F = np.where((idx[:, None] + idx[None, :]) % 2 == 1, H, 0.0)
    S = np.eye(n)
    inds = _contacts(n)
    if n >= 4:                       # contacts off the first rows: the first pivot candidates are the bare diagonal
        nc = len(inds[0])
        inds = [list(range(n // 2 - nc, n // 2)), inds[1]]
    if confined:                     # -i GAMMA on the contact diagonal only: the compact Gamma products apply
        sigs = [np.zeros((n, n), dtype=np.complex128) for _ in inds]
        for s, ix in zip(sigs, inds):
            s[ix, ix] = -1j * GAMMA
        return Case("G2c", n, F, S, inds, sigs, [1e-3, 0.5j, 0.3 + 2j])
    return Case("G2", n, F, S, inds, _sigmas(n, S, inds), [0.0, 1e-3, 0.5j, 0.3 + 2j])


def graded(n, seed=0):
    """G4: a random system whose 'core' orbitals (every fifth, off the contacts) carry on-site energies 1e3 ... 1e5."""
    F, S = random_system(n, 9000 + n + seed)
    inds = _contacts(n)
    cont = set(inds[0]) | set(inds[1])
    core = [i for i in range(1, n, 5) if i not in cont]
    if core:
        F[core, core] += np.logspace(3, 5, len(core))
    return Case("G4", n, F, S, inds, _sigmas(n, S, inds), [-0.7, 0.25, 0.3 + 2j])


def rotated(c):
    """G3: F -> iF, E -> iE, Sigma -> i Sigma, so A -> iA and G -> -iG, all exactly (S stays real)."""
    return Case(c.name + "rot", c.n, 1j * c.F, c.S, c.inds, [1j * s for s in c.sigs], 1j * c.energies,
                resonant=c.resonant, base=c, factor=-1j)


def scaled(c, k):
    """G5: E, F and Sigma times 2^k, so A -> 2^k A and G -> 2^-k G, all exactly."""
    f = 2.0 ** k
    return Case(f"{c.name}x2^{k}", c.n, f * c.F, c.S, c.inds, [f * s for s in c.sigs], f * c.energies,
                resonant=c.resonant, base=c, factor=2.0 ** -k)


def case_table(n):
    """[G1, G2, G3 (the rotated G1 and G2), G4] at dimension n."""
    g1, g2, g4 = ladder(n), bipartite(n), graded(n)
    return [g1, g2, rotated(g1), rotated(g2), g4]


class ForeignConst:
    """Energy-independent self-energies in the duck-typed provider protocol (sigma / sigmaTot only): the engine sees
    them through its precomputed-Sigma path, exactly as given -- the rotated and scaled cases need that."""

    def __init__(self, case):
        self.sigs = case.sigs
        self.tot = case.sig_tot
        self.size = case.n

    def sigmaTot(self, E):
        return self.tot

    def sigma(self, E, ind):
        return self.sigs[ind]


# --------------------------------------------------------------------------- #
# the reference
# --------------------------------------------------------------------------- #
def sample_columns(case, seed=0):
    """Every column up to FULL_COLUMNS_UPTO; above, the first and last column of every 32-column sub-window (which
    includes those of every 64-column window), the contact columns, the column with the largest weight on the
    resonant eigenvector and four seeded random columns."""
    n = case.n
    if n <= FULL_COLUMNS_UPTO:
        return np.arange(n)
    s = set()
    for w0 in range(0, n, 32):
        s.add(w0); s.add(min(w0 + 31, n - 1))
    s.update(case.contact_columns())
    if case.resonant is not None:
        s.add(case.resonant)
    s.update(int(j) for j in np.random.default_rng(seed + n).choice(n, 4, replace=False))
    return np.array(sorted(s))


def refine(systems, tols):
    """Iterative refinement of columns of A^-1 for several systems at once: `systems` = [(A_ld, cols)], `tols` the
    convergence bar of each.  Returns [(X clongdouble [n, len(cols)], last relative correction)] and asserts that every
    last correction is below its bar.  The fp64 LU factorizations and solves run in this thread (LAPACK threads
    itself); the extended-precision residuals, real and imaginary parts apart (np.longdouble products run in
    parallel threads, np.clongdouble ones much less), run on a thread pool."""
    require_extended()
    jobs = []
    for (A_ld, cols), tol in zip(systems, tols):
        n = A_ld.shape[0]
        lu = sla.lu_factor(A_ld.astype(np.complex128), check_finite=True)
        B = np.zeros((n, len(cols)), dtype=np.complex128)
        B[np.asarray(cols), np.arange(len(cols))] = 1
        X = sla.lu_solve(lu, B)
        jobs.append(dict(Ar=np.ascontiguousarray(A_ld.real), Ai=np.ascontiguousarray(A_ld.imag), lu=lu, B=B,
                         Xr=X.real.astype(np.longdouble), Xi=X.imag.astype(np.longdouble),
                         prev=np.inf, rel=np.inf, tol=tol, done=False))

    def residual(j):
        return (j["B"].real - (j["Ar"] @ j["Xr"] - j["Ai"] @ j["Xi"]), -(j["Ar"] @ j["Xi"] + j["Ai"] @ j["Xr"]))
    for _ in range(12):
        active = [j for j in jobs if not j["done"]]
        if not active:
            break
        for j, (Rr, Ri) in zip(active, pmap(residual, active)):
            D = sla.lu_solve(j["lu"], Rr.astype(np.float64) + 1j * Ri.astype(np.float64))
            j["Xr"] += D.real; j["Xi"] += D.imag
            xn = np.hypot(np.linalg.norm(j["Xr"].astype(np.float64), axis=0),
                          np.linalg.norm(j["Xi"].astype(np.float64), axis=0))
            rel = float(np.max(np.linalg.norm(D, axis=0) / xn))
            j["done"] = rel <= 2.0 ** -64 or rel > 0.5 * j["prev"]
            j["prev"] = j["rel"] = rel
    out = []
    for j in jobs:
        assert j["rel"] <= j["tol"], f"iterative refinement did not converge: last correction {j['rel']:.3g} > {j['tol']:.3g}"
        X = np.empty(j["Xr"].shape, dtype=LD)
        X.real, X.imag = j["Xr"], j["Xi"]
        out.append((X, j["rel"]))
    return out


class Truth:
    """Columns `cols` of G(E_m) for every energy of a base case (clongdouble [M, n, ncols]) with kappa_2 and the bar."""

    def __init__(self, case, cols=None):
        assert case.base is None, "derive the truth of a rotated / scaled case with Truth.of"
        self.case = case
        self.cols = sample_columns(case) if cols is None else np.asarray(cols)
        self.kappa = np.array([kappa2(case.A64(E)) for E in case.energies])
        n, M = case.n, case.energies.size
        chunks = [self.cols[i:i + 32] for i in range(0, self.cols.size, 32)]
        A = [case.A_ld(E) for E in case.energies]
        res = refine([(A[m], c) for m in range(M) for c in chunks],
                     [max(1e-3 * bar(n, self.kappa[m], 1.0), 2.0 ** -58) for m in range(M) for _ in chunks])
        k = len(chunks)
        self.G = np.stack([np.concatenate([r[0] for r in res[m * k:(m + 1) * k]], axis=1) for m in range(M)])
        self.last_correction = np.array([max(r[1] for r in res[m * k:(m + 1) * k]) for m in range(M)])

    @staticmethod
    def of(case, base_truth):
        """The truth of a rotated / scaled case: factor * the truth of its base, exact in clongdouble."""
        t = Truth.__new__(Truth)
        t.case, t.cols, t.kappa = case, base_truth.cols, base_truth.kappa
        t.G = base_truth.G * LD(case.factor)
        t.last_correction = base_truth.last_correction
        return t

    @property
    def full(self):
        return self.cols.size == self.case.n

    def delta(self, m, c=C_BAR):
        return bar(self.case.n, self.kappa[m], c)

    def column_errors(self, m, G):
        """||G e_j - G_true e_j|| / ||G_true e_j|| over the sampled columns of energy m (float64)."""
        T = self.G[m]
        D = np.asarray(G)[:, self.cols].astype(LD) - T
        return (np.linalg.norm(D.astype(np.complex128), axis=0) /
                np.linalg.norm(T.astype(np.complex128), axis=0))

    def ratio(self, m, G, c=C_BAR):
        """worst column error of energy m over the bar."""
        return float(np.max(self.column_errors(m, G)) / self.delta(m, c))


# --------------------------------------------------------------------------- #
# derived quantities: truth and propagated bars
# --------------------------------------------------------------------------- #
def grint_truth_and_bound(truth, w, c=C_BAR):
    """sum_m w_m G_m e_j over the sampled columns (clongdouble) and, per column,
    bound_j = sum_m |w_m| (delta_m + M u) ||G_m e_j||."""
    M = truth.case.energies.size
    w = np.asarray(w, dtype=np.complex128)
    tot = np.zeros(truth.G.shape[1:], dtype=LD)
    bound = np.zeros(truth.cols.size)
    for m in range(M):
        tot += LD(w[m]) * truth.G[m]
        cn = np.linalg.norm(truth.G[m].astype(np.complex128), axis=0)
        bound += abs(w[m]) * (truth.delta(m, c) + M * U) * cn
    return tot, bound


def _gamma_of(case, ind):
    if ind is None:
        s = case.sig_tot
        return 1j * (s - s.conj().T)
    return case.gammas()[ind]


def grless_truth_and_bound(truth, w, ind, c=C_BAR):
    """sum_m w_m G_m Gamma G_m^H (clongdouble, full truth only) and the Frobenius bound
    sum_m |w_m| [2 delta_m ||G_m||_F ||Gamma G_m^H||_2 + gamma_4n || |G_m| |Gamma| |G_m^H| ||_F]
    + M u sum_m |w_m| ||G_m Gamma G_m^H||_F
    (gamma_4n: two products of inner dimension n, gamma_2n, doubled for the normwise bound of 3M complex products)."""
    assert truth.full
    case = truth.case
    n, M = case.n, case.energies.size
    Gam = _gamma_of(case, ind)
    Gam_ld = Gam.astype(LD)
    aGam = np.abs(Gam)
    w = np.asarray(w, dtype=np.complex128)

    def one(m):
        G = truth.G[m]
        P = (G @ Gam_ld) @ G.conj().T
        G64 = G.astype(np.complex128)
        aG = np.abs(G64)
        b = (2 * truth.delta(m, c) * np.linalg.norm(G64) * np.linalg.norm(Gam @ G64.conj().T, 2)
             + gamma_n(4 * n) * np.linalg.norm(aG @ aGam @ aG.T))
        return P, b, np.linalg.norm(P.astype(np.complex128))
    res = pmap(one, range(M))
    tot = np.zeros((n, n), dtype=LD)
    bound = 0.0
    for m, (P, b, pn) in enumerate(res):
        tot += LD(w[m]) * P
        bound += abs(w[m]) * (b + M * U * pn)
    return tot, bound


def transmission_truth_and_bound(truth, c=C_BAR):
    """T_m = Re Tr(Gamma_1 G Gamma_2 G^H) (full truth) and
    |dT_m| <= 2 delta_m ||G||_F ||Gamma_1 G Gamma_2||_F + gamma_4n Tr(|Gamma_1| |G| |Gamma_2| |G^H|)."""
    assert truth.full
    case = truth.case
    n = case.n
    g1, g2 = case.gammas()
    g1l, g2l = g1.astype(LD), g2.astype(LD)
    a1, a2 = np.abs(g1), np.abs(g2)

    def one(m):
        G = truth.G[m]
        X = (g1l @ G) @ g2l
        T = np.sum(X * G.conj()).real
        G64 = G.astype(np.complex128)
        aG = np.abs(G64)
        b = (2 * truth.delta(m, c) * np.linalg.norm(G64) * np.linalg.norm(X.astype(np.complex128))
             + gamma_n(4 * n) * np.sum((a1 @ aG @ a2) * aG))
        return float(T), b
    res = pmap(one, range(case.energies.size))
    return np.array([r[0] for r in res]), np.array([r[1] for r in res])


def dos_truth_and_bound(truth, c=C_BAR):
    """per-site -Im G_ii / pi and its sum (full truth) with
    |d dos_i| <= (delta ||G e_i|| + u |G_ii|) / pi,  |d dos| <= sum_i (delta ||G e_i|| + n u |G_ii|) / pi."""
    assert truth.full
    n, M = truth.case.n, truth.case.energies.size
    site = np.zeros((M, n)); total = np.zeros(M)
    bsite = np.zeros((M, n)); btot = np.zeros(M)
    for m in range(M):
        G = truth.G[m]
        d = np.diagonal(G)
        site[m] = (-d.imag / np.longdouble(np.pi)).astype(np.float64)
        total[m] = float(np.sum(-d.imag) / np.longdouble(np.pi))
        cn = np.linalg.norm(G.astype(np.complex128), axis=0)
        ad = np.abs(d.astype(np.complex128))
        bsite[m] = (truth.delta(m, c) * cn + U * ad) / np.pi
        btot[m] = np.sum(truth.delta(m, c) * cn + n * U * ad) / np.pi
    return total, site, btot, bsite


# --------------------------------------------------------------------------- #
# textbook Gauss-Jordan (calibration and planted defects)
# --------------------------------------------------------------------------- #
def gauss_jordan(A, pivot="abs1", recip_rel=0.0):
    """In-place-style Gauss-Jordan on [A | I] in complex128.  pivot: "abs1" = izamax (|re| + |im|), "re" = |re| only
    (a planted defect), "none" = no row exchanges (a planted defect); recip_rel: relative error planted in 1/p."""
    A = np.asarray(A, dtype=np.complex128)
    n = A.shape[0]
    M = np.concatenate([A, np.eye(n, dtype=np.complex128)], axis=1)
    for k in range(n):
        if pivot != "none":
            col = M[k:, k]
            key = np.abs(col.real) + (np.abs(col.imag) if pivot == "abs1" else 0.0)
            p = k + int(np.argmax(key))
            if p != k:
                M[[k, p]] = M[[p, k]]
        r = (1.0 / M[k, k]) * (1.0 + recip_rel)
        M[k] *= r
        f = M[:, k].copy()
        f[k] = 0.0
        M -= np.outer(f, M[k])
    return M[:, n:]
