"""Extended-precision truth and first-order bars for the 1-D chain fixed point (the chain contact self-energy,
oracle.chain1d_g / surfG1D.py:223-295), the lead case table and planted defects of the chain kernels.  Shared by
test_chain_accuracy_host.py (CPU) and test_chain_accuracy_gpu.py (MI355X).

Truth at a fixed sweep count K, in np.clongdouble from the float64 inputs (every inverse by xprec.refine):
    z = E + i eta (formed in float64, as every implementation does),  A = z Sa - a,  B = z Sb - b,  t = E St - tau,
    g_0 = A^-1,  M_k = A - B g_k B^H,  h_k = M_k^-1,  g_{k+1} = r h_k + (1 - r) g_k,  Sigma = t g_K t^H.

Bar.  First-order propagation of the rounding errors along the truth's own iterates, Frobenius norms:
    d_0     = c sqrt(n) u kappa_2(A) ||g_0|| + ||g_0||_2^2 e_A
    d_{k+1} = (1 - r) d_k + r ||h_k B||_2 ||B^H h_k||_2 d_k + r ||h_k||_2^2 e_k + r c sqrt(n) u kappa_2(M_k) ||h_k||
              + 2 u ||g_{k+1}||
    e_k     = e_A + 2 e_B ||g_k||_2 ||B||_2 + gamma_4n || |B| |g_k| |B^H| || + u ||M_k||
(e_A, e_B: forming A and B, gamma_4 || |z| |S| + |a| ||; the two 3M products of inner dimension n as in
xprec.grless_truth_and_bound; the subtraction) and
    ||Sigma_hat - Sigma|| <= ||t||_2^2 d_K + 2 e_t ||t||_2 ||g_K||_2 + gamma_4n || |t| |g_K| |t^H| || + u ||Sigma||.
c = C_BAR = 2, the constant of the inverse bar (test_chain_accuracy_host.py calibrates it on the float64 oracle).
The per-sweep factor (1 - r) + r ||h_k B||_2 ||B^H h_k||_2 is the bound's growth: where its product over K sweeps
exceeds MAX_GROWTH the bound says nothing any more, and the tests keep K below that (checked_k).
"""
import numpy as np

import xprec
from helpers import chain_lead
from xprec import C_BAR, LD, U, gamma_n, kappa2

RELAX = 0.1                          # relFactor of the reference (SURFACE_RELAXATION_FACTOR)
ETA = 1e-4
MAX_GROWTH = 1e3                     # largest growth of the first-order bound over K sweeps that a test relies on
K_CHECKED = (0, 1, 3, 10)            # sweep counts checked where the growth allows (checked_k)


def _ld(X):
    return np.asarray(X).astype(LD)


def mm(X, Y):
    """clongdouble product through four np.longdouble ones (much faster than the complex loop)."""
    Xr, Xi = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)
    Yr, Yi = np.ascontiguousarray(Y.real), np.ascontiguousarray(Y.imag)
    out = np.empty((X.shape[0], Y.shape[1]), dtype=LD)
    out.real = Xr @ Yr - Xi @ Yi
    out.imag = Xr @ Yi + Xi @ Yr
    return out


def _inv_ld(A, kappa):
    n = A.shape[0]
    X, _ = xprec.refine([(A, np.arange(n))], [max(1e-3 * xprec.bar(n, kappa, 1.0), 2.0 ** -58)])[0]
    return X


def _n2(X):
    return float(np.linalg.norm(np.asarray(X, dtype=np.complex128), 2))


def _nf(X):
    return float(np.linalg.norm(np.asarray(X, dtype=np.complex128)))


# --------------------------------------------------------------------------- #
# the lead case table
# --------------------------------------------------------------------------- #
class Lead:
    """One lead (alpha, S_alpha, beta, S_beta, tau, S_tau, eta) and its energies.  `base` / `k`: an L3 case is its
    base with alpha, beta, tau, E and eta times 2^k (overlaps unchanged), so g -> 2^-k g and Sigma -> 2^k Sigma."""

    def __init__(self, name, alpha, Salpha, beta, Sbeta, tau, Stau, energies, eta=ETA, base=None, k=0):
        self.name = name
        self.alpha, self.Salpha, self.beta, self.Sbeta, self.tau, self.Stau = (
            np.asarray(m, dtype=np.float64) if np.isrealobj(m) else np.asarray(m)
            for m in (alpha, Salpha, beta, Sbeta, tau, Stau))
        self.energies = np.asarray(energies, dtype=np.complex128)
        self.eta, self.base, self.k = eta, base, k

    @property
    def n(self):
        return self.alpha.shape[0]

    def z(self, E):
        return complex(E) + 1j * self.eta

    def A64(self, E):
        return self.z(E) * self.Salpha - self.alpha

    def B64(self, E):
        return self.z(E) * self.Sbeta - self.beta

    def t64(self, E):
        return complex(E) * self.Stau - self.tau

    def kwargs(self):
        """surfG / oracle.Chain1DSigma keyword arguments of a one-contact provider."""
        return dict(taus=[self.tau], staus=[self.Stau], alphas=[self.alpha], aOverlaps=[self.Salpha],
                    betas=[self.beta], bOverlaps=[self.Sbeta])


def lead_l1(n, seed=0, eta=ETA):
    """L1: C3-style random lead (helpers.chain_lead, tau = beta as in the C3 configuration); energies in band,
    complex and the near-band-edge point (edge_energy)."""
    a, sa, b, sb = chain_lead(n, 500 + n + seed)
    lead = Lead("L1", a, sa, b, sb, b.copy(), sb.copy(), [0.3, 0.2 + 0.3j], eta=eta)
    lead.energies = np.append(lead.energies, edge_energy(lead))
    return lead


def lead_l2(n, seed=0, eta=ETA):
    """L2: L1 with core levels 1e2 ... 1e4 on every fifth diagonal entry of alpha (an all-electron basis in eV)."""
    l1 = lead_l1(n, seed, eta)
    a = l1.alpha.copy()
    core = np.arange(2, n, 5)
    a[core, core] += np.logspace(2, 4, core.size)
    return Lead("L2", a, l1.Salpha, l1.beta, l1.Sbeta, l1.tau, l1.Stau, l1.energies, eta=eta)


def scaled(lead, k):
    """L3: alpha, beta, tau, E and eta times 2^k, the overlaps unchanged: A, B, t -> 2^k (A, B, t) exactly."""
    f = 2.0 ** k
    return Lead(f"{lead.name}x2^{k}", f * lead.alpha, lead.Salpha, f * lead.beta, lead.Sbeta, f * lead.tau,
                lead.Stau, f * lead.energies, eta=f * lead.eta, base=lead, k=k)


EDGE_GRID = np.linspace(-3.0, 3.0, 200)
EDGE_K = 10


def edge_energy(lead, K=EDGE_K):
    """The energy of a 200-point grid on [-3, 3] where kappa_2(M_K) is largest (the near-band-edge case), from the
    float64 iterates (kappa to its leading digits)."""
    best, arg = -1.0, EDGE_GRID[0]
    for E in EDGE_GRID:
        A, B = lead.A64(E), lead.B64(E)
        g = np.linalg.inv(A)
        for _ in range(K):
            M = A - B @ g @ B.conj().T
            g = RELAX * np.linalg.inv(M) + (1 - RELAX) * g
        M = A - B @ g @ B.conj().T
        kap = kappa2(M)
        if kap > best:
            best, arg = kap, E
    return float(arg)


# --------------------------------------------------------------------------- #
# truth and bound
# --------------------------------------------------------------------------- #
class ChainTruth:
    """Iterates g_0 .. g_Kmax of one (lead, energy) in clongdouble with the bound d_k of every one, Sigma_K and its
    bound, and the growth of the first-order bound.  An L3 lead derives everything from its base exactly."""

    def __init__(self, lead, E, Kmax, c=C_BAR, r=RELAX):
        assert lead.base is None, "derive the truth of a scaled lead with ChainTruth.of"
        self.lead, self.E, self.Kmax, self.c, self.r = lead, complex(E), Kmax, c, r
        n = lead.n
        z = lead.z(E)
        A = LD(z) * _ld(lead.Salpha) - _ld(lead.alpha)
        B = LD(z) * _ld(lead.Sbeta) - _ld(lead.beta)
        t = LD(complex(E)) * _ld(lead.Stau) - _ld(lead.tau)
        Bh = B.conj().T
        A64, B64 = A.astype(np.complex128), B.astype(np.complex128)
        aB = np.abs(B64)
        eA = gamma_n(4) * _nf(abs(z) * np.abs(lead.Salpha) + np.abs(lead.alpha))
        eB = gamma_n(4) * _nf(abs(z) * np.abs(lead.Sbeta) + np.abs(lead.beta))
        nB = _n2(B64)
        self.kappa_A = kappa2(A64)
        g = _inv_ld(A, self.kappa_A)
        g64 = g.astype(np.complex128)
        d = c * np.sqrt(n) * U * self.kappa_A * _nf(g64) + _n2(g64) ** 2 * eA
        self.g, self.d, self.kappa_M, self.rho = [g], [d], [], []
        for _ in range(Kmax):
            M = A - mm(mm(B, g), Bh)
            M64 = M.astype(np.complex128)
            kM = kappa2(M64)
            h = _inv_ld(M, kM)
            h64 = h.astype(np.complex128)
            rho = _n2(h64 @ B64) * _n2(B64.conj().T @ h64)
            e = (eA + 2 * eB * _n2(g64) * nB + gamma_n(4 * n) * _nf(aB @ np.abs(g64) @ aB.T) + U * _nf(M64))
            g = LD(r) * h + (LD(1) - LD(r)) * g
            g64 = g.astype(np.complex128)
            d = ((1 - r) * d + r * rho * d + r * _n2(h64) ** 2 * e + r * c * np.sqrt(n) * U * kM * _nf(h64)
                 + 2 * U * _nf(g64))
            self.g.append(g); self.d.append(d); self.kappa_M.append(kM); self.rho.append(rho)
        self.growth = np.cumprod([1.0] + [(1 - r) + r * p for p in self.rho])
        self.t = t
        t64 = t.astype(np.complex128)
        self.sigma, self.sigma_bound = [], []
        eT = gamma_n(4) * _nf(abs(complex(E)) * np.abs(lead.Stau) + np.abs(lead.tau))
        at = np.abs(t64)
        for K in range(Kmax + 1):
            gK = self.g[K]
            S = mm(mm(t, gK), t.conj().T)
            gK64 = gK.astype(np.complex128)
            self.sigma.append(S)
            self.sigma_bound.append(_n2(t64) ** 2 * self.d[K] + 2 * eT * _n2(t64) * _n2(gK64)
                                    + gamma_n(4 * n) * _nf(at @ np.abs(gK64) @ at.T)
                                    + U * _nf(S.astype(np.complex128)))

    @staticmethod
    def of(lead, base_truth):
        """The truth of a scaled (L3) lead: g_k -> 2^-k g_k, Sigma -> 2^k Sigma, bounds likewise, all exact."""
        t = ChainTruth.__new__(ChainTruth)
        f = 2.0 ** lead.k
        t.lead, t.E, t.Kmax, t.c, t.r = lead, base_truth.E * f, base_truth.Kmax, base_truth.c, base_truth.r
        t.kappa_A, t.kappa_M, t.rho, t.growth = base_truth.kappa_A, base_truth.kappa_M, base_truth.rho, base_truth.growth
        t.g = [g * LD(1.0 / f) for g in base_truth.g]
        t.d = [d / f for d in base_truth.d]
        t.sigma = [s * LD(f) for s in base_truth.sigma]
        t.sigma_bound = [b * f for b in base_truth.sigma_bound]
        t.t = base_truth.t * LD(f)
        return t

    def usable(self, K):
        return self.growth[K] <= MAX_GROWTH

    def g_ratio(self, K, g_hat, readback=0.0):
        """||g_hat - g_K||_F / (d_K + readback * ||g_K||_F)."""
        gK = self.g[K]
        err = _nf((np.asarray(g_hat).astype(LD) - gK).astype(np.complex128))
        return err / (self.d[K] + readback * _nf(gK.astype(np.complex128)))

    def sigma_ratio(self, K, s_hat):
        err = _nf((np.asarray(s_hat).astype(LD) - self.sigma[K]).astype(np.complex128))
        return err / self.sigma_bound[K]


def checked_k(truth, kmax):
    """The sweep counts a test checks on one truth: 0, 1, 3 and 10 where the bound's growth stays below MAX_GROWTH,
    and the last such K <= kmax."""
    usable = [K for K in range(min(kmax, truth.Kmax) + 1) if truth.usable(K)]
    return sorted({K for K in K_CHECKED if K in usable} | {usable[-1]})


READBACK_U = 4 * U
"""g read back through the identity-tau variant (tau = -I, S_tau = 0: its 'self-energy' t g t^H is g): the final pass
runs the two products of Sigma = t g t^H in 3M form, whose real parts are exact for t = I (a sum of one product
g_ij * 1 and zeros) but whose imaginary parts are (g_re + g_im) - g_re - 0, one rounding of the sum and one of the
difference per pass: at most 4 u |g_ij| over the two passes, 4 u ||g e_j|| per column."""


# --------------------------------------------------------------------------- #
# float64 fixed points: the oracle's and planted defects
# --------------------------------------------------------------------------- #
def gauss_jordan_phat(A):
    """In-place Gauss-Jordan (implicit izamax pivoting, no row exchanges) whose pivot rows are updated in the stored
    form P - E of the LDS chain kernel before its fix: the pivot element is kept as 1/p - 1, every other column j of
    the pivot row becomes q_j + (1/p - 1) q_j, and the inverse is read back as (x - 1) + 1 at (pivot row, column)."""
    W = np.array(A, dtype=np.complex128)
    n = W.shape[0]
    used = np.zeros(n, dtype=bool)
    piv = np.empty(n, dtype=int)
    for k in range(n):
        key = np.where(used, -1.0, np.abs(W[:, k].real) + np.abs(W[:, k].imag))
        p = int(np.argmax(key))
        piv[k] = p; used[p] = True
        pv = W[p, k]
        ip = np.conj(pv) * (1.0 / (pv.real * pv.real + pv.imag * pv.imag))
        f = -W[:, k] * ip
        q = W[p].copy()
        coef = f.copy(); coef[p] = ip - 1.0                 # P - E: the pivot row's multiplier is one short
        W += np.outer(coef, q)
        W[:, k] = f; W[p, k] = ip - 1.0
    G = np.empty_like(W)
    colof = np.empty(n, dtype=int); colof[piv] = np.arange(n)
    for i in range(n):
        G[i] = W[piv[i], colof]
    G[np.arange(n), piv] += 1.0                             # (the stored x - 1 at (pivot row, its column))
    return G


def chain64(lead, E, K, inv=np.linalg.inv, prod=None, r=RELAX):
    """g_K and Sigma_K of the float64 fixed point (oracle.chain1d_g / chain1d_sigma_block with force_iters = K when
    inv and prod are the defaults); `inv` / `prod(B, g)` = B g B^H replace the inverse / product for a planted defect."""
    A, B, t = lead.A64(E), lead.B64(E), lead.t64(E)
    Bh = B.conj().T
    prod = prod or (lambda B_, g_: B_ @ g_ @ B_.conj().T)
    g = inv(A)
    for _ in range(K):
        h = inv(A - prod(B, g))
        g = h * r + g * (1 - r)
    return g, t @ g @ t.conj().T


def prod_c64(B, g):
    """B g B^H summed in complex64 (a planted defect)."""
    return (B.astype(np.complex64) @ g.astype(np.complex64) @ B.conj().T.astype(np.complex64)).astype(np.complex128)
