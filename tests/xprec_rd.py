"""Extended-precision truth, float64 restatements, bar and planted defects of the renormalisation-decimation
("doubling") solver of the 1-D chain surface Green's function (negf_sigma_chain1d_rd, k_chain1d_rd.hip).  Shared by
test_chain_rd_host.py (CPU) and test_chain_rd_gpu.py (MI355X).

The recursion (the definition the kernel is held to), with z = E + i eta formed in float64:
    es = e = A = z Sa - a,  a = B = z Sb - b,  b = B^H
    step:  G = inv(e);  P = a G;  Q = b G;  D = P b
           es <- es - D;   e <- (e - D) - Q a;   a <- P a;   b <- Q b;   steps += 1
    stop after the step in which  max |D_ij| <= tol * max |es_ij|  (es updated; |x| = |re| + |im|), or at max_steps
    g = inv(es);   Sigma = t g t^H,  t = E St - tau.

Truth: the recursion in np.clongdouble from the float64 inputs (products by xprec_chain.mm, inverses by xprec.refine as
xprec_chain._inv_ld), run TWO steps past its own stop; the states after 0, 1 and 3 steps are kept as the truths at a
fixed step count.  A scaled lead (xprec_chain.scaled) derives everything from its base exactly.

Bar.  The error amplification of the recursion is not first order in any single condition number, so the bar is relative
to what float64 arithmetic achieves on the case:
    bar_g = C_RD * max(err_numpy, err_gj) + READBACK_U + xprec.bar(n, kappa_2(es))
every term a Frobenius error relative to ||g||; err_numpy is the recursion with numpy.linalg.inv and @, err_gj the same
with xprec.gauss_jordan, both against the truth; the last two terms are what the chain tests already allow the last
inverse and the identity-tau read-back.  For Sigma the g term (without the read-back) is propagated through t . t^H as
xprec_chain.ChainTruth does for its sigma_bound.  C_RD = 2 R_host rounded up to a power of two, R_host the worst ratio
between the two restatements' errors over the host case table (test_chain_rd_host.py measures it and asserts that the
constant below still covers it); the factor two because the kernel differs from BOTH restatements at once (pivot ties,
3M products).
"""
import numpy as np

import xprec
import xprec_chain as xc
from xprec import LD, U, gamma_n, kappa2

TOL = 2.0 ** -52
MAX_STEPS = 64
K_FIXED = (0, 1, 3)
C_RD = 16.0                           # 2 * R_host (6.4 on the host table, free running) rounded up to a power of two
ETAS = (1e-4, 1e-6)
HOST_SIZES = (9, 33, 50)


def abs1(X):
    X = np.asarray(X)
    return np.abs(X.real) + np.abs(X.imag)


def _nf(X):
    return float(np.linalg.norm(np.asarray(X, dtype=np.complex128)))


def _n2(X):
    return float(np.linalg.norm(np.asarray(X, dtype=np.complex128), 2))


def leads(n):
    """The base leads of size n: L1 and L2 at both eta (their scaled forms are derived, see RdTruth.of)."""
    out = []
    for eta in ETAS:
        out += [xc.lead_l1(n, eta=eta), xc.lead_l2(n, eta=eta)]
    return out


def cases(n):
    """[(lead, E)]: every base lead of size n with its three energies (in band, complex, near-edge)."""
    return [(lead, complex(E)) for lead in leads(n) for E in lead.energies]


# --------------------------------------------------------------------------- #
# the recursion: float64 restatements and planted defects
# --------------------------------------------------------------------------- #
def rd64(lead, E, K=None, inv=np.linalg.inv, prod=None, tol=TOL, max_steps=MAX_STEPS, defect=None):
    """(g, Sigma, steps, converged) of the float64 recursion; K >= 0 runs exactly K steps.  inv / prod(X, Y) replace
    the inverse / the six products; defect: None, "no_qa" (the Q a term dropped from the e update), "bT" (b = B^T
    without the conjugate)."""
    A, B, t = lead.A64(E), lead.B64(E), lead.t64(E)
    prod = prod or (lambda X, Y: X @ Y)
    es, e, a = A.copy(), A.copy(), B.copy()
    b = B.T.copy() if defect == "bT" else B.conj().T.copy()
    steps, conv = 0, False
    while (steps < K) if K is not None and K >= 0 else (not conv and steps < max_steps):
        G = inv(e)
        P, Q = prod(a, G), prod(b, G)
        D = prod(P, b)
        es = es - D
        e = (e - D) if defect == "no_qa" else (e - D) - prod(Q, a)
        a, b = prod(P, a), prod(Q, b)
        steps += 1
        with np.errstate(invalid="ignore", over="ignore"):
            conv = bool(np.max(abs1(D)) <= tol * np.max(abs1(es))) and bool(np.isfinite(np.max(abs1(es))))
    g = inv(es)
    return g, t @ g @ t.conj().T, steps, conv


def prod_c64(X, Y):
    """A product summed in complex64 (a planted defect)."""
    return (X.astype(np.complex64) @ Y.astype(np.complex64)).astype(np.complex128)


def unrelaxed_ld(lead, E, sweeps):
    """`sweeps` sweeps of g <- inv(A - B g B^H) from inv(A), in clongdouble."""
    z = lead.z(E)
    A = LD(z) * xc._ld(lead.Salpha) - xc._ld(lead.alpha)
    B = LD(z) * xc._ld(lead.Sbeta) - xc._ld(lead.beta)
    Bh = B.conj().T
    g = xc._inv_ld(A, kappa2(A.astype(np.complex128)))
    for _ in range(sweeps):
        M = A - xc.mm(xc.mm(B, g), Bh)
        g = xc._inv_ld(M, kappa2(M.astype(np.complex128)))
    return g


# --------------------------------------------------------------------------- #
# truth
# --------------------------------------------------------------------------- #
class RdTruth:
    """The clongdouble recursion of one (base lead, energy): g and Sigma free running (two steps past its own stop:
    .g, .sigma, .stop = the step at which the stop rule fired) and after K in K_FIXED steps (.gK[K], .sigmaK[K]),
    kappa_2 of the matrix of the last inverse (.kappa, .kappaK[K]), and the fixed-point residual of g (.residual)."""

    def __init__(self, lead, E, ks=K_FIXED, extra=2):
        assert lead.base is None, "derive the truth of a scaled lead with RdTruth.of"
        self.lead, self.E = lead, complex(E)
        z = lead.z(E)
        A = LD(z) * xc._ld(lead.Salpha) - xc._ld(lead.alpha)
        B = LD(z) * xc._ld(lead.Sbeta) - xc._ld(lead.beta)
        self.t = LD(complex(E)) * xc._ld(lead.Stau) - xc._ld(lead.tau)
        Bh = B.conj().T
        es, e, a, b = A, A, B, Bh
        inv = lambda M: xc._inv_ld(M, kappa2(M.astype(np.complex128)))
        self.gK, self.sigmaK, self.kappaK = {}, {}, {}
        steps, stop = 0, None
        while True:
            if steps in ks:
                self.kappaK[steps] = kappa2(es.astype(np.complex128))
                self.gK[steps] = inv(es)
                self.sigmaK[steps] = self._sigma(self.gK[steps])
            if (stop is not None and steps >= stop + extra) or steps >= MAX_STEPS:
                break
            G = inv(e)
            P, Q = xc.mm(a, G), xc.mm(b, G)
            D = xc.mm(P, b)
            es = es - D
            e = (e - D) - xc.mm(Q, a)
            a, b = xc.mm(P, a), xc.mm(Q, b)
            steps += 1
            if stop is None and float(np.max(abs1(D))) <= TOL * float(np.max(abs1(es))):
                stop = steps
        assert stop is not None, "the extended-precision recursion did not stop"
        self.stop, self.steps = stop, steps
        self.kappa = kappa2(es.astype(np.complex128))
        self.g = inv(es)
        self.sigma = self._sigma(self.g)
        M = A - xc.mm(xc.mm(B, self.g), Bh)
        self.residual = _nf(self.g - inv(M)) / _nf(self.g)

    def _sigma(self, g):
        return xc.mm(xc.mm(self.t, g), self.t.conj().T)

    @staticmethod
    def of(lead, base_truth):
        """The truth of a scaled lead: g -> 2^-k g, Sigma -> 2^k Sigma, exactly."""
        t = RdTruth.__new__(RdTruth)
        f = 2.0 ** lead.k
        t.lead, t.E = lead, base_truth.E * f
        t.t = base_truth.t * LD(f)
        t.stop, t.steps, t.kappa, t.kappaK, t.residual = (base_truth.stop, base_truth.steps, base_truth.kappa,
                                                          base_truth.kappaK, base_truth.residual)
        t.g, t.sigma = base_truth.g * LD(1.0 / f), base_truth.sigma * LD(f)
        t.gK = {K: g * LD(1.0 / f) for K, g in base_truth.gK.items()}
        t.sigmaK = {K: s * LD(f) for K, s in base_truth.sigmaK.items()}
        return t

    def g_of(self, K=None):
        return self.g if K is None else self.gK[K]

    def sigma_of(self, K=None):
        return self.sigma if K is None else self.sigmaK[K]

    def g_err(self, g_hat, K=None):
        """||g_hat - g|| / ||g||, Frobenius."""
        g = self.g_of(K)
        return _nf(np.asarray(g_hat).astype(LD) - g) / _nf(g)

    def sigma_err_abs(self, s_hat, K=None):
        return _nf(np.asarray(s_hat).astype(LD) - self.sigma_of(K))


class RdBar:
    """The bar of one (base lead, energy) at step count K (None: free running), from the two float64 restatements."""

    def __init__(self, truth, K=None):
        lead, E = truth.lead, truth.E
        assert lead.base is None
        self.truth, self.K = truth, K
        n = lead.n
        gn, _, self.steps_numpy, self.conv_numpy = rd64(lead, E, K)
        gj, _, self.steps_gj, self.conv_gj = rd64(lead, E, K, inv=xprec.gauss_jordan)
        self.err_numpy, self.err_gj = truth.g_err(gn, K), truth.g_err(gj, K)
        kap = truth.kappa if K is None else truth.kappaK[K]
        self.core = C_RD * max(self.err_numpy, self.err_gj) + xprec.bar(n, kap)
        self.g_bar = self.core + xc.READBACK_U
        # Sigma = t g t^H: the g term through ||t||_2^2, forming t, the two products, the final rounding
        g64 = np.asarray(truth.g_of(K), dtype=np.complex128)
        t64 = np.asarray(truth.t, dtype=np.complex128)
        eT = gamma_n(4) * _nf(abs(E) * np.abs(lead.Stau) + np.abs(lead.tau))
        at = np.abs(t64)
        self.sigma_bar_abs = (_n2(t64) ** 2 * self.core * _nf(g64) + 2 * eT * _n2(t64) * _n2(g64)
                              + gamma_n(4 * n) * _nf(at @ np.abs(g64) @ at.T) + U * _nf(truth.sigma_of(K)))

    def g_ratio(self, g_hat, truth=None):
        """error / bar of a g (of the base lead, or of the scaled lead whose derived truth is given)."""
        return (truth or self.truth).g_err(g_hat, self.K) / self.g_bar

    def sigma_ratio(self, s_hat, truth=None):
        t = truth or self.truth
        f = 2.0 ** (t.lead.k if t.lead.base is not None else 0)
        return t.sigma_err_abs(s_hat, self.K) / (self.sigma_bar_abs * f)


def build(lead, E):
    """(truth, {K: bar}) of one base case, K in (None,) + K_FIXED."""
    t = RdTruth(lead, E)
    return t, {K: RdBar(t, K) for K in (None,) + K_FIXED}
