"""Extended-precision truth, first-order bars and the case table of the eigenchannel path (pchol_kernel, jacobi_kernel,
gauge_kernel and the products between them in negf_transmission_channels / negf_channel_states), shared by
test_channels_accuracy_host.py (CPU) and test_channels_accuracy_gpu.py (MI355X).

Truth, independent of the device's algorithm (np.clongdouble, 64-bit mantissa).  With B = G[:, I_s] from the iterative
refinement of xprec.py, G_ds = B[I_d], M = G_ds^H Gamma_d G_ds and Gamma_s[I_s, I_s] = R R^H, R = V sqrt(max(w, 0)) from
herm_eig_ld (no pivoting, no cut):  T = eig(R^H M R) descending,  psi_n = B R u_n in the gauge of fix_gauge.  For chain
leads the truth takes the device's own Sigma(E) as data (the Sigma kernels have their own bars).

herm_eig_ld: LAPACK's fp64 eigenvectors, orthonormalised in clongdouble (Newton-Schulz), bring A close to diagonal; a cyclic
two-sided Jacobi in clongdouble, round-robin order, the disjoint rotations of a step applied together (each touches its
two rows and two columns only), finishes at the clongdouble epsilon.  Clusters are Jacobi's to resolve, so they are.
test_channels_accuracy_host.py checks it against mpmath at 40 digits.

Bars (u = 2^-53, delta = xprec.bar(n, kappa_2(A)), gamma_k = k u / (1 - k u), EIGH_C of channel_states_ref; r the rank
the implementation under test used).  Every check is  error <= C_CHAN * beta:
  beta_T     |T^_n - T_n| (Weyl), the sum of
               inverse    2 delta ||B||_F ||R||_2 ||Gamma_d G_ds R||_2
               products   gamma_{4(K_s+K_d)} || |R^H| |G_ds^H| |Gamma_d| |G_ds| |R| ||_F
               Jacobi     EIGH_C K_s u ||H||_F
               Cholesky   (gamma_{K_s+1} ||Gamma_s||_2 + (K_s - r) 1e-14 max diag Gamma_s) ||M||_2
  beta_orth  ||Psi^H Gamma_d Psi - diag T||_max of the outputs themselves: products + Jacobi only (H and Psi[I_d] come
             from the same G^: the inverse's error cancels to first order, so this bar does not grow with kappa)
  beta_spec  ||Psi Psi^H - B Gamma_s B^H||_F:  (2 delta + EIGH_C K_s u + gamma_{4 K_s}) ||B||_F ||B Gamma_s||_F
             + the Cholesky factor times ||B||_2^2
  beta_state ||P^_C - P_C||_F, P_C = sum_{n in C} psi_n psi_n^H over clusters C of the true T with gap_C >= 1e-3 max T:
             2 ||B R||_2^2 beta_T / gap_C + 2 delta ||P_C||_F;  a singleton's gauge-fixed psi_n:
             ||B R||_2 beta_T / gap_C + 2 delta ||psi_n||
  solver     |w^_i - w_i| <= EIGH_C K u ||A||_F;  ||V^_C V^_C^H - V_C V_C^H||_F <= 2 EIGH_C K u ||A||_F / gap_C

C_CHAN = 2^-5: the smallest power of two at least twice the worst error / beta that two fp64 numpy references reach on the
case table (both with G from LAPACK's inv): channel_states_ref with numpy.linalg.eigh, and with jacobi_eigh on the same
pivoted_cholesky.  Worst ratios measured on the CPU (test_channels_accuracy_host.test_calibration recomputes them):
  T     0.00159  (70,9,80) dgraded16 E[0], eigh          orth  0.00939  (9,5,40) ladder E[2] (kappa 4e5), jacobi_eigh
  rank  2.0e-05  (21,30,70) dgraded16 E[0], eigh         spec  0.00706  (9,5,40) graded12 E[1], eigh
  sum   0.00021  (9,5,40) ladder E[5], eigh              proj  0.00274  (9,5,40) ladder E[5], jacobi_eigh
  psi   0.00333  (9,5,40) ladder E[5], jacobi_eigh       chan  0.00371  (9,5,40) ladder E[5], jacobi_eigh
worst 0.00939, twice that 0.0188 -> C_CHAN = 2^-5 = 0.03125.  The constant is below one because the bars are worst-case
first-order bounds (gamma_k times a norm of absolute values; EIGH_C carries the orthonormality defect of 96 x 96
accumulations) while float64 errors on these inputs are a few u: the calibrated bar is what separates a correct
implementation from one that stops its sweeps at 1e-12 (planted, caught by orth at 95 times the bar).
The rule's margin is thin on one side: below a worst ratio of 0.0078 it gives 2^-6, and the worst ratio comes from
jacobi_eigh on one ladder energy, so another LAPACK / BLAS build may move test_calibration's strict equality (the other
calibration tests of the project assert their constants the same way).
"""
import functools

import numpy as np

import channel_states_ref as R
import xprec
from helpers import random_system, chain_lead
from xprec import LD, U, gamma_n

C_CHAN = 2.0 ** -5
EIGH_C = R.EIGH_C
CUT = 1e-14                          # the device's pivoted-Cholesky cut, relative to max diag Gamma_s
GAP = 1e-3                           # clusters: separated by >= GAP * max T
LR = np.longdouble
EPS_LD = float(np.finfo(LR).eps)


# --------------------------------------------------------------------------- #
# Hermitian eigensolver in extended precision
# --------------------------------------------------------------------------- #
def _rr_pairs(N):
    """The N - 1 steps of the round-robin schedule on N (even) players: [(p [N/2], q [N/2])]."""
    M = N - 1
    out = []
    P = np.arange(1, N // 2)
    for st in range(M):
        p = np.concatenate([[M], (st + P) % M])
        q = np.concatenate([[st], (st - P + M) % M])
        out.append((p, q))
    return out


def jacobi_ld(A, max_sweeps=40):
    """Cyclic two-sided Jacobi on the Hermitian clongdouble A: (diagonal, accumulated rotations X, sweeps).  A step's
    N/2 disjoint rotations are applied together; each touches its two rows and columns only (O(N) per rotation)."""
    K = A.shape[0]
    N = K + (K & 1)
    M = np.zeros((N, N), dtype=LD)
    M[:K, :K] = 0.5 * (A + A.conj().T)
    X = np.eye(N, dtype=LD)
    fro = np.sqrt(np.sum(M.real ** 2 + M.imag ** 2))
    tol = EPS_LD * fro
    skip = tol / (4 * max(N, 1))
    steps = _rr_pairs(N) if N >= 2 else []
    one = LR(1)
    for sweep in range(max_sweeps + 1):
        off = M - np.diag(np.diagonal(M))
        if np.sqrt(np.sum(off.real ** 2 + off.imag ** 2)) <= tol:
            break
        assert sweep < max_sweeps, "jacobi_ld did not converge"
        for p, q in steps:
            b = M[p, q]
            ab = np.abs(b)
            act = ab > skip
            if not np.any(act):
                continue
            abs_ = np.where(act, ab, one)
            z = (M[q, q].real - M[p, p].real) / (2 * abs_)
            t = np.where(z >= 0, one, -one) / (np.abs(z) + np.sqrt(z * z + one))
            c = one / np.sqrt(t * t + one)
            s = t * c
            c = np.where(act, c, one)
            sw = np.where(act, s * (b / abs_), 0).astype(LD)             # J = [[c, s w], [-s conj(w), c]]
            swc = sw.conj()
            Cp, Cq = M[:, p], M[:, q]                                    # columns: A J
            M[:, p], M[:, q] = Cp * c - Cq * swc, Cp * sw + Cq * c
            Rp, Rq = M[p, :], M[q, :]                                    # rows: J^H (A J)
            M[p, :], M[q, :] = Rp * c[:, None] - Rq * sw[:, None], Rp * swc[:, None] + Rq * c[:, None]
            M[p, q] = np.where(act, 0, M[p, q]); M[q, p] = np.where(act, 0, M[q, p])
            M[p, p] = M[p, p].real; M[q, q] = M[q, q].real
            Xp, Xq = X[:, p], X[:, q]
            X[:, p], X[:, q] = Xp * c - Xq * swc, Xp * sw + Xq * c
    return np.diagonal(M).real[:K].copy(), X[:K, :K], sweep


def herm_eig_ld(A):
    """(w ascending [K] longdouble, V [K, K] clongdouble) of the Hermitian A, to the clongdouble epsilon times ||A||_F."""
    xprec.require_extended()
    A = np.asarray(A).astype(LD)
    A = 0.5 * (A + A.conj().T)
    K = A.shape[0]
    A64 = A.astype(np.complex128)
    if K > 2 and np.all(np.isfinite(A64)):
        _, V0 = np.linalg.eigh(A64)
        V0 = V0.astype(LD)
        eye = np.eye(K, dtype=LD)
        for _ in range(3):                                               # Newton-Schulz: the defect squares each time
            V0 = V0 @ (1.5 * eye - 0.5 * (V0.conj().T @ V0))
    else:
        V0 = np.eye(K, dtype=LD)
    w, X, _ = jacobi_ld(V0.conj().T @ A @ V0)
    V = V0 @ X
    order = np.argsort(w, kind="stable")
    return w[order], V[:, order]


def f64(x):
    return np.asarray(x).astype(np.complex128)


def fro(x):
    return float(np.linalg.norm(f64(x)))


def nrm2(x):
    x = f64(x)
    return float(np.linalg.norm(x, 2)) if x.size else 0.0


# --------------------------------------------------------------------------- #
# the case table
# --------------------------------------------------------------------------- #
def coupling_sigma(n, idx, gam, rng):
    """A self-energy confined to idx with the coupling gam: h - i gam / 2, h a real symmetric shift (block_sigma's)."""
    K = len(idx)
    B = rng.standard_normal((K, K)); h = 0.05 * (B + B.T)
    s = np.zeros((n, n), complex)
    s[np.ix_(idx, idx)] = h - 0.5j * gam
    return s


def graded_coupling(K, g, rng):
    """U diag(0.15 logspace(0, -g, K)) U^H with a random unitary U."""
    Q, _ = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))
    G = (Q * (0.15 * np.logspace(0, -g, K))) @ Q.conj().T
    return 0.5 * (G + G.conj().T)


def diagonally_graded_coupling(K, g, rng):
    """0.15 D (A A^H / K) D with D = logspace(-g/2, 0, K): the weakest orbitals come first, so the pivot order and the
    separately tracked diagonal decide what the factorisation keeps."""
    A = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
    D = np.logspace(-g / 2, 0, K)
    G = 0.15 * D[:, None] * (A @ A.conj().T / K) * D[None, :]
    return 0.5 * (G + G.conj().T)


class ChanCase:
    """One channel-state input: system, the two contact self-energies per energy (source first), orbital lists and
    energies.  sig_at(m) -> (Sigma_s, Sigma_d) as complex128 n x n; const cases return the same pair for every m."""

    def __init__(self, name, F, S, Is, Id, E, ss=None, sd=None, ladder=False, chain=None):
        self.name, self.F, self.S = name, F, S
        self.n = F.shape[0]
        self.Is, self.Id = np.asarray(Is), np.asarray(Id)
        self.Ks, self.Kd = len(Is), len(Id)
        self.E = np.asarray(E, dtype=np.complex128)
        self.ss, self.sd, self.ladder, self.chain = ss, sd, ladder, chain
        self.sig_dev = None                                              # chain: [(Sigma_s, Sigma_d)] per energy, from the device

    @property
    def const(self):
        return self.chain is None

    def sig_at(self, m):
        if self.const:
            return self.ss, self.sd
        assert self.sig_dev is not None, "a chain case needs the device's Sigma(E) (set sig_dev)"
        return self.sig_dev[m]


def _free_mid(Ks, Kd, n):
    return (Ks + n - Kd) // 2


def _system(Ks, Kd, n, ladder):
    """random_system, or its confined ladder variant: a spectator orbital off the contacts at a real level eps in a
    gap of the rest's spectrum, coupled at 1e-7; energies eps + d + 2e-9 i, d in {1, 1e-2, 1e-5, 1e-8, 0}, and
    0.3 + 2i: kappa_2(A) from ~1e1 to ~1e9."""
    F, S = random_system(n, Ks * 100 + Kd)
    if not ladder:
        return F, S, np.array([-0.7, 0.45], dtype=np.complex128)
    import scipy.linalg as sla
    k = _free_mid(Ks, Kd, n)
    assert Ks <= k < n - Kd
    keep = [i for i in range(n) if i != k]
    ev = np.sort(sla.eigh(F[np.ix_(keep, keep)], S[np.ix_(keep, keep)], eigvals_only=True))
    mids = (ev[1:] + ev[:-1]) / 2
    eps = float(mids[np.argmin(np.abs(mids - 0.1))])
    v = 1e-7 * np.random.default_rng(17 + n).standard_normal(n)
    F[k, :] = v; F[:, k] = v; F[k, k] = eps
    S[k, :] = 0.0; S[:, k] = 0.0; S[k, k] = 1.0
    E = [eps + d + 2e-9j for d in (1.0, 1e-2, 1e-5, 1e-8, 0.0)] + [0.3 + 2j]
    return F, S, np.array(E, dtype=np.complex128)


@functools.lru_cache(maxsize=None)
def const_case(Ks, Kd, n, family="block", ladder=False, swap=False):
    """family: "block" (block_sigma), "rank<r>" (block_sigma of exact rank r), "graded<g>" (graded_coupling),
    "dgraded<g>" (diagonally_graded_coupling).  I_s the first K_s orbitals,
    I_d the last K_d; swap=True puts the source last and the destination first."""
    assert not (swap and ladder)
    F, S, E = _system(Ks, Kd, n, ladder)
    rng = np.random.default_rng(n + Ks)
    Is = np.arange(n - Ks, n) if swap else np.arange(Ks)
    Id = np.arange(Kd) if swap else np.arange(n - Kd, n)
    if family == "block":
        ss = R.block_sigma(n, Is, rng)
    elif family.startswith("rank"):
        ss = R.block_sigma(n, Is, rng, rank=int(family[4:]))
    elif family.startswith("dgraded"):
        ss = coupling_sigma(n, Is, diagonally_graded_coupling(Ks, int(family[7:]), rng), rng)
    else:
        ss = coupling_sigma(n, Is, graded_coupling(Ks, int(family[6:]), rng), rng)
    sd = R.block_sigma(n, Id, rng)
    name = f"({Ks},{Kd},{n}) {family}" + (" ladder" if ladder else "") + (" swapped" if swap else "")
    return ChanCase(name, F, S, Is, Id, E, ss=ss, sd=sd, ladder=ladder)


LADDER_SHAPES = [(9, 5, 40), (70, 9, 80), (40, 30, 300)]
STATE_SPECS = ([(s, "block", True) for s in LADDER_SHAPES] +
               [((69, 9, 80), "block", False), ((96, 5, 110), "block", False), ((71, 30, 130), "rank33", False),
                ((21, 30, 70), "block", False), ((21, 30, 70), "rank10", False)] +
               [((9, 5, 40), f"graded{g}", False) for g in (6, 12, 17)] +
               [((70, 9, 80), f"graded{g}", False) for g in (12, 17)] +
               [((21, 30, 70), "dgraded16", False), ((70, 9, 80), "dgraded16", False)])
# transmission_channels only: (K_L, K_R) = (90, 75) on n = 180 (the mirror form above 69) and (96, 96) on n = 200, as
# channel-state cases with the source last (transmission_channels(L, R) = the channels injected by R, collected by L)
CHANNEL_ONLY_SPECS = [((75, 90, 180), "block", False), ((96, 96, 200), "block", False)]
SCALE_SPECS = [((9, 5, 40), "block", True), ((70, 9, 80), "block", True), ((71, 30, 130), "rank33", False)]
NCHAN_SPECS = [((70, 9, 80), "block", True), ((71, 30, 130), "rank33", False)]


def state_cases():
    return [const_case(*shape, family=f, ladder=l) for shape, f, l in STATE_SPECS]


def channel_only_cases():
    return [const_case(*shape, family=f, ladder=l, swap=True) for shape, f, l in CHANNEL_ONLY_SPECS]


def host_cases():
    """What the host tests run the fp64 references on: every CONST case."""
    return state_cases() + channel_only_cases()


CHAIN_NC, CHAIN_N = 72, 200
CHAIN_E = np.array([-0.8, 0.1, 0.9])


def chain_system(solver):
    """The chain provider of test_chain_provider at n_c = 72 on n = 200: (F, S, surfG provider, contact lists)."""
    from gaunegf_amd.surfG1D import surfG
    n, nc = CHAIN_N, CHAIN_NC
    F, S = random_system(n, 7)
    lead = [chain_lead(nc, 40 + k) for k in range(2)]
    ci = [list(range(nc)), list(range(n - nc, n))]
    rng = np.random.default_rng(7)
    taus = [0.2 * rng.standard_normal((nc, nc)) for _ in range(2)]
    staus = [0.02 * rng.standard_normal((nc, nc)) for _ in range(2)]
    g = surfG(F, S, ci, taus=taus, staus=staus, alphas=[l[0] for l in lead], aOverlaps=[l[1] for l in lead],
              betas=[l[2] for l in lead], bOverlaps=[l[3] for l in lead], eta=1e-3, solver=solver)
    return F, S, g, ci


def chain_case(solver, F, S, ci, sig_s, sig_d):
    c = ChanCase(f"chain {solver} ({CHAIN_NC},{CHAIN_NC},{CHAIN_N})", F, S, ci[0], ci[1], CHAIN_E, chain=solver)
    c.sig_dev = [(sig_s[m], sig_d[m]) for m in range(CHAIN_E.size)]
    return c


def scaled_case(c, k):
    """E, F, Sigma times 2^k (S stays): T unchanged, psi times 2^(-k/2), all exactly for an even k."""
    f = 2.0 ** k
    return ChanCase(f"{c.name} x2^{k}", f * c.F, c.S, c.Is, c.Id, f * c.E, ss=f * c.ss, sd=f * c.sd, ladder=c.ladder)


# --------------------------------------------------------------------------- #
# the truth
# --------------------------------------------------------------------------- #
def gamma_ld(sig, idx):
    s = np.asarray(sig)[np.ix_(idx, idx)].astype(LD)
    return LD(1j) * (s - s.conj().T)


def psd_factor_ld(gam):
    """R with gam = R R^H over the non-negative part of the spectrum (no cut), and the ascending spectrum."""
    w, V = herm_eig_ld(gam)
    return V * np.sqrt(np.maximum(w, 0)).astype(LD), w


def fix_gauge_ld(psi):
    """channel_states_ref.fix_gauge on clongdouble rows."""
    out = np.array(psi, dtype=LD)
    for k in range(out.shape[0]):
        a2 = out[k].real ** 2 + out[k].imag ** 2
        i = int(np.argmax(a2))
        a = np.sqrt(a2[i])
        if a > 0:
            out[k] = out[k] * (out[k, i].conj() / a)
    return out


class Core:
    """The eigenproblem of one (G_ds, Gamma_d, Gamma_s) in clongdouble and the norms its bars need."""

    def __init__(self, Gds, gam_d, gam_s, Rf=None):
        self.Ks = gam_s.shape[0]; self.Kd = gam_d.shape[0]
        self.gam_s, self.gam_d = gam_s, gam_d
        self.R = psd_factor_ld(gam_s)[0] if Rf is None else Rf
        self.M = Gds.conj().T @ gam_d @ Gds
        self.M = 0.5 * (self.M + self.M.conj().T)
        H = self.R.conj().T @ self.M @ self.R
        w, V = herm_eig_ld(H)
        self.T = w[::-1].copy(); self.Uv = V[:, ::-1].copy()
        self.trace = float(np.sum(self.M * gam_s.T).real)                # Tr[Gamma_d G Gamma_s G^H] = Tr[M Gamma_s]
        a = lambda x: np.abs(f64(x))
        self.n_R = nrm2(self.R)
        self.n_gdGR = nrm2(gam_d @ Gds @ self.R)
        self.n_abs = float(np.linalg.norm(a(self.R).T @ a(Gds).T @ a(gam_d) @ a(Gds) @ a(self.R)))
        self.n_H = fro(H)
        self.n_gs = nrm2(gam_s)
        self.dmax = float(np.max(np.diagonal(gam_s).real))
        self.n_M = nrm2(self.M)

    def chol_factor(self, rank):
        return gamma_n(self.Ks + 1) * self.n_gs + max(self.Ks - rank, 0) * CUT * self.dmax

    def terms(self, delta, nB, rank):
        """The four terms of beta_T (inverse, products, Jacobi, Cholesky); nB = ||B||_F."""
        return dict(inverse=2 * delta * nB * self.n_R * self.n_gdGR,
                    products=gamma_n(4 * (self.Ks + self.Kd)) * self.n_abs,
                    jacobi=EIGH_C * self.Ks * U * self.n_H,
                    cholesky=self.chol_factor(rank) * self.n_M)


class ChannelTruth:
    """Truth of one energy of a case.  `states`: the source-side problem (T, psi, B); `chan`: the problem
    transmission_channels(dst, src) solves -- the same where K_s < K_d (the mirror form factors the source), else the
    one factored on the destination's K_d orbitals: H = L_d^H B[I_d] Gamma_s B[I_d]^H L_d."""

    def __init__(self, case, m, B, kappa):
        self.case, self.m, self.B, self.kappa = case, m, B, kappa
        self.delta = xprec.bar(case.n, kappa)
        ss, sd = case.sig_at(m)
        gs, gd = gamma_ld(ss, case.Is), gamma_ld(sd, case.Id)
        Gds = B[case.Id]
        self.states = Core(Gds, gd, gs)
        self.chan = self.states if case.Ks < case.Kd else Core(Gds.conj().T, gs, gd)
        s = self.states
        self.T = s.T
        self.BR = B @ s.R
        self.psi = fix_gauge_ld((self.BR @ s.Uv).T)                      # [K_s, n]
        self.spec = B @ s.gam_s @ B.conj().T                             # G Gamma_s G^H
        self.n_B, self.n_B2 = fro(B), nrm2(B)
        self.n_BG = fro(B @ s.gam_s)
        self.n_BR = nrm2(self.BR)
        self.clusters = R.clusters(f64(self.T).real, GAP * float(self.T[0]))

    # ---- bars
    def beta_T(self, rank, which="states"):
        # (n_B = ||G[:, I_s]||_F also for which="chan" factored on the destination: its G block B[I_d] is a part of the
        #  same columns, whose column-wise error delta ||B e_j|| is what the inverse term propagates)
        c = getattr(self, which)
        return sum(c.terms(self.delta, self.n_B, rank).values())

    def beta_orth(self):
        t = self.states.terms(self.delta, self.n_B, self.case.Ks)
        return t["products"] + t["jacobi"]

    def beta_spec(self, rank):
        s = self.states
        return ((2 * self.delta + EIGH_C * s.Ks * U + gamma_n(4 * s.Ks)) * self.n_B * self.n_BG
                + s.chol_factor(rank) * self.n_B2 ** 2)

    def gap(self, g):
        T = f64(self.T).real
        lo = T[g[0] - 1] - T[g[0]] if g[0] > 0 else np.inf
        hi = T[g[-1]] - T[g[-1] + 1] if g[-1] + 1 < T.size else np.inf
        return float(min(lo, hi))

    def P(self, g, psi=None):
        p = (self.psi if psi is None else np.asarray(psi).astype(LD))[g]
        return p.T @ p.conj()

    # ---- the ratios error / beta of one implementation's outputs
    def ratios_T(self, T, rank, which="states"):
        """(worst |T^_n - T_n| / beta_T over n < rank, worst true T_n / beta_T over n >= rank, sum rule / (K beta_T))."""
        c = getattr(self, which)
        T = np.asarray(T, dtype=np.float64)
        k = min(T.size, c.T.size)
        bT = self.beta_T(rank, which)
        rk = min(rank, k)
        err = np.abs(T[:rk].astype(LR) - c.T[:rk])
        beyond = np.abs(c.T[rk:])
        tot = abs(float(np.sum(T[:k].astype(LR)) - LR(c.trace)))
        return (float(np.max(err, initial=0)) / bT, float(np.max(beyond, initial=0)) / bT, tot / (c.Ks * bT))

    def ratio_orth(self, T, psi):
        sd = self.case.sig_at(self.m)[1]
        P = np.asarray(psi).astype(LD)
        gd = LD(1j) * (np.asarray(sd).astype(LD) - np.asarray(sd).astype(LD).conj().T)
        D = P.conj() @ gd @ P.T - np.diag(np.asarray(T, dtype=np.float64)).astype(LD)
        return float(np.max(np.abs(f64(D)))) / self.beta_orth()

    def ratio_spec(self, psi, rank):
        P = np.asarray(psi).astype(LD)
        return fro(P.T @ P.conj() - self.spec) / self.beta_spec(rank)

    def ratios_state(self, psi, rank):
        """(worst ||P^_C - P_C||_F / beta_state(C), worst gauge-fixed singleton ||psi^_n - psi_n|| / its bar)."""
        bT = self.beta_T(rank)
        wp = ws = 0.0
        for g in self.clusters:
            gap = self.gap(g)
            if not gap >= GAP * float(self.T[0]) or g[-1] >= rank:
                continue
            PC = self.P(g)
            bar = 2 * self.n_BR ** 2 * bT / gap + 2 * self.delta * fro(PC)
            wp = max(wp, fro(self.P(g, psi) - PC) / bar)
            if len(g) == 1:
                t = self.psi[g[0]]
                bar = self.n_BR * bT / gap + 2 * self.delta * fro(t)
                ws = max(ws, fro(np.asarray(psi[g[0]]).astype(LD) - t) / bar)
        return wp, ws


def green_columns(case):
    """[(B = G[:, I_s] clongdouble, kappa_2(A))] per energy, by xprec's iterative refinement."""
    out = []
    systems, tols, kap = [], [], []
    for m, E in enumerate(case.E):
        ss, sd = case.sig_at(m)
        A = LD(E) * case.S.astype(LD) - case.F.astype(LD) - np.asarray(ss).astype(LD) - np.asarray(sd).astype(LD)
        k = xprec.kappa2(A)
        kap.append(k)
        for c0 in range(0, case.Ks, 32):
            systems.append((A, case.Is[c0:c0 + 32])); tols.append(max(1e-3 * xprec.bar(case.n, k, 1.0), 2.0 ** -58))
    res = xprec.refine(systems, tols)
    per = len(range(0, case.Ks, 32))
    for m in range(case.E.size):
        out.append((np.concatenate([r[0] for r in res[m * per:(m + 1) * per]], axis=1), kap[m]))
    return out


def truths(case):
    """[ChannelTruth] per energy."""
    return xprec.pmap(lambda a: ChannelTruth(case, a[0], a[1][0], a[1][1]), list(enumerate(green_columns(case))))


# --------------------------------------------------------------------------- #
# fp64 references (calibration) and their planted defects
# --------------------------------------------------------------------------- #
def reference(case, m, eig="lapack", chol="max", cut=CUT, jac_tol=None, x0_conj=False, permute=True, gds="H"):
    """channel_states_ref in float64 with G from LAPACK's inv: (T [K_s], psi [K_s, n], rank), zeros beyond the rank.
    eig: "lapack" or "jacobi" (jacobi_eigh).  The remaining arguments plant defects: chol="first" pivots by the lowest
    index, cut the Cholesky cut, jac_tol the Jacobi stop (relative to ||H||_F), x0_conj psi from conj(L), permute=False
    sorts T without permuting the vectors, gds="T" builds H from G_ds^T."""
    ss, sd = case.sig_at(m)
    G = np.linalg.inv(case.E[m] * case.S - case.F - ss - sd)
    gs, gd = R.gamma(ss)[np.ix_(case.Is, case.Is)], R.gamma(sd)[np.ix_(case.Id, case.Id)]
    L = pivoted_cholesky(gs, cut, chol)
    r = L.shape[1]
    Gds = G[np.ix_(case.Id, case.Is)]
    GdsH = Gds.conj().T if gds == "H" else Gds.T
    H = L.conj().T @ GdsH @ gd @ GdsH.conj().T @ L
    H = 0.5 * (H + H.conj().T)
    if r == 0:
        w, Uv = np.zeros(0), np.zeros((0, 0), complex)
    elif eig == "lapack":
        w, Uv = np.linalg.eigh(H)
    else:
        w, Uv = jacobi_eigh_tol(H, jac_tol)
    if permute:
        w, Uv = w[::-1], Uv[:, ::-1]
    else:
        w = w[::-1]
    X0 = L.conj() if x0_conj else L
    psi = R.fix_gauge((G[:, case.Is] @ X0 @ Uv).T)
    T = np.zeros(case.Ks); T[:r] = w
    P = np.zeros((case.Ks, case.n), complex); P[:r] = psi
    return T, P, r


def reference_channels(case, m, eig="lapack"):
    """What transmission_channels(dst, src) computes, in float64: (T [min(K_s, K_d)], rank)."""
    if case.Ks < case.Kd:
        T, _, r = reference(case, m, eig)
        return T, r
    ss, sd = case.sig_at(m)
    G = np.linalg.inv(case.E[m] * case.S - case.F - ss - sd)
    gs, gd = R.gamma(ss)[np.ix_(case.Is, case.Is)], R.gamma(sd)[np.ix_(case.Id, case.Id)]
    L = R.pivoted_cholesky(gd)
    r = L.shape[1]
    Gds = G[np.ix_(case.Id, case.Is)]
    H = L.conj().T @ Gds @ gs @ Gds.conj().T @ L
    H = 0.5 * (H + H.conj().T)
    w = (np.linalg.eigvalsh(H) if eig == "lapack" else R.jacobi_eigh(H)[0])[::-1]
    T = np.zeros(case.Kd); T[:r] = w
    return T, r


def pivoted_cholesky(G, cut=CUT, pivot="max"):
    """channel_states_ref.pivoted_cholesky; pivot="first" takes the lowest remaining index (a planted defect)."""
    if pivot == "max":
        return R.pivoted_cholesky(G, cut)
    G = np.array(G, dtype=complex)
    K = G.shape[0]
    d = G.diagonal().real.copy()
    thr = cut * np.max(d)
    cols = []
    for p in range(K):
        if not (d[p] > thr and d[p] > 0.0):
            break
        l = np.zeros(K, complex)
        l[p:] = G[p:, p] / np.sqrt(d[p])
        l[p] = np.sqrt(d[p])
        cols.append(l)
        G = G - np.outer(l, l.conj())
        d = d - np.abs(l) ** 2
    return np.array(cols).T.reshape(K, len(cols))


def jacobi_eigh_tol(A, rel_tol=None):
    """channel_states_ref.jacobi_eigh; rel_tol stops it at off^2 <= (rel_tol ||A||_F)^2 instead (a planted defect)."""
    return R.jacobi_eigh(A) if rel_tol is None else R.jacobi_eigh(A, stop_eps=rel_tol)


def all_ratios(t, T, psi, rank):
    """Every error / beta of one implementation's (T, psi, rank) against the truth t, by bar name."""
    eT, beyond, srule = t.ratios_T(T, rank)
    sp, ss = t.ratios_state(psi, rank)
    return dict(T=eT, rank=beyond, sum=srule, orth=t.ratio_orth(T, psi), spec=t.ratio_spec(psi, rank), proj=sp, psi=ss)


def device_rank(T, psi=None):
    """The rank the device used: its outputs are exact zeros from there on."""
    nz = np.nonzero(np.any(np.asarray(psi) != 0, axis=1))[0] if psi is not None else np.nonzero(np.asarray(T) != 0)[0]
    return int(nz[-1]) + 1 if nz.size else 0


def check_outputs(case, truths, T, psi, Tc, label):
    """Every bar of the channel states (T [M, K_s], psi [M, K_s, n]) and of Tc = transmission_channels(dst, src) at every
    energy of the case: prints one ACC line (error / (C_CHAN beta) per bar, worst over the energies) and asserts <= 1."""
    Ks, Kd = case.Ks, case.Kd
    assert T.shape == (case.E.size, Ks) and psi.shape == (case.E.size, Ks, case.n)
    assert Tc is None or Tc.shape == (case.E.size, min(Ks, Kd))
    worst = {}
    for m, t in enumerate(truths):
        r = device_rank(T[m], psi[m])
        assert np.all(T[m, r:] == 0.0) and np.all(psi[m, r:] == 0.0), (label, m, r)        # exact zeros beyond the rank
        assert np.all(np.diff(T[m, :r]) <= 0), (label, m)
        got = all_ratios(t, T[m], psi[m], r)
        if Tc is None:
            pass
        elif Ks < Kd:                                                                      # the mirror form: the same H
            assert np.array_equal(Tc[m], T[m]), (label, m)
            rc = r
        else:
            rc = device_rank(Tc[m])
            assert np.all(Tc[m, rc:] == 0.0)
        if Tc is not None:
            got["chan"] = max(t.ratios_T(Tc[m], rc, "chan"))
        for b, v in got.items():
            worst[b] = max(worst.get(b, 0.0), v / C_CHAN)
    kap = max(t.kappa for t in truths)
    print(f"ACC channel_states {label}: kappa <= {kap:.1e} " + " ".join(f"{b} {v:.3g}" for b, v in worst.items()))
    bad = {b: v for b, v in worst.items() if not v <= 1.0}
    assert not bad, (label, bad)


def from_ref_case(c, name):
    """A channel_states_ref.const_case dict as a ChanCase."""
    return ChanCase(name, c["F"], c["S"], c["Is"], c["Id"], c["E"], ss=c["ss"], sd=c["sd"])


# --------------------------------------------------------------------------- #
# solver-alone spectra
# --------------------------------------------------------------------------- #
SOLVER_KS = (17, 69, 70, 96)


def solver_spectra(K):
    """{name: Hermitian K x K}: graded D X D, a cluster of five eigenvalues at gaps 1e-10 ||A|| beside separated ones, the
    Wilkinson tridiagonal W+ of the largest odd order <= K (zero-padded), and the 2^+-64 copies of all three."""
    rng = np.random.default_rng(500 + K)
    X = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
    X = X + X.conj().T
    D = np.logspace(0, -6, K)
    graded = D[:, None] * X * D[None, :]
    vals = np.concatenate([1.0 + 1e-10 * np.sqrt(K) * np.arange(5), np.linspace(-2.0, 0.5, K - 5)])
    Q, _ = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))
    cluster = (Q * vals) @ Q.conj().T
    cluster = 0.5 * (cluster + cluster.conj().T)
    mw = (K - 1) // 2
    W = np.zeros((K, K), complex)
    k = 2 * mw + 1
    W[np.arange(k), np.arange(k)] = np.abs(np.arange(k) - mw)
    W[np.arange(k - 1), np.arange(1, k)] = 1.0; W[np.arange(1, k), np.arange(k - 1)] = 1.0
    out = {"graded": graded, "cluster": cluster, "wilkinson": W}
    for name in list(out):
        for k in (64, -64):
            out[f"{name}*2^{k}"] = out[name] * 2.0 ** k
    return out


def solver_ratios(A, w, V=None, truth=None):
    """(worst |w^_i - w_i| / (EIGH_C K u ||A||_F), worst group ||V^_C V^_C^H - V_C V_C^H||_F gap / (2 EIGH_C K u ||A||_F))
    against herm_eig_ld; groups are the eigenvalues separated from all others by >= 1e-3 of the spectrum's width."""
    K = A.shape[0]
    Ah = np.tril(A) + np.tril(A, -1).conj().T
    Ah[np.diag_indices(K)] = Ah.diagonal().real
    wt, Vt = herm_eig_ld(Ah) if truth is None else truth
    nA = float(np.linalg.norm(Ah))
    if nA == 0:
        return 0.0 if not np.any(w) else np.inf, 0.0
    bar = EIGH_C * K * U * nA
    rw = float(np.max(np.abs(np.asarray(w).astype(LR) - wt))) / bar
    rv = 0.0
    if V is not None:
        wd = f64(wt).real
        sep = 1e-3 * max(wd[-1] - wd[0], 0.0)
        Vl = np.asarray(V).astype(LD)
        for g in R.clusters(wd, sep) if sep > 0 else [list(range(K))]:
            lo = wd[g[0]] - wd[g[0] - 1] if g[0] > 0 else np.inf
            hi = wd[g[-1] + 1] - wd[g[-1]] if g[-1] + 1 < K else np.inf
            gap = min(lo, hi)
            if not np.isfinite(gap):
                continue
            D = Vl[:, g] @ Vl[:, g].conj().T - Vt[:, g] @ Vt[:, g].conj().T
            rv = max(rv, fro(D) * gap / (2 * bar))
    return rw, rv
