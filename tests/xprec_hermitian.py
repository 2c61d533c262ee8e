"""Complex-Hermitian members of the extended-precision case tables, on which rows and columns differ, and the planted
defects that only such inputs can see.  Shared by test_hermitian_host.py (CPU) and test_hermitian_gpu.py (MI355X).

Every other truth case of the dense path (xprec.ladder / bipartite / graded, their rotations and scalings) has a
complex-SYMMETRIC A(E) = E S - F - Sigma: F and S real symmetric, Sigma from formSigma.  There G = G^T to rounding and
G^H = conj(G), so a transposed inverse, a G^H that is conjugated but not transposed, contact rows taken for contact
columns and exchanged contacts all pass.  Here F and S are complex Hermitian and Sigma is a general block, so that
||A - A^T||_F / ||A||_F >= 0.5 at every energy.  xprec.Case, Truth and bar are reused unchanged; C_BAR is not
recalibrated (the cases are admitted only where numpy.linalg.inv and xprec.gauss_jordan stay within HALF the bar).

  G6   hermitian_ladder(n)    the ladder (xprec.ladder) on Hermitian F, S: a spectator orbital coupled at 1e-7, energies
                              Re lambda0 + {1, 1e-2, 1e-5, 1e-8, 0} (kappa_2 ~ 1e1 ... 1e9) and 0.3 + 2i; Sigma_c is
                              -1e-9 i S plus a non-symmetric block on the contact orbitals
  G6c  hermitian_confined(n)  the same F and S with the contact blocks only (the compact Gamma products apply),
                              energies -0.7, 0.25 and 0.3 + 2i: kappa_2 <= 2e2, so that the bound of G Gamma G^H is tight
  L4   hermitian_lead(n)      a lead for xprec_chain: alpha, S_alpha complex Hermitian, beta, S_beta complex general
  h    rgf_case()             three Hermitian layers (40, 100, 33) for the layered path, beside rgf_ref.cases()

Measured on the CPU (test_hermitian_host.py prints all of it):
  admission   worst ratio to the bar over n in {2, 17, 64, 100, 257}: numpy.linalg.inv 0.27 (G6), 0.32 (G6c), both at
              n = 2 (0.15 and 0.14 above it); xprec.gauss_jordan (n <= 100) 0.26 (G6), 0.34 (G6c) at n = 2 (0.24 and
              0.21 above it); smallest ||A - A^T|| / ||A|| 0.75 (n = 2, 0.89 above it); kappa_2 1.5 ... 2.0e9 (G6),
              at most 1.9e2 (G6c, n >= 17); L4 at n in {9, 17, 50, 64}: the float64 fixed point at most 0.059 on g
              and 0.0076 on Sigma
  detection   smallest ratio to the bar of a planted defect: the transposed inverse on G6 1.4e6 (n = 17; up to 4.3e14);
              GrLessInt on G6c (n = 17, 64; the float64 reference at most 0.0056): conj-only G^H 5.1e11, transposed G
              5.1e11, rows for columns 5.1e11 (on a confined Gamma the last two are the same matrix); exchanged
              contacts at 0.3 + 2i 5.1e10 (at the real energies 7.5e-5 ... 2.1e-3: reciprocal, it passes there);
              chain64 with a transposed inverse on L4 3.6e7 over every checked K (5.1e9 at K = 0)
  blindness   the transposed inverse on xprec.ladder(64): 0.114 of the bar at worst -- it passes
  case h      the two float64 sweeps' errors differ by at most 2.28 against C_RGF / 2 = 16; T into the right and into
              the left terminal agree at the four real energies and are 2.598e-3 and 2.405e-3 at 0.3 + 0.5i
"""
import functools

import numpy as np
import scipy.linalg as sla

import rgf_ref as rr
import tmatrix_ref
import xprec
import xprec_chain as xc
from xprec import Case

SPECTATOR_FROM = 8                   # below: no spectator orbital (k = n // 2 + 3 needs n >= 8)
SEED_OF = {2: 30}
"""Seeds by dimension where seed 0 misses an admission condition (test_hermitian_host.test_admission): at n = 2 seed 0
has ||A - A^T|| / ||A|| = 0.41 at 0.3 + 2i and numpy.linalg.inv at 0.59 of the bar there (kappa_2 = 1.7: the bar is
5e-16); seed 30 is the one of 1 ... 59 with the smallest worst ratio among those with an asymmetry of at least 0.7."""


def _cgauss(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def sigma_block(k, rng):
    """tmatrix_ref.sigma_block (-i Gamma / 2 with Gamma Hermitian positive definite plus a real symmetric shift) with
    the shift made complex Hermitian: 0.05 (B + B^H) - 0.5 i Gamma, a general non-symmetric, non-Hermitian block."""
    blk = tmatrix_ref.sigma_block(k, rng)
    C = rng.standard_normal((k, k))
    return blk + 0.05j * (C - C.T)


def _system(n, seed):
    """F = (A + A^H) / sqrt(4n) * 2, S = I + 0.1 (B + B^H) / sqrt(4n), A and B complex Gaussian: helpers.random_system
    with the entries' variance kept.  The generator is handed on for the spectator's coupling."""
    rng = np.random.default_rng(7600 + n + seed + SEED_OF.get(n, 0))
    A = _cgauss(rng, n, n)
    F = (A + A.conj().T) / np.sqrt(4 * n) * 2
    B = _cgauss(rng, n, n)
    S = np.eye(n) + 0.1 * (B + B.conj().T) / np.sqrt(4 * n)
    return F, S, rng


MIDGAP_UPTO = 1100                   # above: the spectator's level sits at 0.1 without the mid-gap search


@functools.lru_cache(maxsize=8)
def _ladder_parts(n, seed):
    F, S, rng = _system(n, seed)
    inds = xprec._contacts(n)
    if n > MIDGAP_UPTO:
        # (the search is an eigenproblem of dimension n - 1; these sizes carry no ladder energies, see matrices())
        k = n // 2 + 3
        v = 1e-7 * _cgauss(rng, n)
        F[k, :] = v; F[:, k] = v.conj(); F[k, k] = 0.1
        S[k, :] = 0.0; S[:, k] = 0.0; S[k, k] = 1.0
        return F, S, inds, k, 0.1
    if n < SPECTATOR_FROM:
        # too small for the ladder's spectator (at n = 2 it would leave A diagonal to 1e-7, that is symmetric): the
        # ladder hangs on the eigenvalue of the pencil nearest 0.1 instead
        return F, S, inds, None, 0.1
    k = n // 2 + 3
    keep = [i for i in range(n) if i != k]
    ev = np.sort(sla.eigh(F[np.ix_(keep, keep)], S[np.ix_(keep, keep)], eigvals_only=True))
    mids = (ev[1:] + ev[:-1]) / 2
    eps = float(mids[np.argmin(np.abs(mids - 0.1))])
    v = 1e-7 * _cgauss(rng, n)
    F[k, :] = v; F[:, k] = v.conj(); F[k, k] = eps
    S[k, :] = 0.0; S[:, k] = 0.0; S[k, k] = 1.0
    return F, S, inds, k, eps


def _contact_blocks(n, inds, seed):
    rng = np.random.default_rng(7700 + n + seed + SEED_OF.get(n, 0))
    return [sigma_block(len(ix), rng) for ix in inds]


def matrices(n, seed=0):
    """(F, S, inds, sigs, resonant, eps) of G6 without its energies: what the sizes beyond any truth (2049, 4097) use."""
    F, S, inds, k, eps = _ladder_parts(n, seed)
    F, S = F.copy(), S.copy()
    sigs = []
    for ix, blk in zip(inds, _contact_blocks(n, inds, seed)):
        s = -1e-9j * S
        s[np.ix_(ix, ix)] += blk
        sigs.append(s)
    return F, S, inds, sigs, k, eps


def level(H, S, eps, k):
    """The eigenvalue of the pencil (H, S) nearest eps -- xprec.ladder's lambda0.  With a spectator orbital k it is
    1e-9 from eps and the next one some 1e-3: four steps of inverse iteration from e_k with the shift eps give it to
    rounding (each gains a factor 1e-6) at the cost of one LU, where all n eigenvalues cost seconds at n = 1025.
    test_hermitian_host.test_admission checks it against scipy.linalg.eig.  Without a spectator: all eigenvalues."""
    if k is None:
        lam = sla.eig(H, S, right=False)
        return lam[np.argmin(np.abs(lam - eps))]
    lu = sla.lu_factor(H - eps * S)
    x = np.zeros(H.shape[0], dtype=np.complex128)
    x[k] = 1.0
    for _ in range(4):
        y = sla.lu_solve(lu, S @ x)
        mu = y[k]                                   # (H - eps S)^-1 S x = x / (lambda - eps), x[k] = 1
        x = y / mu
    return eps + 1.0 / mu


def hermitian_ladder(n, seed=0):
    """G6 (see the module docstring)."""
    assert n <= MIDGAP_UPTO
    F, S, inds, sigs, k, eps = matrices(n, seed)
    lam0 = level(F + sigs[0] + sigs[1], S, eps, k)
    E = [lam0.real + d for d in (1.0, 1e-2, 1e-5, 1e-8, 0.0)] + [0.3 + 2j]
    return Case("G6", n, F, S, inds, sigs, E, resonant=k)


def hermitian_confined(n, seed=0):
    """G6c: G6's F and S with the contact blocks only, no background."""
    F, S, inds, k, _ = _ladder_parts(n, seed)
    sigs = []
    for ix, blk in zip(inds, _contact_blocks(n, inds, seed)):
        s = np.zeros((n, n), dtype=np.complex128)
        s[np.ix_(ix, ix)] = blk
        sigs.append(s)
    return Case("G6c", n, F.copy(), S.copy(), inds, sigs, [-0.7, 0.25, 0.3 + 2j], resonant=k)


def exchanged(case):
    """The same system with its two contacts in the other order: T asked as (1, 0)."""
    return Case(case.name + "x", case.n, case.F, case.S, case.inds[::-1], case.sigs[::-1], case.energies,
                resonant=case.resonant)


def truth_of_exchanged(truth):
    """The Truth of exchanged(truth.case): G does not depend on the order of the contacts."""
    t = xprec.Truth.__new__(xprec.Truth)
    t.__dict__.update(truth.__dict__)
    t.case = exchanged(truth.case)
    return t


def subset(truth, idx):
    """The Truth (and Case) of some of a case's energies."""
    c = truth.case
    idx = np.asarray(idx)
    t = xprec.Truth.__new__(xprec.Truth)
    t.__dict__.update(truth.__dict__)
    t.case = Case(c.name, c.n, c.F, c.S, c.inds, c.sigs, c.energies[idx], resonant=c.resonant)
    t.kappa, t.G, t.last_correction = truth.kappa[idx], truth.G[idx], truth.last_correction[idx]
    return t


def asymmetry(A):
    return float(np.linalg.norm(A - A.T) / np.linalg.norm(A))


def hermitian_lead(n, seed=0, eta=xc.ETA):
    """L4: helpers.chain_lead's scales with the entries' variance kept (complex Gaussians of unit variance), alpha and
    S_alpha complex Hermitian, beta and S_beta complex general, tau = beta; energies as xprec_chain.lead_l1."""
    rng = np.random.default_rng(900 + n + seed)
    c = lambda *s: _cgauss(rng, *s) / np.sqrt(2)
    a = c(n, n); alpha = (a + a.conj().T) * 0.5 * 0.5
    beta = c(n, n) * 0.2
    s = c(n, n); Sa = np.eye(n) + 0.05 * (s + s.conj().T) * 0.5 / np.sqrt(n)
    Sb = 0.05 * c(n, n) / np.sqrt(n)
    lead = xc.Lead("L4", alpha, Sa, beta, Sb, beta.copy(), Sb.copy(), [0.3, 0.2 + 0.3j], eta=eta)
    lead.energies = np.append(lead.energies, xc.edge_energy(lead))
    return lead


# --------------------------------------------------------------------------- #
# the layered case
# --------------------------------------------------------------------------- #
RGF_SEED = 61
RGF_COMPLEX_E = 0.3 + 0.5j


@functools.lru_cache(maxsize=None)
def rgf_case():
    """Case h: Hermitian layers of 40, 100 and 33 orbitals -- every layer takes the single-workgroup blocked inverse,
    40 and 33 at the foreign stride nmax^2 = 100^2.  Not an entry of rgf_ref.cases() (test_rgf_host.test_calibration
    measures over those); admitted like rgf_ref.window_case(): the two float64 sweeps' errors may differ by at most
    C_RGF / 2 = 16 on every quantity (test_hermitian_host.test_layered_case_is_within_the_calibration)."""
    return rr.RCase("h", (40, 100, 33), RGF_SEED, hermitian_complex=True)


def _rgf_entry(c, E):
    ent = dict(case=c, E=E, w=None, keys=("T", "dos", "pdos"))
    for form, fn in (("truth", rr.truth_pieces), ("lr", rr.sweep_lr), ("rl", rr.sweep_rl), ("dense", rr.dense)):
        dtype = rr.LD if form == "truth" else complex
        per = xprec.pmap(lambda e: rr._quantities(c, fn(c, e), dtype), list(E))
        ent[form] = dict(T=np.array([p[0] for p in per]), dos=np.array([p[1] for p in per]),
                         pdos=np.array([p[2] for p in per]), single=np.array([p[3] for p in per]))
    for form in ("lr", "rl", "dense"):
        ent["err_" + form] = {k: rr.rel_err(ent[form][k], ent["truth"][k]) for k in ent["keys"]}
        ent["err_" + form]["single"] = [rr.rel_err(ent[form]["single"][j], ent["truth"]["single"][j])
                                        for j in range(len(E))]
    return ent


@functools.lru_cache(maxsize=None)
def rgf_truth():
    """(entry of case h, entry of its mirror image), each in the form of rgf_ref.window_truth(): T, dos, pdos and
    'single', the blocks of G(E_j) on the pattern of S for each energy alone, over rgf_energies().  The mirror's T is
    the transmission from the right terminal into the left one of case h (rgf_ref's quantities hold the other one)."""
    c = rgf_case()
    return _rgf_entry(c, rgf_energies()), _rgf_entry(c.mirrored(), rgf_energies())


def rgf_energies():
    """The case's four real energies and one complex one: a two-terminal T is reciprocal at real energies whatever the
    matrices, so only the complex energy tells the two directions of T apart."""
    return np.append(rgf_case().energies.astype(complex), RGF_COMPLEX_E)


# --------------------------------------------------------------------------- #
# planted defects
# --------------------------------------------------------------------------- #
def inv_transposed(A):
    """An inverse written back transposed: inv[i][j] = W[pivrow[i]][colof[j]] read the other way round."""
    return np.linalg.inv(A).T


def _support(Gam):
    return np.flatnonzero(np.any(Gam != 0, axis=0) | np.any(Gam != 0, axis=1))


def gless(G, Gam, defect=None):
    """G Gamma G^H in float64, or one of its planted defects:
      "conj"  G^H conjugated but not transposed: G Gamma conj(G)
      "trans" the transposed inverse throughout: G^T Gamma conj(G)
      "rows"  the compact product G[:, I] Gamma_II G[:, I]^H (I the support of Gamma) with the contact ROWS of G taken
              for its contact columns: G[I, :]^T Gamma_II conj(G[I, :])"""
    if defect is None:
        return G @ Gam @ G.conj().T
    if defect == "conj":
        return G @ Gam @ G.conj()
    if defect == "trans":
        return G.T @ Gam @ G.conj()
    assert defect == "rows", defect
    I = _support(Gam)
    R = G[I, :]
    return R.T @ Gam[np.ix_(I, I)] @ R.conj()


def gless_int(case, w, ind, defect=None):
    """sum_m w_m G_m Gamma G_m^H with numpy.linalg.inv, the defect planted in every term."""
    Gam = xprec._gamma_of(case, ind)
    return sum(w[m] * gless(np.linalg.inv(case.A64(E)), Gam, defect) for m, E in enumerate(case.energies))


def transmission(case, E, exchange=False):
    """Re Tr(Gamma_1 G Gamma_2 G^H) in float64; exchange: the two contacts the other way round (a planted defect)."""
    g1, g2 = case.gammas()[::-1] if exchange else case.gammas()
    G = np.linalg.inv(case.A64(E))
    return float(np.sum((g1 @ G @ g2) * G.conj()).real)
