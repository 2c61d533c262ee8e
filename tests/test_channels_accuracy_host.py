"""
Host checks of the yardstick the eigenchannel kernels are held to (tests/xprec_channels.py); no GPU.

  1. herm_eig_ld against mpmath's eighe at 40 digits, K <= 12: random, graded over 12 decades, a cluster of gap 1e-10 and
     a rank-deficient PSD spectrum -- eigenvalues to 4 K eps ||A||_F (eps = 2^-63), invariant subspaces to that over the gap;
     and the whole channel truth of one (9, 5, 40) energy against the same computation in mpmath.
  2. calibration: the two fp64 numpy references (channel_states_ref with numpy.linalg.eigh, and with jacobi_eigh, both on
     pivoted_cholesky and LAPACK's inv) stay below C_CHAN * beta for every bar on every case, and C_CHAN is the smallest
     power of two at least twice their worst error / beta.  The fp64 solvers stay below the solver bars on the solver
     spectra.
  3. planted defects: each of six variants of the restatement exceeds C_CHAN * beta on at least one case.  Measured worst
     error / (C_CHAN beta) and the bar that catches it:
       lowest-index Cholesky pivot   8.6e12  spec, (21,30,70) dgraded16 (the first diagonal is below the cut: rank 0)
       cut at 1e-8                   4.0e4   spec, (21,30,70) dgraded16
       Jacobi stopped at 1e-12       95      orth, (9,5,40) graded12 (the stop rule alone; the skip threshold stays)
       X0 = conj(L)                  1.5e14  spec, (9,5,40) ladder
       sorted, vectors not permuted  3.2e14  orth, (9,5,40) graded12
       G_ds^T for G_ds^H             1.6e14  orth, (9,5,40) ladder
  4. the flat tolerances the older GPU tests use (|T^ - T| <= 1e-10 max T, identities and projectors 1e-8, on
     channel_states_ref.CONST_CASES and the rank-3 case) miss the early-stopped Jacobi, the 1e-8 cut and the lowest-index
     pivot: those variants pass every flat check there (worst error / tolerance 1.7e-2, 9.3e-8 and 1.5e-4; the other
     three are caught there too, by 4e8 ... 1e10).
"""
import functools

import numpy as np
import pytest

import channel_states_ref as R
import xprec
import xprec_channels as X

xprec.require_extended()

BARS = ("T", "rank", "sum", "orth", "spec", "proj", "psi", "chan")


@functools.lru_cache(maxsize=None)
def _truths(i):
    return X.truths(X.host_cases()[i])


def _ratios(case, m, t, **kw):
    T, psi, r = X.reference(case, m, **kw)
    return X.all_ratios(t, T, psi, r)


# --------------------------------------------------------------------------- truth against mpmath
def _mp_matrix(mp, A):
    K = A.shape[0]
    return mp.matrix([[mp.mpc(float(A[i, j].real), float(A[i, j].imag)) for j in range(A.shape[1])] for i in range(K)])


def _from_mp(mp, M, rows, cols):
    out = np.zeros((rows, cols), dtype=X.LD)
    for i in range(rows):
        for j in range(cols):
            out[i, j] = np.longdouble(mp.nstr(mp.re(M[i, j]), 30)) + 1j * np.longdouble(mp.nstr(mp.im(M[i, j]), 30))
    return out


def _mp_spectra():
    rng = np.random.default_rng(77)
    out = {}
    for K in (1, 2, 5, 12):
        A = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
        out[f"random K={K}"] = A + A.conj().T
    Q, _ = np.linalg.qr(rng.standard_normal((12, 12)) + 1j * rng.standard_normal((12, 12)))
    out["graded 12 decades"] = (Q * np.logspace(0, -12, 12)) @ Q.conj().T
    vals = np.concatenate([1.0 + 1e-10 * np.arange(4), [-1.0, -0.3, 0.2, 0.6, 2.0, 3.0, 4.5]])
    Q11, _ = np.linalg.qr(rng.standard_normal((11, 11)) + 1j * rng.standard_normal((11, 11)))
    out["cluster 1e-10"] = (Q11 * vals) @ Q11.conj().T
    B = rng.standard_normal((9, 3)) + 1j * rng.standard_normal((9, 3))
    out["rank 3 PSD"] = B @ B.conj().T
    return {k: 0.5 * (v + v.conj().T) for k, v in out.items()}


@pytest.mark.parametrize("name", list(_mp_spectra()))
def test_herm_eig_ld_against_mpmath(name):
    import mpmath as mp
    A = _mp_spectra()[name]
    K = A.shape[0]
    w, V = X.herm_eig_ld(A)
    with mp.workdps(40):
        E, Q = mp.eighe(_mp_matrix(mp, A))
        wm = np.array([np.longdouble(mp.nstr(E[i], 30)) for i in range(K)])
        Qm = _from_mp(mp, Q, K, K)
    order = np.argsort(wm, kind="stable")
    wm, Qm = wm[order], Qm[:, order]
    tol = 4 * K * X.EPS_LD * np.linalg.norm(A)
    err = float(np.max(np.abs(w - wm)))
    worst = 0.0
    wd = wm.astype(np.float64)
    for g in R.clusters(wd, 1e-6 * np.linalg.norm(A)):
        lo = wd[g[0]] - wd[g[0] - 1] if g[0] > 0 else np.inf
        hi = wd[g[-1] + 1] - wd[g[-1]] if g[-1] + 1 < K else np.inf
        gap = min(lo, hi)
        D = V[:, g] @ V[:, g].conj().T - Qm[:, g] @ Qm[:, g].conj().T
        worst = max(worst, X.fro(D) * (gap if np.isfinite(gap) else 0.0))
    orth = X.fro(V.conj().T @ V - np.eye(K))
    print(f"herm_eig_ld {name}: eigenvalue error {err:.2e}, subspace error x gap {worst:.2e} (tolerance {tol:.2e}), "
          f"orthonormality {orth:.2e}")
    assert err <= tol and worst <= tol and orth <= 4 * K * X.EPS_LD


def test_channel_truth_against_mpmath():
    """One energy of (9, 5, 40): G by mpmath's LU, Gamma_s = R R^H and the eigenvalues by eighe, all at 40 digits."""
    import mpmath as mp
    case = X.const_case(9, 5, 40, family="block", ladder=True)
    m = 1
    t = X.truths(case)[m]
    with mp.workdps(40):
        A = _mp_matrix(mp, case.S) * mp.mpc(case.E[m].real, case.E[m].imag) - _mp_matrix(mp, case.F) \
            - _mp_matrix(mp, case.ss) - _mp_matrix(mp, case.sd)
        G = mp.inverse(A)
        Is, Id = [int(i) for i in case.Is], [int(i) for i in case.Id]
        gam = lambda s, ix: mp.matrix([[mp.mpc(0, 1) * (mp.mpc(complex(s[i, j])) - mp.conj(mp.mpc(complex(s[j, i])))) for j in ix]
                                       for i in ix])
        gs, gd = gam(case.ss, Is), gam(case.sd, Id)
        Gds = mp.matrix([[G[i, j] for j in Is] for i in Id])
        Es, Qs = mp.eighe(gs)
        Rf = Qs * mp.diag([mp.sqrt(max(e, 0)) for e in Es])
        H = Rf.H * Gds.H * gd * Gds * Rf
        Et, _ = mp.eighe((H + H.H) / 2)
        Tm = np.sort(np.array([np.longdouble(mp.nstr(e, 30)) for e in Et]))[::-1]
        Bm = _from_mp(mp, mp.matrix([[G[i, j] for j in Is] for i in range(case.n)]), case.n, len(Is))
    eB = X.fro(t.B - Bm) / X.fro(Bm)
    eT = float(np.max(np.abs(t.T - Tm)) / Tm[0])
    print(f"channel truth vs mpmath: G[:, I_s] {eB:.2e}, T {eT:.2e} (kappa {t.kappa:.1e})")
    assert eB <= 64 * t.kappa * X.EPS_LD and eT <= 64 * t.kappa * X.EPS_LD


# --------------------------------------------------------------------------- calibration
@functools.lru_cache(maxsize=None)
def _reference_table():
    """[(case name, energy index, reference, {bar: ratio})] over every case, energy and the two references."""
    out = []
    for i, case in enumerate(X.host_cases()):
        for m, t in enumerate(_truths(i)):
            for eig in ("lapack", "jacobi"):
                r = _ratios(case, m, t, eig=eig)
                Tc, rc = X.reference_channels(case, m, eig)
                cT, cB, cS = t.ratios_T(Tc, rc, "chan")
                r["chan"] = max(cT, cB, cS)
                out.append((case.name, m, eig, r))
    return out


def test_calibration():
    worst = {b: (0.0, None) for b in BARS}
    for name, m, eig, r in _reference_table():
        for b in BARS:
            if r[b] > worst[b][0]:
                worst[b] = (r[b], f"{name} E[{m}] {eig}")
    for b in BARS:
        print(f"channel calibration: {b:5s} worst error / beta {worst[b][0]:.3g} at {worst[b][1]}")
    top = max(v[0] for v in worst.values())
    c = 2.0 ** np.ceil(np.log2(2.0 * top))
    print(f"channel calibration: worst {top:.3g} -> C_CHAN {c:g} (xprec_channels.C_CHAN = {X.C_CHAN:g})")
    assert top <= X.C_CHAN                                   # the correct restatement stays below every bar on every case
    assert c == X.C_CHAN, (top, c, X.C_CHAN)


def test_solver_bars_hold_for_fp64_solvers():
    worst = [0.0, 0.0]
    for K in X.SOLVER_KS:
        for name, A in X.solver_spectra(K).items():
            truth = X.herm_eig_ld(A)
            for solver in (np.linalg.eigh, R.jacobi_eigh):
                w, V = solver(A)
                rw, rv = X.solver_ratios(A, w, V, truth=truth)
                worst = [max(worst[0], rw), max(worst[1], rv)]
                assert rw <= 1.0 and rv <= 1.0, (K, name, solver.__name__, rw, rv)
    print(f"solver bars on the solver spectra, fp64 solvers: eigenvalues {worst[0]:.3g}, subspaces {worst[1]:.3g} of the bar")


# --------------------------------------------------------------------------- planted defects
DEFECTS = {
    "lowest-index pivot": dict(chol="first"),
    "cut at 1e-8": dict(cut=1e-8),
    "Jacobi stopped at 1e-12": dict(eig="jacobi", jac_tol=1e-12),
    "X0 = conj(L)": dict(x0_conj=True),
    "sorted, not permuted": dict(permute=False),
    "G_ds^T for G_ds^H": dict(gds="T"),
}
DEFECT_CASES = [((9, 5, 40), "block", True), ((9, 5, 40), "graded12", False), ((21, 30, 70), "dgraded16", False),
                ((21, 30, 70), "rank10", False)]


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_is_caught(defect):
    names = [c.name for c in X.host_cases()]
    top, at = 0.0, None
    for shape, f, l in DEFECT_CASES:
        case = X.const_case(*shape, family=f, ladder=l)
        for m, t in enumerate(_truths(names.index(case.name))):
            for b, v in _ratios(case, m, t, **DEFECTS[defect]).items():
                if v > top:
                    top, at = v, f"{b} on {case.name} E[{m}]"
    print(f"planted defect '{defect}': worst error / (C_CHAN beta) {top / X.C_CHAN:.3g} ({at})")
    assert top > X.C_CHAN, (defect, top)


def _flat_checks(case, defect_kw):
    """The older tests' flat checks of a variant against the correct fp64 restatement: worst of
    |T^ - T| / (1e-10 max T), identities / 1e-8, cluster projectors / 1e-8 (<= 1: the variant passes them)."""
    gs, gd = R.gamma(case["ss"]), R.gamma(case["sd"])
    cc = X.ChanCase("flat", case["F"], case["S"], case["Is"], case["Id"], case["E"], ss=case["ss"], sd=case["sd"])
    worst = 0.0
    for m, e in enumerate(case["E"]):
        G = R.case_green(case, e)
        Tr, pr = R.channel_states_ref(G, gs, gd, case["Is"], case["Id"])
        T, psi, r = X.reference(cc, m, **defect_kw)
        k = len(Tr)
        worst = max(worst, np.max(np.abs(T[:k] - Tr)) / (1e-10 * Tr[0]))
        orth, srule, spec = R.identity_errors(T[:r], psi[:r], G, gs, gd)
        worst = max(worst, orth / 1e-8, srule / 1e-8, spec / 1e-8)
        for g in R.clusters(Tr, 1e-3 * Tr[0]):
            if g[-1] < r:
                worst = max(worst, np.linalg.norm(R.projector(psi[g]) - R.projector(pr[g])) / 1e-8)
    return worst


def test_flat_tolerances_miss_subtle_defects():
    cases = [R.const_case(*c) for c in R.CONST_CASES] + [R.rank_deficient_case()]
    got = {}
    for name, kw in DEFECTS.items():
        got[name] = max(_flat_checks(c, kw) for c in cases)
        print(f"flat tolerances, '{name}': worst error / tolerance {got[name]:.3g} -> {'missed' if got[name] <= 1 else 'caught'}")
    assert got["Jacobi stopped at 1e-12"] <= 1.0 and got["cut at 1e-8"] <= 1.0
