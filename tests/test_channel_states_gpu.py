"""Eigenchannel scattering states on the GPU (negf_eigh_batched, negf_channel_states): the eigenvector form of the batched
Jacobi solver against its values-only form (bitwise) and against calibrated residual / orthonormality bounds; the
states' identities, parity with the numpy restatement (tests/channel_states_ref.py), rank-deficient couplings, gauge,
chain / Bethe / surfGTest providers, batch streaming, spin layouts, refusals and singular energies.

eigh bounds: max_j ||A v_j - w_j v_j||_2 <= C K u ||A||_F and ||V^H V - I||_F <= C K u with u = 2^-53 and C = 64, the
smallest power of two at least twice the worst ratio reached on these inputs by numpy.linalg.eigh (residual 2.20,
orthonormality 3.12) and by the numpy restatement of the same cyclic Jacobi (1.68, 19.53; the orthonormality defect of
accumulated rotations grows with K and the sweep count).  Worst device ratios on one MI355X: residual 0.75 (K = 3),
orthonormality 18.77 (K = 64, two 32-fold eigenvalues).
"""
import os
import warnings

import numpy as np
import pytest

import channel_states_ref as R
import xprec_channels as X
from helpers import random_system, swept

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- eigh
def _check_eigh(engine, A, label):
    A = np.asarray(A)
    w, V = engine.eigh(A)
    assert not np.any(engine.last_info)
    assert np.array_equal(w, engine.eigvalsh(A)), label                    # the same rotations: bit for bit
    worst = [0.0, 0.0]
    for k in range(A.shape[0]):
        rr, ro = R.eigh_ratios(A[k], w[k], V[k])
        worst = [max(worst[0], rr), max(worst[1], ro)]
    print(f"eigh {label}: residual ratio {worst[0]:.3f} orthonormality ratio {worst[1]:.3f} (C = {R.EIGH_C})")
    assert worst[0] <= R.EIGH_C and worst[1] <= R.EIGH_C, (label, worst)


@pytest.mark.parametrize("K", R.EIGH_KS)
def test_eigh_random(engine, K):
    _check_eigh(engine, R.eigh_random(K), f"K={K}")


def test_eigh_special_spectra(engine):
    for i, A in enumerate(R.eigh_special()):
        _check_eigh(engine, A[None], f"special {i} (K={A.shape[0]})")
    w, V = engine.eigh(np.zeros((30, 30)))
    assert np.array_equal(w, np.zeros(30)) and np.array_equal(V, np.eye(30))


def test_eigh_reads_lower_triangle_and_single_matrix(engine):
    rng = np.random.default_rng(5)
    A = R.eigh_random(20, 1)[0]
    Al = np.tril(A) + np.triu(rng.standard_normal((20, 20)), 1)
    w, V = engine.eigh(Al)
    assert w.shape == (20,) and V.shape == (20, 20)
    w2, V2 = engine.eigh(A[None])
    assert np.array_equal(w, w2[0]) and np.array_equal(V, V2[0])


@pytest.mark.parametrize("K", [20, 80])
def test_eigh_nan_matrix(engine, K):
    A = R.eigh_random(K, 3)
    A[1, 5, 2] = np.nan
    with pytest.warns(RuntimeWarning, match="non-finite"):
        w, V = engine.eigh(A)
    assert np.all(np.isnan(w[1])) and np.all(np.isnan(V[1].real)) and np.all(np.isnan(V[1].imag))
    assert engine.last_info[1] == 1 and engine.last_info[0] == 0 and engine.last_info[2] == 0
    for k in (0, 2):
        assert np.all(np.isfinite(w[k])) and max(R.eigh_ratios(A[k], w[k], V[k])) <= R.EIGH_C


# --------------------------------------------------------------------------- identities and parity
def _run_const(engine, case, nchan=None):
    engine.set_system(case["F"], case["S"])
    h = engine.sigma_const([case["ss"], case["sd"]])
    try:
        T, psi = engine.channel_states(h, 0, 1, case["E"], nchan)
        Tt = engine.transmission(h, 1, 0, case["E"])
        Tc = engine.transmission_channels(h, 1, 0, case["E"])
    finally:
        engine.sigma_free(h)
    return T, psi, Tt, Tc


def _check_identities(T, psi, Tt, Tc, greens, gam_s, gam_d, label, spectral=True):
    """greens(k) -> numpy G at energy k.  T [m, K_s], psi [m, K_s, n] with all channels."""
    for k in range(T.shape[0]):
        tmax = np.max(T[k])
        P = psi[k].T
        orth = np.max(np.abs(P.conj().T @ gam_d(k) @ P - np.diag(T[k]))) / tmax
        srule = abs(T[k].sum() - Tt[k]) / abs(Tt[k])
        nz = min(T.shape[1], Tc.shape[1])
        chan = max(np.max(np.abs(T[k, :nz] - Tc[k, :nz])), np.max(np.abs(T[k, nz:]), initial=0.0),
                   np.max(np.abs(Tc[k, nz:]), initial=0.0)) / tmax
        spec = 0.0
        if spectral:
            G = greens(k)
            A = G @ gam_s(k) @ G.conj().T
            spec = np.linalg.norm(P @ P.conj().T - A) / np.linalg.norm(A)
        print(f"identities {label} E[{k}]: orth {orth:.2e} sum {srule:.2e} channels {chan:.2e} spectral {spec:.2e}")
        assert orth <= 1e-8 and srule <= 1e-8 and chan <= 1e-10 and spec <= 1e-8, (label, k, orth, srule, chan, spec)
        assert np.all(np.diff(T[k]) <= 0)


@pytest.fixture(scope="module")
def const_runs(engine):
    """Each CONST case run once on the device, with the numpy reference and the extended-precision truth
    (tests/xprec_channels.py) per energy, shared by the tests below."""
    out = {}
    for c in R.CONST_CASES:
        case = R.const_case(*c)
        gs, gd = R.gamma(case["ss"]), R.gamma(case["sd"])
        G = [R.case_green(case, e) for e in case["E"]]
        ref = [R.channel_states_ref(g, gs, gd, case["Is"], case["Id"]) for g in G]
        cc = X.from_ref_case(case, f"const {c}")
        out[c] = (case, gs, gd, G, ref, _run_const(engine, case), (cc, X.truths(cc)))
    return out


@pytest.mark.parametrize("c", R.CONST_CASES)
def test_const_identities(const_runs, c):
    case, gs, gd, G, ref, (T, psi, Tt, Tc), truth = const_runs[c]
    assert T.shape == (3, c[0]) and psi.shape == (3, c[0], c[2])
    _check_identities(T, psi, Tt, Tc, lambda k: G[k], lambda k: gs, lambda k: gd, f"const {c}")
    X.check_outputs(*truth, T, psi, Tc, f"const {c}")        # every identity and T itself against the calibrated bars


@pytest.mark.parametrize("c", R.CONST_CASES)
def test_const_state_parity(const_runs, c):
    """Cluster by cluster (T_n separated from all others by >= 1e-3 max T) the device's states span what the truth's
    span: T within C_CHAN beta_T and the cluster projectors P_C within C_CHAN beta_state(C) (tests/xprec_channels.py; the
    T bar replaces the flat 1e-10 max T), and, as before, the orthogonal projectors on the device's and the numpy
    restatement's cluster spans equal to 1e-8 in Frobenius norm (on weak channels that is the tighter of the two)."""
    case, gs, gd, G, ref, (T, psi, Tt, Tc), truth = const_runs[c]
    for k in range(3):
        Tr, pr = ref[k]
        t = truth[1][k]
        assert len(Tr) == T.shape[1]
        eT = t.ratios_T(T[k], X.device_rank(T[k], psi[k]))[0] / X.C_CHAN
        assert sum(len(g) == 1 for g in t.clusters) >= 2, (c, k, [len(g) for g in t.clusters])
        wp, ws = (v / X.C_CHAN for v in t.ratios_state(psi[k], X.device_rank(T[k], psi[k])))
        flat = 0.0
        for g in R.clusters(Tr, 1e-3 * Tr[0]):
            flat = max(flat, np.linalg.norm(R.projector(psi[k][g]) - R.projector(pr[g])))
        print(f"parity const {c} E[{k}]: {len(t.clusters)} clusters; of the bar: T {eT:.3g}, projectors {wp:.3g}, singleton states {ws:.3g}; "
              f"worst orthogonal-projector distance {flat:.2e}")
        assert eT <= 1.0 and wp <= 1.0 and ws <= 1.0 and flat <= 1e-8, (c, k, eT, wp, ws, flat)


@pytest.mark.parametrize("c", R.CONST_CASES)
def test_gauge(const_runs, c):
    case, gs, gd, G, ref, (T, psi, Tt, Tc), truth = const_runs[c]
    for k in range(3):
        for s in psi[k]:
            if not np.any(s != 0):
                continue
            i = int(np.argmax(np.abs(s) ** 2))
            assert abs(s[i].imag) <= 1e-14 * abs(s[i]) and s[i].real > 0
    # singleton clusters: the gauge-fixed states themselves agree with the truth's within the calibrated state bar, and
    # with the reference's to 1e-8 of their norm
    t = truth[1][0]
    assert t.ratios_state(psi[0], X.device_rank(T[0], psi[0]))[1] <= X.C_CHAN
    Tr, pr = ref[0]
    for g in R.clusters(Tr, 1e-3 * Tr[0]):
        if len(g) == 1:
            assert np.linalg.norm(psi[0][g[0]] - pr[g[0]]) <= 1e-8 * np.linalg.norm(pr[g[0]])


def test_rank_deficient_gamma(engine):
    case = R.rank_deficient_case()
    T, psi, Tt, Tc = _run_const(engine, case)
    assert T.shape == (3, 9) and psi.shape == (3, 9, 40)
    assert np.all(T[:, 3:] == 0.0) and np.all(psi[:, 3:, :] == 0.0)          # exact zeros beyond the rank
    assert np.all(T[:, :3] > 0) and np.all(np.any(psi[:, :3, :] != 0, axis=2))
    gs, gd = R.gamma(case["ss"]), R.gamma(case["sd"])
    G = [R.case_green(case, e) for e in case["E"]]
    _check_identities(T, psi, Tt, Tc, lambda k: G[k], lambda k: gs, lambda k: gd, "rank 3 of 9")
    cc = X.from_ref_case(case, "rank 3 of 9")
    X.check_outputs(cc, X.truths(cc), T, psi, Tc, cc.name)
    # nchan beyond K_s: zero columns too; fewer than K_s: the leading ones
    engine.set_system(case["F"], case["S"])
    h = engine.sigma_const([case["ss"], case["sd"]])
    try:
        Tw, pw = engine.channel_states(h, 0, 1, case["E"], nchan=11)
        T2, p2 = engine.channel_states(h, 0, 1, case["E"], nchan=2)
    finally:
        engine.sigma_free(h)
    assert np.array_equal(Tw[:, :9], T) and np.array_equal(pw[:, :9], psi) and np.all(Tw[:, 9:] == 0) and np.all(pw[:, 9:] == 0)
    assert np.array_equal(T2, T[:, :2]) and np.array_equal(p2, psi[:, :2])


# --------------------------------------------------------------------------- providers
def _provider_check(engine, h, F, S, E, s, d, label):
    T, psi = engine.channel_states(h, s, d, E)
    Tt = engine.transmission(h, d, s, E)
    Tc = engine.transmission_channels(h, d, s, E)
    sS = engine.sigma_eval(h, s, E, 2); sD = engine.sigma_eval(h, d, E, 2)
    _check_identities(T, psi, Tt, Tc, None, None, lambda k: R.gamma(sD[k]), label, spectral=False)
    return T, psi, sS, sD


def test_surfgtest_provider(engine):
    """formSigma-style constant contacts: the -1e-9 i S background makes every orbital part of both supports (K_s = n)."""
    from gaunegf_amd.surfGTester import surfGTest
    from gaunegf_amd.transport import SigmaCalculator, calculate_channel_states, calculate_transmission
    n = 30
    F, S = random_system(n, 31)
    g = surfGTest(F, S, [list(range(4)), list(range(n - 4, n))], -0.1j)
    E = np.linspace(-1.5, 1.5, 5)
    sc = SigmaCalculator(g)
    T, psi = calculate_channel_states(F, S, sc, E)
    assert T.shape == (5, n) and psi.shape == (5, n, n)
    Tt = calculate_transmission(F, S, sc, E)
    gd = R.gamma(g.sig[1])
    for k in range(E.size):
        P = psi[k].T
        assert np.max(np.abs(P.conj().T @ gd @ P - np.diag(T[k]))) <= 1e-8 * T[k, 0]
        assert abs(T[k].sum() - Tt[k]) <= 1e-8 * abs(Tt[k])
    # injected from the other end: the same total (Tr[Gamma_L G Gamma_R G^H] = Tr[Gamma_R G Gamma_L G^H] for two contacts)
    T2, psi2 = calculate_channel_states(F, S, sc, E, source=-1)
    assert np.all(np.abs(T2.sum(axis=1) - Tt) <= 1e-8 * np.abs(Tt))


@pytest.mark.parametrize("solver", ["fixed-point", "doubling"])
def test_chain_provider(engine, solver):
    from helpers import chain_lead
    from gaunegf_amd.surfG1D import surfG
    from gaunegf_amd.transport import SigmaCalculator, cohTransChannelStatesE
    n, nc = 120, 20
    F, S = random_system(n, 7)
    lead = [chain_lead(nc, 40 + k) for k in range(2)]
    ci = [list(range(nc)), list(range(n - nc, n))]
    rng = np.random.default_rng(7)
    taus = [0.2 * rng.standard_normal((nc, nc)) for _ in range(2)]
    staus = [0.02 * rng.standard_normal((nc, nc)) for _ in range(2)]
    g = surfG(F, S, ci, taus=taus, staus=staus, alphas=[l[0] for l in lead], aOverlaps=[l[1] for l in lead],
              betas=[l[2] for l in lead], bOverlaps=[l[3] for l in lead], eta=1e-3, solver=solver)
    E = np.linspace(-1.0, 1.0, 5)
    engine.set_system(F, S)
    h = g._negf_lower(engine)
    T, psi, sS, sD = _provider_check(engine, h, F, S, E, 0, 1, f"chain {solver}")
    assert T.shape == (5, nc) and psi.shape == (5, nc, n)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T2, psi2 = cohTransChannelStatesE(E, F, S, g)
    assert np.array_equal(T2, T) and np.array_equal(psi2, psi)


def test_bethe_provider(engine):
    from gaunegf_amd.surfGBethe import read_bethe_params, construct_sk_matrix, gen_neighbors
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaunegf_amd", "data", "Au")
    ne, Ed, Vd, Sd, H0 = read_bethe_params(here)
    dirs = gen_neighbors(np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.2, 0.0]))
    Sl = np.array([construct_sk_matrix(Sd, d) for d in dirs]); Vl = np.array([construct_sk_matrix(Vd, d) for d in dirs])
    n = 45
    F, S = random_system(n, 17)
    F = F - 5.0 * S
    orbs = [[list(range(9))], [list(range(n - 18, n - 9)), list(range(n - 9, n))]]   # K_0 = 9, K_1 = 18
    nbs = [[[0, 1, 2]], [[0, 1, 2], [6, 7, 8]]]
    engine.set_system(F, S)
    h = engine.sigma_bethe(orbs, nbs, [H0, H0], [Sl, Sl], [Vl, Vl], None, 1e-4, 1e-8)
    try:
        E = np.linspace(-3.8, -2.6, 4)
        T, psi, _, _ = _provider_check(engine, h, F, S, E, 0, 1, "bethe 9 -> 18")
        assert T.shape == (4, 9)
        T, psi, _, _ = _provider_check(engine, h, F, S, E, 1, 0, "bethe 18 -> 9")
        assert T.shape == (4, 18) and psi.shape == (4, 18, n)
    finally:
        engine.sigma_free(h)


# --------------------------------------------------------------------------- streaming, spin, refusals, singular energies
def test_batch_streaming_bitwise(engine):
    n = 60
    F, S = random_system(n, 61)
    rng = np.random.default_rng(6)
    ss = R.block_sigma(n, np.arange(8), rng); sd = R.block_sigma(n, np.arange(n - 6, n), rng)
    E = np.linspace(-2.0, 2.0, 7)
    engine.set_system(F, S)
    h = engine.sigma_const([ss, sd])
    try:
        engine.set_batch(3)
        try:
            T3, p3 = engine.channel_states(h, 0, 1, E)
            swept(engine, 3, E.size)
        finally:
            engine.set_batch(0)
        T0, p0 = engine.channel_states(h, 0, 1, E)
    finally:
        engine.sigma_free(h)
    assert np.all(np.isfinite(T0)) and np.any(p0 != 0)
    assert np.array_equal(T3, T0) and np.array_equal(p3, p0)


def test_spin_layouts(engine):
    from gaunegf_amd.transport import SigmaCalculator, calculate_channel_states
    N = 20
    Fa, S = random_system(N, 71)
    Fb, _ = random_system(N, 72)
    rng = np.random.default_rng(8)
    sL = R.block_sigma(N, np.arange(4), rng); sR = R.block_sigma(N, np.arange(N - 5, N), rng)
    Z = np.zeros((N, N))
    F2 = np.block([[Fa, Z], [Z, Fb]]); S2 = np.block([[S, Z], [Z, S]])
    E = np.linspace(-1.5, 1.5, 5)
    sc = SigmaCalculator(sL, sR)
    (Tu, pu), (Td, pd) = calculate_channel_states(F2, S2, sc, E, spin='u')
    Ta, pa = calculate_channel_states(Fa, S, sc, E)
    Tb, pb = calculate_channel_states(Fb, S, sc, E)
    assert Tu.shape == (5, 4) and pu.shape == (5, 4, N)
    assert np.array_equal(Tu, Ta) and np.array_equal(pu, pa) and np.array_equal(Td, Tb) and np.array_equal(pd, pb)
    with pytest.raises(NotImplementedError, match="spinor"):
        calculate_channel_states(F2, S2, sc, E, spin='g')
    F2m = F2.copy(); F2m[0, N] = F2m[N, 0] = 0.01
    with pytest.raises(NotImplementedError, match="spin mixing"):
        calculate_channel_states(F2m, S2, sc, E, spin='u')


def test_refusals(engine):
    from helpers import MockSigma
    from gaunegf_amd import _lib
    from gaunegf_amd.transport import SigmaCalculator, calculate_channel_states
    n = 110
    F, S = random_system(n, 81)
    base = np.zeros((n, n), complex)
    with pytest.raises(NotImplementedError):
        calculate_channel_states(F, S, SigmaCalculator(MockSigma(base, [base, base])), np.array([0.1]))
    # K_s = 97 is refused, K_d = 97 is not
    s97 = np.zeros((n, n), complex); s97[np.arange(97), np.arange(97)] = -0.05j
    s5 = np.zeros((n, n), complex); s5[np.arange(n - 5, n), np.arange(n - 5, n)] = -0.05j
    with pytest.raises(NotImplementedError, match="96"):
        calculate_channel_states(F, S, SigmaCalculator(s97, s5), np.array([0.1]))
    T, psi = calculate_channel_states(F, S, SigmaCalculator(s97, s5), np.array([0.1]), source=-1)
    assert T.shape == (1, 5) and psi.shape == (1, 5, n) and np.all(np.isfinite(T))
    engine.set_system(F, S)
    E = np.array([0.1, 0.2])
    # PRECOMPUTED providers and the total self-energy as a contact
    hp = engine.sigma_precomputed(np.stack([s97 + s5] * 2), np.stack([np.stack([s97, s5])] * 2))
    hc = engine.sigma_const([s5, s5])
    try:
        with pytest.raises(NotImplementedError):
            engine.channel_states(hp, 0, 1, E)
        with pytest.raises(NotImplementedError):
            engine.channel_states_count(hc, _lib.NEGF_IND_TOTAL)
        with pytest.raises(NotImplementedError):
            engine.channel_states(hc, 0, _lib.NEGF_IND_TOTAL, E)
        assert engine.channel_states_count(hc, 0) == 5
    finally:
        engine.sigma_free(hp); engine.sigma_free(hc)
    with pytest.raises(ValueError):
        engine.eigh(np.zeros((1, 97, 97)))


def test_bethe_with_xi_refused(engine):
    from gaunegf_amd.surfGBethe import read_bethe_params, construct_sk_matrix, gen_neighbors
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaunegf_amd", "data", "Au")
    ne, Ed, Vd, Sd, H0 = read_bethe_params(here)
    dirs = gen_neighbors(np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.2, 0.0]))
    Sl = np.array([construct_sk_matrix(Sd, d) for d in dirs]); Vl = np.array([construct_sk_matrix(Vd, d) for d in dirs])
    n = 27
    F, S = random_system(n, 19)
    engine.set_system(F, S)
    h = engine.sigma_bethe([[list(range(9))], [list(range(n - 9, n))]], [[[0, 1, 2]], [[0, 1, 2]]], [H0, H0], [Sl, Sl],
                           [Vl, Vl], np.eye(n), 1e-4, 1e-8)
    try:
        with pytest.raises(NotImplementedError):
            engine.channel_states(h, 0, 1, np.array([-3.0]))
    finally:
        engine.sigma_free(h)


def test_singular_energy_nan_rows(engine):
    """An exactly singular energy: NaN in every column of T and psi (also beyond K_s), its info set; the others finite."""
    n = 8
    sL = np.zeros((n, n), complex); sL[0, 0] = -0.5j
    sR = np.zeros((n, n), complex); sR[n - 1, n - 1] = -0.25j
    S = np.eye(n, dtype=complex)
    F = S - sL - sR                                                       # E S - F - Sigma = (E - 1) S: zero at E = 1
    E = np.array([0.3, 1.0, 1.7])
    engine.set_system(F, S)
    h = engine.sigma_const([sL, sR])
    try:
        with pytest.warns(RuntimeWarning, match="singular"):
            T, psi = engine.channel_states(h, 0, 1, E, nchan=3)
        assert engine.last_info[1] > 0 and engine.last_info[0] == 0 and engine.last_info[2] == 0
    finally:
        engine.sigma_free(h)
    assert np.all(np.isnan(T[1])) and np.all(np.isnan(psi[1].real)) and np.all(np.isnan(psi[1].imag))
    assert np.all(np.isfinite(T[[0, 2]])) and np.all(np.isfinite(psi[[0, 2]]))
    assert np.all(T[[0, 2], 1:] == 0.0) and np.all(psi[[0, 2], 1:] == 0.0) and np.all(psi[[0, 2], 0, 0].real > 0)
