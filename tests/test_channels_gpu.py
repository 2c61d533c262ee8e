"""Transmission eigenchannels on the GPU (negf_eigvalsh_batched, negf_transmission_channels): the batched Jacobi
eigensolver against numpy, analytic Breit-Wigner channels, rank-deficient couplings, parity with a numpy restatement on
CONST / chain / Bethe providers, independence of the compact transmission path, batch streaming and spin layouts."""
import os
import warnings

import numpy as np
import pytest

from helpers import random_system, swept

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- numpy restatement
def _psd_sqrt(G):
    w, V = np.linalg.eigh(0.5 * (G + G.conj().T))
    return (V * np.sqrt(np.clip(w, 0.0, None))) @ V.conj().T


def np_channels(G, gamL, gamR, IL, IR):
    """T_n = eigenvalues of t^H t, t = Gamma_R^{1/2} G[I_R, I_L] Gamma_L^{1/2} on the contact orbitals, descending,
    the min(K_L, K_R) largest."""
    gl = _psd_sqrt(gamL[np.ix_(IL, IL)])
    gr = _psd_sqrt(gamR[np.ix_(IR, IR)])
    t = gr @ G[np.ix_(IR, IL)] @ gl
    w = np.linalg.eigvalsh(t.conj().T @ t)[::-1]
    return w[:min(len(IL), len(IR))]


def np_transmission(G, gamL, gamR):
    return np.real(np.trace(gamL @ G @ gamR @ G.conj().T))


def gamma(sig):
    return 1j * (sig - sig.conj().T)


def support(sig):
    return np.nonzero(np.any(sig != 0, axis=0) | np.any(sig != 0, axis=1))[0]


def check_parity(T, F, S, sigs_at, E, IL, IR, tol=1e-10):
    """sigs_at(k) -> (Sigma_L, Sigma_R) at energy E[k]; T [m, nchan] from the engine."""
    for k, e in enumerate(E):
        sL, sR = sigs_at(k)
        G = np.linalg.inv(e * S - F - sL - sR)
        ref = np_channels(G, gamma(sL), gamma(sR), IL, IR)
        assert T.shape[1] == ref.size
        assert np.all(np.abs(T[k] - ref) <= tol * max(1.0, ref[0])), (k, T[k][:4], ref[:4])
        assert np.all(np.diff(T[k][T[k] != 0]) <= 0)                        # descending


def block_sigma(n, idx, rng, scale=0.15):
    """A contact self-energy confined to the orbitals idx: -i (PD coupling) / 2 + a Hermitian level shift."""
    K = len(idx)
    A = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
    gam = scale * (A @ A.conj().T) / K
    B = rng.standard_normal((K, K)); h = 0.05 * (B + B.T)
    s = np.zeros((n, n), complex)
    s[np.ix_(idx, idx)] = h - 0.5j * gam
    return s


# --------------------------------------------------------------------------- eigensolver
@pytest.mark.parametrize("K", [1, 2, 3, 17, 50, 64, 96])
def test_eigvalsh_random(engine, K):
    rng = np.random.default_rng(K)
    A = rng.standard_normal((6, K, K)) + 1j * rng.standard_normal((6, K, K))
    A = A + A.conj().transpose(0, 2, 1)
    w = engine.eigvalsh(A)
    ref = np.linalg.eigvalsh(A)
    for k in range(A.shape[0]):
        assert np.all(np.abs(w[k] - ref[k]) <= 1e-12 * np.linalg.norm(A[k]))
        assert np.all(np.diff(w[k]) >= 0)
    assert not np.any(engine.last_info)
    # only the lower triangle is read, like numpy's default
    Al = np.tril(A[0]) + np.triu(rng.standard_normal((K, K)), 1)
    assert np.allclose(engine.eigvalsh(Al), np.linalg.eigvalsh(Al), rtol=0, atol=1e-12 * np.linalg.norm(A[0]))


def test_eigvalsh_special_spectra(engine):
    rng = np.random.default_rng(3)
    mats = []
    for K, vals in ((50, np.repeat([1.0, -2.0, 3.0, 0.5, 0.0], 10)), (64, np.repeat([2.0, -1.0], 32)),
                    (17, np.full(17, 0.7))):
        U, _ = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))
        mats.append((U * vals) @ U.conj().T)                              # exactly degenerate spectra
    mats.append(np.diag(rng.standard_normal(40)).astype(complex))          # diagonal
    mats.append(np.zeros((30, 30), complex))                              # zero
    X = rng.standard_normal((33, 33)) + 1j * rng.standard_normal((33, 33))
    mats.append(1e-8 * (X + X.conj().T))                                   # tiny scale
    for A in mats:
        w = engine.eigvalsh(A[None])[0]
        ref = np.linalg.eigvalsh(A)
        assert np.all(np.abs(w - ref) <= 1e-12 * np.linalg.norm(A)), (A.shape, np.max(np.abs(w - ref)))
        assert np.all(np.diff(w) >= 0)
    assert np.array_equal(engine.eigvalsh(np.zeros((1, 30, 30))), np.zeros((1, 30)))


def test_eigvalsh_nan_row(engine):
    rng = np.random.default_rng(4)
    A = rng.standard_normal((3, 20, 20)) + 0j
    A = A + A.transpose(0, 2, 1)
    A[1, 5, 2] = np.nan
    with pytest.warns(RuntimeWarning, match="non-finite"):
        w = engine.eigvalsh(A)
    assert np.all(np.isnan(w[1])) and engine.last_info[1] != 0
    assert engine.last_info[0] == 0 and engine.last_info[2] == 0
    assert np.allclose(w[[0, 2]], np.linalg.eigvalsh(A[[0, 2]]), rtol=0, atol=1e-11)


# --------------------------------------------------------------------------- analytic channels
def test_breit_wigner_channels_and_rotation(engine):
    k = 5
    rng = np.random.default_rng(11)
    eps = np.array([-0.8, -0.3, 0.05, 0.4, 1.1])
    gL = rng.uniform(0.02, 0.2, k); gR = rng.uniform(0.02, 0.2, k)
    F = np.diag(eps).astype(complex); S = np.eye(k, dtype=complex)
    sL = np.diag(-0.5j * gL); sR = np.diag(-0.5j * gR)
    E = np.linspace(-1.2, 1.3, 41)
    engine.set_system(F, S)
    h = engine.sigma_const([sL, sR])
    try:
        T = engine.transmission_channels(h, 0, 1, E)
    finally:
        engine.sigma_free(h)
    bw = gL * gR / ((E[:, None] - eps) ** 2 + ((gL + gR) / 2) ** 2)
    assert np.all(np.abs(T - -np.sort(-bw, axis=1)) <= 1e-12)
    # a unitary rotation of the contact orbitals leaves the channels unchanged
    U, _ = np.linalg.qr(rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k)))
    rot = lambda M: U @ M @ U.conj().T
    engine.set_system(rot(F), S)
    h = engine.sigma_const([rot(sL), rot(sR)])
    try:
        Tr = engine.transmission_channels(h, 0, 1, E)
    finally:
        engine.sigma_free(h)
    assert np.all(np.abs(Tr - T) <= 1e-11)


def test_rank_deficient_gamma(engine):
    n = 12
    F, S = random_system(n, 21)
    v = np.array([0.3, -0.2 + 0.1j, 0.25])
    sL = np.zeros((n, n), complex); sL[:3, :3] = -0.5j * np.outer(v, v.conj())     # rank-1 Gamma_L on 3 orbitals
    sR = np.zeros((n, n), complex); sR[np.arange(n - 3, n), np.arange(n - 3, n)] = -0.1j
    E = np.linspace(-1.0, 1.0, 9)
    engine.set_system(F, S)
    h = engine.sigma_const([sL, sR])
    try:
        T = engine.transmission_channels(h, 0, 1, E)
        Tt = engine.transmission(h, 0, 1, E)
    finally:
        engine.sigma_free(h)
    assert T.shape == (E.size, 3)
    assert np.all(T[:, 1:] == 0.0)                                        # exact zeros beyond the rank
    assert np.all(T[:, 0] > 0) and np.allclose(T[:, 0], Tt, rtol=1e-11, atol=0)


# --------------------------------------------------------------------------- parity
@pytest.mark.parametrize("KL,KR,n", [(5, 9, 40), (9, 5, 40), (40, 30, 130), (12, 20, 150)])
def test_const_parity_and_sum_rule(engine, KL, KR, n):
    """K_L != K_R in both orders; contacts covering more than half of the orbitals (the compact transmission path is
    off there) on the single-kernel (n <= 96) and on the kernel-sequence path."""
    from gaunegf_amd.transport import SigmaCalculator, calculate_transmission, calculate_transmission_channels
    F, S = random_system(n, KL * 100 + KR)
    rng = np.random.default_rng(n)
    IL = np.arange(KL); IR = np.arange(n - KR, n)
    sL = block_sigma(n, IL, rng); sR = block_sigma(n, IR, rng)
    E = np.linspace(-2.0, 2.0, 37)
    sc = SigmaCalculator(sL, sR)
    T = calculate_transmission_channels(F, S, sc, E)
    assert T.shape == (E.size, min(KL, KR))
    check_parity(T, F, S, lambda k: (sL, sR), E, IL, IR)
    Tt = calculate_transmission(F, S, sc, E)
    assert np.all(np.abs(T.sum(axis=1) - Tt) <= 1e-11 * np.maximum(np.abs(Tt), 1e-3))
    if 2 * (KL + KR) > n:
        from gaunegf_amd.engine import get_engine
        get_engine().set_gamma_algo(1)                                    # the dense transmission: same sum
        try:
            Td = calculate_transmission(F, S, sc, E)
        finally:
            get_engine().set_gamma_algo(0)
        assert np.allclose(T.sum(axis=1), Td, rtol=1e-11, atol=1e-14)


def test_surfgtest_parity(engine):
    """formSigma-style constant contacts (the -i 1e-9 S background makes every orbital part of the support)."""
    from gaunegf_amd.surfGTester import surfGTest
    from gaunegf_amd.transport import SigmaCalculator, calculate_transmission, calculate_transmission_channels
    n = 30
    F, S = random_system(n, 31)
    g = surfGTest(F, S, [list(range(4)), list(range(n - 4, n))], -0.1j)
    E = np.linspace(-1.5, 1.5, 13)
    T = calculate_transmission_channels(F, S, SigmaCalculator(g), E)
    Ifull = np.arange(n)
    check_parity(T, F, S, lambda k: (g.sig[0], g.sig[1]), E, Ifull, Ifull)
    Tt = calculate_transmission(F, S, SigmaCalculator(g), E)
    assert np.allclose(T.sum(axis=1), Tt, rtol=1e-11, atol=1e-13)


def _chain_system(n=120, nc=20, seed=7):
    from helpers import chain_lead
    from gaunegf_amd.surfG1D import surfG
    F, S = random_system(n, seed)
    lead = [chain_lead(nc, 40 + k) for k in range(2)]
    ci = [list(range(nc)), list(range(n - nc, n))]
    rng = np.random.default_rng(seed)
    taus = [0.2 * rng.standard_normal((nc, nc)) for _ in range(2)]
    staus = [0.02 * rng.standard_normal((nc, nc)) for _ in range(2)]
    g = surfG(F, S, ci, taus=taus, staus=staus, alphas=[l[0] for l in lead], aOverlaps=[l[1] for l in lead],
              betas=[l[2] for l in lead], bOverlaps=[l[3] for l in lead], eta=1e-3)
    return F, S, g, ci


def test_chain_parity(engine):
    from gaunegf_amd.transport import SigmaCalculator, calculate_transmission, calculate_transmission_channels, \
        cohTransChannelsE
    F, S, g, ci = _chain_system()
    E = np.linspace(-1.0, 1.0, 11)
    sc = SigmaCalculator(g)
    T = calculate_transmission_channels(F, S, sc, E)
    h = g._negf_lower(engine)
    sL = engine.sigma_eval(h, 0, E, 2); sR = engine.sigma_eval(h, 1, E, 2)
    check_parity(T, F, S, lambda k: (sL[k], sR[k]), E, np.array(ci[0]), np.array(ci[1]))
    Tt = calculate_transmission(F, S, sc, E)
    assert np.all(np.abs(T.sum(axis=1) - Tt) <= 1e-11 * np.maximum(np.abs(Tt), 1e-3))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.array_equal(np.asarray(cohTransChannelsE(E, F, S, g)), T)


def test_bethe_parity(engine):
    from gaunegf_amd.surfGBethe import read_bethe_params, construct_sk_matrix, gen_neighbors
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaunegf_amd", "data", "Au")
    ne, Ed, Vd, Sd, H0 = read_bethe_params(here)
    dirs = gen_neighbors(np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.2, 0.0]))
    Sl = np.array([construct_sk_matrix(Sd, d) for d in dirs]); Vl = np.array([construct_sk_matrix(Vd, d) for d in dirs])
    n = 45
    F, S = random_system(n, 17)
    F = F - 5.0 * S                                                       # around the Au d band
    orbs = [[list(range(9))], [list(range(n - 18, n - 9)), list(range(n - 9, n))]]   # K_L = 9, K_R = 18
    nbs = [[[0, 1, 2]], [[0, 1, 2], [6, 7, 8]]]                          # Gamma PSD on this window (an arbitrary
                                                                          #  direction set can give an indefinite one)
    engine.set_system(F, S)
    h = engine.sigma_bethe(orbs, nbs, [H0, H0], [Sl, Sl], [Vl, Vl], None, 1e-4, 1e-8)
    try:
        E = np.linspace(-3.8, -2.6, 7)
        T = engine.transmission_channels(h, 0, 1, E)
        Tt = engine.transmission(h, 0, 1, E)
        sL = engine.sigma_eval(h, 0, E, 2); sR = engine.sigma_eval(h, 1, E, 2)
    finally:
        engine.sigma_free(h)
    IL = np.array(orbs[0][0]); IR = np.concatenate([np.array(a) for a in orbs[1]])
    assert T.shape == (E.size, 9)
    check_parity(T, F, S, lambda k: (sL[k], sR[k]), E, IL, IR)
    assert np.all(np.abs(T.sum(axis=1) - Tt) <= 1e-11 * np.maximum(np.abs(Tt), 1e-3))


# --------------------------------------------------------------------------- streaming, spin, refusals
def test_batch_streaming_bitwise(engine):
    n = 60
    F, S = random_system(n, 61)
    rng = np.random.default_rng(6)
    sL = block_sigma(n, np.arange(8), rng); sR = block_sigma(n, np.arange(n - 6, n), rng)
    E = np.linspace(-2.0, 2.0, 23)
    engine.set_system(F, S)
    h = engine.sigma_const([sL, sR])
    try:
        one = engine.transmission_channels(h, 0, 1, E)
        engine.set_batch(5)
        try:
            streamed = engine.transmission_channels(h, 0, 1, E)
            swept(engine, 5, E.size)
        finally:
            engine.set_batch(0)
        wide = engine.transmission_channels(h, 0, 1, E, nchan=9)
    finally:
        engine.sigma_free(h)
    assert np.array_equal(one, streamed)
    assert np.array_equal(wide[:, :6], one) and np.all(wide[:, 6:] == 0.0)


def test_spin_layouts(engine):
    from gaunegf_amd.transport import SigmaCalculator, calculate_transmission_channels
    N = 20
    Fa, S = random_system(N, 71)
    Fb, _ = random_system(N, 72)
    rng = np.random.default_rng(8)
    sL = block_sigma(N, np.arange(4), rng); sR = block_sigma(N, np.arange(N - 5, N), rng)
    Z = np.zeros((N, N))
    F2 = np.block([[Fa, Z], [Z, Fb]]); S2 = np.block([[S, Z], [Z, S]])
    E = np.linspace(-1.5, 1.5, 9)
    sc = SigmaCalculator(sL, sR)
    up, down = calculate_transmission_channels(F2, S2, sc, E, spin='u')
    assert np.allclose(up, calculate_transmission_channels(Fa, S, sc, E), rtol=0, atol=1e-13)
    assert np.allclose(down, calculate_transmission_channels(Fb, S, sc, E), rtol=0, atol=1e-13)
    with pytest.raises(NotImplementedError, match="spinor"):
        calculate_transmission_channels(F2, S2, sc, E, spin='g')
    F2m = F2.copy(); F2m[0, N] = F2m[N, 0] = 0.01                       # spin mixing
    with pytest.raises(NotImplementedError, match="spin mixing"):
        calculate_transmission_channels(F2m, S2, sc, E, spin='u')


def test_unserved_providers_raise(engine):
    from helpers import MockSigma
    from gaunegf_amd.transport import SigmaCalculator, calculate_transmission_channels
    n = 110
    F, S = random_system(n, 81)
    base = np.zeros((n, n), complex)
    mock = MockSigma(base, [base, base])
    with pytest.raises(NotImplementedError):
        calculate_transmission_channels(F, S, SigmaCalculator(mock), np.array([0.1]))
    # a CONST contact pair whose smaller list exceeds 96 orbitals
    s1 = -0.05j * np.eye(n); s2 = -0.05j * np.eye(n)
    with pytest.raises(NotImplementedError, match="96"):
        calculate_transmission_channels(F, S, SigmaCalculator(s1, s2), np.array([0.1]))
    with pytest.raises(ValueError):
        engine.eigvalsh(np.zeros((1, 97, 97)))


def test_eigvalsh_extreme_scales(engine):
    """A power-of-two prescale keeps the norms finite and nonzero: entries near 1e160 (whose squares overflow) and
    near 1e-170 (whose squares underflow to zero) give the eigenvalues of the same matrix at unit scale, scaled."""
    rng = np.random.default_rng(12)
    X = rng.standard_normal((24, 24)) + 1j * rng.standard_normal((24, 24))
    A = X + X.conj().T
    w1 = engine.eigvalsh(A[None])[0]
    for scale in (2.0 ** 532, 2.0 ** -565, 1e160, 1e-170, 1e-300):
        As = A * scale
        w = engine.eigvalsh(As[None])[0]
        assert engine.last_info[0] == 0 and np.all(np.isfinite(w))
        ref = np.linalg.eigvalsh(A) * scale
        tol = 1e-12 * 24 * np.max(np.abs(A)) * scale
        assert np.all(np.abs(w - ref) <= tol), (scale, np.max(np.abs(w - ref)) / scale)
    assert np.array_equal(engine.eigvalsh((A * 2.0 ** 532)[None])[0], w1 * 2.0 ** 532)   # a power of two: exactly


def test_channels_nan_row_covers_every_column(engine):
    """An exactly singular energy: the whole row is NaN, also in the columns beyond K_s; other energies keep their
    values and zeros, and the warning names the singular energy."""
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
            T = engine.transmission_channels(h, 0, 1, E, nchan=3)
        assert engine.last_info[1] > 0
    finally:
        engine.sigma_free(h)
    assert np.all(np.isnan(T[1]))
    assert np.all(np.isfinite(T[[0, 2]])) and np.all(T[[0, 2], 1:] == 0.0)


def test_full_support_const_keeps_block_staging_empty():
    """formSigma-style contacts (-1e-9 i S on every orbital) have full supports: their contact blocks (2 n^2 per energy)
    serve the channel path only and must not size the workspace's Sigma-block staging, which no CONST path reads."""
    from oracle import form_sigma
    from gaunegf_amd.engine import Engine
    eng = Engine(0)
    try:
        for n in (80, 200):
            F, S = random_system(n, n)
            s1 = form_sigma(list(range(6)), -0.1j, n, S); s2 = form_sigma(list(range(n - 6, n)), -0.1j, n, S)
            eng.set_system(F, S)
            h = eng.sigma_const([s1, s2])
            try:
                E = np.linspace(-1.0, 1.0, 40)
                eng.gr_int(h, E, np.full(E.size, 0.05))
                eng.gless_int(h, 0, E, np.full(E.size, 0.05))
                eng.transmission(h, 0, 1, E)
                if n <= 96:
                    assert eng.channel_count(h, 0, 1) == n
                    T = eng.transmission_channels(h, 0, 1, E)
                    assert np.allclose(T.sum(axis=1), eng.transmission(h, 0, 1, E), rtol=1e-11, atol=1e-14)
                work, blocks = eng.workspace_bytes()
                assert work > 0 and blocks == 0, (n, work, blocks)
            finally:
                eng.sigma_free(h)
    finally:
        eng.close()
