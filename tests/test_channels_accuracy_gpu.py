"""The eigenchannel kernels (pchol_kernel, jacobi_kernel<false|true>, gauge_kernel and the products between them in
negf_transmission_channels / negf_channel_states) against the extended-precision truth and the first-order bars of
tests/xprec_channels.py, on its case table: K_s = 69 / 70 / 96 (the eigenvector accumulator in LDS, in global memory,
K_MAX), odd and truncated ranks with the accumulator in global memory, graded couplings (also across the 1e-14 cut and
with the weakest orbitals first), ill-conditioned energies (kappa_2(A) up to 2e9), the windowed inverse, chain leads
of n_c = 72 (a factorisation per energy), and the solver alone on graded, clustered and Wilkinson spectra.

Every `ACC` line gives error / (C_CHAN beta) per bar, worst over the case's energies: <= 1 passes.  C_CHAN is calibrated
on fp64 numpy references on the CPU (test_channels_accuracy_host.py), never on the device.
"""
import functools

import numpy as np
import pytest

import channel_states_ref as R
import xprec
import xprec_channels as X

pytestmark = pytest.mark.gpu
xprec.require_extended()


@functools.lru_cache(maxsize=None)
def _const(shape, family, ladder, swap=False):
    case = X.const_case(*shape, family=family, ladder=ladder, swap=swap)
    return case, X.truths(case)


def _run(engine, case, nchan=None, states=True):
    """Contact 0 = the source, contact 1 = the destination.  (T, psi, T of transmission_channels(dst, src))."""
    engine.set_system(case.F, case.S)
    h = engine.sigma_const([case.ss, case.sd])
    try:
        T, psi = engine.channel_states(h, 0, 1, case.E, nchan) if states else (None, None)
        assert not np.any(engine.last_info)
        Tc = engine.transmission_channels(h, 1, 0, case.E)
        assert not np.any(engine.last_info)
    finally:
        engine.sigma_free(h)
    return T, psi, Tc


# --------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("spec", X.STATE_SPECS, ids=lambda s: f"{s[0]}-{s[1]}{'-ladder' if s[2] else ''}".replace(" ", ""))
def test_channel_states(engine, spec):
    case, truths = _const(*spec)
    T, psi, Tc = _run(engine, case)
    X.check_outputs(case, truths, T, psi, Tc, case.name)


@pytest.mark.parametrize("spec", X.CHANNEL_ONLY_SPECS, ids=lambda s: f"{s[0]}".replace(" ", ""))
def test_transmission_channels_large(engine, spec):
    """(K_L, K_R) = (90, 75): the mirror form with K_s = 75; (96, 96): K_MAX on both sides.  The contact of the first
    orbitals is L."""
    case, truths = _const(*spec, swap=True)
    engine.set_system(case.F, case.S)
    h = engine.sigma_const([case.sd, case.ss])                       # contact 0 = L = the first orbitals
    try:
        Tc = engine.transmission_channels(h, 0, 1, case.E)
        assert not np.any(engine.last_info)
        assert engine.channel_count(h, 0, 1) == min(case.Ks, case.Kd)
    finally:
        engine.sigma_free(h)
    worst = 0.0
    for m, t in enumerate(truths):
        rc = X.device_rank(Tc[m])
        assert np.all(np.diff(Tc[m, :rc]) <= 0)
        worst = max(worst, max(t.ratios_T(Tc[m], rc, "chan")) / X.C_CHAN)
    print(f"ACC transmission_channels (K_L, K_R, n) = ({case.Kd}, {case.Ks}, {case.n}): T/rank/sum {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("solver", ["fixed-point", "doubling"])
def test_chain_states(engine, solver):
    """Chain leads of n_c = 72: a factorisation per energy (L^H and rank strides 1) with the accumulator in global
    memory; transmission_channels (K_L = K_R) factors the other contact.  The truth takes the device's Sigma(E) as data:
    one evaluation of the total self-energy, whose two contact blocks are the contacts' (their orbital lists are
    disjoint; every evaluation solves the leads again, and the fixed point takes seconds)."""
    F, S, g, ci = X.chain_system(solver)
    engine.set_system(F, S)
    h = g._negf_lower(engine)
    E = X.CHAIN_E
    T, psi = engine.channel_states(h, 0, 1, E)
    assert not np.any(engine.last_info)
    Tc = engine.transmission_channels(h, 1, 0, E)
    assert not np.any(engine.last_info)
    tot = engine.sigma_eval(h, None, E, 2)
    sigs = []
    for idx in ci:
        s_c = np.zeros_like(tot)
        s_c[:, np.ix_(idx, idx)[0], np.ix_(idx, idx)[1]] = tot[:, np.ix_(idx, idx)[0], np.ix_(idx, idx)[1]]
        sigs.append(s_c)
    assert np.array_equal(sigs[0] + sigs[1], tot)                    # nothing outside the two contact blocks
    case = X.chain_case(solver, F, S, ci, sigs[0], sigs[1])
    X.check_outputs(case, X.truths(case), T, psi, Tc, case.name)


# --------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("spec", X.SCALE_SPECS, ids=lambda s: f"{s[0]}-{s[1]}".replace(" ", ""))
def test_scale_equivariance(engine, spec):
    """E, F, Sigma -> 2^k (E, F, Sigma), k = +-64: T bitwise unchanged, psi bitwise 2^(-k/2) times the unscaled one
    (k even: the square roots of the Cholesky scale exactly; pivot order and the Jacobi prescale are invariant)."""
    case, _ = _const(*spec)
    T, psi, Tc = _run(engine, case)
    for k in (64, -64):
        Ts, ps, Tcs = _run(engine, X.scaled_case(case, k))
        assert np.array_equal(Ts, T), (case.name, k, np.max(np.abs(Ts - T)))
        assert np.array_equal(Tcs, Tc), (case.name, k)
        assert np.array_equal(ps, psi * 2.0 ** (-k // 2)), (case.name, k)
    print(f"ACC scale equivariance {case.name}: T and psi bitwise at 2^+-64")


@pytest.mark.parametrize("spec", X.NCHAN_SPECS, ids=lambda s: f"{s[0]}-{s[1]}".replace(" ", ""))
def test_nchan_variants(engine, spec):
    case, _ = _const(*spec)
    T, psi, _ = _run(engine, case)
    T3, p3, _ = _run(engine, case, nchan=3)
    Tw, pw, _ = _run(engine, case, nchan=case.Ks + 2)
    assert np.array_equal(T3, T[:, :3]) and np.array_equal(p3, psi[:, :3])
    assert np.array_equal(Tw[:, :case.Ks], T) and np.array_equal(pw[:, :case.Ks], psi)
    assert np.all(Tw[:, case.Ks:] == 0.0) and np.all(pw[:, case.Ks:] == 0.0)


# --------------------------------------------------------------------------- the solver alone
def _solver_check(engine, A, label):
    w, V = engine.eigh(A)
    assert not np.any(engine.last_info), label
    assert np.array_equal(engine.eigvalsh(A), w), label
    return X.solver_ratios(A, w, V)


@pytest.mark.parametrize("K", X.SOLVER_KS)
def test_solver_spectra(engine, K):
    worst = {}
    for name, A in X.solver_spectra(K).items():
        worst[name] = _solver_check(engine, A, f"{name} K={K}")
    worst["random"] = tuple(np.max([_solver_check(engine, A, f"random K={K}") for A in R.eigh_random(K, 2)], axis=0))
    print(f"ACC eigh K={K}: " + " ".join(f"{n} w {a:.3g} V {b:.3g}" for n, (a, b) in worst.items()))
    bad = {n: v for n, v in worst.items() if not max(v) <= 1.0}
    assert not bad, (K, bad)


def test_solver_special_spectra(engine):
    worst = (0.0, 0.0)
    for i, A in enumerate(R.eigh_special()):
        worst = tuple(np.maximum(worst, _solver_check(engine, A, f"special {i}")))
    print(f"ACC eigh special spectra: w {worst[0]:.3g} V {worst[1]:.3g}")
    assert max(worst) <= 1.0
