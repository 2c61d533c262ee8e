"""
The multi-terminal transmission matrix and the dephasing probes on the MI355X (negf_transmission_matrix[_dev],
k_tmatrix.hip, and the front ends of transport.py) against tests/tmatrix_ref.py.

Shapes (tmatrix_ref.cases()): n = 24 with four contacts K = (1, 5, 9, 4) and no probes; n = 40 (complex Hermitian) with
contacts (5, 9) and probes K = 1, 1, 3, 9 -- one on a lead's orbital, two overlapping, one with Sigma = 0 --; n = 130 with
contacts (40, 30) and ten probes of 9; n = 200 (complex Hermitian) with terminals of K = 100, 17, 63, 64, 65, which
cross every class of the pair routing (64 / 256-thread pair kernel, the product sequence for two lead-sized blocks and
for K_a K_b > 1536).  n <= 96 and n > 96 run the two inverse routes.  Four real energies each, one 5e-4 above an
eigenvalue of (F, S).

Bars: against the clongdouble truth C_TM x the larger error of the two float64 forms on that input (C_TM = 4, calibrated
on the CPU, test_tmatrix_host.test_calibration); parity with the restatement at the project's 1e-8; the two input
routes (probes as arguments / as extra CONST contacts of Engine.transmission) and the identities on the device's own
output at 1e-10 max T.
"""
import os
import socket
import warnings

import numpy as np
import pytest

import tmatrix_ref as tr
from helpers import chain_lead, random_system, swept

pytestmark = pytest.mark.gpu

BAR = tr.PROJECT_BAR


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _device_T(engine, c, E=None):
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.contact_sigmas())
    try:
        return engine.transmission_matrix(h, c.energies if E is None else E, c.probes)
    finally:
        engine.sigma_free(h)


# --------------------------------------------------------------------------- accuracy, parity, identities
@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_truth_parity_and_identities(engine, idx):
    c = tr.cases()[idx]
    T = _device_T(engine, c)
    C = len(c.terms)
    assert T.shape == (c.energies.size, C, C)
    rows = [r for r in tr.truth_table() if r[1] is c]
    for k, (tag, _, E, truth, ea, eb) in enumerate(rows):
        err = tr.rel_err(T[k], truth)
        par = _rel(T[k], tr.tmatrix(c.F, c.S, c.terms, E))
        bar = tr.C_TM * max(ea, eb)
        tmax = np.abs(T[k]).max()
        cons = np.abs(T[k].sum(axis=1) - T[k].sum(axis=0)).max() / tmax
        print(f"tmatrix {tag}: error {err:.3g} (bar {bar:.3g}, float64 forms {ea:.3g} / {eb:.3g}), parity {par:.3g}, "
              f"conservation {cons:.3g}, min T / max T {T[k].min() / tmax:.3g}")
        assert err <= bar, (tag, err, bar)
        assert par <= BAR, (tag, par)
        assert cons <= 1e-10, (tag, cons)
        assert T[k].min() >= -1e-10 * tmax, (tag, T[k].min())
        if c.real:
            assert np.abs(T[k] - T[k].T).max() <= 1e-10 * tmax, tag
        else:
            assert np.abs(T[k] - T[k].T).max() > 1e-4 * tmax, tag
        if len(c.probes):
            ab, ba = tr.t_eff(T[k], c.n_c, d=1, s=0), tr.t_eff(T[k], c.n_c, d=0, s=1)
            assert abs(ab - ba) <= 1e-10 * tmax, (tag, ab, ba)
    if c.name == "n40":                                    # the probe with Sigma = 0 is terminal 3: exact zeros
        assert not np.any(T[:, 3, :]) and not np.any(T[:, :, 3])


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_probes_as_arguments_equal_probes_as_contacts(engine, idx):
    """Every off-diagonal T[a][b] against Engine.transmission(h, a, b) on a CONST provider that carries the probes as
    extra contacts: the two input routes."""
    c = tr.cases()[idx]
    T = _device_T(engine, c)
    C = len(c.terms)
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.contact_sigmas(c.terms))
    try:
        worst = 0.0
        tmax = np.abs(T).max(axis=(1, 2))
        for a in range(C):
            for b in range(C):
                if a == b:
                    continue
                d = (np.abs(engine.transmission(h, a, b, c.energies) - T[:, a, b]) / tmax).max()
                worst = max(worst, d)
                assert d <= 1e-10, (c.name, a, b, d)
        print(f"tmatrix {c.name}: probes as contacts, worst |dT| / max T {worst:.3g} over {C * (C - 1)} pairs")
    finally:
        engine.sigma_free(h)


# --------------------------------------------------------------------------- other providers
def _probe_set(n, S, rng, lists):
    return [(np.asarray(ix), tr.sigma_block(len(ix), rng)) for ix in lists]


def _check_provider(engine, h, F, S, inds, E, probes, what):
    """parity with the restatement; the contacts' blocks are what the provider itself evaluates (sigma_eval)"""
    F = F.astype(complex); S = S.astype(complex)
    sig = [engine.sigma_eval(h, k, E, len(inds)) for k in range(len(inds))]
    T = engine.transmission_matrix(h, E, probes)
    for k, e in enumerate(E):
        terms = [(np.asarray(ix), sig[q][k][np.ix_(ix, ix)]) for q, ix in enumerate(inds)] + list(probes)
        ref = tr.tmatrix_alt(F, S, terms, e)
        tmax = np.abs(T[k]).max()
        cons = np.abs(T[k].sum(axis=1) - T[k].sum(axis=0)).max() / tmax
        print(f"tmatrix {what} E={e:.6g}: parity {_rel(T[k], ref):.3g} (bar {BAR:g}), conservation {cons:.3g}")
        assert _rel(T[k], ref) <= BAR, (what, e)
        assert cons <= 1e-8, (what, e, cons)
    return T


@pytest.mark.parametrize("solver", ["fixed-point", "doubling"])
def test_chain_provider(engine, solver):
    from gaunegf_amd.surfG1D import surfG
    n, ncs = 60, (6, 20)
    F, S = random_system(n, 67)
    lead = [chain_lead(k, 40 + q) for q, k in enumerate(ncs)]
    ci = [list(range(ncs[0])), list(range(n - ncs[1], n))]
    rng = np.random.default_rng(67)
    taus = [0.2 * rng.standard_normal((k, k)) for k in ncs]
    staus = [0.02 * rng.standard_normal((k, k)) for k in ncs]
    g = surfG(F, S, ci, taus=taus, staus=staus, alphas=[l[0] for l in lead], aOverlaps=[l[1] for l in lead],
              betas=[l[2] for l in lead], bOverlaps=[l[3] for l in lead], eta=1e-3, solver=solver)
    probes = _probe_set(n, S, rng, [[3], list(range(10, 19)), list(range(15, 24)), [30, 45, 59]])
    engine.set_system(F, S)
    h = g._negf_lower(engine)
    E = np.array([-1.0, 0.2, 1.1])
    T = _check_provider(engine, h, F, S, ci, E, probes, f"chain {solver} n={n}")
    assert np.array_equal(engine.transmission_matrix(h, E, probes), T)     # (the g(E) cache hit returns the same bits)


def test_bethe_provider_and_refusals(engine):
    from gaunegf_amd.surfGBethe import read_bethe_params, construct_sk_matrix, gen_neighbors
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaunegf_amd", "data", "Au")
    ne, Ed, Vd, Sd, H0 = read_bethe_params(here)
    dirs = gen_neighbors(np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.2, 0.0]))
    Sl = np.array([construct_sk_matrix(Sd, d) for d in dirs]); Vl = np.array([construct_sk_matrix(Vd, d) for d in dirs])
    n = 45
    F, S = random_system(n, 17)
    F = F - 5.0 * S
    orbs = [[list(range(9))], [list(range(n - 18, n - 9)), list(range(n - 9, n))]]
    nbs = [[[0, 1, 2]], [[0, 1, 2], [6, 7, 8]]]
    rng = np.random.default_rng(5)
    probes = _probe_set(n, S, rng, [list(range(9, 18)), [20], list(range(14, 23))])
    E = np.linspace(-3.8, -2.6, 3)
    engine.set_system(F, S)
    h = engine.sigma_bethe(orbs, nbs, [H0, H0], [Sl, Sl], [Vl, Vl], None, 1e-4, 1e-8)
    try:
        _check_provider(engine, h, F, S, [list(range(9)), list(range(n - 18, n))], E, probes, "Bethe n=45")
    finally:
        engine.sigma_free(h)
    # Bethe with the Xi Sigma Xi transform and PRECOMPUTED have no contact orbital lists
    h = engine.sigma_bethe(orbs, nbs, [H0, H0], [Sl, Sl], [Vl, Vl], np.eye(n), 1e-4, 1e-8)
    try:
        with pytest.raises(NotImplementedError, match="orbital lists"):
            engine.transmission_matrix(h, E, probes)
    finally:
        engine.sigma_free(h)
    sig = [np.zeros((n, n), complex), np.zeros((n, n), complex)]
    sig[0][0, 0] = -0.1j; sig[1][n - 1, n - 1] = -0.1j
    h = engine.sigma_precomputed(np.stack([sig[0] + sig[1]] * E.size), np.stack([np.stack(sig)] * E.size))
    try:
        with pytest.raises(NotImplementedError, match="orbital lists"):
            engine.transmission_matrix(h, E)
    finally:
        engine.sigma_free(h)


# --------------------------------------------------------------------------- exact checks
@pytest.mark.parametrize("idx", [1, 2])
def test_bitwise_run_to_run_batch_and_probe_order(engine, idx):
    c = tr.cases()[idx]
    E = np.linspace(-2.0, 2.0, 7)
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.contact_sigmas())
    try:
        ref = engine.transmission_matrix(h, E, c.probes)
        assert np.array_equal(engine.transmission_matrix(h, E, c.probes), ref)
        for batch in (1, 3):
            engine.set_batch(batch)
            try:
                cut = engine.transmission_matrix(h, E, c.probes)
                swept(engine, batch, E.size)
            finally:
                engine.set_batch(0)
            assert np.array_equal(cut, ref), batch
        # probe q of the permuted call is probe perm[q] of the original one
        npr = len(c.probes)
        perm = np.random.default_rng(idx).permutation(npr)
        Tp = engine.transmission_matrix(h, E, [c.probes[q] for q in perm])
        full = np.concatenate([np.arange(c.n_c), c.n_c + perm])
        assert np.array_equal(Tp, ref[:, full[:, None], full[None, :]])
        # without probes: the matrix over the contacts alone, and its [0][1] entry is Engine.transmission's T up to rounding
        T0 = engine.transmission_matrix(h, E)
        assert T0.shape == (E.size, c.n_c, c.n_c)
        assert np.abs(T0[:, 0, 1] - engine.transmission(h, 0, 1, E)).max() <= 1e-10 * np.abs(T0).max()
    finally:
        engine.sigma_free(h)


@pytest.mark.parametrize("idx", [1, 3])
def test_scale_equivariance(engine, idx):
    """(E, F, Sigma) -> 2^k (E, F, Sigma), k = +-64, S as it is: A scales by 2^k, G by 2^-k, Gamma by 2^k -- T bitwise
    unchanged."""
    c = tr.cases()[idx]
    T = _device_T(engine, c)
    for k in (64, -64):
        f = 2.0 ** k
        engine.set_system(c.F * f, c.S)
        h = engine.sigma_const([s * f for s in c.contact_sigmas()])
        try:
            Ts = engine.transmission_matrix(h, c.energies * f, [(i, b * f) for i, b in c.probes])
        finally:
            engine.sigma_free(h)
        assert np.array_equal(Ts, T), (c.name, k, np.abs(Ts - T).max())


def test_device_pointer_form(engine):
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    c = tr.cases()[1]
    E = np.ascontiguousarray(c.energies, dtype=np.complex128)
    Cn = len(c.terms)
    out = np.zeros((E.size, Cn, Cn))
    dE, dT = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dE), E.nbytes) == 0 and hip.hipMalloc(C.byref(dT), out.nbytes) == 0
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.contact_sigmas())
    try:
        assert hip.hipMemcpy(dE, E.ctypes.data_as(C.c_void_p), E.nbytes, 1) == 0
        engine.transmission_matrix_dev(h, E.size, dE.value, dT.value, c.probes)
        engine.sync()
        assert not np.any(engine.last_info_dev(E.size))
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), dT, out.nbytes, 2) == 0
        assert np.array_equal(out, engine.transmission_matrix(h, E, c.probes))
    finally:
        engine.sigma_free(h)
        hip.hipFree(dE); hip.hipFree(dT)


@pytest.mark.parametrize("n", [8, 120])
def test_singular_energy(engine, n):
    """An exactly singular energy: a NaN matrix for that energy only, info set, a warning in the front end."""
    sL = np.zeros((n, n), complex); sL[0, 0] = -0.5j
    sR = np.zeros((n, n), complex); sR[n - 1, n - 1] = -0.25j
    probes = [(np.array([2, 3]), np.array([[-0.25j, 0.0], [0.0, -0.125j]])), (np.array([3]), np.array([[-0.5j]]))]
    S = np.eye(n, dtype=complex)
    F = S - sL - sR
    for ix, b in probes:
        F[np.ix_(ix, ix)] -= b                             # E S - F - Sigma - probes = (E - 1) S: zero at E = 1
    E = np.array([0.25, 1.0, 1.75])
    engine.set_system(F, S)
    h = engine.sigma_const([sL, sR])
    try:
        with pytest.warns(RuntimeWarning, match="singular"):
            got = engine.transmission_matrix(h, E, probes)
        assert engine.last_info[1] > 0 and engine.last_info[0] == 0 and engine.last_info[2] == 0
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            clean = engine.transmission_matrix(h, E[[0, 2]], probes)
        assert np.all(np.isnan(got[1]))
        assert np.array_equal(got[[0, 2]], clean) and np.all(np.isfinite(clean))
    finally:
        engine.sigma_free(h)


def test_invalid_probe_lists_and_empty_grid(engine):
    c = tr.cases()[0]
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.contact_sigmas())
    one = np.array([[-0.1j]])
    try:
        for bad in ([([c.n], one)], [([-1], one)], [([2, 2], np.zeros((2, 2)))], [([], np.zeros((0, 0)))],
                    [([1, 2], one)], [([1.5], one)]):
            with pytest.raises(ValueError):
                engine.transmission_matrix(h, c.energies, bad)
        with pytest.raises(NotImplementedError):           # C > 1024
            engine.transmission_matrix(h, c.energies, [([q % c.n], one) for q in range(1021)])
        # the C ABI refuses the same lists itself
        import ctypes as C
        from gaunegf_amd import _lib
        E = np.ascontiguousarray(c.energies, dtype=np.complex128)
        T = np.zeros((E.size, 5, 5)); info = np.zeros(E.size, dtype=np.int32)
        for nk, inds in (([1], [c.n]), ([1], [-1]), ([2], [3, 3]), ([0], [0]), ([c.n + 1], list(range(c.n + 1)))):
            nk = np.array(nk, dtype=np.int32); inds = np.array(inds, dtype=np.int32)
            sg = np.zeros(max(int(nk[0]) ** 2, 4), dtype=np.complex128)
            rc = engine._lib.negf_transmission_matrix(engine._ctx, h, 1, nk.ctypes.data_as(C.c_void_p), inds.ctypes.data_as(C.c_void_p),
                                                      sg.ctypes.data_as(C.c_void_p), E.size, E.ctypes.data_as(C.c_void_p),
                                                      T.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p))
            assert rc == _lib.NEGF_EINVAL, (nk, inds, rc)
        assert engine.transmission_matrix(h, np.zeros(0), None).shape == (0, 4, 4)
    finally:
        engine.sigma_free(h)


def test_neighbouring_entry_points_unchanged(engine):
    """negf_transmission, negf_dos and negf_gless_int before and after the new call in one process: the resident F (the
    CONST provider's F + Sigma) is back in place after the probes' copy stood in for it."""
    c = tr.cases()[2]
    E = np.linspace(-1.5, 1.5, 9)
    w = (np.cos(np.arange(E.size)) + 1.5) + 0.0j
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.contact_sigmas())
    try:
        before = (engine.transmission(h, 0, 1, E), engine.dos(h, E)[1], engine.gless_int(h, 0, E, w))
        engine.transmission_matrix(h, E, c.probes)
        after = (engine.transmission(h, 0, 1, E), engine.dos(h, E)[1], engine.gless_int(h, 0, E, w))
    finally:
        engine.sigma_free(h)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------- front ends
def _static(c):
    from gaunegf_amd.transport import SigmaCalculator
    sig = c.contact_sigmas()
    return SigmaCalculator(sig[0], sig[1])


def test_spin_layouts(engine):
    from gaunegf_amd.transport import calculate_transmission_matrix, cohTransMatrix
    c = tr.cases()[1]
    N = c.n
    sc = _static(c)
    E = c.energies
    Fa, S = c.F, c.S
    Fb = c.F + 0.1 * np.diag(np.cos(np.arange(N)))
    Z = np.zeros((N, N))
    F2 = np.block([[Fa, Z], [Z, Fb]]); S2 = np.block([[S, Z], [Z, S]])
    up, down = calculate_transmission_matrix(F2, S2, sc, E, probes=c.probes, spin='u')
    assert np.array_equal(up, calculate_transmission_matrix(Fa, S, sc, E, probes=c.probes))
    assert np.array_equal(down, calculate_transmission_matrix(Fb, S, sc, E, probes=c.probes))
    assert np.array_equal(up, cohTransMatrix(E, Fa, S, sc.sig1, sc.sig2, probes=c.probes))
    # 'g': the 2N system in spinor order with spin mixing; probes in the caller's (spinor) order
    perm = np.concatenate([np.arange(0, 2 * N, 2), np.arange(1, 2 * N, 2)])       # spinor -> block
    inv = np.argsort(perm)
    F2m = F2.copy(); F2m[1, N + 2] = F2m[N + 2, 1] = 0.05; F2m[N - 6, 2 * N - 7] = F2m[2 * N - 7, N - 6] = -0.03
    Fg = F2m[np.ix_(inv, inv)]; Sg = S2[np.ix_(inv, inv)]
    rng = np.random.default_rng(3)
    probes = [(np.array([4, 5]), tr.sigma_block(2, rng)), (np.array([41, 7, 22]), tr.sigma_block(3, rng))]
    Tg = calculate_transmission_matrix(Fg, Sg, sc, E, probes=probes, spin='g')
    terms = []
    for s in c.contact_sigmas():
        big = np.kron(s, np.eye(2))
        ix = np.nonzero(np.abs(big).sum(axis=0) + np.abs(big).sum(axis=1))[0]
        terms.append((ix, big[np.ix_(ix, ix)]))
    for k, e in enumerate(E):
        assert _rel(Tg[k], tr.tmatrix_alt(Fg, Sg, terms + probes, e)) <= BAR, e
    # 'u' with spin mixing: static, the 2N system as it is
    Tm = calculate_transmission_matrix(F2m, S2, sc, E, probes=[(inv[i], b) for i, b in probes], spin='u')
    assert _rel(Tm, Tg) <= 1e-10
    # energy-dependent providers in those layouts are refused
    from gaunegf_amd.surfGTester import surfGTest
    from gaunegf_amd.transport import SigmaCalculator
    g = surfGTest(np.real(Fa), np.real(S), [list(range(5)), list(range(N - 9, N))], -0.25j)
    with pytest.raises(NotImplementedError, match="static"):
        calculate_transmission_matrix(Fg, Sg, SigmaCalculator(g), E, spin='g')


def test_effective_transmission_and_current(engine):
    from gaunegf_amd.transport import (calculate_effective_current, calculate_effective_transmission, cohTransDephased,
                                       current_grid, dephasing_probes, eoverh, kB)
    from scipy.integrate import trapezoid
    c = tr.cases()[2]
    sc = _static(c)
    probes = dephasing_probes(c.S, [ix for ix, _ in c.probes], np.linspace(0.1, 0.6, len(c.probes)))
    terms = list(c.contacts) + probes
    ref = lambda E: np.array([tr.t_eff(tr.tmatrix_alt(c.F, c.S, terms, e), 2) for e in E])
    eff, coh = calculate_effective_transmission(c.F, c.S, sc, c.energies, probes)
    r = ref(c.energies)
    assert np.abs(eff - r).max() <= BAR * np.abs(r).max()
    assert np.all(eff > coh)                                # the probes re-inject what they absorb
    back, _ = calculate_effective_transmission(c.F, c.S, sc, c.energies, probes, source=-1, drain=0)
    assert np.abs(back - eff).max() <= 1e-10 * np.abs(eff).max()
    assert np.array_equal(np.asarray(cohTransDephased(c.energies, c.F, c.S, sc.sig1, sc.sig2, probes)), eff)
    zero = dephasing_probes(c.S, [ix for ix, _ in c.probes], 0.0)
    e0, c0 = calculate_effective_transmission(c.F, c.S, sc, c.energies, zero)
    assert np.array_equal(e0, c0)
    for T in (0.0, 300.0):
        fermi, qV, dE = 0.1, 0.4, 0.05
        grid, muL, muR = current_grid(fermi, qV, T, dE)
        occ = 1.0 if T == 0 else np.abs(1 / (np.exp((grid - muR) / (kB * T)) + 1) - 1 / (np.exp((grid - muL) / (kB * T)) + 1))
        want = 2 * eoverh * trapezoid(ref(grid) * occ, grid)
        got = calculate_effective_current(c.F, c.S, sc, fermi, qV, probes, T=T, dE=dE)
        assert abs(got - want) <= BAR * abs(want), (T, got, want)


# --------------------------------------------------------------------------- sharded = local
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _front_ends():
    from gaunegf_amd.transport import calculate_effective_transmission, calculate_transmission_matrix
    c = tr.cases()[1]
    sc = _static(c)
    E = np.linspace(-1.0, 1.0, 13)
    return {"tmat": calculate_transmission_matrix(c.F, c.S, sc, E, probes=c.probes),
            "teff": calculate_effective_transmission(c.F, c.S, sc, E, c.probes)[0]}


def _worker(port, q):
    import torch.distributed as dist
    from gaunegf_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_RANK"] = "0"
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        D.enable(single_rank_ok=True)
        assert D.is_active()
        q.put(_front_ends())
    finally:
        D.disable()
        dist.destroy_process_group()


def test_sharded_equals_local(engine):
    """The sharded leg (all-gather of the per-energy rows of C^2 doubles) in a one-rank group."""
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    res = None
    for _ in range(60):
        try:
            res = q.get(timeout=5)
            break
        except queue.Empty:
            if p.exitcode not in (None, 0):
                break
    if res is None:
        p.kill()
        pytest.fail("the rank died (its traceback is on stderr)")
    p.join(timeout=120)
    assert p.exitcode == 0
    ref = _front_ends()
    for key in ref:
        assert np.array_equal(res[key], ref[key]), key
