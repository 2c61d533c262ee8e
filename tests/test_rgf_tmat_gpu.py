"""The transmission matrix of a layered device with probes on any layer on the MI355X (negf_layered_transmission_matrix,
gaunegf_amd/layered.py) against the extended-precision truth of rgf_tmat_ref.py, against the dense engine, and against
itself (conservation, exactness, refusals, singular energies, workspace)."""
import warnings

import numpy as np
import pytest

import rgf_ref as rr
import rgf_tmat_ref as tm
from helpers import chain_lead
from gaunegf_amd.layered import (Lead, LayeredSystem, calculate_effective_current_layered,
                                 calculate_effective_transmission_layered, calculate_transmission_layered,
                                 calculate_transmission_matrix_layered, dephasing_probes_layered)

pytestmark = pytest.mark.gpu


def bind(eng, c):
    """handle of a TmCase with its end terminals, const"""
    b = c.base
    h = eng.layered_create(b.F_diag, b.F_up, b.S_diag, b.S_up)
    for lay, idx, blk in c.leads:
        eng.layered_terminal_const(h, lay, idx, blk)
    return h


def probes_of(c):
    return c.global_terms(c.probes)


def gpu_matrix(eng, c, E, probes="case"):
    h = bind(eng, c)
    try:
        return eng.layered_transmission_matrix(h, E, probes_of(c) if probes == "case" else probes)
    finally:
        eng.layered_free(h)


def dense_matrix(eng, c, E, probes="case"):
    F, S = c.to_dense()
    eng.set_system(F, S)
    sig = []
    for gi, blk in c.global_terms(c.leads):
        s = np.zeros((c.N, c.N), complex); s[np.ix_(gi, gi)] = blk
        sig.append(s)
    hd = eng.sigma_const(sig)
    try:
        return eng.transmission_matrix(hd, E, probes_of(c) if probes == "case" else probes)
    finally:
        eng.sigma_free(hd)


@pytest.fixture(scope="module")
def gpu_table(engine):
    """{case name: T [m, C, C] of the engine at the case's energies}: one call per case, shared"""
    return {c.name: gpu_matrix(engine, c, np.asarray(c.energies)) for c in tm.cases()}


# --------------------------------------------------------------------------- truth
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_truth(gpu_table, name):
    """within C_RTM times the larger error of the float64 recursion run forwards and on the mirrored case"""
    ents = [e for e in tm.truth_table() if e["case"].name == name]
    got = gpu_table[name]
    assert len(ents) == got.shape[0]
    res = []
    for k, ent in enumerate(ents):
        err, bar = tm.rel_err(got[k], ent["truth"]), tm.bar(ent)
        print(f"{ent['tag']:22s} err {err:.3g}  bar {bar:.3g}  (fwd {ent['err_fwd']:.3g}, mirror {ent['err_mir']:.3g})")
        res.append((ent["tag"], err, bar))
    for tag, err, bar in res:
        assert err <= bar, tag


# --------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_parity_with_the_dense_engine(engine, gpu_table, name):
    c = next(x for x in tm.cases() if x.name == name)
    Td = dense_matrix(engine, c, np.asarray(c.energies))
    assert gpu_table[name].shape == Td.shape
    assert tm.rel_err(gpu_table[name], Td) <= tm.PROJECT_BAR


def test_without_probes_it_is_the_matrix_of_the_end_terminals(engine):
    c = tm.cases()[1]                                                   # left, right, a second terminal on layer 0
    E = np.asarray(c.energies)
    h = bind(engine, c)
    try:
        T = engine.layered_transmission_matrix(h, E)
        assert T.shape == (E.size, 3, 3) and engine.layered_terminal_count(h) == 3
        for a, b in ((1, 0), (0, 1), (1, 2), (2, 1)):                   # opposite ends: layered_transmission's corner blocks
            assert tm.rel_err(T[:, a, b], engine.layered_transmission(h, a, b, E)) <= tm.PROJECT_BAR, (a, b)
        with pytest.raises(ValueError):
            engine.layered_transmission(h, 0, 2, E)                     # the same end: refused there, served here
    finally:
        engine.layered_free(h)
    Td = dense_matrix(engine, c, E, probes=None)
    assert tm.rel_err(T, Td) <= tm.PROJECT_BAR
    for a, b in ((0, 2), (2, 0), (0, 0), (2, 2), (1, 1)):               # same-end pairs
        assert tm.rel_err(T[:, a, b], Td[:, a, b]) <= tm.PROJECT_BAR, (a, b)


# --------------------------------------------------------------------------- conservation
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_conservation(gpu_table, name):
    c = next(x for x in tm.cases() if x.name == name)
    for k, E in enumerate(c.energies):
        if np.imag(E) != 0:
            continue
        T = gpu_table[name][k]
        dev = np.abs(T.sum(axis=0) - T.sum(axis=1)).max()
        print(f"{name} E={E:.6g}: |row sums - column sums| = {dev:.3g}, max T = {np.abs(T).max():.3g}")
        assert dev <= 1e-11 * np.abs(T).max()


# --------------------------------------------------------------------------- exactness
def test_runs_and_batches_do_not_change_a_bit(engine, gpu_table):
    for name in ("b", "c"):
        c = next(x for x in tm.cases() if x.name == name)
        E = np.asarray(c.energies)
        assert np.array_equal(gpu_matrix(engine, c, E), gpu_table[name]), name
        for nb in (1, 3):
            engine.set_batch(nb)
            try:
                assert np.array_equal(gpu_matrix(engine, c, E), gpu_table[name]), (name, nb)
            finally:
                engine.set_batch(0)


def test_permuted_probes_permute_the_matrix_bit_for_bit(engine, gpu_table):
    c = tm.cases()[1]                                                   # its probes on layer 1 overlap
    pr = probes_of(c)
    p = np.array([2, 0, 3, 1])
    T = gpu_matrix(engine, c, np.asarray(c.energies), probes=[pr[k] for k in p])
    full = np.concatenate([np.arange(c.n_t), c.n_t + p])
    assert np.array_equal(T, gpu_table["b"][:, full][:, :, full])


def test_permuted_energies_permute_the_results(engine, gpu_table):
    c = tm.cases()[3]
    p = np.array([2, 0, 3, 1])
    assert np.array_equal(gpu_matrix(engine, c, np.asarray(c.energies)[p]), gpu_table["d"][p])


def test_device_resident_form(engine, gpu_table):
    """grid and result in HBM (buffers through the HIP runtime the library itself is linked against): bitwise the
    host-pointer form"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    c = tm.cases()[1]
    E = np.ascontiguousarray(c.energies, dtype=np.complex128)
    Cn = len(c.terms)
    res = np.full((E.size, Cn, Cn), np.nan)
    dE, dT = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dE), E.nbytes) == 0 and hip.hipMalloc(C.byref(dT), res.nbytes) == 0
    h = bind(engine, c)
    try:
        assert hip.hipMemcpy(dE, E.ctypes.data_as(C.c_void_p), E.nbytes, 1) == 0            # host -> device
        assert hip.hipMemcpy(dT, res.ctypes.data_as(C.c_void_p), res.nbytes, 1) == 0
        engine.layered_transmission_matrix_dev(h, E.size, dE.value, dT.value, probes_of(c))
        engine.sync()
        assert hip.hipMemcpy(res.ctypes.data_as(C.c_void_p), dT, res.nbytes, 2) == 0        # device -> host
        assert np.array_equal(res, gpu_table["b"])
        with pytest.raises(ValueError):
            engine.layered_transmission_matrix_dev(h, E.size, dE.value, dT.value, [([6, 7], np.zeros((2, 2)))])
    finally:
        engine.layered_free(h)
        hip.hipFree(dE); hip.hipFree(dT)


# --------------------------------------------------------------------------- chain terminals
@pytest.mark.parametrize("solver", ["fixed-point", "doubling"])
def test_chain_terminals_with_probes(engine, solver):
    c = tm.cases()[3]
    b = c.base
    E = np.asarray(c.energies)
    nl = c.sizes[-1]
    il, ir = np.arange(6), np.arange(nl - 6, nl)
    leads = [chain_lead(6, 41), chain_lead(6, 42)]
    eta, conv, rel = 1e-4, 1e-7, 0.1
    probes = probes_of(c)[3:17]
    h = engine.layered_create(b.F_diag, b.F_up, b.S_diag, b.S_up)
    F, S = c.to_dense()
    engine.set_system(F, S)
    hd = None
    try:
        ts = []
        for layer, idx, (a, Sa, bb, Sb) in ((0, il, leads[0]), (len(c.sizes) - 1, ir, leads[1])):
            ts.append(engine.layered_terminal_chain(h, layer, idx, a, Sa, bb, Sb, bb, Sb, eta, conv, rel, solver=solver))
        sig0 = [engine.layered_terminal_sigma(h, t, E, 6) for t in ts]
        T = engine.layered_transmission_matrix(h, E, probes)
        sig1 = [engine.layered_terminal_sigma(h, t, E, 6) for t in ts]
        assert all(np.array_equal(x, y) for x, y in zip(sig0, sig1))   # the terminals' Sigma: unchanged by the matrix call
        glob = [il, c.offsets[-2] + ir]
        hd = engine.sigma_chain1d(glob, *[[leads[0][k], leads[1][k]] for k in range(4)],
                                  [leads[0][2], leads[1][2]], [leads[0][3], leads[1][3]], eta, conv, rel, solver=solver)
        Td = engine.transmission_matrix(hd, E, probes)
        assert np.all(np.isfinite(T)) and T.shape == Td.shape == (E.size, 16, 16)
        assert tm.rel_err(T, Td) <= tm.PROJECT_BAR
        # `blocks` terminals fed with that Sigma give the chain terminals' matrix bit for bit
        hb = engine.layered_create(b.F_diag, b.F_up, b.S_diag, b.S_up)
        try:
            engine.layered_terminal_blocks(hb, 0, il, sig0[0])
            engine.layered_terminal_blocks(hb, len(c.sizes) - 1, ir, sig0[1])
            assert np.array_equal(engine.layered_transmission_matrix(hb, E, probes), T)
            with pytest.raises(ValueError):
                engine.layered_transmission_matrix(hb, np.concatenate([E, [0.1]]), probes)   # m beyond the blocks
        finally:
            engine.layered_free(hb)
    finally:
        engine.layered_free(h)
        if hd is not None:
            engine.sigma_free(hd)


# --------------------------------------------------------------------------- physics
def _chain(N, gamma):
    """uniform nearest-neighbour chain, S = 1, layers of 4 sites, wide-band leads on the two end sites"""
    F = -1.0 * (np.eye(N, k=1) + np.eye(N, k=-1))
    S = np.eye(N)
    ls = LayeredSystem.from_dense(F, S, [4] * (N // 4))
    leads = [Lead.const([0], [[-0.5j]]), Lead.const([N - 1], [[-0.5j]])]
    probes = dephasing_probes_layered(ls, [[i] for i in range(N)], gamma)
    return F, S, ls, leads, probes


def test_ohmic_chain(engine):
    from gaunegf_amd.transport import SigmaCalculator, calculate_effective_current, calculate_effective_transmission
    E = np.array([-0.5, 0.0, 0.3])
    inv = []
    for N in (16, 32, 64):
        F, S, ls, leads, probes = _chain(N, 0.2)
        eff, coh = calculate_effective_transmission_layered(ls, leads, E, probes, engine=engine)
        sl = np.zeros((N, N), complex); sl[0, 0] = -0.5j
        sr = np.zeros((N, N), complex); sr[-1, -1] = -0.5j
        sc = SigmaCalculator(sl, sr)
        effd, cohd = calculate_effective_transmission(F, S, sc, E, probes)
        assert tm.rel_err(eff, effd) <= tm.PROJECT_BAR and tm.rel_err(coh, cohd) <= tm.PROJECT_BAR
        inv.append(1.0 / eff)
        # no dephasing: T_eff = T_coherent = the coherent transmission
        _, _, _, _, zero = _chain(N, 0.0)
        e0, c0 = calculate_effective_transmission_layered(ls, leads, E, zero, engine=engine)
        T = calculate_transmission_layered(ls, leads, E, pair=(1, 0), engine=engine)
        assert np.array_equal(e0, c0) and tm.rel_err(c0, T) <= tm.PROJECT_BAR
        if N == 16:
            for temp in (0.0, 300.0):
                I = calculate_effective_current_layered(ls, leads, 0.0, 0.4, probes, T=temp, dE=0.05, engine=engine)
                Id = calculate_effective_current(F, S, sc, 0.0, 0.4, probes, T=temp, dE=0.05)
                assert abs(I - Id) <= tm.PROJECT_BAR * abs(Id) and I > 0
    print("1/T_eff at N = 16, 32, 64:", inv)
    assert np.all(inv[1] > inv[0]) and np.all(inv[2] > inv[1])


# --------------------------------------------------------------------------- refusals
def test_refusals(engine):
    c = tm.cases()[1]
    E = np.asarray(c.energies)
    o = c.offsets
    one = np.array([[-0.1j]])
    h = bind(engine, c)
    bare = engine.layered_create(c.base.F_diag, c.base.F_up, c.base.S_diag, c.base.S_up)
    engine.profile(True)
    engine.profile_reset()
    try:
        with pytest.raises(ValueError):
            engine.layered_transmission_matrix(h, E, [([o[1] - 1, o[1]], np.zeros((2, 2)))])     # spans layers 0 and 1
        with pytest.raises(ValueError):
            engine.layered_transmission_matrix(h, E, [([4, 4], np.zeros((2, 2)))])               # named twice
        with pytest.raises(ValueError):
            engine.layered_transmission_matrix(h, E, [([c.N], one)])                             # outside the system
        with pytest.raises(ValueError):
            engine.layered_transmission_matrix(h, E, [([k % c.N], one) for k in range(1022)])    # C = 1025
        with pytest.raises(ValueError):
            engine.layered_transmission_matrix(bare, E)                                          # C = 0
        with pytest.raises(ValueError):
            engine.layered_transmission_matrix(17, E)                                            # no such system
        with pytest.raises(ValueError):
            engine.layered_terminal_const(h, 1, [0], one)                                        # an interior TERMINAL: still refused
        for fam in ("rgf", "inverse", "zgemm", "tmat"):
            assert engine.profile_read(fam)[1] == 0, fam
        T = engine.layered_transmission_matrix(h, E, [([k % c.N], one) for k in range(1021)])    # C = 1024 is served
        assert T.shape == (E.size, 1024, 1024) and np.all(np.isfinite(T))
        for fam in ("rgf", "inverse", "zgemm", "tmat"):
            assert engine.profile_read(fam)[1] > 0, fam
    finally:
        engine.profile(False)
        engine.layered_free(h)
        engine.layered_free(bare)
    ls = LayeredSystem(c.base.F_diag, c.base.F_up, c.base.S_diag, c.base.S_up)
    leads = [Lead.const(g, blk) for g, blk in c.global_terms(c.leads)]
    with pytest.raises(NotImplementedError):
        calculate_transmission_matrix_layered(ls, leads, E, probes_of(c), spin='u', engine=engine)
    with pytest.raises(NotImplementedError):
        calculate_transmission_matrix_layered(ls, leads, E, probes_of(c), checkpoint_file="x.npz", engine=engine)
    with pytest.raises(ValueError):
        calculate_transmission_matrix_layered(ls, leads, E, [([o[1] - 1, o[1]], np.zeros((2, 2)))], engine=engine)
    T = calculate_transmission_matrix_layered(ls, leads, E, probes_of(c), engine=engine)
    assert np.array_equal(T, gpu_matrix(engine, c, E))


# --------------------------------------------------------------------------- singular energy
def test_a_singular_layer_gives_a_nan_matrix_for_that_energy_only(engine):
    """layer 1 decoupled with F_11 = 0, S_11 = 1 at E = 0, a probe on two of its orbitals: NaN there, its info as
    layered_gr_int names it, the other energy untouched"""
    c = rr.cases()[0]
    Fd = [c.F_diag[0], np.zeros_like(c.F_diag[1])]
    Sd = [c.S_diag[0], np.eye(c.sizes[1])]
    Fu = [np.zeros_like(c.F_up[0])]
    probes = [([1, 2], np.array([[-0.2j, 0.01], [0.01, -0.3j]])),            # on layer 0 (orbitals 0 .. 2)
              ([3, 4], np.array([[-0.1j, 0.0], [0.0, -0.1j]]))]              # on layer 1: its other three orbitals stay singular
    h = engine.layered_create(Fd, Fu, Sd, Fu)
    try:
        engine.layered_terminal_const(h, 0, c.left, c.sig_left)
        E = np.array([0.3, 0.0, -0.2])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            engine.layered_gr_int(h, E, np.ones(3))
            info0 = engine.last_info.copy()
        with pytest.warns(RuntimeWarning, match="singular"):
            T = engine.layered_transmission_matrix(h, E, probes)
        info = engine.last_info.copy()
        good = engine.layered_transmission_matrix(h, E[[0, 2]], probes)
    finally:
        engine.layered_free(h)
    assert info[0] == 0 and info[2] == 0 and info[1] != 0
    assert info[1] > c.sizes[0] and info0[1] > c.sizes[0]               # a column of layer 1, counted over the whole system
    assert np.all(np.isnan(T[1])) and np.array_equal(T[[0, 2]], good) and np.all(np.isfinite(good))


# --------------------------------------------------------------------------- workspace
def test_workspace_is_the_documented_count(engine):
    c = tm.cases()[3]
    E = np.asarray(c.energies)
    L, nmax, Ktot = len(c.sizes), max(c.sizes), c.N                     # a probe on every orbital: K_tot = N
    h = bind(engine, c)
    try:
        engine.layered_transmission_matrix(h, E, probes_of(c))
        got = engine.layered_workspace_bytes(h)
    finally:
        engine.layered_free(h)
    batch = E.size                                                      # the automatic batch holds the whole grid
    static = sum(t[1].size ** 2 for t in c.terms)                       # Gamma of the probes and the const terminals
    # per energy: 10 + L layer matrices, two strips; no Gamma that depends on E, no pair on the matrix-core path
    assert got == 16 * (batch * ((10 + L) * nmax ** 2 + 2 * nmax * Ktot) + static)
