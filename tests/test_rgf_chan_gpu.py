"""Transmission eigenchannels of layered devices on the MI355X (negf_layered_transmission_channels and the wide kernels
of k_eig_wide.hip behind it) against the extended-precision truth and the bars of xprec_channels.py, against the dense
channel call, and against itself (exactness, scaling, singular energies, the device-resident form)."""
import numpy as np
import pytest

import rgf_chan_ref as rc
import rgf_ref as rr
import xprec_channels as xc
from helpers import chain_lead
from gaunegf_amd import _lib
from gaunegf_amd import layered as ly
from gaunegf_amd.layered import Lead, LayeredSystem, calculate_eigenchannels_layered, calculate_transmission_layered

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _defaults(engine):
    """every test starts and ends with the kernels chosen by size and the automatic batch"""
    ly.set_channel_algo(0, engine=engine)
    engine.set_batch(0)
    yield
    ly.set_channel_algo(0, engine=engine)
    engine.set_batch(0)


def bind(eng, c):
    h = eng.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    tl = eng.layered_terminal_const(h, 0, c.left, c.sig_left)
    tr = eng.layered_terminal_const(h, len(c.sizes) - 1, c.right, c.sig_right)
    return h, tl, tr


def channels(eng, c, E, a="right", nchan=None, algo=0):
    """the layered call with a = the right or the left terminal of a case with const terminals"""
    ly.set_channel_algo(algo, engine=eng)
    h, tl, tr = bind(eng, c)
    try:
        ta, tb = (tr, tl) if a == "right" else (tl, tr)
        return ly.layered_transmission_channels(eng, h, ta, tb, E, nchan)
    finally:
        eng.layered_free(h)
        ly.set_channel_algo(0, engine=eng)


def leads_of(c):
    return [Lead.const(c.left_global, c.sig_left), Lead.const(c.right_global, c.sig_right)]


def system_of(c):
    return LayeredSystem(c.F_diag, c.F_up, c.S_diag, c.S_up)


# --------------------------------------------------------------------------- 1. wide, both sides
@pytest.mark.parametrize("a", ["right", "left"])
def test_wide_on_both_sides(engine, a):
    """(130, 40, 120) complex Hermitian, K = (110 not contiguous, 100): each order of the pair against its own truth --
    a = right factors the right list (K = 100, a on the last layer), a = left the same list in the mirror form"""
    c, E = rc.wide_cases()["both"]
    _, truths = rc.truths_of(f"both a={a}")
    T = calculate_eigenchannels_layered(system_of(c), leads_of(c), E, pair=(1, 0) if a == "right" else (0, 1), engine=engine)
    assert T.shape == (E.size, 100)
    rc.check_T(f"wide both a={a}", truths, T)
    # the sum rule against the layered transmission itself
    Tt = calculate_transmission_layered(system_of(c), leads_of(c), E, pair=(1, 0) if a == "right" else (0, 1), engine=engine)
    assert np.allclose(T.sum(axis=1), Tt, rtol=1e-11, atol=0)


# --------------------------------------------------------------------------- 2. the smallest wide K, both corner blocks
@pytest.mark.parametrize("mirrored", [False, True])
def test_the_smallest_wide_size_on_either_end(engine, mirrored):
    """(100, 20, 150), K = (97, 150): a = the 97-orbital terminal, on layer 0 and -- the mirrored twin, the same device
    with its layers reversed, hence the same truth -- on the last layer"""
    c, E = rc.wide_cases()["edge"]
    _, truths = rc.truths_of("edge a=left")
    T = channels(engine, c.mirrored(), E, "right") if mirrored else channels(engine, c, E, "left")
    assert T.shape == (E.size, 97)
    rc.check_T(f"wide K = 97 {'mirrored' if mirrored else 'as it is'}", truths, T)


# --------------------------------------------------------------------------- 3. truncated, odd rank above 96
def test_a_rank_deficient_coupling_is_truncated(engine):
    """K = 128 with a coupling of exact rank 33: zeros from column 33 on, rank and beyond-rank ratios within the bar"""
    c, E = rc.wide_cases()["rank"]
    _, truths = rc.truths_of("rank a=left")
    T = channels(engine, c, E, "left")
    assert T.shape == (E.size, 128)
    assert np.all(T[:, 33:] == 0.0) and np.all(T[:, :33] != 0.0)
    rc.check_T("wide rank 33 of 128", truths, T)


# --------------------------------------------------------------------------- 4. the wide kernels at the smallest shapes
@pytest.mark.parametrize("a", ["right", "left"])
@pytest.mark.parametrize("name", ["a", "b", "d", "tiny"])
def test_small_shapes_on_both_kernel_sets(engine, name, a):
    """K = 1 .. 4: the wide kernels (algo 1) and the LDS kernels (algo 0) within the bar; the latter also within the sum
    of the two bars of the dense channel call on to_dense()"""
    c, E, cc, truths = rc.small_truths(name, a)
    Tw = channels(engine, c, E, a, algo=1)
    T0 = channels(engine, c, E, a, algo=0)
    assert Tw.shape == T0.shape == (E.size, min(c.left.size, c.right.size))
    rc.check_T(f"small {name} a={a} wide", truths, Tw)
    rc.check_T(f"small {name} a={a} lds", truths, T0)
    engine.set_system(cc.F, cc.S)
    hd = engine.sigma_const([cc.ss, cc.sd])                     # contact 0 = the source (b), contact 1 = the destination (a)
    try:
        Td = engine.transmission_channels(hd, 1, 0, E)
    finally:
        engine.sigma_free(hd)
    for m, t in enumerate(truths):
        r = max(xc.device_rank(T0[m]), xc.device_rank(Td[m]))
        assert np.max(np.abs(T0[m] - Td[m])) <= 2 * xc.C_CHAN * t.beta_T(r, "chan"), (name, a, m)


# --------------------------------------------------------------------------- 5. chain and blocks terminals
@pytest.mark.parametrize("solver", ["fixed-point", "doubling"])
def test_chain_and_blocks_terminals(engine, solver):
    """chain leads on case d, factored per energy, by both kernel sets: the truth takes the device's Sigma(E) as data;
    blocks terminals fed with that Sigma give the same values bit for bit"""
    c = rr.cases()[3]
    E = c.energies[:3]
    nl, L = c.sizes[-1], len(c.sizes)
    il, ir = np.arange(6), np.arange(nl - 6, nl)
    leads = [chain_lead(6, 41), chain_lead(6, 42)]
    eta, conv, rel = 1e-4, 1e-7, 0.1
    h = engine.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    hb = engine.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    try:
        ts = [engine.layered_terminal_chain(h, layer, idx, a, Sa, b, Sb, b, Sb, eta, conv, rel, solver=solver)
              for layer, idx, (a, Sa, b, Sb) in ((0, il, leads[0]), (L - 1, ir, leads[1]))]
        sig = [engine.layered_terminal_sigma(h, ts[k], E, 6) for k in range(2)]
        tb = [engine.layered_terminal_blocks(hb, 0, il, sig[0]), engine.layered_terminal_blocks(hb, L - 1, ir, sig[1])]
        got = {}
        for algo in (0, 1):
            ly.set_channel_algo(algo, engine=engine)
            got[algo] = ly.layered_transmission_channels(engine, h, ts[1], ts[0], E)
            assert np.array_equal(ly.layered_transmission_channels(engine, hb, tb[1], tb[0], E), got[algo])
        Tt = engine.layered_transmission(h, ts[1], ts[0], E)
        with pytest.raises(ValueError):                          # more energies than the blocks terminal holds
            ly.layered_transmission_channels(engine, hb, tb[1], tb[0], c.energies)
    finally:
        engine.layered_free(h); engine.layered_free(hb)
    F, S = c.to_dense(complex)
    gl, gr = il, c.offsets[-2] + ir
    cc = xc.ChanCase(f"chain {solver}", F, S, gl, gr, E, chain=solver)
    cc.sig_dev = []
    for m in range(E.size):
        sl = np.zeros((c.N, c.N), complex); sl[np.ix_(gl, gl)] = sig[0][m]
        sr = np.zeros((c.N, c.N), complex); sr[np.ix_(gr, gr)] = sig[1][m]
        cc.sig_dev.append((sl, sr))
    truths = xc.truths(cc)
    for algo in (0, 1):
        assert got[algo].shape == (E.size, 6)
        rc.check_T(f"chain {solver} algo {algo}", truths, got[algo])
        assert np.allclose(got[algo].sum(axis=1), Tt, rtol=1e-10, atol=0)


# --------------------------------------------------------------------------- 6. exact properties
def _scaled(c, k):
    """E, F, Sigma times 2^k (S stays): T_n unchanged"""
    f = 2.0 ** k
    s = object.__new__(rr.RCase)
    s.__dict__.update(c.__dict__)
    s.F_diag = [f * b for b in c.F_diag]; s.F_up = [f * b for b in c.F_up]
    s.sig_left, s.sig_right = f * c.sig_left, f * c.sig_right
    return s, f


@pytest.mark.parametrize("which", ["wide", "forced"])
def test_exact_properties(engine, which):
    """bitwise: run to run, any batch, energy order, nchan, power-of-two scaling -- on a wide pair and, with the wide
    kernels forced, on case b"""
    if which == "wide":
        c, algo, a = rc.wide_cases()["both"][0], 0, "left"
    else:
        c, algo, a = rr.cases()[1], 1, "right"
    E = np.array([-0.7, 0.0, 0.45, 0.2])
    ref = channels(engine, c, E, a, algo=algo)
    count = ref.shape[1]
    assert np.all(np.isfinite(ref)) and ref.max() > 0
    assert np.array_equal(channels(engine, c, E, a, algo=algo), ref)
    for batch in (1, 3):
        engine.set_batch(batch)
        try:
            assert np.array_equal(channels(engine, c, E, a, algo=algo), ref), batch
        finally:
            engine.set_batch(0)
    p = np.array([2, 0, 3, 1])
    assert np.array_equal(channels(engine, c, E[p], a, algo=algo), ref[p])
    assert np.array_equal(channels(engine, c, E, a, nchan=3, algo=algo), ref[:, :3])
    more = channels(engine, c, E, a, nchan=count + 2, algo=algo)
    assert np.array_equal(more[:, :count], ref) and np.all(more[:, count:] == 0.0)
    for k in (64, -64):
        s, f = _scaled(c, k)
        assert np.array_equal(channels(engine, s, f * E, a, algo=algo), ref), k


def test_workspace_is_the_documented_count(engine):
    c, E = rc.wide_cases()["both"]
    h, tl, tr = bind(engine, c)
    try:
        ly.layered_transmission_channels(engine, h, tr, tl, E)
        got = engine.layered_workspace_bytes(h)
    finally:
        engine.layered_free(h)
    m, nmax, Ka, Kb = E.size, max(c.sizes), c.right.size, c.left.size
    Ks = min(Ka, Kb)
    # per energy: the 10 layer matrices, the two Gammas, G_ab, Z, W, H and the wide solver's copy; once: L^H and its rank;
    # the host form's staging
    assert got == 16 * (m * (10 * nmax ** 2 + Ka ** 2 + Kb ** 2 + 3 * Ka * Kb + 2 * Ks ** 2) + Ks ** 2) + 4 + 8 * m * Ks


# --------------------------------------------------------------------------- 7. a numerically singular layer
@pytest.mark.parametrize("algo", [0, 1])
def test_a_singular_layer_gives_a_nan_row_for_that_energy_only(engine, algo):
    """layer 1 decoupled with F_11 = 0, S_11 = 1 at E = 0 and a terminal on four of its five orbitals: an exact zero
    pivot -- a NaN row, the pivot's column in the whole system, a warning; the other energies bit for bit"""
    c = rr.cases()[0]
    Fd = [c.F_diag[0], np.zeros_like(c.F_diag[1])]
    Sd = [c.S_diag[0], np.eye(c.sizes[1])]
    Fu = [np.zeros_like(c.F_up[0])]
    ly.set_channel_algo(algo, engine=engine)
    h = engine.layered_create(Fd, Fu, Sd, Fu)
    try:
        tl = engine.layered_terminal_const(h, 0, c.left, c.sig_left)
        tr = engine.layered_terminal_const(h, 1, c.right, c.sig_right)
        E = np.array([0.3, 0.0, -0.2])
        with pytest.warns(RuntimeWarning, match="singular"):
            T = ly.layered_transmission_channels(engine, h, tr, tl, E)
        info = engine.last_info.copy()
        good = ly.layered_transmission_channels(engine, h, tr, tl, E[[0, 2]])
        assert np.all(engine.last_info == 0)
        rcode = engine._lib.negf_layered_transmission_channels(
            engine._ctx, h, tr, tl, 3, E.astype(complex).ctypes.data_as(_lib._vp), 3,
            np.zeros((3, 3)).ctypes.data_as(_lib._vp), None)
    finally:
        engine.layered_free(h)
    assert rcode == _lib.NEGF_ESINGULAR
    assert info[0] == 0 and info[2] == 0 and info[1] > c.sizes[0]        # a column of layer 1, counted over the whole system
    assert np.all(np.isnan(T[1])) and np.array_equal(T[[0, 2]], good) and np.all(np.isfinite(good))


# --------------------------------------------------------------------------- 8. the wide solver alone
@pytest.mark.parametrize("K", [1, 2, 3, 17, 97, 130, 257])
def test_the_wide_solver_alone(engine, K):
    mats = rc.solver_spectra(K)
    names = list(mats)
    w = ly.eigvalsh_wide(np.array([mats[n] for n in names]), engine=engine)
    assert np.all(engine.last_info == 0) and w.shape == (len(names), K)
    truth = {}
    worst = 0.0
    for k, n in enumerate(names):
        base, _, s = n.partition("*2^")
        if s:                                                       # the scaled copies: bitwise the scaled values
            assert np.array_equal(w[k], w[names.index(base)] * 2.0 ** int(s)), n
            continue
        truth[n] = xc.herm_eig_ld(mats[n])
        assert np.all(np.diff(w[k]) >= 0), n
        r = xc.solver_ratios(mats[n], w[k], truth=truth[n])[0]
        worst = max(worst, r)
        assert r <= 1.0, (K, n, r)
    print(f"ACC wide solver K = {K}: worst {worst:.3g}")
    assert np.array_equal(ly.eigvalsh_wide(mats[names[0]], engine=engine), w[0])        # one matrix, and run to run


def test_the_wide_solver_at_512_and_its_refusals(engine):
    """K = 512 random and graded against numpy.linalg.eigvalsh at twice the solver bar (both are within one bar of the
    truth); non-finite input; K = 513"""
    K = 512
    rng = np.random.default_rng(512)
    X = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
    X = X + X.conj().T
    D = np.logspace(0, -6, K)
    A = np.array([X, D[:, None] * X * D[None, :]])
    w = ly.eigvalsh_wide(A, engine=engine)
    for k in range(2):
        bar = xc.EIGH_C * K * xc.U * np.linalg.norm(A[k])
        err = np.max(np.abs(w[k] - np.linalg.eigvalsh(A[k])))
        print(f"ACC wide solver K = 512 [{k}]: {err / bar:.3g} bars")
        assert err <= 2 * bar and np.all(np.diff(w[k]) >= 0)
    B = np.array([X[:130, :130], X[:130, :130], X[:130, :130]])
    B[1, 70, 3] = np.nan
    with pytest.warns(RuntimeWarning, match="non-finite"):
        wb = ly.eigvalsh_wide(B, engine=engine)
    assert list(engine.last_info) == [0, 1, 0]
    assert np.all(np.isnan(wb[1])) and np.array_equal(wb[0], wb[2]) and np.all(np.isfinite(wb[0]))
    with pytest.raises(ValueError):
        ly.eigvalsh_wide(np.zeros((1, 513, 513)), engine=engine)
    Z = np.zeros((513, 513), complex)
    rcode = engine._lib.negf_eigvalsh_wide_batched(engine._ctx, 513, 1, Z.ctypes.data_as(_lib._vp),
                                                   np.zeros(513).ctypes.data_as(_lib._vp), None)
    assert rcode == _lib.NEGF_EINVAL


def test_refusals(engine):
    c = rr.cases()[1]
    h, tl, tr = bind(engine, c)
    try:
        t2 = engine.layered_terminal_const(h, 0, [1], np.array([[-0.1j]]))
        assert ly.layered_channel_count(engine, h, tr, tl) == 3 and ly.layered_channel_count(engine, h, tl, tr) == 3
        assert ly.layered_channel_count(engine, h, tr, t2) == 1
        for bad in ((tl, t2), (tl, tl), (tl, 9), (-1, tr)):
            with pytest.raises(ValueError):
                ly.layered_channel_count(engine, h, *bad)
            with pytest.raises(ValueError):
                ly.layered_transmission_channels(engine, h, *bad, c.energies, 2)
        with pytest.raises(ValueError):
            ly.layered_transmission_channels(engine, h, tr, tl, c.energies, 0)
        with pytest.raises(ValueError):
            ly.layered_channel_count(engine, 99, tr, tl)
        with pytest.raises(_lib.NegfError):
            ly.set_channel_algo(2, engine=engine)
    finally:
        engine.layered_free(h)
    # more than 512 channels: two layers of 513 orbitals, every one in its terminal (nothing is computed)
    Z, I = np.zeros((513, 513)), np.eye(513)
    h = engine.layered_create([Z, Z], [Z], [I, I], [Z])
    try:
        ta = engine.layered_terminal_const(h, 0, np.arange(513), -0.1j * I)
        tb = engine.layered_terminal_const(h, 1, np.arange(513), -0.1j * I)
        tc = engine.layered_terminal_const(h, 1, np.arange(512), -0.1j * I[:512, :512])
        with pytest.raises(ValueError):
            ly.layered_channel_count(engine, h, ta, tb)
        assert ly.layered_channel_count(engine, h, ta, tc) == 512
    finally:
        engine.layered_free(h)
    with pytest.raises(ValueError):
        calculate_eigenchannels_layered(system_of(c), [Lead.const([0], [[-0.1j]]), Lead.const([1], [[-0.1j]])], c.energies,
                                        engine=engine)
    with pytest.raises(NotImplementedError):
        ly.calculate_transmission_channels_layered()


# --------------------------------------------------------------------------- 9. the device-resident form
@pytest.mark.parametrize("which", ["wide", "small"])
def test_the_device_form_equals_the_host_form_and_overwrites_its_output(engine, which):
    """on buffers of the HIP runtime the library is linked against; the output starts out as NaN"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    c = rc.wide_cases()["edge"][0] if which == "wide" else rr.cases()[1]
    E = np.array([-0.7, 0.2, 0.45], dtype=np.complex128)
    h, tl, tr = bind(engine, c)
    dE, dT = C.c_void_p(), C.c_void_p()
    try:
        count = ly.layered_channel_count(engine, h, tl, tr)
        nchan = count + 1
        host = ly.layered_transmission_channels(engine, h, tl, tr, E, nchan)
        got = np.full((E.size, nchan), np.nan)
        assert hip.hipMalloc(C.byref(dE), E.nbytes) == 0 and hip.hipMalloc(C.byref(dT), got.nbytes) == 0
        assert hip.hipMemcpy(dE, E.ctypes.data_as(C.c_void_p), E.nbytes, 1) == 0            # host -> device
        assert hip.hipMemcpy(dT, got.ctypes.data_as(C.c_void_p), got.nbytes, 1) == 0        # the poison
        calls, points = engine.counters["calls"], engine.counters["points"]
        ly.layered_transmission_channels_dev(engine, h, tl, tr, E.size, dE.value, nchan, dT.value)
        engine.sync()
        assert (engine.counters["calls"], engine.counters["points"]) == (calls + 1, points + E.size)
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), dT, got.nbytes, 2) == 0        # device -> host
    finally:
        engine.layered_free(h)
        hip.hipFree(dE); hip.hipFree(dT)
    assert np.array_equal(got, host) and np.all(got[:, count:] == 0.0)
