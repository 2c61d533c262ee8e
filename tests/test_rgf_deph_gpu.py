"""Floating dephasing probes of a layered device on the MI355X (negf_layered_probe_response, negf_layered_gless_int_probes,
negf_layered_gr_int_probes; gaunegf_amd/layered.py) against the extended-precision truth of rgf_deph_ref.py, against the
dense engine on to_dense(), and against themselves (identities, exactness, undefined occupations, refusals, workspace)."""
import warnings

import numpy as np
import pytest

import rgf_deph_ref as rd
import rgf_less_ref as rl
import rgf_ref as rr
from gaunegf_amd.layered import (Lead, LayeredSystem, GrIntProbesLayered, GrLessIntProbesLayered,
                                 calculate_effective_transmission_layered, calculate_probe_occupations_layered,
                                 calculate_probe_response_layered, dephasing_probes_layered, pattern_to_dense)

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


def flat(blocks):
    return rd.flat_of(*blocks)


def case(name):
    return next(x for x in rd.cases() if x.name == name)


def gpu_results(eng, c, E=None, w=None, probes="case"):
    """dict(R [m, P, n_t], A {s: flat pattern}, G: flat pattern) of the engine: the weighted sums over E with w"""
    E = np.asarray(c.energies) if E is None else E
    w = rd.weights(c) if w is None else w
    pr = probes_of(c) if probes == "case" else probes
    h = bind(eng, c)
    try:
        out = dict(R=eng.layered_probe_response(h, E, pr), A={})
        for s in rd.selections(c):
            out["A"][s] = flat(eng.layered_gless_int_probes(h, s, E, w, pr))
        out["G"] = flat(eng.layered_gr_int_probes(h, E, w, pr))
        return out
    finally:
        eng.layered_free(h)


@pytest.fixture(scope="module")
def gpu_table(engine):
    """{case name: gpu_results at the case's energies and weights}: one set of calls per case, shared"""
    return {c.name: gpu_results(engine, c) for c in rd.cases()}


# --------------------------------------------------------------------------- truth
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_truth(gpu_table, name):
    """R within C_RDEPH times the larger float64 error energy by energy; the sums within C_RDEPH (G: rgf_ref.C_RGF) times
    the strips form's error"""
    c = case(name)
    got = gpu_table[name]
    res = []
    for k, ent in enumerate(rd.entries(c)):
        res.append((f"R {ent['tag']}", rd.rel_err(got["R"][k], ent["truth"]["R"]), rd.bar_R(ent)))
    s = rd.sums(name)
    for key in rd.selections(c) + ["G"]:
        x = got["G"] if key == "G" else got["A"][key]
        res.append((f"sum {name} {key}", rd.rel_err(x, s["truth"][key]), rd.bar_sum(s, key)))
    for tag, err, bar in res:
        print(f"{tag:26s} err {err:.3g}  bar {bar:.3g}  err / bar {err / bar:.3g}")
    for tag, err, bar in res:
        assert err <= bar, tag


# --------------------------------------------------------------------------- parity
def dense_results(eng, c, E, w, probes):
    F, S = c.to_dense()
    eng.set_system(F, S)
    sig = []
    for gi, blk in c.global_terms(c.leads):
        s = np.zeros((c.N, c.N), complex); s[np.ix_(gi, gi)] = blk
        sig.append(s)
    hd = eng.sigma_const(sig)
    try:
        out = dict(R=eng.probe_response(hd, E, probes), A={})
        for s in rd.selections(c):
            out["A"][s] = eng.gless_int_probes(hd, s, E, w, probes)
        out["G"] = eng.gr_int_probes(hd, E, w, probes)
        return out
    finally:
        eng.sigma_free(hd)


def on_pattern(c, M):
    Md, Mu, Ml = rd._cut(c, M)
    return rd.flat_of(Md, Mu, Ml)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_parity_with_the_dense_engine(engine, gpu_table, name):
    c = case(name)
    got = gpu_table[name]
    ref = dense_results(engine, c, np.asarray(c.energies), rd.weights(c), probes_of(c))
    assert got["R"].shape == ref["R"].shape
    assert rd.rel_err(got["R"], ref["R"]) <= rd.PROJECT_BAR
    for s in rd.selections(c):
        assert rd.rel_err(got["A"][s], on_pattern(c, ref["A"][s])) <= rd.PROJECT_BAR, s
    assert rd.rel_err(got["G"], on_pattern(c, ref["G"])) <= rd.PROJECT_BAR
    # and the block lists assemble to the masked dense result
    h = bind(engine, c)
    try:
        blocks = engine.layered_gless_int_probes(h, 0, np.asarray(c.energies), rd.weights(c), probes_of(c))
    finally:
        engine.layered_free(h)
    D = pattern_to_dense(c.sizes, *blocks)
    mask = pattern_to_dense(c.sizes, *[[np.ones(b.shape) for b in kind] for kind in blocks]) > 0
    assert rd.rel_err(D, np.where(mask, ref["A"][0], 0)) <= rd.PROJECT_BAR


# --------------------------------------------------------------------------- identities
def _real(c):
    return np.array([k for k, E in enumerate(c.energies) if np.imag(E) == 0])


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_the_contacts_sums_add_to_the_total(engine, gpu_table, name):
    """(I1) at real energies sum_s R_ps = 1, so sum_s G D_s G^H is the total: within the sum of the bars"""
    c = case(name)
    keep = _real(c)
    ents = [rd.entries(c)[k] for k in keep]
    w = rd.weights(c)[keep]
    got = gpu_table[name] if keep.size == len(c.energies) else gpu_results(engine, c, np.real(np.asarray(c.energies)[keep]), w)
    tol = 0.0
    for s in rd.selections(c):
        t = sum(wk * e["truth"]["A"][s] for wk, e in zip(w, ents))
        x = sum(wk * e["strips"]["A"][s] for wk, e in zip(w, ents))
        tol += rd.C_RDEPH * rd.rel_err(x, t) * np.linalg.norm(got["A"][s])
    dev = np.linalg.norm(sum(got["A"][s] for s in range(c.n_t)) - got["A"][None])
    print(f"{name}: |sum_s A_s - A_total| = {dev:.3g}, the sum of the bars {tol:.3g}")
    assert dev <= tol


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_the_drain_trace_is_the_effective_transmission(engine, name):
    """(I2) Re Tr[Gamma_d A_s[I_d, I_d]] = T_eff[d][s], energy by energy (a one-point grid of weight 1); I_d lies inside an
    end layer's diagonal block.  Bar: C_RDEPH x the strips form's error of A_s x max T."""
    c = case(name)
    b = c.base
    ls = LayeredSystem(b.F_diag, b.F_up, b.S_diag, b.S_up)
    leads = [Lead.const(g, blk) for g, blk in c.global_terms(c.leads)]
    s, d = 0, 1
    lay_d, idx_d, blk_d = c.leads[d]
    gam = 1j * (np.asarray(blk_d) - np.asarray(blk_d).conj().T)
    h = bind(engine, c)
    try:
        for k in _real(c):
            E = np.array([np.real(c.energies[k])])
            eff, _ = calculate_effective_transmission_layered(ls, leads, E, probes_of(c), source=s, drain=d, engine=engine)
            diag, _, _ = engine.layered_gless_int_probes(h, s, E, np.ones(1), probes_of(c))
            tr_ = np.real(np.trace(gam @ diag[lay_d][np.ix_(idx_d, idx_d)]))
            Tmax = np.abs(engine.layered_transmission_matrix(h, E, probes_of(c))).max()
            ent = rd.entries(c)[k]
            bar = rd.C_RDEPH * ent["err_strips"][s] * Tmax
            print(f"{ent['tag']}: trace {tr_:.12g}  T_eff {eff[0]:.12g}  |diff| {abs(tr_ - eff[0]):.3g}  bar {bar:.3g}")
            assert abs(tr_ - eff[0]) <= bar, ent["tag"]
    finally:
        engine.layered_free(h)


@pytest.mark.parametrize("name,sel", [("a", "L"), ("b", "LR"), ("b", "R")])
def test_probes_that_do_nothing(engine, name, sel):
    """(I3) probes with Sigma_p = 0 exactly, and no probes at all: R is exact zeros resp. absent, and the sum is within
    layered_gless_int's bar of the truth of G Gamma G^H (not bitwise layered_gless_int: the columns come through the strips)"""
    c = next(x for x in rr.cases() if x.name == name)
    w = np.array([0.4, 0.7, 1.1, 1.6])
    E = np.asarray(c.energies)
    ent = rl._entry(c, E, w, sel)
    ind = rl.ind_of(sel)
    o = c.offsets
    zero = [(o[1] + np.array([0, 2]), np.zeros((2, 2))), (o[0] + np.array([1]), np.zeros((1, 1))),
            (o[len(c.sizes) - 1] + np.array([1, 0]), np.zeros((2, 2)))]
    h = engine.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    try:
        engine.layered_terminal_const(h, 0, c.left, c.sig_left)
        engine.layered_terminal_const(h, len(c.sizes) - 1, c.right, c.sig_right)
        R = engine.layered_probe_response(h, E, zero)
        assert R.shape == (E.size, 3, 2) and not np.any(R) and not np.any(np.signbit(R))
        assert engine.layered_probe_response(h, E, None).shape == (E.size, 0, 2)
        plain = engine.layered_gless_int(h, ind, E, w)
        for pr in (zero, None):
            d, u, _ = engine.layered_gless_int_probes(h, ind, E, w, pr)
            err = rr.rel_err(rl.flat_of(d, u), ent["truth"]["blocks"])
            print(f"{name} {sel} probes {'zero' if pr else 'none'}: err {err:.3g}  bar {rl.bar(ent, 'blocks'):.3g}")
            assert err <= rl.bar(ent, "blocks")
            assert rr.rel_err(rl.flat_of(d, u), rl.flat_of(plain[0], plain[1])) <= 2 * rl.bar(ent, "blocks")
    finally:
        engine.layered_free(h)


def test_occupations_fall_along_a_dephased_chain(engine):
    """(I4) a uniform chain cut into layers of 4 with equal probes: with f = (1, 0) the probes' occupations fall monotonically
    from the source side to the drain side.  One probe per layer at gamma = 0.2, and one per site at gamma = 2: site by site
    the profile is monotone only once the phase-breaking length 2 |t| sin(k) / gamma is no more than a site (below that the
    float64 restatement shows the coherent oscillation between neighbouring sites as well); a layer's probe averages over it."""
    N = 24
    F = -1.0 * (np.eye(N, k=1) + np.eye(N, k=-1))
    ls = LayeredSystem.from_dense(F, np.eye(N), [4] * (N // 4))
    leads = [Lead.const([0], [[-0.5j]]), Lead.const([N - 1], [[-0.5j]])]
    E = np.array([-0.5, 0.0, 0.3])
    for groups, gamma in ([list(range(i, i + 4)) for i in range(0, N, 4)], 0.2), ([[i] for i in range(N)], 2.0):
        probes = dephasing_probes_layered(ls, groups, gamma)
        f = calculate_probe_occupations_layered(ls, leads, E, probes, [1.0, 0.0], engine=engine)
        R = calculate_probe_response_layered(ls, leads, E, probes, engine=engine)
        assert f.shape == (3, len(groups)) and np.array_equal(f, R[:, :, 0])
        assert np.all(np.diff(f, axis=1) < 0) and np.all(f > 0) and np.all(f < 1), (gamma, f)
        assert np.abs(R.sum(axis=2) - 1).max() <= 1e-12
    # the front ends of the sums are the engine's calls
    d, u, l = GrLessIntProbesLayered(ls, leads, E, np.ones(3), probes, ind=0, engine=engine)
    g = GrIntProbesLayered(ls, leads, E, np.ones(3), probes, engine=engine)
    assert len(d) == 6 and len(u) == 5 and len(l) == 5 and len(g[0]) == 6
    assert all(np.all(np.isfinite(x)) for x in d + u + l)


# --------------------------------------------------------------------------- exactness
def _same(a, b):
    return (np.array_equal(a["R"], b["R"]) and np.array_equal(a["G"], b["G"]) and
            all(np.array_equal(a["A"][s], b["A"][s]) for s in a["A"]))


@pytest.mark.parametrize("name", ["b", "c"])
def test_runs_and_batches_do_not_change_a_bit(engine, gpu_table, name):
    c = case(name)
    assert _same(gpu_results(engine, c), gpu_table[name])
    for nb in (1, 3):
        engine.set_batch(nb)
        try:
            assert _same(gpu_results(engine, c), gpu_table[name]), nb
        finally:
            engine.set_batch(0)


def test_permuted_probes_permute_the_rows_bit_for_bit(engine, gpu_table):
    c = case("b")                                                       # its probes on layer 1 overlap
    pr = probes_of(c)
    p = np.array([2, 0, 3, 1])
    got = gpu_results(engine, c, probes=[pr[k] for k in p])
    ref = gpu_table["b"]
    assert np.array_equal(got["R"], ref["R"][:, p])
    assert np.array_equal(got["G"], ref["G"]) and all(np.array_equal(got["A"][s], ref["A"][s]) for s in ref["A"])


def test_permuted_energies_permute_the_response(engine, gpu_table):
    c = case("d")
    p = np.array([2, 0, 3, 1])
    h = bind(engine, c)
    try:
        R = engine.layered_probe_response(h, np.asarray(c.energies)[p], probes_of(c))
    finally:
        engine.layered_free(h)
    assert np.array_equal(R, gpu_table["d"]["R"][p])


def test_device_resident_forms(engine, gpu_table):
    """grid, weights and results in HBM (buffers through the HIP runtime the library itself is linked against): bitwise
    the host-pointer forms; a null result is refused"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    c = case("b")
    E = np.ascontiguousarray(c.energies, dtype=np.complex128)
    w = np.ascontiguousarray(rd.weights(c), dtype=np.complex128)
    pr = probes_of(c)
    h = bind(engine, c)
    npat = engine.layered_pattern_size(h)
    R = np.full((E.size, len(pr), c.n_t), np.nan)
    out = np.full(npat, np.nan + 0j)
    dE, dw, dR, dout = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    for ptr, nbytes in ((dE, E.nbytes), (dw, w.nbytes), (dR, R.nbytes), (dout, out.nbytes)):
        assert hip.hipMalloc(C.byref(ptr), nbytes) == 0
    try:
        assert hip.hipMemcpy(dE, E.ctypes.data_as(C.c_void_p), E.nbytes, 1) == 0            # host -> device
        assert hip.hipMemcpy(dw, w.ctypes.data_as(C.c_void_p), w.nbytes, 1) == 0
        assert hip.hipMemcpy(dR, R.ctypes.data_as(C.c_void_p), R.nbytes, 1) == 0
        engine.layered_probe_response_dev(h, E.size, dE.value, dR.value, pr)
        engine.sync()
        assert hip.hipMemcpy(R.ctypes.data_as(C.c_void_p), dR, R.nbytes, 2) == 0            # device -> host
        assert np.array_equal(R, gpu_table["b"]["R"])
        for key in (1, None, "G"):
            assert hip.hipMemcpy(dout, out.ctypes.data_as(C.c_void_p), out.nbytes, 1) == 0  # NaN: the call overwrites it
            if key == "G":
                engine.layered_gr_int_probes_dev(h, E.size, dE.value, dw.value, dout.value, pr)
            else:
                engine.layered_gless_int_probes_dev(h, key, E.size, dE.value, dw.value, dout.value, pr)
            engine.sync()
            got = np.empty_like(out)
            assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), dout, out.nbytes, 2) == 0
            assert np.array_equal(got, gpu_table["b"]["G"] if key == "G" else gpu_table["b"]["A"][key]), key
        with pytest.raises(ValueError):
            engine.layered_gless_int_probes_dev(h, 0, E.size, dE.value, dw.value, None, pr)
        with pytest.raises(ValueError):
            engine.layered_gr_int_probes_dev(h, E.size, dE.value, dw.value, None, pr)
        with pytest.raises(ValueError):
            engine.layered_probe_response_dev(h, E.size, dE.value, None, pr)
    finally:
        engine.layered_free(h)
        for ptr in (dE, dw, dR, dout):
            hip.hipFree(ptr)


# --------------------------------------------------------------------------- undefined occupations
def test_a_singular_layer_gives_a_nan_response_for_that_energy_only(engine):
    """the system of test_a_singular_layer_gives_a_nan_matrix_for_that_energy_only: NaN R at that energy only, its info, a warning"""
    c = rr.cases()[0]
    Fd = [c.F_diag[0], np.zeros_like(c.F_diag[1])]
    Sd = [c.S_diag[0], np.eye(c.sizes[1])]
    Fu = [np.zeros_like(c.F_up[0])]
    probes = [([1, 2], np.array([[-0.2j, 0.01], [0.01, -0.3j]])), ([3, 4], np.array([[-0.1j, 0.0], [0.0, -0.1j]]))]
    h = engine.layered_create(Fd, Fu, Sd, Fu)
    try:
        engine.layered_terminal_const(h, 0, c.left, c.sig_left)
        E = np.array([0.3, 0.0, -0.2])
        with pytest.warns(RuntimeWarning, match="singular"):
            R = engine.layered_probe_response(h, E, probes)
        info = engine.last_info.copy()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            good = engine.layered_probe_response(h, E[[0, 2]], probes)
    finally:
        engine.layered_free(h)
    assert info[0] == 0 and info[2] == 0 and info[1] > c.sizes[0]
    assert np.all(np.isnan(R[1])) and np.array_equal(R[[0, 2]], good) and np.all(np.isfinite(good))


def _five(cluster=None, lone=None):
    """three layers of 5 orbitals, S = 1, a chain with nearest-neighbour hopping -1/2 through all 15 sites and wide-band
    end terminals; `cluster` (two orbitals of layer 1) couple to each other with hopping 1 and to nothing else, `lone` (one
    orbital of layer 1) to nothing at all.  The chain is closed around the orbitals taken out."""
    N = 15
    out_ = sorted((cluster or []) + ([lone] if lone is not None else []))
    path = [i for i in range(N) if i not in out_]
    F = np.zeros((N, N))
    for a, b in zip(path[:-1], path[1:]):
        F[a, b] = F[b, a] = -0.5
    if cluster:
        F[cluster[0], cluster[1]] = F[cluster[1], cluster[0]] = 1.0
    return F, np.eye(N)


def test_a_cluster_that_sees_only_itself_has_no_occupations(engine):
    """orbitals 7 and 8 of the interior layer couple to each other and to nothing else, a one-orbital probe on each: W is
    singular.  R is NaN for the whole energy, info stays 0, the contact's sum is NaN, the total (no solve) is finite.
    (E = 0 with Sigma_p = -i: E S - F - Sigma on the cluster is [[i, -1], [-1, i]], whose inverse the elimination forms in
    exact arithmetic, so that T_78 = T_87 bit for bit and the second pivot of W is an exact zero.)"""
    F, S = _five(cluster=[7, 8])
    ls = LayeredSystem.from_dense(F, S, [5, 5, 5])
    leads = [Lead.const([0], [[-0.5j]]), Lead.const([14], [[-0.5j]])]
    probes = [([7], np.array([[-1.0j]])), ([8], np.array([[-1.0j]])), ([3], np.array([[-0.1j]]))]
    E = np.array([0.0])
    with pytest.warns(RuntimeWarning, match="without a path"):
        R = calculate_probe_response_layered(ls, leads, E, probes, engine=engine)
    assert not np.any(engine.last_info)
    assert np.all(np.isnan(R))
    d, u, l = GrLessIntProbesLayered(ls, leads, E, np.ones(1), probes, ind=0, engine=engine)
    assert not np.any(engine.last_info)
    assert any(np.isnan(x).any() for x in d)
    tot = GrLessIntProbesLayered(ls, leads, E, np.ones(1), probes, ind=None, engine=engine)
    assert all(np.all(np.isfinite(x)) for kind in tot for x in kind)


def test_a_decoupled_orbital_with_a_probe_has_a_zero_row(engine):
    """orbital 7 couples to nothing: W_pp = 0, its row of R is exact zeros, the other rows are the dense engine's"""
    F, S = _five(lone=7)
    ls = LayeredSystem.from_dense(F, S, [5, 5, 5])
    leads = [Lead.const([0], [[-0.5j]]), Lead.const([14], [[-0.5j]])]
    probes = [([7], np.array([[-0.3j]])), ([3], np.array([[-0.1j]])), ([6, 8], np.array([[-0.2j, 0.0], [0.0, -0.1j]]))]
    E = np.array([-0.3, 0.2])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        R = calculate_probe_response_layered(ls, leads, E, probes, engine=engine)
    assert not np.any(R[:, 0]) and not np.any(np.signbit(R[:, 0]))
    assert np.abs(R[:, 1:].sum(axis=2) - 1).max() <= 1e-12
    engine.set_system(F, S)
    sl = np.zeros((15, 15), complex); sl[0, 0] = -0.5j
    sr = np.zeros((15, 15), complex); sr[14, 14] = -0.5j
    hd = engine.sigma_const([sl, sr])
    try:
        Rd = engine.probe_response(hd, E, probes)
    finally:
        engine.sigma_free(hd)
    assert not np.any(Rd[:, 0]) and rd.rel_err(R, Rd) <= rd.PROJECT_BAR


# --------------------------------------------------------------------------- refusals, workspace
def test_refusals(engine):
    c = case("b")
    E = np.asarray(c.energies)
    w = rd.weights(c)
    o = c.offsets
    h = bind(engine, c)
    bare = engine.layered_create(c.base.F_diag, c.base.F_up, c.base.S_diag, c.base.S_up)
    calls = (lambda hh, pr: engine.layered_probe_response(hh, E, pr), lambda hh, pr: engine.layered_gless_int_probes(hh, 0, E, w, pr),
             lambda hh, pr: engine.layered_gr_int_probes(hh, E, w, pr))
    engine.profile(True)
    engine.profile_reset()
    try:
        for call in calls:
            with pytest.raises(ValueError):
                call(h, [([o[1] - 1, o[1]], np.zeros((2, 2)))])                                  # spans layers 0 and 1
            with pytest.raises(ValueError):
                call(h, [([4, 4], np.zeros((2, 2)))])                                            # named twice
            with pytest.raises(ValueError):
                call(17, probes_of(c))                                                           # no such system
        for bad in (3, -4, 7):
            with pytest.raises(ValueError):
                engine.layered_gless_int_probes(h, bad, E, w, probes_of(c))                      # ind out of range
        with pytest.raises(ValueError):
            engine.layered_gless_int_probes(bare, None, E, w, probes_of(c))                      # the total of no terminal at all
        with pytest.raises(ValueError):
            engine.layered_gless_int_probes(bare, 0, E, w, probes_of(c))
        for fam in ("rgf", "inverse", "zgemm", "tmat", "deph", "accumulate"):
            assert engine.profile_read(fam)[1] == 0, fam
        engine.layered_gless_int_probes(h, 0, E, w, probes_of(c))
        for fam in ("rgf", "inverse", "zgemm", "tmat", "deph", "accumulate"):
            assert engine.profile_read(fam)[1] > 0, fam
    finally:
        engine.profile(False)
        engine.layered_free(h)
        engine.layered_free(bare)


def test_workspace_is_the_documented_count(engine):
    c = case("d")
    E = np.asarray(c.energies)
    w = rd.weights(c)
    L, nmax, Ktot = len(c.sizes), max(c.sizes), c.N                     # a probe on every orbital: K_tot = N, J_q = layer q
    C, P, nt = len(c.terms), len(c.probes), c.n_t
    batch = E.size                                                      # the automatic batch holds the whole grid
    static = sum(t[1].size ** 2 for t in c.terms)                       # Gamma of the probes and the const terminals
    Dtot = sum(n * n for n in c.sizes)
    h = bind(engine, c)
    try:
        engine.layered_gless_int_probes(h, 0, E, w, probes_of(c))
        contact = engine.layered_workspace_bytes(h)
        engine.layered_gless_int_probes(h, None, E, w, probes_of(c))
        total = engine.layered_workspace_bytes(h)
        engine.layered_probe_response(h, E, probes_of(c))
        resp = engine.layered_workspace_bytes(h)
        engine.layered_gr_int_probes(h, E, w, probes_of(c))
        gr = engine.layered_workspace_bytes(h)
    finally:
        engine.layered_free(h)
    # per energy: 10 + L layer matrices, the kept strips and Y of all layers, D; no Gamma that depends on E, no pair on the
    # matrix-core path; T and R when a contact is selected
    per = (10 + L) * nmax ** 2 + 2 * L * nmax * Ktot + Dtot
    assert total == 16 * (batch * per + static)
    assert contact == total + 8 * batch * (C * C + P * nt)
    assert resp == 16 * (batch * ((10 + L) * nmax ** 2 + 2 * nmax * Ktot) + static) + 8 * batch * C * C
    assert gr == 16 * (batch * (10 + L) * nmax ** 2 + static)
