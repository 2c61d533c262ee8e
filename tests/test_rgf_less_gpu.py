"""G Gamma G^H on the pattern of S for layered devices on the MI355X (negf_layered_gless_int, negf_layered_contact_dos,
GrLessIntLayered, calculate_contact_pdos_layered) against the extended-precision truth of rgf_less_ref.py, against the
dense engine, and against the layered path itself (identities, exactness, refusals)."""
import warnings

import numpy as np
import pytest

import rgf_less_ref as lr
import rgf_ref as rr
from helpers import chain_lead
from gaunegf_amd.layered import (GrLessIntLayered, Lead, LayeredSystem, calculate_contact_pdos_layered,
                                 calculate_pdos_layered)

pytestmark = pytest.mark.gpu


def bind(eng, c):
    """(handle, left terminal = 0, right terminal = 1) of a case with its const terminals"""
    h = eng.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    tl = eng.layered_terminal_const(h, 0, c.left, c.sig_left)
    tr = eng.layered_terminal_const(h, len(c.sizes) - 1, c.right, c.sig_right)
    assert (tl, tr) == (0, 1)
    return h


def flat(split):
    d, u, l = split
    return np.concatenate([b.ravel() for b in d + u + l])


def gpu_less(eng, c, E, w, ind):
    """dict(blocks, split, rows, tot) of one terminal selection"""
    h = bind(eng, c)
    try:
        split = eng.layered_gless_int(h, ind, E, w)
        tot, rows = eng.layered_contact_dos(h, ind, E)
        return dict(blocks=flat(split), split=split, rows=rows, tot=tot)
    finally:
        eng.layered_free(h)


def dense_handle(eng, c, extra=()):
    """the dense engine's const provider with the left and right contacts and `extra` = [(global orbitals, Sigma block)]"""
    F, S = c.to_dense()
    eng.set_system(F, S)
    sig = []
    for gi, blk in [(c.left_global, c.sig_left), (c.right_global, c.sig_right)] + list(extra):
        s = np.zeros((c.N, c.N), complex); s[np.ix_(gi, gi)] = blk
        sig.append(s)
    return eng.sigma_const(sig)


def pattern(c, M):
    o = c.offsets
    L = len(c.sizes)
    return np.concatenate([M[o[i]:o[i + 1], o[i]:o[i + 1]].ravel() for i in range(L)] +
                          [M[o[i]:o[i + 1], o[i + 1]:o[i + 2]].ravel() for i in range(L - 1)] +
                          [M[o[i + 1]:o[i + 2], o[i]:o[i + 1]].ravel() for i in range(L - 1)])


INPUTS = {tag: (c, E, w) for tag, c, E, w in lr.inputs()}


# --------------------------------------------------------------------------- truth
@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "contour"])
def test_truth(engine, tag):
    """blocks and contact rows within C_LESS times the larger error of the two float64 sweep forms, for the left
    terminal, the right one and both"""
    c, E, w = INPUTS[tag]
    res = []
    for sel in lr.SELECTIONS:
        ent = lr.truth_table()[(tag, sel)]
        got = gpu_less(engine, c, E, w, lr.ind_of(sel))
        for k in lr.KEYS:
            err, bar = rr.rel_err(got[k], ent["truth"][k]), lr.bar(ent, k)
            print(f"{tag:8s} {sel:2s} {k:6s} err {err:.3g}  bar {bar:.3g}  (lr {ent['err_lr'][k]:.3g}, rl {ent['err_rl'][k]:.3g})")
            res.append((sel, k, err, bar))
        assert np.allclose(got["tot"], got["rows"].sum(axis=1), rtol=1e-13, atol=0)
    for sel, k, err, bar in res:
        assert err <= bar, (tag, sel, k, err, bar)


@pytest.mark.parametrize("algo", [1, 2, 3, 4])
def test_truth_on_every_inverse_route(engine, algo):
    """case c (layers on every route of the block inverse) with the route forced"""
    c, E, w = INPUTS["c"]
    ent = lr.truth_table()[("c", "LR")]
    engine.set_inverse_algo(algo)
    try:
        got = gpu_less(engine, c, E, w, None)
    finally:
        engine.set_inverse_algo(0)
    for k in lr.KEYS:
        err, bar = rr.rel_err(got[k], ent["truth"][k]), lr.bar(ent, k)
        print(f"algo {algo} {k:6s} err {err:.3g}  bar {bar:.3g}")
        assert err <= bar, (algo, k)


# --------------------------------------------------------------------------- parity with the dense engine
@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "contour"])
def test_parity_with_the_dense_engine(engine, tag):
    c, E, w = INPUTS[tag]
    hd = dense_handle(engine, c)
    try:
        for ind in (0, 1, None):
            P = engine.gless_int(hd, ind, E, w)
            pd = engine.population(hd, ind, E, rows=True)
            got = gpu_less(engine, c, E, w, ind)
            assert rr.rel_err(got["blocks"], pattern(c, P)) <= rr.PROJECT_BAR, (tag, ind)
            assert rr.rel_err(got["rows"], pd) <= rr.PROJECT_BAR, (tag, ind)
    finally:
        engine.sigma_free(hd)


def test_two_terminals_on_one_end(engine):
    """a second left terminal that shares orbitals with the first: one column set on the union of both lists"""
    c = rr.cases()[1]
    E, w = c.energies, np.array([0.4, 0.7, 1.1, 1.6])
    rng = np.random.default_rng(99)
    idx2 = np.array([1, 3, 4, 6])
    sig2 = rr.tr.sigma_block(4, rng, real=False)
    h = bind(engine, c)
    hd = dense_handle(engine, c, [(idx2, sig2)])
    try:
        assert engine.layered_terminal_const(h, 0, idx2, sig2) == 2
        for ind in (0, 1, 2, -1, -3, None):
            got = flat(engine.layered_gless_int(h, ind, E, w))
            _, rows = engine.layered_contact_dos(h, ind, E)
            assert rr.rel_err(got, pattern(c, engine.gless_int(hd, ind, E, w))) <= rr.PROJECT_BAR, ind
            assert rr.rel_err(rows, engine.population(hd, ind, E, rows=True)) <= rr.PROJECT_BAR, ind
        assert np.array_equal(flat(engine.layered_gless_int(h, -1, E, w)), flat(engine.layered_gless_int(h, 2, E, w)))
    finally:
        engine.layered_free(h)
        engine.sigma_free(hd)


# --------------------------------------------------------------------------- identities inside the layered path
@pytest.mark.parametrize("idx", range(4))
def test_identities(engine, idx):
    c = rr.cases()[idx]
    E, w = c.energies, np.array([0.4, 0.7, 1.1, 1.6])
    tag = c.name
    ent = lr.truth_table()[(tag, "LR")]
    h = bind(engine, c)
    try:
        both = engine.layered_gless_int(h, None, E, w)
        left = engine.layered_gless_int(h, 0, E, w)
        right = engine.layered_gless_int(h, 1, E, w)
        Pd, Pu, Pl = engine.layered_gr_int(h, E, w)
        tot, rows = engine.layered_contact_dos(h, None, E)
        rows_l = engine.layered_contact_dos(h, 0, E)[1]
        rows_r = engine.layered_contact_dos(h, 1, E)[1]
        mtot, mrows = engine.layered_dos(h, E, mulliken=True)
    finally:
        engine.layered_free(h)
    bar = lr.bar(ent, "blocks")
    # real E, real weights: sum_c G Gamma_c G^H = i (P - P^H) on the pattern
    spec = np.concatenate([(1j * (Pd[i] - Pd[i].conj().T)).ravel() for i in range(len(Pd))] +
                          [(1j * (Pu[i] - Pl[i].conj().T)).ravel() for i in range(len(Pu))] +
                          [(1j * (Pl[i] - Pu[i].conj().T)).ravel() for i in range(len(Pu))])
    err = rr.rel_err(flat(both), spec)
    print(f"{tag}: |A - i(P - P^H)| / |A| = {err:.3g}, bar {bar:.3g}")
    assert err <= bar
    # the terminals add up: each side within its bar of the truth
    assert rr.rel_err(flat(left) + flat(right), flat(both)) <= 2 * bar
    assert rr.rel_err(rows_l + rows_r, rows) <= 2 * lr.bar(ent, "rows")
    # real weights: the lower blocks are the conjugate transposes of the upper ones bit for bit
    for res in (both, left, right):
        d, u, l = res
        for i in range(len(u)):
            assert np.array_equal(l[i], u[i].conj().T), (tag, i)
        # the diagonal blocks are Hermitian: A_ii and A_ii^H are both within the bar of the (Hermitian) truth
        assert rr.rel_err(np.concatenate([b.conj().T.ravel() for b in d]), np.concatenate([b.ravel() for b in d])) <= 2 * bar
    # all terminals together carry the whole Mulliken DOS
    if c.real:
        assert rr.rel_err(rows, mrows) <= 2 * lr.bar(ent, "rows"), tag
    assert rr.rel_err(tot, mtot) <= 2 * lr.bar(ent, "rows"), tag


def test_complex_weights_decouple_the_lower_blocks(engine):
    c, E, w = INPUTS["contour"]
    got = gpu_less(engine, c, E, w, None)
    d, u, l = got["split"]
    assert max(np.abs(l[i] - u[i].conj().T).max() for i in range(len(u))) > 1e-3
    # sum_k w_k conj(A_k)^T = conj(sum_k conj(w_k) A_k)^T
    cc = gpu_less(engine, c, E, np.conj(w), None)["split"]
    for i in range(len(u)):
        assert np.array_equal(l[i], cc[1][i].conj().T), i


# --------------------------------------------------------------------------- exactness
def test_batch_energy_order_and_reruns_do_not_change_a_bit(engine):
    runs = {}
    for tag in ("b", "c", "contour"):
        c, E, w = INPUTS[tag]
        runs[tag] = gpu_less(engine, c, E, w, None)
        again = gpu_less(engine, c, E, w, None)
        for k in ("blocks", "rows", "tot"):
            assert np.array_equal(runs[tag][k], again[k]), (tag, k)
    engine.set_batch(1)
    try:
        for tag in runs:
            c, E, w = INPUTS[tag]
            one = gpu_less(engine, c, E, w, None)
            for k in ("blocks", "rows", "tot"):
                assert np.array_equal(runs[tag][k], one[k]), (tag, k)
    finally:
        engine.set_batch(0)
    c, E, w = INPUTS["c"]
    p = np.array([2, 0, 3, 1])
    perm = gpu_less(engine, c, E[p], w[p], 0)
    ref = gpu_less(engine, c, E, w, 0)
    assert np.array_equal(perm["rows"], ref["rows"][p]) and np.array_equal(perm["tot"], ref["tot"][p])


# --------------------------------------------------------------------------- chain terminals
@pytest.mark.parametrize("solver", ["fixed-point", "doubling"])
def test_chain_terminals(engine, solver):
    c = rr.cases()[3]
    E, w = c.energies, np.array([0.4, 0.7, 1.1, 1.6])
    nl = c.sizes[-1]
    il, ir = np.arange(6), np.arange(nl - 6, nl)
    leads = [chain_lead(6, 41), chain_lead(6, 42)]
    eta, conv, rel = 1e-4, 1e-7, 0.1
    h = engine.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    F, S = c.to_dense()
    engine.set_system(F, S)
    hd = None
    try:
        for layer, idx, (a, Sa, b, Sb) in ((0, il, leads[0]), (len(c.sizes) - 1, ir, leads[1])):
            engine.layered_terminal_chain(h, layer, idx, a, Sa, b, Sb, b, Sb, eta, conv, rel, solver=solver)
        glob = [il, c.offsets[-2] + ir]
        hd = engine.sigma_chain1d(glob, *[[leads[0][k], leads[1][k]] for k in range(4)],
                                  [leads[0][2], leads[1][2]], [leads[0][3], leads[1][3]], eta, conv, rel, solver=solver)
        for ind in (0, 1, None):
            got = flat(engine.layered_gless_int(h, ind, E, w))
            want = pattern(c, engine.gless_int(hd, ind, E, w))
            assert np.all(np.isfinite(got)) and np.abs(got).max() > 0
            assert rr.rel_err(got, want) <= rr.PROJECT_BAR, (solver, ind)
    finally:
        engine.layered_free(h)
        if hd is not None:
            engine.sigma_free(hd)


# --------------------------------------------------------------------------- front ends
def test_front_ends(engine):
    c, E, w = INPUTS["b"]
    ls = LayeredSystem(c.F_diag, c.F_up, c.S_diag, c.S_up)
    leads = [Lead.const(c.left_global, c.sig_left), Lead.const(c.right_global, c.sig_right)]
    for ind in (0, 1, None):
        ref = gpu_less(engine, c, E, w, ind)
        assert np.array_equal(flat(GrLessIntLayered(ls, leads, E, w, ind=ind, engine=engine)), ref["blocks"])
        assert np.array_equal(calculate_contact_pdos_layered(ls, leads, E, ind, engine=engine), ref["rows"])
    assert np.array_equal(flat(GrLessIntLayered(ls, leads, E, w, ind=-1, engine=engine)),
                          gpu_less(engine, c, E, w, 1)["blocks"])
    groups = np.repeat(np.arange(len(c.sizes)), c.sizes)
    pg = calculate_contact_pdos_layered(ls, leads, E, 1, groups=groups, engine=engine)
    ref = gpu_less(engine, c, E, w, 1)
    assert pg.shape == (4, len(c.sizes)) and np.allclose(pg.sum(axis=1), ref["tot"], rtol=1e-12, atol=0)
    with pytest.raises(NotImplementedError, match="calculate_contact_pdos_layered"):
        calculate_pdos_layered(ls, leads, E, contact=0, engine=engine)
    with pytest.raises(ValueError):
        GrLessIntLayered(ls, leads, E, w, ind=2, engine=engine)


def test_device_resident_forms(engine):
    """grid and results in HBM (buffers through the HIP runtime the library itself is linked against): bitwise the
    host-pointer forms"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    bufs = []

    def dev_buf(a):
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), a.nbytes) == 0
        assert hip.hipMemcpy(ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0          # host -> device
        bufs.append(ptr)
        return ptr

    def fetch(ptr, shape, dtype):
        res = np.zeros(shape, dtype=dtype)
        assert hip.hipMemcpy(res.ctypes.data_as(C.c_void_p), ptr, res.nbytes, 2) == 0       # device -> host
        return res
    c, E, w = INPUTS["contour"]
    ref = gpu_less(engine, c, E, w, 1)
    E = np.ascontiguousarray(E, dtype=np.complex128)
    w = np.ascontiguousarray(w, dtype=np.complex128)
    h = bind(engine, c)
    try:
        npat = engine.layered_pattern_size(h)
        dE, dw = dev_buf(E), dev_buf(w)
        out = dev_buf(np.full(npat, np.nan, dtype=np.complex128))
        tot, site = dev_buf(np.full(E.size, np.nan)), dev_buf(np.full((E.size, c.N), np.nan))
        engine.layered_gless_int_dev(h, 1, E.size, dE.value, dw.value, out.value)
        engine.layered_contact_dos_dev(h, 1, E.size, dE.value, tot.value, site.value)
        engine.sync()
        assert np.array_equal(fetch(out, npat, np.complex128), ref["blocks"])
        assert np.array_equal(fetch(site, (E.size, c.N), np.float64), ref["rows"])
        assert np.array_equal(fetch(tot, E.size, np.float64), ref["tot"])
        with pytest.raises(ValueError):
            engine.layered_gless_int_dev(h, 2, E.size, dE.value, dw.value, out.value)
    finally:
        engine.layered_free(h)
        for b in bufs:
            hip.hipFree(b)


def test_workspace_counts_the_column_sets(engine):
    c, E, w = INPUTS["d"]
    h = bind(engine, c)
    try:
        engine.layered_gr_int(h, E, w)
        plain = engine.layered_workspace_bytes(h)
        engine.layered_gless_int(h, None, E, w)
        less = engine.layered_workspace_bytes(h)
    finally:
        engine.layered_free(h)
    L, nmax, K = len(c.sizes), max(c.sizes), max(c.left.size, c.right.size)
    cs = nmax * K
    extra = (L + 4) * cs + c.left.size ** 2 + 3 * cs + c.right.size ** 2
    assert less - plain == 16 * extra * E.size


# --------------------------------------------------------------------------- refusals
def test_refusals(engine):
    c = rr.cases()[1]
    E, w = c.energies, np.ones(4)
    L = len(c.sizes)
    bare = engine.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    h = bind(engine, c)
    engine.profile(True)
    engine.profile_reset()
    try:
        for fn in (lambda hh, ind: engine.layered_gless_int(hh, ind, E, w),
                   lambda hh, ind: engine.layered_contact_dos(hh, ind, E)):
            with pytest.raises(ValueError):
                fn(h + 100, 0)                                    # an unknown handle
            with pytest.raises(ValueError):
                fn(h, 2)                                          # two terminals: 2 and -3 are outside
            with pytest.raises(ValueError):
                fn(h, -3)
            with pytest.raises(ValueError):
                fn(bare, None)                                    # TOTAL on a system without terminals
        lib, ctx = engine._lib, engine._ctx
        buf = np.zeros(engine.layered_pattern_size(h), complex)
        Ec, wc = E.astype(complex), w.astype(complex)
        p = lambda a: a.ctypes.data
        assert lib.negf_layered_gless_int(ctx, h, 0, 4, p(Ec), p(wc), None, None) == -1          # null pointers
        assert lib.negf_layered_gless_int(ctx, h, 0, 4, None, p(wc), p(buf), None) == -1
        assert lib.negf_layered_gless_int_dev(ctx, h, 0, 4, p(Ec), None, p(buf)) == -1
        assert lib.negf_layered_contact_dos(ctx, h, 0, 4, p(Ec), None, None, None) == -1
        assert lib.negf_layered_contact_dos_dev(ctx, h, 0, 4, p(Ec), p(buf), None) == -1
        engine.layered_terminal_blocks(h, L - 1, [0], np.full((3, 1, 1), -0.05j))
        with pytest.raises(ValueError):
            engine.layered_gless_int(h, 0, E, w)                                                  # four energies, three blocks
        with pytest.raises(ValueError):
            engine.layered_contact_dos(h, 0, E)
        # nothing was launched by any of them
        for fam in ("rgf", "inverse", "zgemm", "assemble", "accumulate", "gamma"):
            assert engine.profile_read(fam)[1] == 0, fam
        d, u, l = engine.layered_gless_int(h, 0, E[:3], w[:3])                                    # three energies are served
        assert np.all(np.isfinite(flat((d, u, l))))
        for fam in ("rgf", "inverse", "zgemm", "accumulate", "gamma"):
            assert engine.profile_read(fam)[1] > 0, fam
    finally:
        engine.profile(False)
        engine.layered_free(h)
        engine.layered_free(bare)


def test_a_singular_layer_reports_as_gr_int_does(engine):
    """layer 1 decoupled with F_11 = 0, S_11 = 1 at E = 0 and no terminal on it: the zero pivot is named alike"""
    c = rr.cases()[0]
    Fd = [c.F_diag[0], np.zeros_like(c.F_diag[1])]
    Sd = [c.S_diag[0], np.eye(c.sizes[1])]
    Fu = [np.zeros_like(c.F_up[0])]
    h = engine.layered_create(Fd, Fu, Sd, Fu)
    try:
        engine.layered_terminal_const(h, 0, c.left, c.sig_left)
        E, w = np.array([0.3, 0.0]), np.ones(2)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            engine.layered_gr_int(h, E, w)
            info0 = engine.last_info.copy()
            engine.layered_gless_int(h, 0, E, w)
            info1 = engine.last_info.copy()
        assert info0[0] == 0 and info0[1] != 0 and np.array_equal(info0, info1)
    finally:
        engine.layered_free(h)
