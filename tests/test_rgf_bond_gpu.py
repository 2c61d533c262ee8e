"""Bond currents and local transmission on the pattern of S for layered devices on the MI355X
(negf_layered_local_transmission, negf_layered_bond_int, calculate_bond_transmission_layered,
calculate_interlayer_transmission, calculate_bond_currents_layered) against the extended-precision truth of
rgf_bond_ref.py, against the dense engine, and against the layered path itself (conservation, antisymmetry, groups,
exactness, refusals)."""
import warnings

import numpy as np
import pytest

import rgf_bond_ref as br
import rgf_ref as rr
from gaunegf_amd.layered import (Lead, LayeredSystem, calculate_bond_currents_layered, calculate_bond_transmission_layered,
                                 calculate_interlayer_transmission, pattern_to_dense)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
IND = {"L": 0, "R": 1, "LR": None}


def bind(eng, c):
    """handle of a case with its const terminals: left = 0, right = 1"""
    h = eng.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    tl = eng.layered_terminal_const(h, 0, c.left, c.sig_left)
    tr = eng.layered_terminal_const(h, len(c.sizes) - 1, c.right, c.sig_right)
    assert (tl, tr) == (0, 1)
    return h


def flat(split):
    """(diag, upper, lower) of [m, a, b] blocks -> [m, table]; of [a, b] blocks -> [table]"""
    d, u, l = split
    if d[0].ndim == 3:
        return np.concatenate([b.reshape(b.shape[0], -1) for b in d + u + l], axis=1)
    return np.concatenate([b.ravel() for b in d + u + l])


def gpu_flow(eng, c, E, ind, gpl=None, group_of=None):
    h = bind(eng, c)
    try:
        return eng.layered_local_transmission(h, ind, E, gpl, group_of)
    finally:
        eng.layered_free(h)


def gpu_int(eng, c, E, w, ind):
    h = bind(eng, c)
    try:
        return eng.layered_bond_int(h, ind, E, w)
    finally:
        eng.layered_free(h)


def entry(tag, sel):
    return br.tiny_entry(sel) if tag == "tiny" else br.truth_table()[(tag, sel)]


def system_of(c):
    return (LayeredSystem(c.F_diag, c.F_up, c.S_diag, c.S_up),
            [Lead.const(c.left_global, c.sig_left), Lead.const(c.right_global, c.sig_right)])


# --------------------------------------------------------------------------- truth
@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "tiny", "contour"])
def test_orbital_level_flow_against_the_truth(engine, tag):
    """every table of every selection within C_BOND times the larger error of the two float64 sweep forms; the vanishing
    tables (real case, all terminals) within zero_bar.  The contour's complex energies take the formula literally."""
    res = []
    for sel in br.SELECTIONS:
        ent = entry(tag, sel)
        got = flat(gpu_flow(engine, ent["case"], ent["E"], IND[sel]))
        for j in range(len(ent["E"])):
            val, bar = br.check_table(ent, j, got[j])
            print(f"{tag:8s} {sel:2s} E[{j}] {'max|flow|' if ent['zero'] else 'err'} {val:.3g}  bar {bar:.3g}")
            res.append((sel, j, val, bar))
    for sel, j, val, bar in res:
        assert val <= bar, (tag, sel, j, val, bar)


@pytest.mark.parametrize("algo", [1, 2])
def test_both_inverse_families_meet_the_bar(engine, algo):
    """case c with the unblocked and the blocked inverse forced (18 ... 213: both serve every layer)"""
    ent = entry("c", "L")
    engine.set_inverse_algo(algo)
    try:
        got = flat(gpu_flow(engine, ent["case"], ent["E"], 0))
    finally:
        engine.set_inverse_algo(0)
    for j in range(len(ent["E"])):
        val, bar = br.check_table(ent, j, got[j])
        print(f"algo {algo} E[{j}] err {val:.3g} bar {bar:.3g}")
        assert val <= bar, (algo, j)


# --------------------------------------------------------------------------- the dense engine
@pytest.mark.parametrize("tag", ["b", "d"])
def test_against_the_dense_engine(engine, tag):
    """Engine.local_transmission on to_dense(): the pattern entries agree within the sum of the two bars, the dense
    entries outside the pattern are exactly zero"""
    c = {k.name: k for k in rr.cases()}[tag]
    F, S = c.to_dense()
    engine.set_system(F, S)
    sig = []
    for gi, blk in ((c.left_global, c.sig_left), (c.right_global, c.sig_right)):
        s = np.zeros((c.N, c.N), complex); s[np.ix_(gi, gi)] = blk
        sig.append(s)
    hd = engine.sigma_const(sig)
    layer = np.repeat(np.arange(len(c.sizes)), c.sizes)
    outside = np.abs(layer[:, None] - layer[None, :]) > 1
    try:
        for sel in ("L", "R"):
            ent = entry(tag, sel)
            dense = engine.local_transmission(hd, IND[sel], c.energies)
            got = pattern_to_dense(c.sizes, *gpu_flow(engine, c, c.energies, IND[sel]))
            assert np.all(dense[:, outside] == 0.0) and np.all(got[:, outside] == 0.0)
            for j in range(len(c.energies)):
                err = rr.rel_err(got[j], dense[j])
                print(f"{tag} {sel} E[{j}] layered against dense {err:.3g}, bar 2 x {br.bar_single(ent, j):.3g}")
                assert err <= 2 * br.bar_single(ent, j), (tag, sel, j)
    finally:
        engine.sigma_free(hd)


# --------------------------------------------------------------------------- conservation
@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_the_flow_across_every_boundary_is_the_transmission(engine, tag):
    """one injecting terminal: L - 1 equal columns, the transmission into the other end (negative for the right
    terminal), each within the cut bar (the table's bar times sum|flow_u| of the block) plus T's own bar"""
    c = {k.name: k for k in rr.cases()}[tag]
    ls, leads = system_of(c)
    h = bind(engine, c)
    try:
        T_rl = engine.layered_transmission(h, 1, 0, c.energies)       # into the right terminal from the left one
        T_lr = engine.layered_transmission(h, 0, 1, c.energies)
    finally:
        engine.layered_free(h)
    tbar = rr.bar(rr.truth_table()[tag], "T")
    for sel, want in (("L", T_rl), ("R", -T_lr)):
        ent = entry(tag, sel)
        cut = calculate_interlayer_transmission(ls, leads, c.energies, contact=IND[sel], engine=engine)
        assert cut.shape == (len(c.energies), len(c.sizes) - 1)
        for j in range(len(c.energies)):
            tol = br.cut_bar(ent, j) + tbar * abs(want[j])
            print(f"{tag} {sel} E[{j}] T {want[j]:.6g} worst |cut - T| {np.abs(cut[j] - want[j]).max():.3g} tol {tol.min():.3g}")
            assert np.all(np.abs(cut[j] - want[j]) <= tol), (tag, sel, j, cut[j], want[j])


def test_conservation_with_a_second_terminal_on_the_injecting_end(engine):
    """a second const terminal on layer 0: the flow injected by terminal 0 across every boundary is the sum of the
    transmission matrix's entries from terminal 0 into the terminals of the other end.  No truth exists for this system;
    the added terminal is of the size of the others, so case b's relative bar is taken, against the measured sum|flow_u|."""
    c = rr.cases()[1]
    ent = entry("b", "L")
    rng = np.random.default_rng(99)
    idx2 = np.array([1, 3, 4, 6])
    sig2 = rr.tr.sigma_block(4, rng, real=False)
    h = bind(engine, c)
    try:
        assert engine.layered_terminal_const(h, 0, idx2, sig2) == 2
        T = engine.layered_transmission_matrix(h, c.energies)
        d, u, l = engine.layered_local_transmission(h, 0, c.energies)
        one = engine.layered_local_transmission(h, 0, c.energies, np.ones(len(c.sizes), np.int32), np.zeros(c.N, np.int32))
    finally:
        engine.layered_free(h)
    want = T[:, 1, 0]                                                    # terminal 1 is the only one on the last layer
    assert np.abs(T[:, 2, 0]).max() > 1e-3                               # part of the injected current leaves through terminal 2
    for j in range(len(c.energies)):
        for i in range(len(u)):
            tol = br.bar_single(ent, j) * (np.abs(u[i][j]).sum() + abs(want[j]))
            assert abs(one[1][i][j, 0, 0] - want[j]) <= tol, (j, i, one[1][i][j, 0, 0], want[j])


# --------------------------------------------------------------------------- antisymmetry
def flows_and_A(engine, c):
    """the orbital-level flow of the left terminal and A of each energy (layered_gless_int with one-hot weights)"""
    h = bind(engine, c)
    try:
        flow = engine.layered_local_transmission(h, 0, c.energies)
        A = [engine.layered_gless_int(h, 0, c.energies, np.eye(len(c.energies))[j]) for j in range(len(c.energies))]
    finally:
        engine.layered_free(h)
    return flow, A


@pytest.mark.parametrize("tag", ["b", "c"])
def test_antisymmetry_of_the_coupling_blocks_at_real_energies(engine, tag):
    """|flow_l + flow_u^T| <= 4 eps |K| |A| elementwise (the kernels give exact negatives: the lower block's K is the
    stored conjugate and its A the conjugate of the same element)"""
    c = {k.name: k for k in rr.cases()}[tag]
    (d, u, l), A = flows_and_A(engine, c)
    for j, E in enumerate(c.energies):
        _, Ku, _ = br.k_blocks(c, E)
        for i in range(len(u)):
            assert np.all(np.abs(l[i][j] + u[i][j].T) <= 4 * EPS * (np.abs(Ku[i]) * np.abs(A[j][1][i])).T), (tag, j, i)


@pytest.mark.parametrize("tag", ["b", "c"])
def test_antisymmetry_of_the_diagonal_blocks_at_real_energies(engine, tag):
    """|flow_ii + flow_ii^T| <= 4 eps |K| |A| elementwise.  At real E flow_rc + flow_cr = 2 Im[K_rc conj(A_rc - conj(A_cr))],
    so the bound asks for an A_ii that is Hermitian element by element; negf_layered_gless_int's A_ii = (W Gamma) W^H is
    Hermitian to the rounding of its products only (measured: max |A_ii - A_ii^H| = 1.8 (b) and 2.5 (c) eps max|A_ii|, and
    with it a worst ratio to this bound of 1.91 and 69.8).  The bond visitor therefore takes the Hermitian part of A_ii
    before the flow (rgf_bond_hermitize): the diagonal blocks are then antisymmetric bit for bit, like the coupling blocks."""
    c = {k.name: k for k in rr.cases()}[tag]
    (d, u, l), A = flows_and_A(engine, c)
    worst, worst_norm, herm = 0.0, 0.0, 0.0
    for j, E in enumerate(c.energies):
        Kd, _, _ = br.k_blocks(c, E)
        for i in range(len(d)):
            ka = np.abs(Kd[i]) * np.abs(A[j][0][i])
            dev = np.abs(d[i][j] + d[i][j].T)
            worst = max(worst, float((dev / (4 * EPS * np.maximum(ka, ka.T))).max()))
            worst_norm = max(worst_norm, float(dev.max() / (4 * EPS * np.abs(Kd[i]).max() * np.abs(A[j][0][i]).max())))
            herm = max(herm, float(np.abs(A[j][0][i] - A[j][0][i].conj().T).max() / (EPS * np.abs(A[j][0][i]).max())))
    print(f"{tag}: worst |flow_ii + flow_ii^T| / (4 eps |K||A|) elementwise {worst:.3g}, against 4 eps max|K| max|A| "
          f"{worst_norm:.3g}; max |A_ii - A_ii^H| / (eps max|A_ii|) {herm:.3g}")
    assert worst <= 1.0, (tag, worst)


# --------------------------------------------------------------------------- groups
def atom_groups(c, seed):
    """per layer: groups of 1 ... 9 orbitals scattered over the layer, and one empty group at a seeded place"""
    rng = np.random.default_rng(seed)
    gpl, loc = [], []
    for n in c.sizes:
        sizes = []
        while sum(sizes) < n:
            sizes.append(min(int(rng.integers(1, 10)), n - sum(sizes)))
        lab = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
        empty = int(rng.integers(0, len(sizes) + 1))
        lab = lab + (lab >= empty)
        gpl.append(len(sizes) + 1); loc.append(lab)
    return np.array(gpl, np.int32), loc


@pytest.mark.parametrize("tag", ["b", "c", "tiny"])
def test_group_tables(engine, tag):
    ent = entry(tag, "L")
    c, E = ent["case"], ent["E"]
    gpl, loc = atom_groups(c, 17)
    group_of = np.concatenate(loc).astype(np.int32)
    h = bind(engine, c)
    try:
        orb = engine.layered_local_transmission(h, 0, E)
        grp = engine.layered_local_transmission(h, 0, E, gpl, group_of)
        one = engine.layered_local_transmission(h, 0, E, np.ones(len(c.sizes), np.int32), np.zeros(c.N, np.int32))
        # relabelling: the groups of every layer renumbered by a permutation
        rng = np.random.default_rng(3)
        perms = [rng.permutation(g) for g in gpl]
        relabelled = np.concatenate([perms[i][loc[i]] for i in range(len(c.sizes))]).astype(np.int32)
        rel = engine.layered_local_transmission(h, 0, E, gpl, relabelled)
    finally:
        engine.layered_free(h)
    for j in range(len(E)):
        blocks = tuple([b[j] for b in kind] for kind in orb)
        want = br.group_tables(blocks, loc, gpl)
        mag = br.group_tables(tuple([np.abs(b) for b in kind] for kind in blocks), loc, gpl)
        cnt = br.group_tables(tuple([np.ones_like(b) for b in kind] for kind in blocks), loc, gpl)
        for k in range(3):
            for i in range(len(want[k])):
                # two summation orders of cnt terms each: 2 cnt eps sum|flow|
                assert np.all(np.abs(grp[k][i][j] - want[k][i]) <= 2 * cnt[k][i] * EPS * mag[k][i]), (tag, j, k, i)
                tot, amag = blocks[k][i].sum(), np.abs(blocks[k][i]).sum()
                assert abs(one[k][i][j, 0, 0] - tot) <= 2 * blocks[k][i].size * EPS * amag, (tag, j, k, i)
        empty_rows = [np.nonzero(cnt[0][i].diagonal() == 0)[0] for i in range(len(c.sizes))]
        assert all(len(e) == 1 and np.all(grp[0][i][j][e[0]] == 0.0) for i, e in enumerate(empty_rows))
    # table entry [perm[a], perm[b]] of the relabelled call is entry [a, b] of the first, bit for bit
    L = len(c.sizes)
    for i in range(L):
        assert np.array_equal(rel[0][i][:, perms[i][:, None], perms[i][None, :]], grp[0][i]), (tag, i)
    for i in range(L - 1):
        assert np.array_equal(rel[1][i][:, perms[i][:, None], perms[i + 1][None, :]], grp[1][i]), (tag, i)
        assert np.array_equal(rel[2][i][:, perms[i + 1][:, None], perms[i][None, :]], grp[2][i]), (tag, i)


# --------------------------------------------------------------------------- the integral
@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "tiny"])
def test_bond_int(engine, tag):
    for sel in br.SELECTIONS:
        ent = entry(tag, sel)
        c, E, w = ent["case"], ent["E"], ent["w"]
        h = bind(engine, c)
        try:
            per = flat(engine.layered_local_transmission(h, IND[sel], E))
            got = flat(engine.layered_bond_int(h, IND[sel], E, w))
            hot = [flat(engine.layered_bond_int(h, IND[sel], E, np.eye(len(E))[j])) for j in (0, len(E) - 1)]
        finally:
            engine.layered_free(h)
        # sum_k w_k flow(E_k) of the per-energy call, summed here in extended precision: a chain of m products and sums
        want = (w[:, None].astype(np.longdouble) * per.astype(np.longdouble)).sum(axis=0)
        mag = (np.abs(w)[:, None] * np.abs(per)).sum(axis=0)
        assert np.all(np.abs(got - want) <= 4 * EPS * mag), (tag, sel)
        if not ent["zero"]:
            err = rr.rel_err(got, ent["truth"]["int"])
            print(f"{tag} {sel} integral err {err:.3g} bar {br.bar_int(ent):.3g}")
            assert err <= br.bar_int(ent), (tag, sel)
        # one-hot weights reproduce one energy
        assert np.array_equal(hot[0], per[0]) and np.array_equal(hot[1], per[-1]), (tag, sel)


# --------------------------------------------------------------------------- exactness
def test_batch_energy_order_and_reruns_do_not_change_a_bit(engine):
    ent = entry("c", "LR")
    c, w = ent["case"], ent["w"]
    E = np.concatenate([c.energies, c.energies[:3] + 0.05])             # seven energies: batches of 3 cut them 3 | 3 | 1
    w = np.concatenate([w, w[:3]])
    gpl, loc = atom_groups(c, 5)
    group_of = np.concatenate(loc).astype(np.int32)

    def run(E, w):
        h = bind(engine, c)
        try:
            return (flat(engine.layered_local_transmission(h, None, E)),
                    flat(engine.layered_local_transmission(h, 1, E, gpl, group_of)),
                    flat(engine.layered_bond_int(h, 0, E, w)))
        finally:
            engine.layered_free(h)
    ref = run(E, w)
    again = run(E, w)
    assert all(np.array_equal(a, b) for a, b in zip(ref, again))
    for batch in (1, 3):
        engine.set_batch(batch)
        try:
            cut = run(E, w)
        finally:
            engine.set_batch(0)
        assert all(np.array_equal(a, b) for a, b in zip(ref, cut)), batch
    p = np.array([2, 0, 6, 3, 1, 5, 4])
    perm = run(E[p], w[p])
    assert np.array_equal(perm[0], ref[0][p]) and np.array_equal(perm[1], ref[1][p])


def test_device_resident_forms_equal_the_host_forms(engine):
    """grid, weights and results in HBM (buffers through the HIP runtime the library itself is linked against)"""
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

    def fetch(ptr, shape):
        res = np.zeros(shape, dtype=np.float64)
        assert hip.hipMemcpy(res.ctypes.data_as(C.c_void_p), ptr, res.nbytes, 2) == 0       # device -> host
        return res
    ent = entry("contour", "R")
    c, E, w = ent["case"], np.ascontiguousarray(ent["E"], dtype=np.complex128), np.ascontiguousarray(ent["w"])
    gpl, loc = atom_groups(c, 9)
    group_of = np.concatenate(loc).astype(np.int32)
    h = bind(engine, c)
    try:
        npat = engine.layered_pattern_size(h)
        ntab = engine.layered_table_size(tuple(int(g) for g in gpl))
        ref_orb = flat(engine.layered_local_transmission(h, 1, E))
        ref_grp = flat(engine.layered_local_transmission(h, 1, E, gpl, group_of))
        ref_int = flat(engine.layered_bond_int(h, 1, E, w))
        dE, dw = dev_buf(E), dev_buf(w)
        orb, grp = dev_buf(np.full((E.size, npat), np.nan)), dev_buf(np.full((E.size, ntab), np.nan))
        acc = dev_buf(np.full(npat, np.nan))
        engine.layered_local_transmission_dev(h, 1, E.size, dE.value, orb.value)
        engine.layered_local_transmission_dev(h, 1, E.size, dE.value, grp.value, gpl, group_of)
        engine.layered_bond_int_dev(h, 1, E.size, dE.value, dw.value, acc.value)
        engine.sync()
        assert np.array_equal(fetch(orb, (E.size, npat)), ref_orb)
        assert np.array_equal(fetch(grp, (E.size, ntab)), ref_grp)
        assert np.array_equal(fetch(acc, npat), ref_int)
        with pytest.raises(ValueError):
            engine.layered_bond_int_dev(h, 2, E.size, dE.value, dw.value, acc.value)
    finally:
        engine.layered_free(h)
        for b in bufs:
            hip.hipFree(b)


# --------------------------------------------------------------------------- a singular layer
def test_a_singular_layer_gives_a_nan_table_and_its_info(engine):
    """layer 1 decoupled with F_11 = 0, S_11 = 1 at E = 0 and no terminal on it, as test_rgf_less_gpu builds it: a NaN
    table for that energy, info = the whole-system column, NEGF_ESINGULAR (the engine's warning), the other energy untouched"""
    c = rr.cases()[0]
    Fd = [c.F_diag[0], np.zeros_like(c.F_diag[1])]
    Sd = [c.S_diag[0], np.eye(c.sizes[1])]
    Fu = [np.zeros_like(c.F_up[0])]
    h = engine.layered_create(Fd, Fu, Sd, Fu)
    try:
        engine.layered_terminal_const(h, 0, c.left, c.sig_left)
        E = np.array([0.3, 0.0])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            engine.layered_gless_int(h, 0, E, np.ones(2))
            info_less = engine.last_info.copy()
        alone = flat(engine.layered_local_transmission(h, 0, E[:1]))
        for groups in ((None, None), (np.array([2, 2], np.int32), (np.arange(c.N) % 2).astype(np.int32))):
            with pytest.warns(RuntimeWarning, match="singular"):
                got = flat(engine.layered_local_transmission(h, 0, E, *groups))
            info = engine.last_info.copy()
            assert info[0] == 0 and info[1] > c.sizes[0] and np.array_equal(info, info_less)
            assert np.all(np.isnan(got[1])) and np.all(np.isfinite(got[0]))
            if groups[0] is None:
                assert np.array_equal(got[0], alone[0])
        # the return code itself, through the C ABI with the last loop's groups: the buffer holds [2][table of those groups]
        gpl, go = groups
        Ec, buf = E.astype(complex), np.zeros((2, engine.layered_table_size(tuple(int(g) for g in gpl))))
        assert buf.shape == got.shape
        rc = engine._lib.negf_layered_local_transmission(engine._ctx, h, 0, 2, Ec.ctypes.data, gpl.ctypes.data, go.ctypes.data,
                                                         buf.ctypes.data, None)
        assert np.array_equal(buf, got, equal_nan=True)
        from gaunegf_amd import _lib
        assert rc == _lib.NEGF_ESINGULAR
    finally:
        engine.layered_free(h)


# --------------------------------------------------------------------------- refusals
def test_refusals(engine):
    """every NEGF_EINVAL of the header's list, before anything is launched"""
    c = rr.cases()[1]
    E, w = c.energies, np.ones(4)
    L, N = len(c.sizes), c.N
    gpl = np.full(L, 2, np.int32)
    group_of = (np.arange(N) % 2).astype(np.int32)
    bare = engine.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    h = bind(engine, c)
    engine.profile(True)
    engine.profile_reset()
    try:
        for fn in (lambda hh, ind: engine.layered_local_transmission(hh, ind, E),
                   lambda hh, ind: engine.layered_local_transmission(hh, ind, E, gpl, group_of),
                   lambda hh, ind: engine.layered_bond_int(hh, ind, E, w)):
            with pytest.raises(ValueError):
                fn(h + 100, 0)                                    # an unknown handle
            with pytest.raises(ValueError):
                fn(h, 2)                                          # two terminals: 2 and -3 are outside
            with pytest.raises(ValueError):
                fn(h, -3)
            with pytest.raises(ValueError):
                fn(bare, None)                                    # TOTAL on a system without terminals
        bad = group_of.copy(); bad[c.offsets[2] + 1] = 2          # an entry outside its layer's range
        neg = group_of.copy(); neg[0] = -1
        zero = gpl.copy(); zero[1] = 0                            # g_i < 1 (layer 1's orbitals then have no valid group either)
        for a, b in ((gpl, bad), (gpl, neg), (zero, group_of), (gpl, None), (None, group_of)):
            with pytest.raises(ValueError):
                engine.layered_local_transmission(h, 0, E, a, b)
        with pytest.raises(ValueError):
            engine.layered_local_transmission(h, 0, E, gpl[:-1], group_of)           # lengths: refused by the binding
        with pytest.raises(ValueError):
            engine.layered_local_transmission(h, 0, E, gpl, group_of[:-1])
        lib, ctx = engine._lib, engine._ctx
        buf = np.zeros(4 * engine.layered_pattern_size(h))
        Ec = E.astype(complex)
        p = lambda a: a.ctypes.data
        assert lib.negf_layered_local_transmission(ctx, h, 0, 4, None, None, None, p(buf), None) == -1       # null pointers
        assert lib.negf_layered_local_transmission(ctx, h, 0, 4, p(Ec), None, None, None, None) == -1
        assert lib.negf_layered_local_transmission_dev(ctx, h, 0, 4, p(Ec), None, None, None) == -1
        assert lib.negf_layered_bond_int(ctx, h, 0, 4, p(Ec), None, p(buf), None) == -1
        assert lib.negf_layered_bond_int(ctx, h, 0, 4, p(Ec), p(w), None, None) == -1
        assert lib.negf_layered_bond_int_dev(ctx, h, 0, 4, p(Ec), p(w), None) == -1
        engine.layered_terminal_blocks(h, L - 1, [0], np.full((3, 1, 1), -0.05j))
        with pytest.raises(ValueError):
            engine.layered_local_transmission(h, 0, E)                                # four energies, three blocks
        with pytest.raises(ValueError):
            engine.layered_bond_int(h, 0, E, w)
        # nothing was launched by any of them
        for fam in ("rgf", "inverse", "zgemm", "assemble", "accumulate", "gamma", "bond"):
            assert engine.profile_read(fam)[1] == 0, fam
        got = flat(engine.layered_local_transmission(h, 0, E[:3], gpl, group_of))     # three energies are served
        assert np.all(np.isfinite(got))
        for fam in ("rgf", "inverse", "zgemm", "gamma", "bond"):
            assert engine.profile_read(fam)[1] > 0, fam
        assert engine.profile_read("accumulate")[1] == 0          # the flow pass stands where the accumulate pass stood
    finally:
        engine.profile(False)
        engine.layered_free(h)
        engine.layered_free(bare)


def test_workspace_counts_the_maps_and_the_staging(engine):
    ent = entry("d", "L")
    c, E, w = ent["case"], ent["E"], ent["w"]
    gpl, loc = atom_groups(c, 2)
    group_of = np.concatenate(loc).astype(np.int32)
    h = bind(engine, c)
    try:
        engine.layered_gless_int(h, 0, E, w)
        less = engine.layered_workspace_bytes(h)
        engine.layered_local_transmission(h, 0, E, gpl, group_of)
        grp = engine.layered_workspace_bytes(h)
        engine.layered_bond_int(h, 0, E, w)
        acc = engine.layered_workspace_bytes(h)
        npat = engine.layered_pattern_size(h)
    finally:
        engine.layered_free(h)
    ntab = engine.layered_table_size(tuple(int(g) for g in gpl))
    assert grp - less == 4 * (c.N + int(gpl.sum()) + len(c.sizes)) + 8 * E.size * ntab
    assert acc - less == 8 * npat


# --------------------------------------------------------------------------- front ends
def test_front_ends(engine):
    c = rr.cases()[1]
    ls, leads = system_of(c)
    E = c.energies
    labels = 100 * np.repeat(np.arange(len(c.sizes)), c.sizes) + 7 * (np.arange(c.N) % 3)
    d, u, l, lab = calculate_bond_transmission_layered(ls, leads, E, contact=1, groups=labels, engine=engine)
    assert [list(x) for x in lab] == [[100 * i, 100 * i + 7, 100 * i + 14] for i in range(len(c.sizes))]
    gpl = np.full(len(c.sizes), 3, np.int32)
    group_of = (np.arange(c.N) % 3).astype(np.int32)
    ref = gpu_flow(engine, c, E, 1, gpl, group_of)
    assert np.array_equal(flat((d, u, l)), flat(ref)) and d[0].shape == (4, 3, 3)
    d0, u0, l0, lab0 = calculate_bond_transmission_layered(ls, leads, E, engine=engine)
    assert lab0 is None and np.array_equal(flat((d0, u0, l0)), flat(gpu_flow(engine, c, E, 0)))
    # bond currents: one layered_bond_int call on transport.current_grid's energies with calculate_bond_currents' weights
    from gaunegf_amd import transport as tp
    fermi, qV, T, dE = 0.1, 0.3, 300.0, 0.02
    energies, muL, muR = tp.current_grid(fermi, qV, T, dE)
    wgt = np.zeros(len(energies)); dd = np.diff(energies); wgt[:-1] += dd / 2; wgt[1:] += dd / 2
    wgt = wgt * np.abs(1 / (np.exp((energies - muR) / (tp.kB * T)) + 1) - 1 / (np.exp((energies - muL) / (tp.kB * T)) + 1))
    raw = gpu_int(engine, c, energies, wgt, 0)
    cd, cu, cl, _ = calculate_bond_currents_layered(ls, leads, fermi, qV, T=T, dE=dE, engine=engine)
    assert np.array_equal(flat((cd, cu, cl)), 2 * tp.eoverh * flat(raw))
    gd, gu, gl, glab = calculate_bond_currents_layered(ls, leads, fermi, qV, T=T, dE=dE, groups=labels, engine=engine)
    loc = [group_of[c.offsets[i]:c.offsets[i + 1]] for i in range(len(c.sizes))]
    want = br.group_tables((cd, cu, cl), loc, gpl)
    assert np.allclose(flat((gd, gu, gl)), flat(want), rtol=1e-13, atol=0) and [list(x) for x in glab] == [list(x) for x in lab]
    # every cut carries the current of calculate_current's formula: 2 e/h sum_k w_k T(E_k)
    h = bind(engine, c)
    try:
        Tk = engine.layered_transmission(h, 1, 0, energies)
    finally:
        engine.layered_free(h)
    current = 2 * tp.eoverh * (wgt * Tk).sum()
    for blk in cu:
        assert abs(blk.sum() - current) <= 1e-9 * np.abs(blk).sum()
    zd, zu, zl, _ = calculate_bond_currents_layered(ls, leads, fermi, 0.0, groups=labels, engine=engine)
    assert all(np.all(b == 0) for b in zd + zu + zl) and zd[0].shape == (3, 3) and zl[0].shape == (3, 3)
