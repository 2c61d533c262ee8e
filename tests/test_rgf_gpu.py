"""The recursive Green's function path of layered devices on the MI355X (negf_layered_*, gaunegf_amd/layered.py) against
the extended-precision truth of rgf_ref.py, against the dense engine, and against itself (exactness, orientation,
refusals)."""
import numpy as np
import pytest

import rgf_ref as rr
from helpers import chain_lead
from gaunegf_amd.layered import (GrIntLayered, Lead, LayeredSystem, calculate_dos_layered, calculate_pdos_layered,
                                 calculate_transmission_layered)

pytestmark = pytest.mark.gpu


def bind(eng, c, left=True, right=True):
    """(handle, left terminal, right terminal) of a case with its const terminals"""
    h = eng.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    tl = eng.layered_terminal_const(h, 0, c.left, c.sig_left) if left else None
    tr = eng.layered_terminal_const(h, len(c.sizes) - 1, c.right, c.sig_right) if right else None
    return h, tl, tr


def gpu_quantities(eng, c, E, w=None):
    h, tl, tr = bind(eng, c)
    try:
        out = dict(T=eng.layered_transmission(h, tr, tl, E))
        out["dos_tot"], out["dos"] = eng.layered_dos(h, E)
        out["pdos_tot"], out["pdos"] = eng.layered_dos(h, E, mulliken=True)
        if w is not None:
            d, u, l = eng.layered_gr_int(h, E, w)
            out["blocks"] = np.concatenate([b.ravel() for b in d + u + l])
            out["split"] = (d, u, l)
        return out
    finally:
        eng.layered_free(h)


def dense_handle(eng, c):
    F, S = c.to_dense()
    eng.set_system(F, S)
    sl = np.zeros((c.N, c.N), complex); sl[np.ix_(c.left_global, c.left_global)] = c.sig_left
    sr = np.zeros((c.N, c.N), complex); sr[np.ix_(c.right_global, c.right_global)] = c.sig_right
    return eng.sigma_const([sl, sr])


def pattern(c, M):
    o = c.offsets
    L = len(c.sizes)
    return np.concatenate([M[o[i]:o[i + 1], o[i]:o[i + 1]].ravel() for i in range(L)] +
                          [M[o[i]:o[i + 1], o[i + 1]:o[i + 2]].ravel() for i in range(L - 1)] +
                          [M[o[i + 1]:o[i + 2], o[i]:o[i + 1]].ravel() for i in range(L - 1)])


# --------------------------------------------------------------------------- truth
@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "contour"])
def test_truth(engine, tag):
    """every quantity within C_RGF times the larger error of the two float64 sweep forms on that input"""
    ent = rr.truth_table()[tag]
    got = gpu_quantities(engine, ent["case"], ent["E"], ent["w"])
    for k in ent["keys"]:
        err, bar = rr.rel_err(got[k], ent["truth"][k]), rr.bar(ent, k)
        print(f"{tag:8s} {k:6s} err {err:.3g}  bar {bar:.3g}  (lr {ent['err_lr'][k]:.3g}, rl {ent['err_rl'][k]:.3g})")
    for k in ent["keys"]:
        assert rr.rel_err(got[k], ent["truth"][k]) <= rr.bar(ent, k), (tag, k)
    if "dos" in ent["keys"]:
        assert np.allclose(got["dos_tot"], got["dos"].sum(axis=1), rtol=1e-13, atol=0)
        assert np.allclose(got["pdos_tot"], got["pdos"].sum(axis=1), rtol=1e-13, atol=0)


# --------------------------------------------------------------------------- parity with the dense engine
@pytest.mark.parametrize("idx", range(4))
def test_parity_with_the_dense_engine(engine, idx):
    c = rr.cases()[idx]
    E = c.energies
    got = gpu_quantities(engine, c, E)
    h = dense_handle(engine, c)
    try:
        T = engine.transmission(h, 1, 0, E)                          # from the left contact (0) into the right one (1)
        tot, site = engine.dos(h, E)
        pd = engine.population(h, engine.RETARDED, E, rows=True)
    finally:
        engine.sigma_free(h)
    assert rr.rel_err(got["T"], T) <= rr.PROJECT_BAR
    assert rr.rel_err(got["dos"], site) <= rr.PROJECT_BAR and rr.rel_err(got["dos_tot"], tot) <= rr.PROJECT_BAR
    assert rr.rel_err(got["pdos"], pd) <= rr.PROJECT_BAR


def test_gr_int_parity_on_the_pattern(engine):
    c, E, w = rr.contour()
    got = gpu_quantities(engine, c, E, w)
    h = dense_handle(engine, c)
    try:
        P = engine.gr_int(h, E, w)
    finally:
        engine.sigma_free(h)
    assert rr.rel_err(got["blocks"], pattern(c, P)) <= rr.PROJECT_BAR
    d, u, l = got["split"]
    assert [b.shape for b in d] == [(n, n) for n in c.sizes]
    assert [b.shape for b in l] == [(b_, a_) for a_, b_ in zip(c.sizes[:-1], c.sizes[1:])]


def test_front_ends_follow_their_dense_namesakes(engine):
    c, E, w = rr.contour()
    ls = LayeredSystem(c.F_diag, c.F_up, c.S_diag, c.S_up)
    leads = [Lead.const(c.left_global, c.sig_left), Lead.const(c.right_global, c.sig_right)]
    Er = c.energies
    ref = gpu_quantities(engine, c, Er)
    T = calculate_transmission_layered(ls, leads, Er, pair=(1, 0), engine=engine)
    assert T.shape == (4,) and np.array_equal(T, ref["T"])
    tot, site = calculate_dos_layered(ls, leads, Er, engine=engine)
    assert site.shape == (4, c.N) and np.array_equal(site, ref["dos"]) and np.array_equal(tot, ref["dos_tot"])
    pd = calculate_pdos_layered(ls, leads, Er, engine=engine)
    assert np.array_equal(pd, ref["pdos"])
    groups = np.repeat(np.arange(len(c.sizes)), c.sizes)
    pg = calculate_pdos_layered(ls, leads, Er, groups=groups, engine=engine)
    assert pg.shape == (4, len(c.sizes)) and np.allclose(pg.sum(axis=1), ref["pdos_tot"], rtol=1e-12, atol=0)
    d, u, l = GrIntLayered(ls, leads, E, w, engine=engine)
    assert np.array_equal(np.concatenate([b.ravel() for b in d + u + l]), gpu_quantities(engine, c, E, w)["blocks"])
    with pytest.raises(NotImplementedError):
        calculate_transmission_layered(ls, leads, Er, spin='u', engine=engine)
    with pytest.raises(NotImplementedError):
        calculate_pdos_layered(ls, leads, Er, contact=0, engine=engine)


# --------------------------------------------------------------------------- chain leads
@pytest.mark.parametrize("solver", ["fixed-point", "doubling"])
def test_chain_leads(engine, solver):
    c = rr.cases()[3]
    E = c.energies
    nl = c.sizes[-1]
    il, ir = np.arange(6), np.arange(nl - 6, nl)
    leads = [chain_lead(6, 41), chain_lead(6, 42)]
    eta, conv, rel = 1e-4, 1e-7, 0.1
    h = engine.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    F, S = c.to_dense()
    engine.set_system(F, S)
    hd = None
    try:
        ts = []
        for layer, idx, (a, Sa, b, Sb) in ((0, il, leads[0]), (len(c.sizes) - 1, ir, leads[1])):
            ts.append(engine.layered_terminal_chain(h, layer, idx, a, Sa, b, Sb, b, Sb, eta, conv, rel, solver=solver))
        T = engine.layered_transmission(h, ts[1], ts[0], E)
        glob = [il, c.offsets[-2] + ir]
        hd = engine.sigma_chain1d(glob, *[[leads[0][k], leads[1][k]] for k in range(4)],
                                  [leads[0][2], leads[1][2]], [leads[0][3], leads[1][3]], eta, conv, rel, solver=solver)
        Td = engine.transmission(hd, 1, 0, E)
        print(solver, T, Td)
        assert np.all(np.isfinite(T)) and T.max() > 0
        assert rr.rel_err(T, Td) <= rr.PROJECT_BAR
        # the terminal's Sigma is bitwise the block the dense provider evaluates
        sig = []
        for k in range(2):
            dense_sig = engine.sigma_eval(hd, k, E, n_contacts=2)
            sig.append(engine.layered_terminal_sigma(h, ts[k], E, 6))
            assert np.array_equal(sig[k], dense_sig[:, glob[k]][:, :, glob[k]])
        # a `blocks` terminal fed with that Sigma gives the chain terminal's T bit for bit
        hb = engine.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
        try:
            tb = [engine.layered_terminal_blocks(hb, 0, il, sig[0]),
                  engine.layered_terminal_blocks(hb, len(c.sizes) - 1, ir, sig[1])]
            assert np.array_equal(engine.layered_transmission(hb, tb[1], tb[0], E), T)
        finally:
            engine.layered_free(hb)
    finally:
        engine.layered_free(h)
        if hd is not None:
            engine.sigma_free(hd)


# --------------------------------------------------------------------------- exactness
def test_batch_and_energy_order_do_not_change_a_bit(engine):
    c, Ec, w = rr.contour()
    cc = rr.cases()[2]
    ref = gpu_quantities(engine, c, c.energies)
    ref_c = gpu_quantities(engine, cc, cc.energies)
    ref_w = gpu_quantities(engine, c, Ec, w)
    engine.set_batch(1)
    try:
        one = gpu_quantities(engine, c, c.energies)
        one_c = gpu_quantities(engine, cc, cc.energies)
        one_w = gpu_quantities(engine, c, Ec, w)
    finally:
        engine.set_batch(0)
    for k in ("T", "dos", "pdos", "dos_tot", "pdos_tot"):
        assert np.array_equal(ref[k], one[k]), k
        assert np.array_equal(ref_c[k], one_c[k]), k
    assert np.array_equal(ref_w["blocks"], one_w["blocks"])
    p = np.array([2, 0, 3, 1])
    perm = gpu_quantities(engine, cc, cc.energies[p])
    for k in ("T", "dos", "pdos", "dos_tot", "pdos_tot"):
        assert np.array_equal(perm[k], ref_c[k][p]), k


def test_a_cut_wire_transmits_exactly_nothing(engine):
    c = rr.cases()[1]
    cut = object.__new__(rr.RCase)
    cut.__dict__.update(c.__dict__)
    cut.F_up = [c.F_up[0], np.zeros_like(c.F_up[1]), c.F_up[2]]
    cut.S_up = [c.S_up[0], np.zeros_like(c.S_up[1]), c.S_up[2]]
    E = c.energies
    got = gpu_quantities(engine, cut, E)
    assert np.all(got["T"] == 0.0)
    # layers 0 - 1 alone, with the left terminal only
    h = engine.layered_create(c.F_diag[:2], c.F_up[:1], c.S_diag[:2], c.S_up[:1])
    try:
        engine.layered_terminal_const(h, 0, c.left, c.sig_left)
        _, dos = engine.layered_dos(h, E)
        _, pdos = engine.layered_dos(h, E, mulliken=True)
    finally:
        engine.layered_free(h)
    n01 = c.sizes[0] + c.sizes[1]
    assert np.array_equal(got["dos"][:, :n01], dos)
    assert np.array_equal(got["pdos"][:, :n01], pdos)


# --------------------------------------------------------------------------- orientation
@pytest.mark.parametrize("idx", [0, 2])
def test_real_systems_are_reciprocal(engine, idx):
    c = rr.cases()[idx]
    h, tl, tr = bind(engine, c)
    try:
        Tab = engine.layered_transmission(h, tr, tl, c.energies)
        Tba = engine.layered_transmission(h, tl, tr, c.energies)
    finally:
        engine.layered_free(h)
    assert np.max(np.abs(Tab - Tba)) <= 1e-10 * Tab.max()


def test_complex_hermitian_systems_are_not_reciprocal_and_the_mirror_agrees(engine):
    c = rr.cases()[1]
    E = c.energies
    rng = np.random.default_rng(99)
    idx2 = np.array([1, 3, 4, 6])
    sig2 = rr.tr.sigma_block(4, rng, real=False)
    h, tl, tr = bind(engine, c)
    try:
        t2 = engine.layered_terminal_const(h, 0, idx2, sig2)                      # a second left terminal
        Tab = engine.layered_transmission(h, tr, tl, E)
        Tba = engine.layered_transmission(h, tl, tr, E)
        T2 = engine.layered_transmission(h, tr, t2, E)
    finally:
        engine.layered_free(h)
    assert np.max(np.abs(Tab - Tba)) > 1e-4 * Tab.max()
    # against the dense engine's matrix over the three terminals
    F, S = c.to_dense()
    engine.set_system(F, S)
    sig = []
    for gi, blk in ((c.left_global, c.sig_left), (c.right_global, c.sig_right), (idx2, sig2)):
        s = np.zeros((c.N, c.N), complex); s[np.ix_(gi, gi)] = blk
        sig.append(s)
    hd = engine.sigma_const(sig)
    try:
        Tm = engine.transmission_matrix(hd, E)
    finally:
        engine.sigma_free(hd)
    assert rr.rel_err(Tab, Tm[:, 1, 0]) <= rr.PROJECT_BAR and rr.rel_err(Tba, Tm[:, 0, 1]) <= rr.PROJECT_BAR
    assert rr.rel_err(T2, Tm[:, 1, 2]) <= rr.PROJECT_BAR
    # the mirrored device: what flowed from left into right now flows from right into left
    m = c.mirrored()
    hm, ml, mr = bind(engine, m)
    try:
        t2m = engine.layered_terminal_const(hm, len(m.sizes) - 1, idx2, sig2)
        Tm_ab = engine.layered_transmission(hm, ml, mr, E)
        Tm_ba = engine.layered_transmission(hm, mr, ml, E)
        Tm_2 = engine.layered_transmission(hm, ml, t2m, E)
    finally:
        engine.layered_free(hm)
    for x, y in ((Tm_ab, Tab), (Tm_ba, Tba), (Tm_2, T2)):
        assert np.max(np.abs(x - y)) <= 1e-10 * max(Tab.max(), T2.max())


# --------------------------------------------------------------------------- refusals
def test_refusals(engine):
    c = rr.cases()[1]
    L = len(c.sizes)
    with pytest.raises(ValueError):
        engine.layered_create(c.F_diag[:1], [], c.S_diag[:1], [])                 # L = 1
    with pytest.raises(ValueError):
        LayeredSystem(c.F_diag[:1], [], c.S_diag[:1], [])
    h, tl, tr = bind(engine, c)
    engine.profile(True)
    engine.profile_reset()
    try:
        with pytest.raises(ValueError):
            engine.layered_terminal_const(h, 0, [0, c.sizes[0]], np.zeros((2, 2)))      # outside its layer
        with pytest.raises(ValueError):
            engine.layered_terminal_const(h, 0, [1, 1], np.zeros((2, 2)))               # named twice
        with pytest.raises(ValueError):
            engine.layered_terminal_const(h, 1, [0], np.zeros((1, 1)))                  # an interior layer
        t2 = engine.layered_terminal_const(h, 0, [1], np.array([[-0.1j]]))
        with pytest.raises(ValueError):
            engine.layered_transmission(h, tl, t2, c.energies)                          # two terminals of one end
        with pytest.raises(ValueError):
            engine.layered_transmission(h, tl, 7, c.energies)
        tb = engine.layered_terminal_blocks(h, L - 1, [0], np.full((3, 1, 1), -0.05j))
        with pytest.raises(ValueError):
            engine.layered_transmission(h, tr, tl, c.energies)                          # four energies, three blocks
        with pytest.raises(ValueError):
            engine.layered_dos(h, c.energies)
        assert tb == 3
        # nothing was launched by any of them
        for fam in ("rgf", "inverse", "zgemm", "assemble"):
            assert engine.profile_read(fam)[1] == 0, fam
        T = engine.layered_transmission(h, tr, tl, c.energies[:3])                      # three energies are served
        assert np.all(np.isfinite(T)) and engine.profile_read("rgf")[1] > 0
    finally:
        engine.profile(False)
        engine.layered_free(h)
    # the front end refuses a lead on an interior layer and lists that straddle layers
    ls = LayeredSystem(c.F_diag, c.F_up, c.S_diag, c.S_up)
    with pytest.raises(ValueError):
        calculate_transmission_layered(ls, [Lead.const([8], [[-0.1j]]), Lead.const(c.right_global, c.sig_right)],
                                       c.energies, engine=engine)
    with pytest.raises(ValueError):
        calculate_transmission_layered(ls, [Lead.const([6, 7], np.zeros((2, 2))), Lead.const(c.right_global, c.sig_right)],
                                       c.energies, engine=engine)


# --------------------------------------------------------------------------- the dense path is untouched
def test_the_dense_path_is_untouched(engine):
    c = rr.cases()[2]
    E = c.energies
    h = dense_handle(engine, c)
    try:
        T0 = engine.transmission(h, 0, 1, E)
        tot0, site0 = engine.dos(h, E)
        P0 = engine.gr_int(h, E, np.ones(4))
        other = rr.cases()[3]
        got = gpu_quantities(engine, other, other.energies, np.ones(4))
        assert np.all(np.isfinite(got["T"]))
        T1 = engine.transmission(h, 0, 1, E)                        # the same handle, the same resident system
        tot1, site1 = engine.dos(h, E)
        P1 = engine.gr_int(h, E, np.ones(4))
    finally:
        engine.sigma_free(h)
    assert np.array_equal(T0, T1) and np.array_equal(site0, site1) and np.array_equal(tot0, tot1)
    assert np.array_equal(P0, P1)
