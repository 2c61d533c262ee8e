"""The transmission matrix of a layered device with probes on any layer, on the CPU: the calibration of the accuracy bar,
the sweep-with-strips recursion of rgf_tmat_ref.py against the dense forms and the truth, planted defects, and the
host-side front ends (dephasing_probes_layered)."""
import numpy as np
import pytest

import rgf_tmat_ref as tm
import tmatrix_ref as tr
from gaunegf_amd import transport
from gaunegf_amd.layered import LayeredSystem, dephasing_probes_layered


def test_calibration():
    """R = the worst ratio between the errors of the recursion run forwards and on the mirrored case against the truth
    over all inputs (each error floored at 2^-52); C_RTM is the smallest power of two >= 2 R, written into
    rgf_tmat_ref.py with R."""
    R = 1.0
    for ent in tm.truth_table():
        a, b = ent["err_fwd"], ent["err_mir"]
        print(f"{ent['tag']:22s} fwd {a:.3g} mirror {b:.3g} dense {ent['err_dense']:.3g}")
        R = max(R, a / b, b / a)
    C = 2.0 ** np.ceil(np.log2(2 * R))
    print(f"R = {R:.3f} -> C_RTM = {C:g}")
    assert tm.C_RTM == C, f"rgf_tmat_ref.C_RTM = {tm.C_RTM} but the measured R = {R:.3f} asks for {C:g}"
    assert abs(tm.R_MEASURED - R) <= 0.05 * R, f"rgf_tmat_ref.R_MEASURED = {tm.R_MEASURED}, measured {R:.3f}"


def test_the_recursion_agrees_with_the_dense_forms():
    for ent in tm.truth_table():
        for form in ("fwd", "mir"):
            assert tm.rel_err(ent[form], ent["dense"]) <= tm.PROJECT_BAR, (ent["tag"], form)
            assert ent["err_" + form] <= tm.PROJECT_BAR, (ent["tag"], form)
        assert ent["err_dense"] <= tm.PROJECT_BAR, ent["tag"]
        c = ent["case"]
        F, S = c.to_dense()
        assert tm.rel_err(tr.tmatrix(F, S, c.global_terms(), ent["E"]), ent["dense"]) <= tm.PROJECT_BAR, ent["tag"]


def test_the_cases_are_what_they_claim():
    a, b, c, d = tm.cases()
    lay = lambda cs: [t[0] for t in cs.probes]
    assert sorted(lay(a)) == [0, 1] and set(a.probes[0][1]) <= set(a.base.left)
    assert 2 not in lay(b) and lay(b).count(1) == 2 and b.n_t == 3
    assert set(b.probes[0][1]) & set(b.probes[1][1])                      # the two probes of layer 1 overlap
    K = sorted(t[1].size for t in c.probes)
    assert K.count(9) == 14 and K.count(1) == 2 and 6 in K and 17 in K and 40 in K and 41 in K
    assert sum(t[1].size for t in d.probes) == d.N and len(d.probes) == 32


def test_conservation_at_real_energies():
    """row sums against column sums (current conservation) at the GPU test's bound, the figure printed"""
    worst = 0.0
    for ent in tm.truth_table():
        if np.imag(ent["E"]) != 0:
            continue
        T = ent["fwd"]
        worst = max(worst, np.abs(T.sum(axis=0) - T.sum(axis=1)).max() / np.abs(T).max())
    print(f"worst |row sum - column sum| / max T = {worst:.3g}")
    assert worst <= 1e-11


def test_effective_transmission_of_the_layered_matrix_is_the_dense_one():
    for ent in tm.truth_table():
        c = ent["case"]
        if np.imag(ent["E"]) != 0:
            continue
        a, b = tr.t_eff(ent["fwd"], c.n_t, d=1, s=0), tr.t_eff(ent["dense"], c.n_t, d=1, s=0)
        assert abs(a - b) <= tm.PROJECT_BAR * abs(b), ent["tag"]
        # and transport.effective_transmission is that formula
        e = transport.effective_transmission(ent["fwd"][None], c.n_t, source=0, drain=1)[0]
        assert abs(e - a) <= 1e-12 * abs(a), ent["tag"]


@pytest.mark.parametrize("defect,names", [("no_probes", "abcd"), ("offset", "abcd"),
                                          # G is symmetric for the real cases a and c: transposition shows on b and d only
                                          ("gba", "bd"), ("mirror_orientation", "bd")])
def test_planted_defects_miss_the_bar_by_orders_of_magnitude(defect, names):
    tab = tm.truth_table()
    for c in tm.cases():
        if c.name not in names:
            continue
        ent = next(e for e in tab if e["case"] is c and e["E"] == c.energies[1])
        err = tm.rel_err(tm.strips(c, ent["E"], defect=defect), ent["truth"])
        print(f"{defect:20s} case {c.name}: err {err:.3g}, bar {tm.bar(ent):.3g}")
        assert err > 1e6 * tm.bar(ent), (defect, c.name)


def _system(c):
    b = c.base
    return LayeredSystem(b.F_diag, b.F_up, b.S_diag, b.S_up)


def test_dephasing_probes_layered_is_dephasing_probes_on_the_dense_overlap():
    c = tm.cases()[1]
    ls = _system(c)
    S = ls.to_dense()[1]
    o = c.offsets
    lists = [o[lay] + idx for lay, idx, _ in c.probes]
    gam = np.array([0.1, 0.2, 0.05, 0.3])
    got = dephasing_probes_layered(ls, lists, gam)
    want = transport.dephasing_probes(S, lists, gam)
    assert len(got) == len(want)
    for (i0, b0), (i1, b1) in zip(got, want):
        assert np.array_equal(i0, i1) and np.array_equal(b0, b1)
    # a label per orbital, one probe per layer, a scalar gamma
    labels = np.repeat(np.arange(len(c.sizes)), c.sizes)
    labels[0] = -1
    got = dephasing_probes_layered(ls, labels, 0.07)
    want = transport.dephasing_probes(S, labels, 0.07)
    for (i0, b0), (i1, b1) in zip(got, want):
        assert np.array_equal(i0, i1) and np.array_equal(b0, b1)


def test_dephasing_probes_layered_refuses_a_group_that_spans_layers():
    c = tm.cases()[1]
    ls = _system(c)
    with pytest.raises(ValueError, match=r"group 1 spans layers 0 and 1"):
        dephasing_probes_layered(ls, [[0, 1], [c.sizes[0] - 1, c.sizes[0]]], 0.1)
    with pytest.raises(ValueError):
        dephasing_probes_layered(ls, [[0, 0]], 0.1)
    with pytest.raises(ValueError):
        dephasing_probes_layered(ls, [[c.N]], 0.1)
    with pytest.raises(ValueError):
        dephasing_probes_layered(ls, [[0], [1]], [0.1, 0.2, 0.3])


def test_the_entry_points_are_bound():
    from gaunegf_amd import _lib
    base = "negf_layered_transmission_matrix"
    for name in (base, base + "_dev"):
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
    # the device form takes the host form's arguments without `info`, and negf_transmission_matrix's behind the handle
    assert _lib.SIGNATURES[base][1][:-1] == _lib.SIGNATURES[base + "_dev"][1]
    assert _lib.SIGNATURES[base] == _lib.SIGNATURES["negf_transmission_matrix"]
    import gaunegf_amd.layered as ly
    for fn in ("calculate_transmission_matrix_layered", "calculate_effective_transmission_layered",
               "calculate_effective_current_layered", "dephasing_probes_layered"):
        assert callable(getattr(ly, fn))
    for fn in (ly.calculate_transmission_channels_layered, ly.calculate_local_transmission_layered):   # the stubs that stay
        with pytest.raises(NotImplementedError):
            fn()
