"""CPU checks of the references of the local (bond) transmission on layered devices (rgf_bond_ref.py): the float64 forms
against the truth, the flow outside the pattern, conservation and antisymmetry on the truth, the calibration of the
accuracy bar, the four entry points in header and ctypes table, pattern_to_dense and the front end's group validation."""
import os
import re

import numpy as np
import pytest

import rgf_bond_ref as br
import rgf_less_ref as lr
import rgf_ref as rr

ENTRY_POINTS = ("negf_layered_local_transmission", "negf_layered_local_transmission_dev", "negf_layered_bond_int",
                "negf_layered_bond_int_dev")


def entries():
    tab = dict(br.truth_table())
    for sel in br.SELECTIONS:
        tab[("tiny", sel)] = br.tiny_entry(sel)
    return tab


def test_the_float64_forms_meet_the_truth():
    """per energy and for the weighted integral; a vanishing table is held to zero_bar instead"""
    for key, ent in entries().items():
        for form in ("lr", "rl", "dense"):
            for j in range(len(ent["E"])):
                got, bar = br.check_table(ent, j, ent[form]["flow"][j])
                assert got <= bar, (key, form, j, got, bar)
            if not ent["zero"]:
                assert ent["err_" + form] <= br.bar_int(ent), (key, form)
        if not ent["zero"]:
            t = np.abs(np.asarray(ent["truth"]["flow"]).astype(float))
            assert 1e-3 < t.max() < 1e3, (key, t.max())             # flows of order one: the relative error means something
        else:
            assert np.abs(np.asarray(ent["truth"]["flow"]).astype(float)).max() <= 2.0 ** -60 * max(ent["scale"]), key


def test_the_dense_flow_vanishes_outside_the_pattern():
    """flow = 2 Im[K o A^T] of the assembled N x N system: exactly zero wherever S and F are, and the pattern entries are
    the blocks' flow"""
    for c in rr.cases()[:2] + (br.tiny_case(),):
        F, S = c.to_dense()
        layer = np.repeat(np.arange(len(c.sizes)), c.sizes)
        outside = np.abs(layer[:, None] - layer[None, :]) > 1
        for E in c.energies[:2]:
            G = np.linalg.inv(rr.assembled(c, E))
            W = G[:, c.left_global]
            A = W @ lr.gamma_of(c.sig_left) @ W.conj().T
            flow = 2 * ((E * S - F) * A.T).imag
            assert np.all(flow[outside] == 0.0), c.name
            assert len(c.sizes) < 3 or np.abs(A[outside]).max() > 1e-6           # A itself does not vanish there
            Ad, Au = lr._cut(c, A)
            o = c.offsets
            fd, fu, fl = br.flow_blocks(c, E, Ad, Au)
            for i in range(len(c.sizes) - 1):
                # (A is Hermitian to rounding only: the upper block's flow reads conj(A_ij) where the dense form reads A_ji)
                assert np.allclose(fu[i], flow[o[i]:o[i + 1], o[i + 1]:o[i + 2]], rtol=0, atol=1e-12)
                assert np.allclose(fl[i], flow[o[i + 1]:o[i + 2], o[i]:o[i + 1]], rtol=0, atol=1e-12)


def test_conservation_and_antisymmetry_on_the_truth():
    """one injecting terminal, real E: the flow across every one of the L - 1 boundaries is the transmission (its negative
    for the right terminal), and flow_l = -flow_u^T.  The truth's columns are refined to 2^-55; a cut adds n_i n_{i+1}
    terms that cancel, so it is held to 2^-50 sum|flow_u|."""
    for tag in ("a", "b", "c", "d"):
        T = np.asarray(rr.truth_table()[tag]["truth"]["T"]).astype(float)
        for sel, sign in (("L", 1.0), ("R", -1.0)):
            ent = br.truth_table()[(tag, sel)]
            c = ent["case"]
            for j in range(len(ent["E"])):
                flow = ent["truth"]["flow"][j]
                cut, mag = br.cuts(c, flow)
                worst = np.abs(np.asarray(cut).astype(float) - sign * T[j]) / np.asarray(mag).astype(float)
                print(f"{tag} {sel} E[{j}]: T {T[j]:.6g}  worst |cut - T| / sum|flow_u| {worst.max():.3g}")
                assert worst.max() <= 2.0 ** -50, (tag, sel, j)
                d, u, l = br.split(c.sizes, flow)
                for i in range(len(u)):
                    assert np.abs(l[i] + u[i].T).max() <= 2.0 ** -60 * ent["scale"][j], (tag, sel, j, i)
                for i in range(len(d)):
                    assert np.abs(d[i] + d[i].T).max() <= 2.0 ** -55 * ent["scale"][j], (tag, sel, j, i)
    # at a complex energy the lower block is on its own
    ent = br.truth_table()[("contour", "L")]
    d, u, l = br.split(ent["case"].sizes, ent["truth"]["flow"][0])
    assert float(np.abs(l[0] + u[0].T).max()) > 1e-3


def test_calibration():
    """R = the worst ratio between the two float64 sweep forms' errors against the truth over all inputs and terminal
    selections, energy by energy and for the weighted integral (each error floored at 2^-52), without the vanishing tables;
    C_BOND is the smallest power of two >= 2 R, written into rgf_bond_ref.py with R."""
    R, where = 1.0, None
    lo, hi, dlo, dhi = 1.0, 0.0, 1.0, 0.0
    for key, ent in br.truth_table().items():
        if ent["zero"]:
            continue
        pairs = list(zip(ent["err1_lr"], ent["err1_rl"], ent["err1_dense"])) + [(ent["err_lr"], ent["err_rl"], ent["err_dense"])]
        for j, (a, b, d) in enumerate(pairs):
            if max(a / b, b / a) > 4:
                print(f"{key} energy {j if j < len(ent['E']) else 'sum'}: lr {a:.3g} rl {b:.3g} dense {d:.3g}")
            if max(a / b, b / a) > R:
                R, where = max(a / b, b / a), (key, j, a, b)
            lo, hi, dlo, dhi = min(lo, a, b), max(hi, a, b), min(dlo, d), max(dhi, d)
    C = 2.0 ** np.ceil(np.log2(2 * R))
    print(f"R = {R:.3f} at {where} -> C_BOND = {C:g}; sweeps {lo:.3g} ... {hi:.3g}, dense {dlo:.3g} ... {dhi:.3g}")
    assert br.C_BOND == C, f"rgf_bond_ref.C_BOND = {br.C_BOND} but the measured R = {R:.3f} asks for {C:g}"
    assert abs(br.R_MEASURED - R) <= 0.05 * R, f"rgf_bond_ref.R_MEASURED = {br.R_MEASURED}, measured {R:.3f}"


def test_group_tables_and_cuts_of_the_reference():
    """one group per layer: the table's upper entry is the cut; singletons: the table is the flow itself"""
    ent = br.truth_table()[("b", "L")]
    c = ent["case"]
    blocks = br.split(c.sizes, np.asarray(ent["dense"]["flow"][1]))
    one = br.group_tables(blocks, [np.zeros(n, int) for n in c.sizes], [1] * len(c.sizes))
    cut, _ = br.cuts(c, ent["dense"]["flow"][1])
    assert np.allclose([b[0, 0] for b in one[1]], cut, rtol=1e-13, atol=0)
    same = br.group_tables(blocks, [np.arange(n) for n in c.sizes], list(c.sizes))
    assert np.array_equal(br.flat_of(same), br.flat_of(blocks))


def test_the_entry_points_are_declared_and_bound():
    from gaunegf_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "negf.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/negf.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
    # host and device forms differ by the trailing info pointer only
    for base in ("negf_layered_local_transmission", "negf_layered_bond_int"):
        assert _lib.SIGNATURES[base][1][:-1] == _lib.SIGNATURES[base + "_dev"][1]
    assert _lib.SIGNATURES["negf_layered_bond_int"] == _lib.SIGNATURES["negf_bond_int"]


def test_pattern_to_dense_round_trips():
    from gaunegf_amd.layered import pattern_to_dense
    c = rr.cases()[1]
    rng = np.random.default_rng(5)
    M = rng.standard_normal((3, c.N, c.N))
    layer = np.repeat(np.arange(len(c.sizes)), c.sizes)
    M[:, np.abs(layer[:, None] - layer[None, :]) > 1] = 0.0
    o = c.offsets
    L = len(c.sizes)
    d = [M[:, o[i]:o[i + 1], o[i]:o[i + 1]] for i in range(L)]
    u = [M[:, o[i]:o[i + 1], o[i + 1]:o[i + 2]] for i in range(L - 1)]
    l = [M[:, o[i + 1]:o[i + 2], o[i]:o[i + 1]] for i in range(L - 1)]
    assert np.array_equal(pattern_to_dense(c.sizes, d, u, l), M)
    assert np.array_equal(pattern_to_dense(c.sizes, [b[0] for b in d], [b[0] for b in u], [b[0] for b in l]), M[0])
    with pytest.raises(ValueError):
        pattern_to_dense(c.sizes, d, u[:-1], l)


def test_the_front_end_validates_the_group_labels():
    """before anything is bound to an engine: these run without a GPU"""
    import gaunegf_amd.layered as ly
    c = rr.cases()[1]
    ls = ly.LayeredSystem(c.F_diag, c.F_up, c.S_diag, c.S_up)
    leads = [ly.Lead.const(c.left_global, c.sig_left), ly.Lead.const(c.right_global, c.sig_right)]
    good = np.repeat(10 * np.arange(len(c.sizes)), c.sizes) + np.arange(c.N) % 3
    gpl, group_of, labels = ly._layer_groups(ls, good)
    assert list(gpl) == [3] * len(c.sizes) and [list(x) for x in labels] == [[10 * i, 10 * i + 1, 10 * i + 2] for i in range(len(c.sizes))]
    assert np.array_equal(np.concatenate(labels)[np.repeat(np.cumsum([0] + list(gpl[:-1])), c.sizes) + group_of], good)
    spanning = good.copy(); spanning[c.offsets[2]] = good[0]            # layer 2's first orbital takes a label of layer 0
    for fn in (lambda g: ly.calculate_bond_transmission_layered(ls, leads, c.energies, groups=g),
               lambda g: ly.calculate_bond_currents_layered(ls, leads, 0.0, 0.2, groups=g)):
        with pytest.raises(ValueError, match=f"label {good[0]} spans layers 0 and 2"):
            fn(spanning)
        with pytest.raises(ValueError, match="length"):
            fn(good[:-1])
        neg = good.copy(); neg[4] = -1
        with pytest.raises(ValueError, match="non-negative"):
            fn(neg)
    with pytest.raises(NotImplementedError):
        ly.calculate_bond_transmission_layered(ls, leads, c.energies, spin='u')
    # the stubbed names still raise, the second one pointing at the front end that serves it
    with pytest.raises(NotImplementedError):
        ly.calculate_transmission_channels_layered()
    with pytest.raises(NotImplementedError, match="calculate_bond_transmission_layered"):
        ly.calculate_local_transmission_layered()
