"""CPU checks of the references of G Gamma G^H on layered devices (rgf_less_ref.py): calibration of the accuracy bar,
agreement of the restatements, the sum rule against i (G - G^H), and the four entry points in header, ctypes table and
library."""
import os
import re

import numpy as np

import rgf_less_ref as lr
import rgf_ref as rr

ENTRY_POINTS = ("negf_layered_gless_int", "negf_layered_gless_int_dev", "negf_layered_contact_dos",
                "negf_layered_contact_dos_dev")


def test_calibration():
    """R = the worst ratio between the two float64 sweep forms' errors against the truth over all inputs, terminal
    selections and quantities, each input taken whole and energy by energy (each error floored at 2^-52); C_LESS is the
    smallest power of two >= 2 R, written into rgf_less_ref.py with R."""
    tab = lr.truth_table()
    R = 1.0
    for (tag, sel), ent in tab.items():
        for k in lr.KEYS:
            a, b = ent["err_lr"][k], ent["err_rl"][k]
            print(f"{tag:8s} {sel:2s} {k:6s} lr {a:.3g} rl {b:.3g} dense {ent['err_dense'][k]:.3g}")
            R = max(R, a / b, b / a)
        for j, (e_lr, e_rl) in enumerate(zip(ent["err1_lr"], ent["err1_rl"])):
            for k, a, b in zip(lr.KEYS, e_lr, e_rl):
                if max(a / b, b / a) > 4:
                    print(f"{tag:8s} {sel:2s} {k:6s} energy {j}: lr {a:.3g} rl {b:.3g}")
                R = max(R, a / b, b / a)
    C = 2.0 ** np.ceil(np.log2(2 * R))
    print(f"R = {R:.3f} -> C_LESS = {C:g}")
    assert lr.C_LESS == C, f"rgf_less_ref.C_LESS = {lr.C_LESS} but the measured R = {R:.3f} asks for {C:g}"
    assert abs(lr.R_MEASURED - R) <= 0.05 * R, f"rgf_less_ref.R_MEASURED = {lr.R_MEASURED}, measured {R:.3f}"


def test_restatements_agree_within_the_bar():
    """the two sweeps and the dense form: each within the calibrated bar of the truth, and within the project's bar of
    each other"""
    tab = lr.truth_table()
    for key, ent in tab.items():
        for k in lr.KEYS:
            for form in ("lr", "rl", "dense"):
                assert ent["err_" + form][k] <= lr.bar(ent, k), (key, k, form)
            for form in ("lr", "rl"):
                assert rr.rel_err(ent[form][k], ent["dense"][k]) <= lr.PROJECT_BAR, (key, k, form)


def test_inputs_are_meaningful():
    """no quantity is a difference of large numbers: every block list and row table has entries of order one"""
    for key, ent in lr.truth_table().items():
        for k in lr.KEYS:
            t = np.abs(np.asarray(ent["truth"][k]).astype(complex))
            assert 1e-3 < t.max() < 1e3, (key, k, t.max())
    c, E, w = rr.contour()
    assert np.abs(np.imag(w)).max() > 0.1                      # complex weights: the lower blocks are on their own


def test_all_terminals_add_up_to_the_spectral_function():
    """sum_c G Gamma_c G^H = i (G - G^H) on the pattern for real E (an identity of G^-1 - G^-H = -(Sigma - Sigma^H))"""
    for c in rr.cases():
        for E in c.energies:
            for form in (lr.sweep_lr, lr.sweep_rl, lr.dense):
                Ad, Au = form(c, E, "LR")
                Gd, Gu, Gl, _ = rr.dense(c, E)
                want = [1j * (Gd[i] - Gd[i].conj().T) for i in range(len(Gd))] + \
                       [1j * (Gu[i] - Gl[i].conj().T) for i in range(len(Gu))]
                got = np.concatenate([b.ravel() for b in list(Ad) + list(Au)])
                assert rr.rel_err(got, np.concatenate([b.ravel() for b in want])) <= lr.PROJECT_BAR, (c.name, E, form.__name__)
    # and the single terminals add up to both
    ent = lr.truth_table()
    for tag, *_ in lr.inputs():
        for k in lr.KEYS:
            s = ent[(tag, "L")]["truth"][k] + ent[(tag, "R")]["truth"][k]
            assert rr.rel_err(s, ent[(tag, "LR")]["truth"][k]) <= 2.0 ** -50, (tag, k)


def test_rows_are_the_rows_of_the_dense_population():
    """the contact rows computed from the pattern blocks equal (1/2pi) Re sum_j A_ij conj(S_ij) over the whole matrix"""
    c = rr.cases()[1]
    E = c.energies[2]
    G = np.linalg.inv(rr.assembled(c, E))
    W = G[:, c.right_global]
    A = W @ lr.gamma_of(c.sig_right) @ W.conj().T
    S = c.to_dense()[1]
    want = (A * S.conj()).real.sum(axis=1) / (2 * np.pi)
    Ad, Au = lr.dense(c, E, "R")
    assert np.allclose(lr.rows_of(c, Ad, Au, complex), want, rtol=1e-12, atol=1e-15)


def test_the_entry_points_are_declared_bound_and_built():
    from gaunegf_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "negf.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/negf.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    # host and device forms differ by the trailing info pointer only
    for base in ("negf_layered_gless_int", "negf_layered_contact_dos"):
        assert _lib.SIGNATURES[base][1][:-1] == _lib.SIGNATURES[base + "_dev"][1]
