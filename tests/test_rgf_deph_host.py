"""Floating dephasing probes of a layered device on the CPU: the calibration of the accuracy bar, the kept-strips recursion
of rgf_deph_ref.py against the dense form and the truth, planted defects, and the host-side front ends."""
import numpy as np
import pytest

import rgf_deph_ref as rd
from gaunegf_amd.layered import LayeredSystem, Lead


def test_calibration():
    """R = the worst ratio between the errors of the two float64 forms (the strips recursion, the dense form) against the
    truth over cases x energies x (the response, every end terminal's G D_s G^H, the total), each error floored at 2^-52;
    C_RDEPH is the smallest power of two >= 2 R, written into rgf_deph_ref.py with R."""
    R = 1.0
    for ent in rd.truth_table():
        for k in ["R"] + rd.selections(ent["case"]):
            a, b = ent["err_strips"][k], ent["err_dense"][k]
            print(f"{ent['tag']:22s} {str(k):5s} strips {a:.3g} dense {b:.3g}")
            R = max(R, a / b, b / a)
    C = 2.0 ** np.ceil(np.log2(2 * R))
    print(f"R = {R:.3f} -> C_RDEPH = {C:g}")
    assert rd.C_RDEPH == C, f"rgf_deph_ref.C_RDEPH = {rd.C_RDEPH} but the measured R = {R:.3f} asks for {C:g}"
    # (R moves with the host's BLAS -- 2.68 and 3.05 on two hosts, rgf_deph_ref.py -- inside the interval that gives C)
    assert abs(rd.R_MEASURED - R) <= 0.2 * R, f"rgf_deph_ref.R_MEASURED = {rd.R_MEASURED}, measured {R:.3f}"


def test_the_inputs_are_what_the_bars_assume():
    """every probe floats (is in P'), the rows of R sum to one and R stays away from 0 and 1, at every case and energy"""
    import dephase_ref as dr
    import rgf_tmat_ref as rt
    for c, E in [(c, E) for c in rd.cases() for E in c.energies]:
        tag = f"{c.name} E={E:.6g}"
        R = dr.response(rt.dense(c, E), c.n_t)
        assert np.isfinite(R).all() and (R.sum(axis=1) > 0).all(), tag
        # (the rounding of a solve with at most 32 unknowns: 2.3e-15 and 2.6e-15 on two hosts' BLAS)
        assert np.abs(R.sum(axis=1) - 1).max() <= 1e-13, tag
        assert 0.06 <= R.min() and R.max() <= 0.87, (tag, R.min(), R.max())


def test_the_strips_restatement_is_the_dense_form_on_the_pattern():
    for ent in rd.truth_table():
        c = ent["case"]
        for form in ("strips", "dense"):
            for k, e in ent["err_" + form].items():
                assert e <= rd.PROJECT_BAR, (ent["tag"], form, k)
        assert rd.rel_err(ent["strips"]["R"], ent["dense"]["R"]) <= rd.PROJECT_BAR, ent["tag"]
        assert rd.rel_err(ent["strips"]["G"], ent["dense"]["G"]) <= rd.PROJECT_BAR, ent["tag"]
        for s in rd.selections(c):
            assert rd.rel_err(ent["strips"]["A"][s], ent["dense"]["A"][s]) <= rd.PROJECT_BAR, (ent["tag"], s)


@pytest.mark.parametrize("defect", rd.DEFECTS)
def test_planted_defects_miss_the_bar_by_orders_of_magnitude(defect):
    """the reversed pass's columns dropped, R_ps taken for the wrong s, Gamma_s left out of D_s, A_{i,i+1} formed with
    Cfull_i on both sides: each misses the calibrated bar of every end terminal's G D_s G^H by the factor printed"""
    for c in rd.cases():
        ent = next(e for e in rd.entries(c) if e["E"] == c.energies[1])
        x = rd.strips(c, ent["E"], defect=defect)
        for s in range(c.n_t):
            bar = rd.C_RDEPH * max(ent["err_strips"][s], ent["err_dense"][s])
            factor = rd.rel_err(x["A"][s], ent["truth"]["A"][s]) / bar
            print(f"{defect:12s} case {c.name} s = {s}: misses the bar {bar:.3g} by a factor {factor:.3g}")
            assert factor >= 100, (defect, c.name, s)


def _system(c):
    b = c.base
    return LayeredSystem(b.F_diag, b.F_up, b.S_diag, b.S_up)


def test_the_front_ends_exist_and_refuse_what_the_module_refuses():
    import gaunegf_amd.layered as ly
    c = rd.cases()[0]
    ls = _system(c)
    o = c.offsets
    leads = [Lead.const(o[lay] + idx, blk) for lay, idx, blk in c.leads]
    probes = c.global_terms(c.probes)
    E, w = np.array(c.energies[:2]), np.ones(2)
    calls = {
        "calculate_probe_response_layered": lambda **kw: ly.calculate_probe_response_layered(ls, leads, E, probes, **kw),
        "calculate_probe_occupations_layered": lambda **kw: ly.calculate_probe_occupations_layered(ls, leads, E, probes, [1.0, 0.0], **kw),
        "GrLessIntProbesLayered": lambda **kw: ly.GrLessIntProbesLayered(ls, leads, E, w, probes, ind=0, **kw),
        "GrIntProbesLayered": lambda **kw: ly.GrIntProbesLayered(ls, leads, E, w, probes, **kw),
    }
    for name, call in calls.items():
        assert callable(getattr(ly, name))
        with pytest.raises(NotImplementedError, match="spin='r' only"):
            call(spin='u')
        with pytest.raises(NotImplementedError, match="checkpoint"):
            call(checkpoint_file="deph.ckpt")


def test_the_entry_points_are_bound():
    from gaunegf_amd import _lib
    from gaunegf_amd.engine import Engine
    for layered, dense in (("negf_layered_probe_response", "negf_probe_response"),
                           ("negf_layered_gless_int_probes", "negf_gless_int_probes"),
                           ("negf_layered_gr_int_probes", "negf_gr_int_probes")):
        for name in (layered, layered + "_dev"):
            assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        # the device form takes the host form's arguments without `info`; both take the dense call's behind the handle
        assert _lib.SIGNATURES[layered][1][:-1] == _lib.SIGNATURES[layered + "_dev"][1]
        assert _lib.SIGNATURES[layered] == _lib.SIGNATURES[dense]
    for fn in ("layered_probe_response", "layered_gless_int_probes", "layered_gr_int_probes"):
        assert callable(getattr(Engine, fn)) and callable(getattr(Engine, fn + "_dev"))
