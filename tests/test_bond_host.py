"""
Host checks of the yardstick the local (bond) transmission is held to (tests/bond_ref.py), and of the front end's
existence.  Inputs: bond_ref.const_cases() -- n = 24, 60 (complex Hermitian F, S), 130, random overlaps of ~0.02, contacts
of 4 ... 30 orbitals with |Gamma| ~ 0.3 ... 1, four real energies each, one of them 5e-4 above an eigenvalue of (F, S).

  1. the float64 restatement obeys the conservation law (cuts between the contacts sum to the transmission, interior rows
     sum to zero, the table is antisymmetric) a factor >= 100 inside the 1e-8 bar test_bond_gpu.py uses, and is a factor
     >= 100 inside that parity bar against the clongdouble truth -- on the inputs the GPU test uses, so that a bar missed
     there cannot be the inputs' fault;
  2. the two-integral identity: sum_k w_k flow(E_k) from two GrLessInt sums (K is linear in E);
  3. calibration: R = worst ratio between the errors of the two float64 forms against the truth, C_BOND the smallest
     power of two >= 2 R; planted defects (A in complex64, K without E S, A_ij for A_ji, Gamma_total for Gamma_c) miss
     the calibrated bar by >= 10x on every input;
  4. the C ABI and the Python front end exist (fails before the feature).
"""
import functools
import os
import re

import numpy as np
import pytest

import bond_ref as br
import xprec

xprec.require_extended()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("negf_local_transmission", "negf_local_transmission_dev", "negf_bond_int", "negf_bond_int_dev")


@functools.lru_cache(maxsize=None)
def _table():
    """[(case, E, truth, err_a, err_b)] over every (case, energy)."""
    rows = [(c, float(E)) for c in br.const_cases() for E in c.energies]

    def make(row):
        c, E = row
        t = br.flow_truth(c.F, c.S, c.sigmas, E)
        return c, E, t, br.rel_err(br.flow(c.F, c.S, c.sigmas, E), t), br.rel_err(br.flow_alt(c.F, c.S, c.sigmas, E), t)
    return xprec.pmap(make, rows)


def _tag(c, E):
    return f"n={c.n} E={E:.6g}"


def test_restatement_conserves():
    worst = 0.0
    for c in br.const_cases():
        groups = c.atom_groups()
        for E in c.energies:
            fl = br.flow(c.F, c.S, c.sigmas, E)
            T = br.transmission(c.F, c.S, c.sigmas, E)
            for P in c.cuts():
                d, scale = br.cut_defect(fl, T, P)
                worst = max(worst, d / scale)
                assert d <= 1e-10 * scale, (_tag(c, E), d, scale)
            tot = np.abs(fl).sum()
            interior = np.arange(c.nc[0], c.n - c.nc[1])
            assert np.all(np.abs(fl[interior].sum(axis=1)) <= 1e-10 * np.abs(fl[interior]).sum(axis=1).max())
            assert np.abs(fl + fl.T).max() <= 1e-10 * np.abs(fl).max()
            fg = br.group_table(fl, groups)
            for P in c.group_cuts(groups):
                blockPQ = fg[np.ix_(P, ~P)]
                assert abs(blockPQ.sum() - T) <= 1e-10 * max(abs(T), np.abs(fl).sum()), _tag(c, E)
            assert np.abs(np.diag(fg)).max() <= 1e-10 * tot
    print(f"bond restatement: worst cut defect / max(|T|, sum_cut |flow|) {worst:.3g} (allowed 1e-10)")


def test_restatement_is_inside_the_parity_bar():
    worst = max(max(ea, eb) for _, _, _, ea, eb in _table())
    print(f"bond restatement: worst float64 error against the truth {worst:.3g} (allowed {br.PROJECT_BAR / 100:g})")
    for c, E, _, ea, eb in _table():
        assert max(ea, eb) <= br.PROJECT_BAR / 100, (_tag(c, E), ea, eb)


def test_two_integral_identity():
    """sum_k w_k flow(E_k) = 2 Im[S_ij (sum w E A)_ji - F_ij (sum w A)_ji], both sums GrLessInt(ind = 0)."""
    import oracle
    from scipy.special import roots_legendre
    x, w = roots_legendre(40)
    E = 2.0 * x; w = 2.0 * w
    for c in br.const_cases()[:2]:
        prov = xprec.ForeignConst(type("C", (), dict(sigs=c.sigmas, sig_tot=c.sigmas[0] + c.sigmas[1], n=c.n)))
        direct = sum(wk * br.flow(c.F, c.S, c.sigmas, Ek) for Ek, wk in zip(E, w))
        A0 = oracle.GrLessInt(c.F, c.S, prov, E, w, 0)
        A1 = oracle.GrLessInt(c.F, c.S, prov, E, w * E, 0)
        two = 2.0 * np.imag(c.S * A1.T - c.F * A0.T)
        err = np.linalg.norm(direct - two) / np.linalg.norm(direct)
        print(f"two-integral identity n={c.n}: {err:.3g}")
        assert err <= 1e-12, (c.n, err)


def test_calibration():
    r, worst, at = 1.0, 0.0, None
    for c, E, _, ea, eb in _table():
        r = max(r, ea / eb, eb / ea)
        if max(ea, eb) > worst:
            worst, at = max(ea, eb), _tag(c, E)
    c_bond = 2.0 ** np.ceil(np.log2(2.0 * r))
    print(f"bond calibration: R {r:.3g} -> C {c_bond:g} (bond_ref.C_BOND = {br.C_BOND:g}); float64 errors "
          f"{min(min(ea, eb) for *_, ea, eb in _table()):.3g} ... {worst:.3g} (worst at {at})")
    assert c_bond == br.C_BOND, (r, c_bond, br.C_BOND)


def _defect_c64(F, S, sigmas, E):
    G = np.linalg.inv(E * S - F - sum(sigmas)).astype(np.complex64)
    Ac = (G @ br.gamma(sigmas[0]).astype(np.complex64)) @ G.conj().T
    return 2.0 * np.imag((E * S - F) * Ac.astype(complex).T)


def _defect_no_es(F, S, sigmas, E):
    G = np.linalg.inv(E * S - F - sum(sigmas))
    Ac = (G @ br.gamma(sigmas[0])) @ G.conj().T
    return 2.0 * np.imag((-F) * Ac.T)


def _defect_untransposed(F, S, sigmas, E):
    G = np.linalg.inv(E * S - F - sum(sigmas))
    Ac = (G @ br.gamma(sigmas[0])) @ G.conj().T
    return 2.0 * np.imag((E * S - F) * Ac)


def _defect_gamma_total(F, S, sigmas, E):
    G = np.linalg.inv(E * S - F - sum(sigmas))
    Ac = (G @ br.gamma(sigmas[0] + sigmas[1])) @ G.conj().T
    return 2.0 * np.imag((E * S - F) * Ac.T)


DEFECTS = {"a_in_complex64": _defect_c64, "k_without_es": _defect_no_es, "a_ij_for_a_ji": _defect_untransposed,
           "gamma_total": _defect_gamma_total}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_defects_miss_the_bar(name):
    least = np.inf
    for c, E, t, ea, eb in _table():
        bar = br.C_BOND * max(ea, eb)
        ratio = br.rel_err(DEFECTS[name](c.F, c.S, c.sigmas, E), t) / bar
        least = min(least, ratio)
        assert ratio >= 10.0, (_tag(c, E), name, ratio)
    print(f"bond planted defect {name}: least error / calibrated bar {least:.3g}")


def test_abi_and_front_end_exist():
    from gaunegf_amd import _lib, transport
    with open(os.path.join(ROOT, "include", "negf.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/negf.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
    for fn in ("calculate_local_transmission", "calculate_bond_currents", "localTrans", "localTransE"):
        assert callable(getattr(transport, fn, None)), fn
    for m in ("local_transmission", "local_transmission_dev", "bond_int", "bond_int_dev"):
        from gaunegf_amd.engine import Engine
        assert callable(getattr(Engine, m, None)), m


def test_no_cpu_fallback():
    """Without a GPU the front ends raise (there is no CPU fallback); with one this check has nothing to say."""
    from gaunegf_amd import _lib
    from gaunegf_amd.transport import SigmaCalculator, calculate_bond_currents, calculate_local_transmission
    if os.path.exists(_lib.LIB_PATH) and _lib.load().negf_device_count() > 0:
        return
    c = br.const_cases()[0]
    sc = SigmaCalculator(c.sigmas[0], c.sigmas[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        calculate_local_transmission(c.F, c.S, sc, c.energies, groups=c.atom_groups())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        calculate_bond_currents(c.F, c.S, sc, 0.0, 0.2, T=0)
