"""
Host checks of the yardstick the transmission matrix and the dephasing probes are held to (tests/tmatrix_ref.py), and of
the front end's existence.  Inputs: tmatrix_ref.cases() -- n = 24 (four contacts), 40 (complex Hermitian, probes that
overlap, sit on a lead and vanish), 130 (ten probes of 9), 200 (complex Hermitian, K = 17 ... 100) --, four real
energies each, one of them 5e-4 above an eigenvalue of (F, S).

  1. identities of the float64 restatement: row sums = column sums, T >= 0, T = T^T on the real-symmetric cases, T != T^T
     but T_eff[d][s] = T_eff[s][d] on the complex-Hermitian ones, C = 2 without probes = Tr[Gamma_L G Gamma_R G^H],
     gamma = 0 probes drop out, T_eff = T_coherent for gamma = 0;
  2. the Ohmic limit of a uniform chain with one probe per site: 1 / T_eff linear in N;
  3. calibration: R = worst ratio between the errors of the two float64 forms against the truth over every (case, energy);
     C_TM the smallest power of two >= 2 R.  Measured: R = 1.40 (n = 200, E = -1), C_TM = 4; the float64 errors are
     6.4e-17 ... 5.9e-16;
  4. planted defects miss C_TM x (float64 error) by at least 100 x on every input they apply to;
  5. the C ABI, the bindings and the front-end names exist (fails before the feature).
"""
import os
import re

import numpy as np
import pytest

import tmatrix_ref as tr
import xprec

xprec.require_extended()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("negf_transmission_matrix", "negf_transmission_matrix_dev")


_table = tr.truth_table


def test_restatement_identities():
    worst = dict(conservation=0.0, negative=0.0, symmetric=0.0, t_eff=0.0)
    asym = []
    for c in tr.cases():
        for E in c.energies:
            T = tr.tmatrix(c.F, c.S, c.terms, E)
            tmax = np.abs(T).max()
            d = np.abs(T.sum(axis=1) - T.sum(axis=0)).max() / tmax
            worst["conservation"] = max(worst["conservation"], d)
            assert d <= 1e-10, (c.name, E, d)
            worst["negative"] = max(worst["negative"], -T.min() / tmax)
            assert T.min() >= -1e-12 * tmax, (c.name, E, T.min())
            if c.real:
                d = np.abs(T - T.T).max() / tmax
                worst["symmetric"] = max(worst["symmetric"], d)
                assert d <= 1e-10, (c.name, E, d)
            else:
                asym.append(np.abs(T - T.T).max() / tmax)
            if len(c.probes):
                ab, ba = tr.t_eff(T, c.n_c, d=1, s=0), tr.t_eff(T, c.n_c, d=0, s=1)
                d = abs(ab - ba) / max(abs(ab), abs(ba))
                worst["t_eff"] = max(worst["t_eff"], d)
                assert d <= 1e-10, (c.name, E, ab, ba)
    assert min(asym) > 1e-4, asym                          # complex-Hermitian F: T is NOT symmetric
    print("tmatrix restatement: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) +
          f"; asymmetry of the complex-Hermitian cases {min(asym):.3g} ... {max(asym):.3g}")


def test_two_terminals_without_probes_is_the_landauer_trace():
    c = tr.cases()[1]
    terms = c.contacts
    for E in c.energies:
        sig = c.contact_sigmas()
        G = np.linalg.inv(E * c.S - c.F - sig[0] - sig[1])
        gl, gr = (1j * (s - s.conj().T) for s in sig)
        ref = np.real(np.trace(gl @ G @ gr @ G.conj().T))
        for form in (tr.tmatrix, tr.tmatrix_alt):
            T = form(c.F, c.S, terms, E)
            assert T.shape == (2, 2) and abs(T[0, 1] - ref) <= 1e-11 * abs(ref), (E, T[0, 1], ref)


def test_probes_of_zero_strength_drop_out():
    from gaunegf_amd.transport import dephasing_probes, effective_transmission
    c = tr.cases()[2]
    lists = [idx for idx, _ in c.probes]
    zero = dephasing_probes(c.S, lists, 0.0)
    assert all(np.array_equal(i, j) for (i, _), j in zip(zero, lists)) and all(not np.any(b) for _, b in zero)
    for E in c.energies[:2]:
        T0 = tr.tmatrix(c.F, c.S, list(c.contacts), E)
        T = tr.tmatrix(c.F, c.S, list(c.contacts) + zero, E)
        assert np.array_equal(T[:2, :2], T0) and not np.any(T[2:]) and not np.any(T[:, 2:])
        assert tr.t_eff(T, 2) == T[1, 0]
        assert effective_transmission(T[None], 2, source=0, drain=-1)[0] == T[1, 0]


def test_front_end_t_eff_is_the_restatement():
    """transport.effective_transmission (batched, with dropped probes and NaN matrices) against tmatrix_ref.t_eff."""
    from gaunegf_amd.transport import dephasing_probes, effective_transmission
    c = tr.cases()[1]
    T = np.stack([tr.tmatrix(c.F, c.S, c.terms, E) for E in c.energies] + [np.full((6, 6), np.nan)])
    got = effective_transmission(T, 2, source=0, drain=1)
    ref = [tr.t_eff(t, 2, d=1, s=0) for t in T[:-1]]
    assert np.isnan(got[-1]) and np.allclose(got[:-1], ref, rtol=1e-13, atol=0)
    assert np.allclose(effective_transmission(T, 2, source=1, drain=0)[:-1], [tr.t_eff(t, 2, d=0, s=1) for t in T[:-1]], rtol=1e-13)
    # the label map and the list form name the same probes; gamma per probe
    lab = -np.ones(c.n, dtype=int); lab[[3, 4]] = 0; lab[[20]] = 1
    a = dephasing_probes(c.S, lab, [0.5, 0.2])
    b = dephasing_probes(c.S, [[3, 4], [20]], [0.5, 0.2])
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    assert np.array_equal(a[0][1], -0.25j * c.S[np.ix_([3, 4], [3, 4])])


def _chain_t_eff(N, gam):
    F = np.zeros((N, N), complex)
    F[np.arange(N - 1), np.arange(1, N)] = F[np.arange(1, N), np.arange(N - 1)] = -1.0
    S = np.eye(N, dtype=complex)
    terms = [(np.array([0]), np.array([[-1j]])), (np.array([N - 1]), np.array([[-1j]]))]
    terms += [(np.array([i]), np.array([[-0.5j * gam]])) for i in range(N)]
    return tr.t_eff(tr.tmatrix_alt(F, S, terms, 0.0), 2)


def test_ohmic_limit():
    """Uniform chain, hopping -1, S = 1, lead Sigma = -i on the end sites, one probe per site with gamma = 0.5, E = 0:
    1 / T_eff grows linearly with N (second differences <= 1 % of the first); without dephasing T_eff = 1 at every N."""
    Ns = np.arange(4, 25, 4)
    inv = np.array([1.0 / _chain_t_eff(N, 0.5) for N in Ns])
    d1 = np.diff(inv)
    d2 = np.diff(d1)
    print("ohmic limit: 1 / T_eff", np.round(inv, 4).tolist(), "increments", np.round(d1, 4).tolist())
    assert np.all(d1 > 0) and np.abs(d2).max() <= 0.01 * np.abs(d1).min()
    for N in Ns:
        assert abs(_chain_t_eff(N, 0.0) - 1.0) <= 1e-12


def test_restatement_is_inside_the_parity_bar():
    worst = max(max(ea, eb) for *_, ea, eb in _table())
    print(f"tmatrix restatement: worst float64 error against the truth {worst:.3g} (allowed {tr.PROJECT_BAR / 100:g})")
    for tag, *_, ea, eb in _table():
        assert max(ea, eb) <= tr.PROJECT_BAR / 100, (tag, ea, eb)


def test_calibration():
    r, worst, at, r_at = 1.0, 0.0, None, None
    for tag, *_, ea, eb in _table():
        if max(ea / eb, eb / ea) > r:
            r, r_at = max(ea / eb, eb / ea), tag
        if max(ea, eb) > worst:
            worst, at = max(ea, eb), tag
    c_tm = 2.0 ** np.ceil(np.log2(2.0 * r))
    print(f"tmatrix calibration: R {r:.3g} (at {r_at}) -> C {c_tm:g} (tmatrix_ref.C_TM = {tr.C_TM:g}); float64 errors "
          f"{min(min(ea, eb) for *_, ea, eb in _table()):.3g} ... {worst:.3g} (worst at {at})")
    assert c_tm == tr.C_TM, (r, c_tm, tr.C_TM)


# --------------------------------------------------------------------------- planted defects
def _blocks(c, E):
    G = np.linalg.inv(tr.assembled(c.F, c.S, c.terms, E))
    return G, [tr.gamma(b) for _, b in c.terms]


def _from_blocks(c, G, gams, pick=lambda G, ia, ib: G[np.ix_(ia, ib)], conj=np.conj):
    C = len(c.terms)
    T = np.zeros((C, C))
    for a, (ia, _) in enumerate(c.terms):
        for b, (ib, _) in enumerate(c.terms):
            Gab = pick(G, ia, ib)
            T[a, b] = np.real(np.sum((gams[a] @ Gab @ gams[b]) * conj(Gab)))
    return T


def _defect_gamma_total(c, E):
    """Gamma_total used for Gamma_b"""
    n = c.n
    G = np.linalg.inv(tr.assembled(c.F, c.S, c.terms, E))
    gams = [tr.dense(n, idx, tr.gamma(blk)) for idx, blk in c.terms]
    Mtot = (G @ sum(gams)) @ G.conj().T
    return np.array([[np.real(np.trace(ga @ Mtot)) for _ in gams] for ga in gams])


def _defect_g_ba(c, E):
    """G_ba used for G_ab (the block taken transposed, so that the shapes fit)"""
    G, gams = _blocks(c, E)
    return _from_blocks(c, G, gams, pick=lambda G, ia, ib: G[np.ix_(ib, ia)].T)


def _defect_transpose_for_dagger(c, E):
    """G_ab^T used for G_ab^H: the final conjugation left out"""
    G, gams = _blocks(c, E)
    return _from_blocks(c, G, gams, conj=lambda x: x)


def _defect_probes_left_out_of_a(c, E):
    G = np.linalg.inv(tr.assembled(c.F, c.S, c.contacts, E))
    return _from_blocks(c, G, [tr.gamma(b) for _, b in c.terms])


def _defect_minus_two_im(c, E):
    """Gamma = -2 Im Sigma elementwise instead of i (Sigma - Sigma^H)"""
    G = np.linalg.inv(tr.assembled(c.F, c.S, c.terms, E))
    return _from_blocks(c, G, [(-2.0 * np.imag(b)).astype(complex) for _, b in c.terms])


# name -> (defect, the cases it applies to)
DEFECTS = {
    "gamma_total_for_gamma_b": (_defect_gamma_total, lambda c: True),
    "g_ba_for_g_ab": (_defect_g_ba, lambda c: not c.real),
    "transpose_for_dagger": (_defect_transpose_for_dagger, lambda c: True),
    "probes_left_out_of_a": (_defect_probes_left_out_of_a, lambda c: len(c.probes) > 0),
    "minus_two_im_sigma": (_defect_minus_two_im, lambda c: not c.real),
}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_defects_miss_the_bar(name):
    fn, applies = DEFECTS[name]
    least, count = np.inf, 0
    for tag, c, E, t, ea, eb in _table():
        if not applies(c):
            continue
        count += 1
        bar = tr.C_TM * max(ea, eb)
        ratio = tr.rel_err(fn(c, E), t) / bar
        least = min(least, ratio)
        assert ratio >= 100.0, (tag, name, ratio)
    assert count >= 8
    print(f"tmatrix planted defect {name}: least error / calibrated bar {least:.3g} over {count} inputs")


# --------------------------------------------------------------------------- existence
def test_abi_and_front_end_exist():
    from gaunegf_amd import _lib, transport
    with open(os.path.join(ROOT, "include", "negf.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/negf.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
    for fn in ("dephasing_probes", "effective_transmission", "calculate_transmission_matrix",
               "calculate_effective_transmission", "calculate_effective_current", "cohTransMatrix", "cohTransMatrixE",
               "cohTransDephased", "cohTransDephasedE"):
        assert callable(getattr(transport, fn, None)), fn
    from gaunegf_amd.engine import Engine
    for m in ("transmission_matrix", "transmission_matrix_dev"):
        assert callable(getattr(Engine, m, None)), m


def test_no_cpu_fallback():
    """Without a GPU the front ends raise (there is no CPU fallback); with one this check has nothing to say."""
    from gaunegf_amd import _lib
    from gaunegf_amd.transport import SigmaCalculator, calculate_transmission_matrix
    if os.path.exists(_lib.LIB_PATH) and _lib.load().negf_device_count() > 0:
        return
    c = tr.cases()[1]
    sig = c.contact_sigmas()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        calculate_transmission_matrix(c.F, c.S, SigmaCalculator(sig[0], sig[1]), c.energies, probes=c.probes)
