"""
Host checks of the yardstick the populations and the projected DOS are held to (tests/population_ref.py), and of the
front end's existence.  Inputs: bond_ref.const_cases() -- n = 24, 60 (complex Hermitian F, S), 130, four real energies each,
one of them 5e-4 above an eigenvalue of (F, S); the projection vectors are w = S c for the complete S-orthonormal set of
(F, S)'s eigenvectors.

  1. identities of the float64 restatement on those inputs: sum_c pop_c = (pop + pop^T) / 2, the rows of the S table are
     -Im (G S)_ii / pi, sum_c p_c,a = p_a, and the complete-set sum rule sum_a p_a = -Im Tr(G S) / pi;
  2. the restatement is a factor >= 100 inside the 1e-8 parity bar against the clongdouble truth;
  3. calibration: R = worst ratio between the errors of the two float64 forms against the truth over every (case, energy,
     form, op) table, its row sums and every projection; C_POP the smallest power of two >= 2 R.  Measured: R = 6.02 (the n = 24 contact-0
     projection), C_POP = 16; the float64 errors are 1.5e-16 ... 1.3e-14;
  4. planted defects miss the calibrated bar by a wide margin on every input they apply to.  Measured least
     error / bar: X_ij for conj(X_ij) (complex-Hermitian case) 4.7e+11, Gamma_total for Gamma_c 3.5e+12, Re for Im
     1.1e+13, w = c without S 3.0e+11 (asserted: >= 100);
  5. the C ABI and the Python front end exist (fails before the feature).
"""
import functools
import os
import re

import numpy as np
import pytest

import population_ref as pr
import xprec

xprec.require_extended()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("negf_population", "negf_population_dev", "negf_projected_dos", "negf_projected_dos_dev")


@functools.lru_cache(maxsize=None)
def _rows():
    """[(case, E, {c: truth matrix G / A_c})] over every (case, energy)."""
    items = [(c, float(E)) for c in pr.const_cases() for E in c.energies]

    def make(item):
        c, E = item
        G = pr.spectral_truth(c.F, c.S, c.sigmas, E)
        return c, E, {f: pr.spectral_truth(c.F, c.S, c.sigmas, E, f, G=G) for f in pr.FORMS}
    return xprec.pmap(make, items)


@functools.lru_cache(maxsize=None)
def _vectors(n):
    c = [x for x in pr.const_cases() if x.n == n][0]
    _, C = pr.complete_set(c.F, c.S)
    return C, pr.vectors(c.F, c.S, C)


@functools.lru_cache(maxsize=None)
def _table():
    """[(tag, kind, case, E, form, op, truth, err_a, err_b)]: every table (kind 'table'), its row sums ('rows') and every
    projection ('proj')."""
    out = []
    for c, E, M in _rows():
        _, W = _vectors(c.n)
        for f in pr.FORMS:
            for op in pr.OPS:
                t = pr.table_truth_of(M[f], c.S if op == "S" else c.F, f)
                out.append((f"n={c.n} E={E:.6g} c={f} X={op}", "table", c, E, f, op, t,
                            pr.rel_err(pr.table(c.F, c.S, c.sigmas, E, f, op), t),
                            pr.rel_err(pr.table_alt(c.F, c.S, c.sigmas, E, f, op), t)))
                out.append((f"n={c.n} E={E:.6g} c={f} X={op} rows", "rows", c, E, f, op, t.sum(axis=1),
                            pr.rel_err(pr.table(c.F, c.S, c.sigmas, E, f, op).sum(axis=1), t.sum(axis=1)),
                            pr.rel_err(pr.table_alt(c.F, c.S, c.sigmas, E, f, op).sum(axis=1), t.sum(axis=1))))
            t = pr.proj_truth_of(M[f], W, f)
            out.append((f"n={c.n} E={E:.6g} c={f} proj", "proj", c, E, f, None, t,
                        pr.rel_err(pr.proj(c.F, c.S, c.sigmas, E, W, f), t),
                        pr.rel_err(pr.proj_alt(c.F, c.S, c.sigmas, E, W, f), t)))
    return out


def test_restatement_identities():
    worst = dict(sum_c=0.0, rows=0.0, proj=0.0, complete=0.0)
    for c in pr.const_cases():
        C, W = _vectors(c.n)
        for E in c.energies:
            G = pr.spectral(c.F, c.S, c.sigmas, E)
            mull = -np.imag(np.diag(G @ c.S)) / np.pi
            for op in pr.OPS:
                ret = pr.table(c.F, c.S, c.sigmas, E, None, op)
                parts = sum(pr.table(c.F, c.S, c.sigmas, E, k, op) for k in (0, 1))
                d = np.linalg.norm(parts - 0.5 * (ret + ret.T)) / np.linalg.norm(ret)
                worst["sum_c"] = max(worst["sum_c"], d)
                assert d <= 1e-12, (c.n, E, op, d)
            rows = pr.table(c.F, c.S, c.sigmas, E, None, "S").sum(axis=1)
            d = np.abs(rows - mull).max() / np.abs(mull).max()
            worst["rows"] = max(worst["rows"], d)
            assert d <= 1e-12, (c.n, E, d)
            p = pr.proj(c.F, c.S, c.sigmas, E, W)
            pc = sum(pr.proj(c.F, c.S, c.sigmas, E, W, k) for k in (0, 1))
            d = np.linalg.norm(pc - p) / np.linalg.norm(p)
            worst["proj"] = max(worst["proj"], d)
            assert d <= 1e-11, (c.n, E, d)
            d = abs(p.sum() - mull.sum()) / np.abs(p).sum()
            worst["complete"] = max(worst["complete"], d)
            assert d <= 1e-11, (c.n, E, d)
        assert np.abs(C.conj().T @ c.S @ C - np.eye(c.n)).max() <= 1e-12
    print("population restatement: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_restatement_is_inside_the_parity_bar():
    worst = max(max(ea, eb) for *_, ea, eb in _table())
    print(f"population restatement: worst float64 error against the truth {worst:.3g} (allowed {pr.PROJECT_BAR / 100:g})")
    for tag, *_, ea, eb in _table():
        assert max(ea, eb) <= pr.PROJECT_BAR / 100, (tag, ea, eb)


def test_calibration():
    r, worst, at, r_at = 1.0, 0.0, None, None
    for tag, *_, ea, eb in _table():
        if max(ea / eb, eb / ea) > r:
            r, r_at = max(ea / eb, eb / ea), tag
        if max(ea, eb) > worst:
            worst, at = max(ea, eb), tag
    c_pop = 2.0 ** np.ceil(np.log2(2.0 * r))
    print(f"population calibration: R {r:.3g} (at {r_at}) -> C {c_pop:g} (population_ref.C_POP = {pr.C_POP:g}); float64 errors "
          f"{min(min(ea, eb) for *_, ea, eb in _table()):.3g} ... {worst:.3g} (worst at {at})")
    assert c_pop == pr.C_POP, (r, c_pop, pr.C_POP)


# --------------------------------------------------------------------------- planted defects
def _defect_unconjugated_x(c, E, f, op, W):
    """X_ij read for conj(X_ij) (shows on the complex-Hermitian case only)."""
    M = pr.spectral(c.F, c.S, c.sigmas, E, f)
    X = c.S if op == "S" else c.F
    return -pr.INV_PI * np.imag(M * X) if f is None else 0.5 * pr.INV_PI * np.real(M * X)


def _defect_gamma_total(c, E, f, op, W):
    G = np.linalg.inv(E * c.S - c.F - sum(c.sigmas))
    Ac = (G @ pr.br.gamma(c.sigmas[0] + c.sigmas[1])) @ G.conj().T
    return pr.table_of(Ac, c.S if op == "S" else c.F, f)


def _defect_re_for_im(c, E, f, op, W):
    G = pr.spectral(c.F, c.S, c.sigmas, E)
    return -pr.INV_PI * np.real(G * np.conj(c.S if op == "S" else c.F))


def _defect_missing_s(c, E, f, op, W):
    C, _ = _vectors(c.n)
    return pr.proj(c.F, c.S, c.sigmas, E, np.ascontiguousarray(C.T).astype(complex), f)


# name -> (defect, the rows of _table() it applies to)
DEFECTS = {
    "x_ij_for_conj_x_ij": (_defect_unconjugated_x, lambda kind, c, f: kind == "table" and np.iscomplexobj(c.S) and np.abs(c.S.imag).max() > 0),
    "gamma_total_for_gamma_c": (_defect_gamma_total, lambda kind, c, f: kind == "table" and f is not None),
    "re_for_im": (_defect_re_for_im, lambda kind, c, f: kind == "table" and f is None),
    "w_without_s": (_defect_missing_s, lambda kind, c, f: kind == "proj"),
}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_defects_miss_the_bar(name):
    fn, applies = DEFECTS[name]
    least, count = np.inf, 0
    for tag, kind, c, E, f, op, t, ea, eb in _table():
        if not applies(kind, c, f):
            continue
        count += 1
        bar = pr.C_POP * max(ea, eb)
        ratio = pr.rel_err(fn(c, E, f, op, None), t) / bar
        least = min(least, ratio)
        assert ratio >= 100.0, (tag, name, ratio)
    assert count >= 8
    print(f"population planted defect {name}: least error / calibrated bar {least:.3g} over {count} inputs")


# --------------------------------------------------------------------------- existence
def test_abi_and_front_end_exist():
    from gaunegf_amd import _lib, transport
    with open(os.path.join(ROOT, "include", "negf.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/negf.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
    assert re.search(r"#define\s+NEGF_IND_RETARDED\b", header) and _lib.NEGF_IND_RETARDED != _lib.NEGF_IND_TOTAL
    for fn in ("calculate_pdos", "calculate_overlap_population", "calculate_projected_dos", "fragment_orbitals", "PDOS",
               "PDOSE"):
        assert callable(getattr(transport, fn, None)), fn
    from gaunegf_amd.engine import Engine
    for m in ("population", "population_dev", "projected_dos", "projected_dos_dev"):
        assert callable(getattr(Engine, m, None)), m


def test_fragment_orbitals_are_s_normalised():
    from gaunegf_amd.transport import fragment_orbitals
    c = pr.const_cases()[1]
    idx = np.array([20, 21, 22, 25, 31, 40])
    e, C = fragment_orbitals(c.F, c.S, idx)
    assert C.shape == (c.n, idx.size) and np.all(np.diff(e) >= 0)
    outside = np.setdiff1d(np.arange(c.n), idx)
    assert not np.any(C[outside])
    assert np.abs(C.conj().T @ c.S @ C - np.eye(idx.size)).max() <= 1e-13
    assert np.abs(C.conj().T @ c.F @ C - np.diag(e)).max() <= 1e-12


def test_no_cpu_fallback():
    """Without a GPU the front ends raise (there is no CPU fallback); with one this check has nothing to say."""
    from gaunegf_amd import _lib
    from gaunegf_amd.transport import SigmaCalculator, calculate_pdos, calculate_projected_dos
    if os.path.exists(_lib.LIB_PATH) and _lib.load().negf_device_count() > 0:
        return
    c = pr.const_cases()[0]
    sc = SigmaCalculator(c.sigmas[0], c.sigmas[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        calculate_pdos(c.F, c.S, sc, c.energies, groups=c.atom_groups())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        calculate_projected_dos(c.F, c.S, sc, c.energies, fragment=[5, 6, 7])
