"""Overlap / Hamilton populations and projected DOS on the GPU (negf_population, negf_projected_dos and their front ends)
against the numpy restatement and the extended-precision truth of tests/population_ref.py.

Bars (none of them taken from what the device returns):
  * the calibrated bar on the CONST inputs (bond_ref.const_cases() and one n = 300 case): relative Frobenius error against
    the clongdouble truth at most population_ref.C_POP (= 16, test_population_host.test_calibration) times the larger error
    of the two float64 forms on that input -- tables, their row sums and projections, retarded and per contact, X = S and F;
  * parity with the float64 restatement on the Sigma(E) the device itself evaluated: 1e-8 relative Frobenius per energy,
    the project's bar for G(E)-derived quantities;
  * identities on the device's own outputs.  sum_c pop_c = (pop + pop^T) / 2, sum_c p_c,a = p_a and the complete-set sum
    rule join results that are each within their calibrated bar of the truth, so they may differ by the sum of those bars
    (times sqrt(n) where a vector's entries are added up).  The row form is the sum of the table's own entries: it is held
    to the summation bound n_g 2^-53 sum_b |table[a][b]| against the exactly rounded (math.fsum) row sums;
  * bitwise: run to run, negf_set_batch, relabelled groups (the permuted table / rows), projections independent of k.
"""
import functools
import math
import os
import socket
import warnings

import numpy as np
import pytest
import scipy.linalg as sla

import bond_ref as br
import population_ref as pr
import xprec
from helpers import chain_lead, random_system, swept

pytestmark = pytest.mark.gpu

BAR = pr.PROJECT_BAR
RET = "retarded"                                   # Engine.population's name of the retarded form


def _form(f):
    return RET if f is None else f


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def _near_eigenvalue(F, S, target=0.6):
    ev = sla.eigh(F, S, eigvals_only=True)
    return float(ev[np.argmin(np.abs(ev - target))]) + 5e-4


# --------------------------------------------------------------------------- truth and float64 forms, computed once
@functools.lru_cache(maxsize=None)
def _case(idx):
    return pr.case_n300() if idx == 3 else pr.const_cases()[idx]


@functools.lru_cache(maxsize=None)
def _vectors(idx):
    c = _case(idx)
    _, C = pr.complete_set(c.F, c.S)
    return C, pr.vectors(c.F, c.S, C)


def _energies(idx):
    c = _case(idx)
    return c.energies if idx < 3 else c.energies[[1, 2]]       # n = 300: two energies, one 5e-4 above an eigenvalue


@functools.lru_cache(maxsize=None)
def _truth(idx):
    """{(k, form): truth matrix G / A_c} over the energies of case idx (n = 300: the retarded form and contact 0)."""
    xprec.require_extended()
    c = _case(idx)
    forms = pr.FORMS if idx < 3 else (None, 0)

    def make(k):
        E = float(_energies(idx)[k])
        G = pr.spectral_truth(c.F, c.S, c.sigmas, E)
        return {(k, f): pr.spectral_truth(c.F, c.S, c.sigmas, E, f, G=G) for f in forms}
    out = {}
    for d in xprec.pmap(make, list(range(len(_energies(idx))))):
        out.update(d)
    return out


def _bars(idx, k, f, op, kind):
    """(truth, e64): the truth of `kind` ('table', 'rows', 'proj') and the larger error of the two float64 forms."""
    c = _case(idx)
    E = float(_energies(idx)[k])
    M = _truth(idx)[(k, f)]
    if kind == "proj":
        W = _vectors(idx)[1]
        t = pr.proj_truth_of(M, W, f)
        a, b = pr.proj(c.F, c.S, c.sigmas, E, W, f), pr.proj_alt(c.F, c.S, c.sigmas, E, W, f)
    else:
        t = pr.table_truth_of(M, c.S if op == "S" else c.F, f)
        a, b = pr.table(c.F, c.S, c.sigmas, E, f, op), pr.table_alt(c.F, c.S, c.sigmas, E, f, op)
        if kind == "rows":
            t, a, b = t.sum(axis=1), a.sum(axis=1), b.sum(axis=1)
    return t, max(pr.rel_err(a, t), pr.rel_err(b, t))


# --------------------------------------------------------------------------- CONST: the calibrated bar and 1e-8 parity
@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_const_truth_and_parity(engine, idx):
    """n = 24 / 60 (single-kernel path; 60: complex Hermitian F, S) / 130 (blocked inverse) / 300 (the column loops of a
    256-thread workgroup wrap; windowed inverse)."""
    c = _case(idx)
    E = _energies(idx)
    W = _vectors(idx)[1]
    forms = pr.FORMS if idx < 3 else (None, 0)
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.sigmas)
    try:
        got = {}
        for f in forms:
            for op in pr.OPS:
                got[("table", f, op)] = engine.population(h, _form(f), E, op)
                got[("rows", f, op)] = engine.population(h, _form(f), E, op, rows=True)
            got[("proj", f, None)] = engine.projected_dos(h, _form(f), E, W)
    finally:
        engine.sigma_free(h)
    worst = 0.0
    for (kind, f, op), val in got.items():
        assert val.shape == {"table": (E.size, c.n, c.n), "rows": (E.size, c.n), "proj": (E.size, c.n)}[kind]
        for k, e in enumerate(E):
            t, e64 = _bars(idx, k, f, op, kind)
            err = pr.rel_err(val[k], t)
            worst = max(worst, err / e64)
            print(f"CONST n={c.n} E={e:.6g} {kind} c={f} X={op}: device error vs truth {err:.3g}, float64 forms {e64:.3g}, "
                  f"ratio {err / e64:.3g} (allowed {pr.C_POP:g})")
            assert err <= pr.C_POP * e64, (c.n, e, kind, f, op, err, e64)
            if kind == "proj":
                ref = pr.proj(c.F, c.S, c.sigmas, e, W, f)
            else:
                ref = pr.table(c.F, c.S, c.sigmas, e, f, op)
                ref = ref.sum(axis=1) if kind == "rows" else ref
            assert _rel(val[k], ref) <= BAR, (c.n, e, kind, f, op)
    print(f"CONST n={c.n}: worst device error / float64 error {worst:.3g}")


# --------------------------------------------------------------------------- identities on the device's own outputs
@pytest.mark.parametrize("idx", [1, 2])
def test_identities_on_device_outputs(engine, idx):
    c = _case(idx)
    E = _energies(idx)
    C, W = _vectors(idx)
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.sigmas)
    try:
        tab = {(f, op): engine.population(h, _form(f), E, op) for f in pr.FORMS for op in pr.OPS}
        rows = engine.population(h, RET, E, 'S', rows=True)
        p = {f: engine.projected_dos(h, _form(f), E, W) for f in pr.FORMS}
    finally:
        engine.sigma_free(h)
    n = c.n
    for k, e in enumerate(E):
        for op in pr.OPS:
            ret = tab[(None, op)][k]
            sym = 0.5 * (ret + ret.T)
            allowed = pr.C_POP * (_bars(idx, k, None, op, "table")[1] * np.linalg.norm(ret)
                                  + sum(_bars(idx, k, f, op, "table")[1] * np.linalg.norm(tab[(f, op)][k]) for f in (0, 1)))
            d = np.linalg.norm(tab[(0, op)][k] + tab[(1, op)][k] - sym)
            print(f"n={n} E={e:.6g} X={op}: |sum_c pop_c - (pop + pop^T)/2| {d:.3g} (allowed {allowed:.3g}, |pop| {np.linalg.norm(ret):.3g})")
            assert d <= allowed
        allowed = pr.C_POP * sum(_bars(idx, k, f, None, "proj")[1] * np.linalg.norm(p[f][k]) for f in pr.FORMS)
        d = np.linalg.norm(p[0][k] + p[1][k] - p[None][k])
        print(f"n={n} E={e:.6g}: |sum_c p_c - p| {d:.3g} (allowed {allowed:.3g})")
        assert d <= allowed
        # complete S-orthonormal set: sum_a p_a = -Im Tr(G S) / pi = the sum of the rows
        allowed = np.sqrt(n) * pr.C_POP * (_bars(idx, k, None, None, "proj")[1] * np.linalg.norm(p[None][k])
                                           + _bars(idx, k, None, "S", "rows")[1] * np.linalg.norm(rows[k]))
        d = abs(math.fsum(p[None][k]) - math.fsum(rows[k]))
        print(f"n={n} E={e:.6g}: |sum_a p_a - sum_i rows_i| {d:.3g} (allowed {allowed:.3g})")
        assert d <= allowed


def _check_rows_against_table(rows, tab, what):
    """rows [m, ng] against the exactly rounded row sums of tab [m, ng, ng], within n_g 2^-53 sum_b |table[a][b]|."""
    ng = tab.shape[1]
    for k in range(tab.shape[0]):
        for a in range(ng):
            exact = math.fsum(tab[k, a])
            bound = ng * 2.0 ** -53 * math.fsum(np.abs(tab[k, a]))
            assert abs(rows[k, a] - exact) <= bound, (what, k, a, rows[k, a], exact, bound)


@pytest.mark.parametrize("f", [None, 0])
def test_rows_are_the_tables_row_sums(engine, f):
    c = _case(2)
    E = c.energies
    maps = {"orbitals": None, "atoms": c.atom_groups(), "mod7": np.arange(c.n) % 7, "one": np.zeros(c.n, dtype=int)}
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.sigmas)
    try:
        for name, g in maps.items():
            for op in pr.OPS:
                tab = engine.population(h, _form(f), E, op, g)
                rows = engine.population(h, _form(f), E, op, g, rows=True)
                _check_rows_against_table(rows, tab, (name, op))
    finally:
        engine.sigma_free(h)


# --------------------------------------------------------------------------- group shapes
def test_group_shapes(engine):
    """an empty group, a group of more than 64 orbitals, more than 4 groups, n_groups = 1, n_groups = n as an explicit
    map, non-contiguous labels -- retarded and contact form, against the grouped orbital table."""
    c = _case(2)                                                           # n = 130
    E = c.energies[:2]
    n = c.n
    big = np.where(np.arange(n) < 70, 0, 1 + (np.arange(n) - 70) // 12)    # group 0 holds 70 orbitals, 6 groups in all
    scattered = (np.arange(n) * 7) % 5                                     # non-contiguous labels
    with_empty = np.where(big >= 2, big + 2, big)                          # groups 2 and 3 are empty, trailing room too
    maps = {"big": (big, None), "scattered": (scattered, None), "empty": (with_empty, int(with_empty.max()) + 3),
            "one": (np.zeros(n, dtype=int), None), "explicit_n": (np.arange(n), n),
            "shuffled_n": (np.random.default_rng(3).permutation(n), n)}
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.sigmas)
    try:
        for f in (None, 1):
            orb = engine.population(h, _form(f), E, 'S')
            orb_rows = engine.population(h, _form(f), E, 'S', rows=True)
            for name, (g, ng) in maps.items():
                tab = engine.population(h, _form(f), E, 'S', g, ng)
                rows = engine.population(h, _form(f), E, 'S', g, ng, rows=True)
                ngr = int(g.max()) + 1 if ng is None else ng
                assert tab.shape == (E.size, ngr, ngr) and rows.shape == (E.size, ngr)
                for k in range(E.size):
                    ref = pr.group_table(orb[k], g, ngr)
                    assert np.linalg.norm(tab[k] - ref) <= 1e-13 * np.abs(orb[k]).sum(), (name, f)
                _check_rows_against_table(rows, tab, (name, f))
                if name == "explicit_n":
                    assert np.array_equal(tab, orb) and np.array_equal(rows, orb_rows)
                if name == "shuffled_n":                                   # singleton groups under other labels: bitwise
                    assert np.array_equal(tab[:, g[:, None], g[None, :]], orb) and np.array_equal(rows[:, g], orb_rows)
                if name == "empty":
                    used = np.unique(g)
                    unused = np.setdiff1d(np.arange(ngr), used)
                    assert np.all(tab[:, unused, :] == 0.0) and np.all(tab[:, :, unused] == 0.0) and np.all(rows[:, unused] == 0.0)
                if name == "one":
                    assert abs(tab[0, 0, 0] - math.fsum(orb[0].ravel())) <= 1e-13 * np.abs(orb[0]).sum()
    finally:
        engine.sigma_free(h)


# --------------------------------------------------------------------------- determinism
def test_bitwise_run_to_run_batch_and_relabelling(engine):
    c = _case(2)
    E = np.linspace(-2.0, 2.0, 7)
    groups = c.atom_groups()
    ng = int(groups.max()) + 1
    relabel = np.random.default_rng(1).permutation(ng)                     # group g is now called relabel[g]
    W = _vectors(2)[1]
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.sigmas)

    def everything():
        out = []
        for f in (RET, 0):
            out += [engine.population(h, f, E, 'S'), engine.population(h, f, E, 'F', groups),
                    engine.population(h, f, E, 'S', rows=True), engine.population(h, f, E, 'S', groups, rows=True),
                    engine.projected_dos(h, f, E, W)]
        return out
    try:
        ref = everything()
        again = everything()
        for batch in (1, 3):
            engine.set_batch(batch)
            try:
                cut = everything()
                swept(engine, batch, E.size)
            finally:
                engine.set_batch(0)
            for a, b in zip(ref, cut):
                assert np.array_equal(a, b), batch
        for f in (RET, 0):
            tab = engine.population(h, f, E, 'S', groups)
            rows = engine.population(h, f, E, 'S', groups, rows=True)
            ptab = engine.population(h, f, E, 'S', relabel[groups])
            prow = engine.population(h, f, E, 'S', relabel[groups], rows=True)
            assert np.array_equal(ptab[:, relabel[:, None], relabel[None, :]], tab)
            assert np.array_equal(prow[:, relabel], rows)
            # a vector's value does not depend on k or on its neighbours
            full = engine.projected_dos(h, f, E, W)
            for sel in (np.array([5]), np.array([5, 0, 77]), np.arange(40, 107)):
                assert np.array_equal(engine.projected_dos(h, f, E, W[sel]), full[:, sel]), sel.size
    finally:
        engine.sigma_free(h)
    for a, b in zip(ref, again):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------- other providers (parity, one small case each)
def _check_provider(engine, h, F, S, sig_at, E, what, groups):
    """retarded rows, a contact table with groups and projections on four vectors against the restatement."""
    n = F.shape[0]
    _, C = pr.complete_set(F, S)
    W = pr.vectors(F, S, C[:, [0, 3, n // 2, n - 1]])
    ng = int(groups.max()) + 1
    rows = engine.population(h, RET, E, 'S', rows=True)
    tabF = engine.population(h, RET, E, 'F')
    ctab = engine.population(h, 0, E, 'S', groups)
    crow = engine.population(h, 1, E, 'F', groups, rows=True)
    p, p1 = engine.projected_dos(h, RET, E, W), engine.projected_dos(h, 1, E, W)
    for k, e in enumerate(E):
        sig = sig_at(k)
        errs = {
            "rows": _rel(rows[k], pr.table(F, S, sig, e, None, 'S').sum(axis=1)),
            "tableF": _rel(tabF[k], pr.table(F, S, sig, e, None, 'F')),
            "contact table": _rel(ctab[k], pr.group_table(pr.table(F, S, sig, e, 0, 'S'), groups, ng)),
            "contact rows": _rel(crow[k], pr.group_rows(pr.table(F, S, sig, e, 1, 'F'), groups, ng)),
            "proj": _rel(p[k], pr.proj(F, S, sig, e, W)),
            "contact proj": _rel(p1[k], pr.proj(F, S, sig, e, W, 1)),
        }
        print(f"{what} E={e:.6g}: " + ", ".join(f"{a} {b:.3g}" for a, b in errs.items()) + f" (bar {BAR:g})")
        assert max(errs.values()) <= BAR, (what, e, errs)


def test_surfgtest_provider(engine):
    from gaunegf_amd.surfGTester import surfGTest
    n, nc = 40, 5
    F, S = random_system(n, 340)
    g = surfGTest(F, S, [list(range(nc)), list(range(n - nc, n))], -0.25j)
    E = np.array([-1.0, _near_eigenvalue(F, S), 2.0])
    engine.set_system(F, S)
    h = g._negf_lower(engine)
    _check_provider(engine, h, F.astype(complex), S.astype(complex), lambda k: [g.sig[0], g.sig[1]], E, "surfGTest n=40",
                    np.arange(n) // 6)


def _chain_system(n, nc, seed, solver):
    from gaunegf_amd.surfG1D import surfG
    F, S = random_system(n, seed)
    lead = [chain_lead(nc, 40 + k) for k in range(2)]
    ci = [list(range(nc)), list(range(n - nc, n))]
    rng = np.random.default_rng(seed)
    taus = [0.2 * rng.standard_normal((nc, nc)) for _ in range(2)]
    staus = [0.02 * rng.standard_normal((nc, nc)) for _ in range(2)]
    g = surfG(F, S, ci, taus=taus, staus=staus, alphas=[l[0] for l in lead], aOverlaps=[l[1] for l in lead],
              betas=[l[2] for l in lead], bOverlaps=[l[3] for l in lead], eta=1e-3, solver=solver)
    return F, S, g


@pytest.mark.parametrize("solver", ["fixed-point", "doubling"])
def test_chain_provider(engine, solver):
    n, nc = 60, 8
    F, S, g = _chain_system(n, nc, 67, solver)
    E = np.array([-1.0, _near_eigenvalue(F, S), 1.1])
    engine.set_system(F, S)
    h = g._negf_lower(engine)
    sL = engine.sigma_eval(h, 0, E, 2); sR = engine.sigma_eval(h, 1, E, 2)
    _check_provider(engine, h, F.astype(complex), S.astype(complex), lambda k: [sL[k], sR[k]], E, f"chain {solver} n={n}",
                    br.aligned_groups(n, (nc, nc), 10))


def test_bethe_provider(engine):
    from gaunegf_amd.surfGBethe import read_bethe_params, construct_sk_matrix, gen_neighbors
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaunegf_amd", "data", "Au")
    ne, Ed, Vd, Sd, H0 = read_bethe_params(here)
    dirs = gen_neighbors(np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.2, 0.0]))
    Sl = np.array([construct_sk_matrix(Sd, d) for d in dirs]); Vl = np.array([construct_sk_matrix(Vd, d) for d in dirs])
    n = 45
    F, S = random_system(n, 17)
    F = F - 5.0 * S                                                       # around the Au d band
    orbs = [[list(range(9))], [list(range(n - 18, n - 9)), list(range(n - 9, n))]]
    nbs = [[[0, 1, 2]], [[0, 1, 2], [6, 7, 8]]]
    engine.set_system(F, S)
    h = engine.sigma_bethe(orbs, nbs, [H0, H0], [Sl, Sl], [Vl, Vl], None, 1e-4, 1e-8)
    try:
        E = np.linspace(-3.8, -2.6, 3)
        sL = engine.sigma_eval(h, 0, E, 2); sR = engine.sigma_eval(h, 1, E, 2)
        _check_provider(engine, h, F.astype(complex), S.astype(complex), lambda k: [sL[k], sR[k]], E, "Bethe n=45",
                        br.aligned_groups(n, (9, 18), 9))
    finally:
        engine.sigma_free(h)


def test_precomputed_provider_and_refused_gammas(engine):
    """PRECOMPUTED with per-contact Sigma is served in both forms.  With coupling matrices handed in by the caller the
    contact form is refused (NEGF_EINVAL -> NotImplementedError) and the retarded form is served."""
    c = _case(1)
    E = c.energies
    scale = 1.0 + 0.1 * E
    tot = np.stack([(c.sigmas[0] + c.sigmas[1]) * s for s in scale])
    per = np.stack([np.stack([c.sigmas[0] * s, c.sigmas[1] * s]) for s in scale])
    W = _vectors(1)[1][[2, 30]]
    engine.set_system(c.F, c.S)
    h = engine.sigma_precomputed(tot, per)
    try:
        _check_provider(engine, h, c.F, c.S, lambda k: [s * scale[k] for s in c.sigmas], E, "PRECOMPUTED n=60", c.atom_groups())
    finally:
        engine.sigma_free(h)
    gam = np.stack([np.stack([br.gamma(s) for s in c.sigmas])] * E.size)
    h = engine.sigma_precomputed(np.stack([c.sigmas[0] + c.sigmas[1]] * E.size), gammas=gam)
    try:
        for call in (lambda: engine.population(h, 0, E), lambda: engine.population(h, 0, E, rows=True),
                     lambda: engine.projected_dos(h, 0, E, W)):
            with pytest.raises(NotImplementedError, match="Hermitian"):
                call()
        rows = engine.population(h, RET, E, 'S', rows=True)
        p = engine.projected_dos(h, RET, E, W)
    finally:
        engine.sigma_free(h)
    for k, e in enumerate(E):
        assert _rel(rows[k], pr.table(c.F, c.S, c.sigmas, e).sum(axis=1)) <= BAR
        assert _rel(p[k], pr.proj(c.F, c.S, c.sigmas, e, W)) <= BAR


# --------------------------------------------------------------------------- edge behaviour
@pytest.mark.parametrize("n", [8, 120])
def test_singular_energy(engine, n):
    """An exactly singular energy: NaN for that energy only, info set, NEGF_ESINGULAR (a warning in the front end)."""
    sL = np.zeros((n, n), complex); sL[0, 0] = -0.5j
    sR = np.zeros((n, n), complex); sR[n - 1, n - 1] = -0.25j
    S = np.eye(n, dtype=complex)
    F = S - sL - sR                                                       # E S - F - Sigma = (E - 1) S: zero at E = 1
    E = np.array([0.3, 1.0, 1.7])
    groups = np.arange(n) // 2
    W = np.eye(n, dtype=complex)[[0, n - 1, 3]]
    engine.set_system(F, S)
    h = engine.sigma_const([sL, sR])
    calls = [lambda f, e: engine.population(h, f, e, 'S'), lambda f, e: engine.population(h, f, e, 'F', groups),
             lambda f, e: engine.population(h, f, e, 'S', rows=True), lambda f, e: engine.population(h, f, e, 'S', groups, rows=True),
             lambda f, e: engine.projected_dos(h, f, e, W)]
    try:
        for f in (RET, 0):
            for call in calls:
                with pytest.warns(RuntimeWarning, match="singular"):
                    got = call(f, E)
                assert engine.last_info[1] > 0 and engine.last_info[0] == 0 and engine.last_info[2] == 0
                with warnings.catch_warnings():
                    warnings.simplefilter("error")
                    clean = call(f, E[[0, 2]])
                assert np.all(np.isnan(got[1]))
                assert np.array_equal(got[[0, 2]], clean) and np.all(np.isfinite(clean))
    finally:
        engine.sigma_free(h)


def test_invalid_arguments_and_empty_grid(engine):
    import ctypes as C
    from gaunegf_amd import _lib
    c = _case(0)
    n = c.n
    E = np.ascontiguousarray(c.energies, dtype=complex)
    W = np.ascontiguousarray(_vectors(0)[1])
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.sigmas)
    lib, ctx = engine._lib, engine._ctx
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros((E.size, n, n)); info = np.zeros(E.size, dtype=np.int32)
    try:
        pop = lambda ind, op, rows: lib.negf_population(ctx, h, ind, op, rows, E.size, vp(E), n, None, vp(out), vp(info))
        pdos = lambda ind, k: lib.negf_projected_dos(ctx, h, ind, E.size, vp(E), k, vp(W), vp(out), vp(info))
        assert pop(_lib.NEGF_IND_RETARDED, 0, 0) == 0 and pop(0, 1, 1) == 0 and pdos(_lib.NEGF_IND_RETARDED, n) == 0
        for ind in (_lib.NEGF_IND_RETARDED, 0):
            assert pop(ind, 2, 0) == _lib.NEGF_EINVAL and pop(ind, -1, 0) == _lib.NEGF_EINVAL        # op
            assert pop(ind, 0, 2) == _lib.NEGF_EINVAL and pop(ind, 0, -1) == _lib.NEGF_EINVAL        # rows_only
            assert pdos(ind, 0) == _lib.NEGF_EINVAL and pdos(ind, n + 1) == _lib.NEGF_EINVAL         # k outside 1 .. n
        assert pop(5, 0, 0) == _lib.NEGF_EINVAL and pdos(5, 1) == _lib.NEGF_EINVAL                   # no such contact
        # the selector of the retarded form is no contact of any other entry point
        assert lib.negf_local_transmission(ctx, h, _lib.NEGF_IND_RETARDED, E.size, vp(E), n, None, vp(out), vp(info)) == _lib.NEGF_EINVAL
        with pytest.raises(ValueError):
            engine.population(h, RET, E, 'X')
        with pytest.raises(ValueError):
            engine.population(h, RET, E, groups=np.zeros(n - 1, dtype=int))
        with pytest.raises(ValueError):
            engine.projected_dos(h, RET, E, W[:, :-1])
        # m = 0
        assert engine.population(h, RET, []).shape == (0, n, n)
        assert engine.population(h, 0, [], 'F', c.atom_groups(), rows=True).shape == (0, int(c.atom_groups().max()) + 1)
        assert engine.projected_dos(h, RET, [], W[:3]).shape == (0, 3)
        assert engine.projected_dos(h, 1, [], W[:3]).shape == (0, 3)
    finally:
        engine.sigma_free(h)


def test_more_than_8192_orbitals_refused(engine):
    """n = 8193: NEGF_EINVAL (NotImplementedError in the front end) from both forms, table and rows, and from the
    projection -- the check comes before any workspace is allocated.  Diagonal F and S; a 1-D chain provider, whose
    self-energies are two 2 x 2 blocks (a dense CONST Sigma would be another gigabyte per contact)."""
    import ctypes as C
    from gaunegf_amd import _lib
    n = 8193
    F = np.zeros((n, n), dtype=np.complex128); S = np.zeros((n, n), dtype=np.complex128)
    d = np.arange(n)
    F[d, d] = np.linspace(-2.0, 2.0, n); S[d, d] = 1.0
    lead = [chain_lead(2, 40 + k) for k in range(2)]
    engine.set_system(F, S)
    h = engine.sigma_chain1d([[0, 1], [n - 2, n - 1]], [l[0] for l in lead], [l[1] for l in lead], [l[2] for l in lead],
                             [l[3] for l in lead], [l[2] for l in lead], [l[3] for l in lead], 1e-3, 1e-5, 0.1)
    E = np.array([0.3 + 0.0j])
    W = np.zeros((1, n), dtype=np.complex128); W[0, 5] = 1.0
    groups = np.arange(n) // 64
    out = np.zeros(n); info = np.zeros(1, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    try:
        for f in (RET, 0):
            for kw in (dict(rows=True), dict(groups=groups), dict(groups=groups, rows=True)):
                with pytest.raises(NotImplementedError, match="8192"):
                    engine.population(h, f, E, 'S', **kw)
            with pytest.raises(NotImplementedError, match="8192"):
                engine.projected_dos(h, f, E, W)
            # the per-orbital table through the C ABI (the front end would set aside a gigabyte for the result first)
            ind = _lib.NEGF_IND_RETARDED if f == RET else f
            assert engine._lib.negf_population(engine._ctx, h, ind, 0, 0, 1, vp(E), n, None, vp(out), vp(info)) == _lib.NEGF_EINVAL
    finally:
        engine.sigma_free(h)
        small = _case(0)
        engine.set_system(small.F, small.S)


def test_device_pointer_forms(engine):
    """the _dev entry points (grid, vectors and results in HBM; buffers through the HIP runtime the library itself is
    linked against) return the bits of the host-pointer forms"""
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
    c = _case(1)
    E = np.ascontiguousarray(c.energies, dtype=np.complex128)
    W = np.ascontiguousarray(_vectors(1)[1][:7])
    groups = c.atom_groups()
    ng = int(groups.max()) + 1
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.sigmas)
    try:
        dE, dW = dev_buf(E), dev_buf(W)
        tab, rows, p = dev_buf(np.zeros((E.size, ng, ng))), dev_buf(np.zeros((E.size, ng))), dev_buf(np.zeros((E.size, 7)))
        for f in (RET, 1):
            engine.population_dev(h, f, E.size, dE.value, tab.value, 'F', groups)
            engine.population_dev(h, f, E.size, dE.value, rows.value, 'F', groups, rows=True)
            engine.projected_dos_dev(h, f, E.size, dE.value, 7, dW.value, p.value)
            engine.sync()
            assert np.array_equal(fetch(tab, (E.size, ng, ng)), engine.population(h, f, E, 'F', groups))
            assert np.array_equal(fetch(rows, (E.size, ng)), engine.population(h, f, E, 'F', groups, rows=True))
            assert np.array_equal(fetch(p, (E.size, 7)), engine.projected_dos(h, f, E, W))
    finally:
        engine.sigma_free(h)
        for b in bufs:
            hip.hipFree(b)


def test_neighbouring_entry_points_unchanged(engine):
    """negf_dos, negf_gless_int and negf_local_transmission before and after the new calls in one process (the shared
    workspace and staging buffers are what could leak)."""
    c = _case(2)
    E = np.linspace(-1.5, 1.5, 9)
    w = (np.cos(np.arange(E.size)) + 1.5) + 0.0j
    groups = c.atom_groups()
    W = _vectors(2)[1][:5]
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.sigmas)
    try:
        before = (engine.dos(h, E)[1], engine.gless_int(h, 0, E, w), engine.local_transmission(h, 0, E, groups))
        engine.population(h, RET, E, 'S', groups)
        engine.population(h, 1, E, 'F', rows=True)
        engine.projected_dos(h, 0, E, W)
        after = (engine.dos(h, E)[1], engine.gless_int(h, 0, E, w), engine.local_transmission(h, 0, E, groups))
    finally:
        engine.sigma_free(h)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------- front ends
def test_calculate_pdos_sums_to_trace(engine):
    from gaunegf_amd.transport import SigmaCalculator, calculate_overlap_population, calculate_pdos, PDOS
    c = _case(1)
    E = c.energies
    sc = SigmaCalculator(c.sigmas[0], c.sigmas[1])
    pd = calculate_pdos(c.F, c.S, sc, E)
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.sigmas)
    try:
        G = engine.gr_batch(h, E)
    finally:
        engine.sigma_free(h)
    assert pd.shape == (E.size, c.n)
    for k in range(E.size):
        tr = -np.imag(np.trace(G[k] @ c.S)) / np.pi
        per = -np.imag(np.diag(G[k] @ c.S)) / np.pi
        assert abs(pd[k].sum() - tr) <= 1e-12 * np.abs(per).sum()
        assert _rel(pd[k], per) <= 1e-12
    groups = c.atom_groups()
    pg = calculate_pdos(c.F, c.S, sc, E, groups=groups)
    coop = calculate_overlap_population(c.F, c.S, sc, E, groups=groups)
    cohp0 = calculate_overlap_population(c.F, c.S, sc, E, op='F', groups=groups, contact=0)
    shares = calculate_pdos(c.F, c.S, sc, E, groups=groups, contact=0) + calculate_pdos(c.F, c.S, sc, E, groups=groups, contact=1)
    _check_rows_against_table(pg, coop, "front end")
    # sum_c pop_c = (pop + pop^T) / 2: the contacts' shares add up to the rows of the symmetrised table, and their grand
    # total to the retarded form's
    assert _rel(shares, 0.5 * (coop + np.swapaxes(coop, 1, 2)).sum(axis=2)) <= BAR
    assert _rel(shares.sum(axis=1), pg.sum(axis=1)) <= BAR
    for k, e in enumerate(E):
        assert _rel(cohp0[k], pr.group_table(pr.table(c.F, c.S, c.sigmas, e, 0, 'F'), groups)) <= BAR
    tot, per = PDOS(E, c.F, c.S, c.sigmas[0], c.sigmas[1], groups=groups)
    assert np.array_equal(per, pg) and np.allclose(tot, pg.sum(axis=1), rtol=0, atol=0)


def test_spin_layouts(engine):
    from gaunegf_amd.transport import SigmaCalculator, calculate_overlap_population, calculate_pdos, calculate_projected_dos
    c = _case(0)
    N = c.n
    Fa = np.real(c.F); S = np.real(c.S)
    Fb, _ = random_system(N, 72)
    Z = np.zeros((N, N))
    F2 = np.block([[Fa, Z], [Z, Fb]]); S2 = np.block([[S, Z], [Z, S]])
    sc = SigmaCalculator(c.sigmas[0], c.sigmas[1])
    E = c.energies
    groups = c.atom_groups()
    # spin-diagonal 'u': (up, down) equal to the two N-sized runs
    for kw in (dict(), dict(groups=groups), dict(groups=groups, contact=1)):
        up, down = calculate_pdos(F2, S2, sc, E, spin='u', **kw)
        assert np.array_equal(up, calculate_pdos(Fa, S, sc, E, **kw)) and np.array_equal(down, calculate_pdos(Fb, S, sc, E, **kw))
    up, down = calculate_overlap_population(F2, S2, sc, E, op='F', groups=groups, spin='u')
    assert np.array_equal(up, calculate_overlap_population(Fa, S, sc, E, op='F', groups=groups))
    assert np.array_equal(down, calculate_overlap_population(Fb, S, sc, E, op='F', groups=groups))
    (pu, pdn), (eu, ed) = calculate_projected_dos(F2, S2, sc, E, fragment=[6, 7, 8, 9], spin='u')
    p1, e1 = calculate_projected_dos(Fa, S, sc, E, fragment=[6, 7, 8, 9])
    p2, e2 = calculate_projected_dos(Fb, S, sc, E, fragment=[6, 7, 8, 9])
    assert np.array_equal(pu, p1) and np.array_equal(pdn, p2) and np.array_equal(eu, e1) and np.array_equal(ed, e2)
    # spin mixing: the 2N system as a whole, groups of length 2N; 'g' is the same system in spinor order
    F2m = F2.copy(); F2m[1, N + 2] = F2m[N + 2, 1] = 0.05; F2m[N - 6, 2 * N - 7] = F2m[2 * N - 7, N - 6] = -0.03
    g2 = np.concatenate([groups, groups])
    sig2 = [np.kron(np.eye(2), s) for s in c.sigmas]
    tm = calculate_pdos(F2m, S2, sc, E, groups=g2, spin='u')
    perm = np.concatenate([np.arange(0, 2 * N, 2), np.arange(1, 2 * N, 2)])       # spinor -> block
    inv = np.argsort(perm)
    Fg = F2m[np.ix_(inv, inv)]; Sg = S2[np.ix_(inv, inv)]
    tg = calculate_pdos(Fg, Sg, sc, E, groups=np.repeat(groups, 2), spin='g')
    og = calculate_pdos(Fg, Sg, sc, E, spin='g')                                   # per orbital, in the caller's order
    Cm = np.zeros((2 * N, 2)); Cm[3, 0] = 1.0; Cm[N + 5, 1] = 1.0                  # block order
    pm = calculate_projected_dos(F2m, S2, sc, E, orbitals=Cm, spin='u')
    pgm = calculate_projected_dos(Fg, Sg, sc, E, orbitals=Cm[inv], spin='g')
    for k, e in enumerate(E):
        ref = pr.table(F2m.astype(complex), S2.astype(complex), sig2, e).sum(axis=1)
        assert _rel(tm[k], pr.group_rows(pr.table(F2m.astype(complex), S2.astype(complex), sig2, e), g2)) <= BAR
        assert _rel(tg[k], tm[k]) <= 1e-10
        assert _rel(og[k], ref[inv]) <= BAR
        assert _rel(pm[k], pr.proj(F2m.astype(complex), S2.astype(complex), sig2, e, pr.vectors(F2m, S2, Cm))) <= BAR
        assert _rel(pgm[k], pm[k]) <= 1e-10


def test_fragment_projection(engine):
    """fragment= returns the S-normalised molecular orbitals' energies; for a fragment decoupled from the rest (zero F
    and S coupling, no self-energy on it) its projected DOS peaks at those energies."""
    from gaunegf_amd.transport import SigmaCalculator, calculate_projected_dos, calculate_pdos, fragment_orbitals
    n, nf = 40, 6
    F, S = random_system(n, 91)
    frag = np.arange(17, 17 + nf)
    rest = np.setdiff1d(np.arange(n), frag)
    F[np.ix_(frag, rest)] = 0.0; F[np.ix_(rest, frag)] = 0.0
    S[np.ix_(frag, rest)] = 0.0; S[np.ix_(rest, frag)] = 0.0
    eta = 1e-3
    sig = [np.zeros((n, n), complex), np.zeros((n, n), complex)]
    sig[0][np.ix_(rest[:5], rest[:5])] = -0.3j * np.eye(5)
    sig[1][np.ix_(rest[-5:], rest[-5:])] = -0.2j * np.eye(5)
    sc = SigmaCalculator(sig[0], sig[1])
    e_mo, C = fragment_orbitals(F, S, frag)
    assert np.abs(C.conj().T @ S @ C - np.eye(nf)).max() <= 1e-13
    # around every orbital energy: the peak of the Lorentzian of width eta (complex energies E + i eta) sits on it
    offs = np.array([-3, -1, 0, 1, 3]) * eta
    E = (e_mo[:, None] + offs[None, :]).ravel() + 1j * eta
    p, e_ret = calculate_projected_dos(F, S, sc, E, fragment=frag)
    assert np.array_equal(e_ret, e_mo) and p.shape == (E.size, nf)
    p = p.reshape(nf, offs.size, nf)
    for a in range(nf):
        line = p[a, :, a]
        assert np.argmax(line) == 2, (a, line)
        # -(1/pi) Im 1 / (x + i eta) = eta / (pi (x^2 + eta^2)), alone in its own projection
        assert np.allclose(line, eta / (np.pi * (offs ** 2 + eta ** 2)), rtol=1e-6), (a, line)
    # the same projections through orbitals=C, and the fragment's Mulliken PDOS is their sum
    assert np.array_equal(calculate_projected_dos(F, S, sc, E, orbitals=C), p.reshape(E.size, nf))
    grp = np.zeros(n, dtype=int); grp[frag] = 1
    pd = calculate_pdos(F, S, sc, E, groups=grp)
    assert _rel(pd[:, 1], p.reshape(E.size, nf).sum(axis=1)) <= 1e-9


# --------------------------------------------------------------------------- sharded = local
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _front_ends():
    from gaunegf_amd.transport import SigmaCalculator, calculate_overlap_population, calculate_pdos, calculate_projected_dos
    c = pr.const_cases()[1]
    sc = SigmaCalculator(c.sigmas[0], c.sigmas[1])
    groups = c.atom_groups()
    E = np.linspace(-1.0, 1.0, 13)
    return {"pdos": calculate_pdos(c.F, c.S, sc, E, groups=groups),
            "coop": calculate_overlap_population(c.F, c.S, sc, E, groups=groups, contact=0),
            "proj": calculate_projected_dos(c.F, c.S, sc, E, fragment=[20, 21, 22, 23])[0]}


def _worker(port, q):
    import torch.distributed as dist
    from gaunegf_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_RANK"] = "0"
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        D.enable(single_rank_ok=True)
        assert D.is_active()
        q.put(_front_ends())
    finally:
        D.disable()
        dist.destroy_process_group()


def test_sharded_equals_local(engine):
    """The sharded leg (all-gather of the per-energy rows) in a one-rank group."""
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    res = None
    for _ in range(60):
        try:
            res = q.get(timeout=5)
            break
        except queue.Empty:
            if p.exitcode not in (None, 0):
                break
    if res is None:
        p.kill()
        pytest.fail("the rank died (its traceback is on stderr)")
    p.join(timeout=120)
    assert p.exitcode == 0
    ref = _front_ends()
    for key in ref:
        assert np.array_equal(res[key], ref[key]), key
