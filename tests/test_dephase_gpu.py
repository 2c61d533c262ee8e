"""
The floating dephasing probes on the MI355X (negf_probe_response, negf_gless_int_probes, negf_gr_int_probes and their _dev
forms, k_dephase.hip) against tests/dephase_ref.py.

Shapes: (a) n = 24, two contacts of 4, six probes of 1 - 3 orbitals (two overlapping, one on a lead, one decoupled);
(b) n = 40 complex Hermitian (T != T^T), three contacts, five probes; (c) probe-count edges P = 1, 2, 63, 64, 65 and the
two sides of the response kernel's LDS / global boundary (Engine.DEPH_LDS_MAX_P), one-orbital probes on n = P + 8;
(d) n = 130, two chain leads (both solvers), ten probes of 9; (e) a Bethe provider.  Three or four real energies each.

Bars.  R and the weighted sums of G D_s G^H against the clongdouble truth: C_DEPH x the float64 forms' own error on that
input (relative Frobenius; C_DEPH = 4, calibrated on the CPU, test_dephase_host.test_calibration).  What follows from
that bar for quantities derived from R, in the same norm: the truth's coupled rows sum to 1 exactly, so the vector of
the device's row sums is within sqrt(n_c) bar |R|_F of 1, and no entry lies below -bar |R|_F.  (I1) compares sums of
results that are each within their bar of a truth for which the identity is exact: the bars add.  (I2): the calibrated
bar scaled by max T.  The row sums are not held to the literal |sum - 1| <= bar row by row: the bar measures R as a whole
(relative Frobenius), a row's share of it is not fixed, and the worst row is printed as a multiple of the bar instead
(0 ... 0.93 up to P = 65, 1.07 at P = 80, 1.50 at P = 81: the literal reading is not met there).  The solve's parity with
the host form on the device's own T takes 1e-10 (entries of R are O(1)); it is reported, the truth is the yardstick.
Hermiticity: elements (i, j) and (j, i) of a diagonal tile are sums of K <= n products in different orders, each sum
bounded by sqrt(out_ii out_jj) for D >= 0: 2 n 2^-53 max |out|.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

import dephase_ref as dr
import tmatrix_ref as tr
from helpers import random_system, swept

pytestmark = pytest.mark.gpu

BAR = dr.PROJECT_BAR
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dephase_tmat_parent.npz")


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


class _Const:
    """the case's CONST provider for the duration of a with block"""
    def __init__(self, engine, c, terms=None):
        self.engine, self.c, self.terms = engine, c, terms

    def __enter__(self):
        self.engine.set_system(self.c.F, self.c.S)
        self.h = self.engine.sigma_const(self.c.contact_sigmas(self.terms))
        return self.h

    def __exit__(self, *exc):
        self.engine.sigma_free(self.h)


def _weights(m):
    return (np.cos(np.arange(m)) + 1.5) + 0.0j


def _edge_sizes():
    from gaunegf_amd.engine import Engine
    lds = Engine.DEPH_LDS_MAX_P
    return sorted({1, 2, 63, 64, 65, lds, lds + 1})


def _check_response(tag, R, truth, ea, eb, coupled, T_dev, n_c):
    """checks 1 and 2 on one energy; returns the error as a fraction of the bar"""
    from gaunegf_amd.transport import probe_response
    err = dr.rel_err(R, truth)
    bar = dr.C_DEPH * max(ea, eb)
    host = probe_response(T_dev[None], n_c)[0]
    par = np.abs(R - host).max()
    norm = np.linalg.norm(R)
    sums = np.linalg.norm(R[coupled].sum(axis=1) - 1.0)
    row = np.abs(R[coupled].sum(axis=1) - 1.0).max()
    print(f"dephase {tag}: R error {err:.3g} (bar {bar:.3g}, float64 forms {ea:.3g} / {eb:.3g}, {err / bar:.2f} of the bar), "
          f"|R - host solve| {par:.3g}, |row sums - 1| {sums:.3g} (worst row {row:.3g} = {row / bar:.2f} bar), min R {R.min():.3g}")
    assert err <= bar, (tag, err, bar)
    assert par <= 1e-10, (tag, par)
    assert sums <= np.sqrt(n_c) * bar * norm, (tag, sums, bar * norm)
    assert not np.any(R[~coupled]), tag
    assert R.min() >= -bar * norm, (tag, R.min())
    return err / bar


# --------------------------------------------------------------------------- the response: checks 1 and 2
def _response_case(engine, c, energies):
    with _Const(engine, c) as h:
        R = engine.probe_response(h, energies, c.probes)
        T = engine.transmission_matrix(h, energies, c.probes)
    assert R.shape == (len(energies), len(c.probes), c.n_c)
    coupled = np.array([bool(np.any(blk)) for _, blk in c.probes])
    worst = 0.0
    for k, E in enumerate(energies):
        truth, _, _, ea, eb = dr.truth_row(c, float(E))
        worst = max(worst, _check_response(f"{c.name} E={E:.6g}", R[k], truth, ea, eb, coupled, T[k], c.n_c))
    print(f"dephase {c.name}: worst R error {worst:.2f} of the bar")


@pytest.mark.parametrize("shape", ["a", "b", "c17"])
def test_response_shapes(engine, shape):
    """c17: 17 contacts, one more than the LDS class takes -- three probes in the global class"""
    c = {"a": dr.shape_a, "b": dr.shape_b, "c17": dr.many_contacts_case}[shape]()
    _response_case(engine, c, c.energies)


def test_response_in_several_chunks(engine):
    """P = 400 one-orbital probes, 220 energies in one batch: 400 x 402 doubles per energy, so the global class' work area
    (negf_common.h: 256 MiB) holds 208 energies and the batch goes through in two launches.  Every energy, those of the
    second launch included, against the host solve on the device's own T of that energy (an energy that read another's
    matrix or work area would be off by O(1); a shorter grid of its own is no bitwise yardstick here, the inverse's
    route at n = 408 follows the number of energies in the batch)."""
    from gaunegf_amd.transport import probe_response
    c = dr.edge_case(400)
    E = np.linspace(-1.5, 1.5, 220)
    engine.set_batch(220)
    try:
        with _Const(engine, c) as h:
            R = engine.probe_response(h, E, c.probes)
            T = engine.transmission_matrix(h, E, c.probes)
            again = engine.probe_response(h, E, c.probes)
            swept(engine, 220, E.size)
    finally:
        engine.set_batch(0)
    par = np.abs(R - probe_response(T, 2)).max(axis=(1, 2))
    print(f"dephase P400 x 220 energies: |R - host solve| {par[:208].max():.3g} (first launch), {par[208:].max():.3g} (second), "
          f"|row sums - 1| {np.abs(R.sum(axis=2) - 1).max():.3g}")
    assert par.max() <= 1e-10
    assert np.array_equal(R, again)


@pytest.mark.parametrize("P", _edge_sizes())
def test_response_probe_count_edges(engine, P):
    c = dr.edge_case(P)
    _response_case(engine, c, c.energies[:3])


@pytest.mark.parametrize("solver", ["fixed-point", "doubling"])
def test_chain_leads_response_and_gless(engine, solver):
    """shape (d): R and every contact's sum against the truth built on the blocks the provider itself evaluates"""
    F, S, ci, _, probes = dr.shape_d()
    Fc, Sc = F.astype(complex), S.astype(complex)
    E = dr.D_ENERGIES
    w = _weights(E.size)
    h, g = dr.lower_d(engine, solver)
    terms = dr.terms_d(engine, h, E)
    R = engine.probe_response(h, E, probes)
    T = engine.transmission_matrix(h, E, probes)
    outs = {s: engine.gless_int_probes(h, s, E, w, probes) for s in (0, 1, None)}
    coupled = np.ones(len(probes), dtype=bool)
    truths = {s: 0 for s in outs}
    refs = {s: 0 for s in outs}
    for k, e in enumerate(E):
        Rt, Ms, _, ea, eb = dr.truth_and_errors(Fc, Sc, terms[k], 2, float(e))
        _check_response(f"chain {solver} E={e:.6g}", R[k], Rt, ea, eb, coupled, T[k], 2)
        for s in outs:
            truths[s] = truths[s] + dr.LD(w[k]) * Ms[-1 if s is None else s]
            refs[s] = refs[s] + dr.gless_probes(Fc, Sc, terms[k], 2, s, [e], [w[k]])
    _check_gless(f"chain {solver}", outs, truths, refs, F.shape[0])


# --------------------------------------------------------------------------- G^<: checks 3 and 4 (I1)
def _check_gless(tag, outs, truths, refs, n):
    slack = 0.0
    for s, out in outs.items():
        err = dr.rel_err(out, truths[s])
        bar = dr.C_DEPH * dr.rel_err(refs[s], truths[s])
        herm = np.abs(out - out.conj().T).max() / np.abs(out).max()
        print(f"dephase {tag} ind={s}: error {err:.3g} (bar {bar:.3g}, {err / bar:.2f} of it), |out - out^H| / max {herm:.3g}")
        assert err <= bar, (tag, s, err, bar)
        assert herm <= 2 * n * 2.0 ** -53, (tag, s, herm)
        slack += bar * float(np.sqrt((np.abs(np.asarray(truths[s], dtype=complex)) ** 2).sum()))
    parts = sum(out for s, out in outs.items() if s is not None)
    i1 = float(np.linalg.norm(parts - outs[None]))
    print(f"dephase {tag}: (I1) |sum_s out_s - out_total| {i1:.3g} (bar {slack:.3g})")
    assert i1 <= slack, (tag, i1, slack)


@pytest.mark.parametrize("shape", ["a", "b", "P65"])
def test_gless_truth_hermiticity_and_sum_rule(engine, shape):
    c = {"a": dr.shape_a, "b": dr.shape_b, "P65": lambda: dr.edge_case(65)}[shape]()
    E = c.energies if shape != "P65" else c.energies[:3]
    w = _weights(E.size)
    with _Const(engine, c) as h:
        outs = {s: engine.gless_int_probes(h, s, E, w, c.probes) for s in list(range(c.n_c)) + [None]}
    truths, refs = {}, {}
    for s in outs:
        truths[s] = sum(dr.LD(wk) * dr.truth_row(c, float(e))[1][-1 if s is None else s] for e, wk in zip(E, w))
        refs[s] = dr.gless_probes(c.F, c.S, c.terms, c.n_c, s, E, w)
    _check_gless(c.name, outs, truths, refs, c.n)


@pytest.mark.parametrize("shape", ["a", "b"])
def test_effective_transmission_identity(engine, shape):
    """(I2): one energy, w = 1: Re Tr[Gamma_d out_s] over I_d is effective_transmission's T_eff[d][s] of the device's T.
    Bar: the calibrated one scaled by max T, C_DEPH max(ea, eb) max T."""
    from gaunegf_amd.transport import effective_transmission
    c = dr.shape_a() if shape == "a" else dr.shape_b()
    worst = 0.0
    with _Const(engine, c) as h:
        for E in c.energies[[0, 1, 3]]:
            T = engine.transmission_matrix(h, [E], c.probes)
            tmax = np.abs(T).max()
            _, _, _, ea, eb = dr.truth_row(c, float(E))
            bar = dr.C_DEPH * max(ea, eb) * tmax
            for s in range(c.n_c):
                out = engine.gless_int_probes(h, s, [E], [1.0], c.probes)
                for d in range(c.n_c):
                    if d == s:
                        continue
                    ix, blk = c.terms[d]
                    mine = float(np.real(np.trace(tr.gamma(blk) @ out[np.ix_(ix, ix)])))
                    theirs = effective_transmission(T, c.n_c, source=s, drain=d)[0]
                    worst = max(worst, abs(mine - theirs) / bar)
                    print(f"dephase {c.name} E={E:.6g} (I2) d={d} s={s}: {mine:.12g} vs {theirs:.12g}, "
                          f"|diff| {abs(mine - theirs):.3g} (bar {bar:.3g})")
                    assert abs(mine - theirs) <= bar, (c.name, E, d, s, mine, theirs, bar)
    print(f"dephase {c.name}: (I2) worst {worst:.2f} of the bar")


# --------------------------------------------------------------------------- (I3), G^r
def test_zero_strength_probes_give_gless_int(engine):
    """check 5: gamma = 0 probes (Gamma_p = 0 exactly, P' empty): both calls within the bar of one truth"""
    a = dr.shape_a()
    zero = [(ix, np.zeros_like(blk)) for ix, blk in a.probes]
    terms = list(a.contacts) + zero
    E = a.energies
    w = _weights(E.size)
    with _Const(engine, a) as h:
        assert not np.any(engine.probe_response(h, E, zero))
        for s in (0, 1, None):
            got = engine.gless_int_probes(h, s, E, w, zero)
            plain = engine.gless_int(h, s, E, w)
            truth = dr.gless_probes_truth(a.F, a.S, terms, 2, s, E, w)
            bar = dr.C_DEPH * dr.rel_err(dr.gless_probes(a.F, a.S, terms, 2, s, E, w), truth)
            e1, e2 = dr.rel_err(got, truth), dr.rel_err(plain, truth)
            print(f"dephase (I3) ind={s}: with zero probes {e1:.3g}, gless_int {e2:.3g} (bar {bar:.3g}); difference {_rel(got, plain):.3g}")
            assert e1 <= bar and e2 <= bar, (s, e1, e2, bar)


@pytest.mark.parametrize("shape", ["a", "d130"])
def test_gr_int_probes_equals_probes_as_contacts(engine, shape):
    """check 6: sum_k w_k G with the probes as arguments against gr_int on a CONST provider that carries them as contacts"""
    c = dr.shape_a() if shape == "a" else tr.cases()[2]
    E = c.energies + 0.05j
    w = _weights(E.size) * (1 + 0.25j)
    with _Const(engine, c) as h:
        got = engine.gr_int_probes(h, E, w, c.probes)
        bare = engine.gr_int(h, E, w)
    with _Const(engine, c, c.terms) as h:
        ref = engine.gr_int(h, E, w)
    print(f"dephase gr_int_probes {c.name}: {_rel(got, ref):.3g} (bar {BAR:g}); without the probes {_rel(bare, ref):.3g}")
    assert _rel(got, ref) <= BAR
    assert _rel(bare, ref) > 1e-3                          # (the probes do change G)


# --------------------------------------------------------------------------- exact checks
def _bitwise(engine, h, E, probes, n_c):
    w = _weights(E.size)
    call = lambda pr: (engine.probe_response(h, E, pr), engine.gless_int_probes(h, 0, E, w, pr),
                       engine.gless_int_probes(h, None, E, w, pr))
    ref = call(probes)
    for a, b in zip(call(probes), ref):
        assert np.array_equal(a, b)
    for batch in (1, 3):
        engine.set_batch(batch)
        try:
            cut = call(probes)
            swept(engine, batch, E.size)
        finally:
            engine.set_batch(0)
        for a, b in zip(cut, ref):
            assert np.array_equal(a, b), batch
    perm = np.random.default_rng(len(probes)).permutation(len(probes))
    Rp, gs, gt = call([probes[q] for q in perm])
    assert np.array_equal(Rp, ref[0][:, perm, :])          # probe q of the permuted call is probe perm[q] of the original
    assert np.array_equal(gs, ref[1]) and np.array_equal(gt, ref[2])


def test_bitwise_shape_a(engine):
    a = dr.shape_a()
    with _Const(engine, a) as h:
        _bitwise(engine, h, np.linspace(-2.0, 2.0, 7), a.probes, 2)


def test_bitwise_shape_b(engine):
    """shape (b) takes the compact products (2 K_U <= n): the gather, X inside the work area, the K_U x K_U D"""
    b = dr.shape_b()
    with _Const(engine, b) as h:
        _bitwise(engine, h, np.linspace(-2.0, 2.0, 7), b.probes, 3)


def test_bitwise_shape_d(engine):
    h, g = dr.lower_d(engine, "doubling")
    _bitwise(engine, h, np.linspace(-1.0, 1.2, 5), dr.shape_d()[4], 2)


@pytest.mark.parametrize("n", [8, 120])
def test_singular_energy(engine, n):
    """check 8: NaN for the singular energy only; gless_int_probes behaves as gless_int does"""
    sL = np.zeros((n, n), complex); sL[0, 0] = -0.5j
    sR = np.zeros((n, n), complex); sR[5, 5] = -0.25j
    probes = [(np.array([2, 3]), np.array([[-0.25j, 0.0], [0.0, -0.125j]])), (np.array([3]), np.array([[-0.5j]]))]
    # a tridiagonal overlap: G = S^-1 / (E - 1) is dense, so the probes reach the contacts (probes that see only each
    # other have a singular W and no defined occupation at any energy)
    S = np.eye(n, dtype=complex) + 0.2 * (np.eye(n, k=1) + np.eye(n, k=-1))
    F = S - sL - sR
    for ix, b in probes:
        F[np.ix_(ix, ix)] -= b                             # E S - F - Sigma - probes = (E - 1) S: zero at E = 1
    E = np.array([0.25, 1.0, 1.75])
    w = np.ones(3, complex)
    engine.set_system(F, S)
    h = engine.sigma_const([sL, sR])
    try:
        with pytest.warns(RuntimeWarning, match="singular"):
            got = engine.probe_response(h, E, probes)
        assert engine.last_info[1] > 0 and engine.last_info[0] == 0 and engine.last_info[2] == 0
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            clean = engine.probe_response(h, E[[0, 2]], probes)
        assert np.all(np.isnan(got[1]))
        assert np.array_equal(got[[0, 2]], clean) and np.all(np.isfinite(clean))
        with pytest.warns(RuntimeWarning, match="singular"):
            out = engine.gless_int_probes(h, 0, E, w, probes)
        assert engine.last_info[1] > 0
        # gless_int on the provider that carries the probes as contacts meets the same singular matrix
        engine.sigma_free(h)
        dense = [tr.dense(n, ix, b) for ix, b in probes]
        h = engine.sigma_const([sL, sR] + dense)
        with pytest.warns(RuntimeWarning, match="singular"):
            plain = engine.gless_int(h, 0, E, w)
        assert np.array_equal(np.isfinite(out), np.isfinite(plain))
    finally:
        engine.sigma_free(h)


def test_probes_without_a_path_to_a_contact(engine):
    """S = 1 and E S - F - Sigma = (E - 1) 1: G is diagonal, the overlapping probes on [2, 3] and [3] see only each other, W is
    singular at every energy.  The whole R of such an energy is NaN, info stays 0, the engine warns; the host form agrees."""
    from gaunegf_amd.transport import probe_response
    n = 8
    sL = np.zeros((n, n), complex); sL[0, 0] = -0.5j
    sR = np.zeros((n, n), complex); sR[n - 1, n - 1] = -0.25j
    probes = [(np.array([2, 3]), np.array([[-0.25j, 0.0], [0.0, -0.125j]])), (np.array([3]), np.array([[-0.5j]]))]
    S = np.eye(n, dtype=complex)
    F = S - sL - sR
    for ix, b in probes:
        F[np.ix_(ix, ix)] -= b
    E = np.array([0.25, 1.75])
    engine.set_system(F, S)
    h = engine.sigma_const([sL, sR])
    try:
        with pytest.warns(RuntimeWarning, match="without a path"):
            R = engine.probe_response(h, E, probes)
        assert not np.any(engine.last_info)
        T = engine.transmission_matrix(h, E, probes)
        out = engine.gless_int_probes(h, 0, E, np.ones(2), probes)
        tot = engine.gless_int_probes(h, None, E, np.ones(2), probes)
    finally:
        engine.sigma_free(h)
    assert np.all(np.isnan(R)) and np.all(np.isnan(probe_response(T, 2)))
    assert np.isnan(out).any() and np.all(np.isfinite(tot))        # the total needs no solve


def test_refusals_and_empty_grid(engine):
    """check 9: as transmission_matrix -- a staged provider, C > 1024, invalid probe lists; an empty grid gives zeros"""
    c = tr.cases()[0]
    one = np.array([[-0.1j]])
    E = c.energies
    w = _weights(E.size)
    calls = (lambda h, pr: engine.probe_response(h, E, pr), lambda h, pr: engine.gless_int_probes(h, 0, E, w, pr),
             lambda h, pr: engine.gr_int_probes(h, E, w, pr))
    with _Const(engine, c) as h:
        for call in calls:
            for bad in ([([c.n], one)], [([-1], one)], [([2, 2], np.zeros((2, 2)))], [([], np.zeros((0, 0)))],
                        [([1, 2], one)], [([1.5], one)]):
                with pytest.raises(ValueError):
                    call(h, bad)
            with pytest.raises(NotImplementedError):       # C > 1024
                call(h, [([q % c.n], one) for q in range(1021)])
        pr = [([3], one)]
        assert engine.probe_response(h, np.zeros(0), pr).shape == (0, 1, 4)
        assert not np.any(engine.gless_int_probes(h, 0, np.zeros(0), np.zeros(0), pr))
        assert not np.any(engine.gr_int_probes(h, np.zeros(0), np.zeros(0), pr))
        from gaunegf_amd._lib import NegfError
        for bad in (4, 7, -5):                             # an invalid contact index: the error gless_int raises for it
            with pytest.raises(NegfError, match="contact index"):
                engine.gless_int_probes(h, bad, E, w, pr)
        with pytest.raises(NegfError):
            engine.gless_int(h, 7, E, w)
    n = c.n
    sig = [np.zeros((n, n), complex), np.zeros((n, n), complex)]
    sig[0][0, 0] = -0.1j; sig[1][n - 1, n - 1] = -0.1j
    engine.set_system(c.F, c.S)
    h = engine.sigma_precomputed(np.stack([sig[0] + sig[1]] * E.size), np.stack([np.stack(sig)] * E.size))
    try:
        for call in calls:
            with pytest.raises(NotImplementedError, match="orbital lists"):
                call(h, [([3], one)])
    finally:
        engine.sigma_free(h)


def test_uniform_chain_occupations_fall_monotonically(engine):
    """check 10: n = 20 nearest-neighbour chain, one-orbital contacts at the ends, 18 equal probes (gamma = 1.5), E = 0.1
    (mid band): with f_source = 1, f_drain = 0 the occupations R[:, 0] decrease from source to drain.  A condition, not a
    tolerance; dephase_ref.response satisfies it with steps of -0.107 ... -0.030 (at gamma <= 0.5 it does not: the
    coherent oscillations survive)."""
    n, gam, E = 20, 1.5, 0.1
    F = np.zeros((n, n), complex)
    for i in range(n - 1):
        F[i, i + 1] = F[i + 1, i] = -1.0
    S = np.eye(n, dtype=complex)
    sL = np.zeros((n, n), complex); sL[0, 0] = -0.5j
    sR = np.zeros((n, n), complex); sR[n - 1, n - 1] = -0.5j
    probes = [(np.array([q]), np.array([[-0.5j * gam]])) for q in range(1, n - 1)]
    terms = [(np.array([0]), sL[:1, :1]), (np.array([n - 1]), sR[-1:, -1:])] + probes
    ref = dr.response(tr.tmatrix(F, S, terms, E), 2)
    assert np.all(np.diff(ref[:, 0]) < 0)                  # the reference alone
    engine.set_system(F, S)
    h = engine.sigma_const([sL, sR])
    try:
        R = engine.probe_response(h, [E], probes)[0]
    finally:
        engine.sigma_free(h)
    occ = R @ np.array([1.0, 0.0])
    print(f"dephase chain: occupations {occ[0]:.4f} ... {occ[-1]:.4f}, steps {np.diff(occ).min():.3g} ... {np.diff(occ).max():.3g}")
    assert np.all(np.diff(occ) < 0) and 0 < occ[-1] < occ[0] < 1


def test_bethe_provider(engine):
    """shape (e): the set-up of test_tmatrix_gpu.test_bethe_provider_and_refusals; R against the host solve of the
    restatement's T, and (I1) on the device's own sums"""
    from gaunegf_amd.surfGBethe import read_bethe_params, construct_sk_matrix, gen_neighbors
    from gaunegf_amd.transport import probe_response
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaunegf_amd", "data", "Au")
    ne, Ed, Vd, Sd, H0 = read_bethe_params(here)
    dirs = gen_neighbors(np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.2, 0.0]))
    Sl = np.array([construct_sk_matrix(Sd, d) for d in dirs]); Vl = np.array([construct_sk_matrix(Vd, d) for d in dirs])
    n = 45
    F, S = random_system(n, 17)
    F = F - 5.0 * S
    orbs = [[list(range(9))], [list(range(n - 18, n - 9)), list(range(n - 9, n))]]
    nbs = [[[0, 1, 2]], [[0, 1, 2], [6, 7, 8]]]
    inds = [list(range(9)), list(range(n - 18, n))]
    rng = np.random.default_rng(5)
    probes = [(np.asarray(ix), tr.sigma_block(len(ix), rng)) for ix in (list(range(9, 18)), [20], list(range(14, 23)))]
    E = np.linspace(-3.8, -2.6, 3)
    w = _weights(E.size)
    engine.set_system(F, S)
    h = engine.sigma_bethe(orbs, nbs, [H0, H0], [Sl, Sl], [Vl, Vl], None, 1e-4, 1e-8)
    try:
        sig = [engine.sigma_eval(h, k, E, 2) for k in range(2)]
        R = engine.probe_response(h, E, probes)
        outs = {s: engine.gless_int_probes(h, s, E, w, probes) for s in (0, 1, None)}
    finally:
        engine.sigma_free(h)
    Fc, Sc = F.astype(complex), S.astype(complex)
    ref = {s: 0 for s in outs}
    for k, e in enumerate(E):
        terms = [(np.asarray(ix), sig[q][k][np.ix_(ix, ix)]) for q, ix in enumerate(inds)] + list(probes)
        want = probe_response(tr.tmatrix_alt(Fc, Sc, terms, e)[None], 2)[0]
        print(f"dephase Bethe E={e:.6g}: R parity {_rel(R[k], want):.3g} (bar {BAR:g}), |row sums - 1| {np.abs(R[k].sum(axis=1) - 1).max():.3g}")
        assert _rel(R[k], want) <= BAR
        assert np.abs(R[k].sum(axis=1) - 1).max() <= 1e-10
        for s in outs:
            ref[s] = ref[s] + dr.gless_probes(Fc, Sc, terms, 2, s, [e], [w[k]])
    for s in outs:
        assert _rel(outs[s], ref[s]) <= BAR, s
    assert _rel(outs[0] + outs[1], outs[None]) <= 1e-10


# --------------------------------------------------------------------------- _dev forms, the untouched neighbour
def test_device_pointer_forms(engine):
    """check 11: the _dev forms return the host forms' bits"""
    C = ctypes
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    c = dr.shape_b()
    E = np.ascontiguousarray(c.energies, dtype=np.complex128)
    w = np.ascontiguousarray(_weights(E.size), dtype=np.complex128)
    R = np.zeros((E.size, len(c.probes), c.n_c))
    out = np.zeros((c.n, c.n), dtype=np.complex128)
    ptrs = [C.c_void_p() for _ in range(4)]
    dE, dw, dR, dout = ptrs
    for p, nbytes in zip(ptrs, (E.nbytes, w.nbytes, R.nbytes, out.nbytes)):
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
    try:
        with _Const(engine, c) as h:
            assert hip.hipMemcpy(dE, E.ctypes.data_as(C.c_void_p), E.nbytes, 1) == 0
            assert hip.hipMemcpy(dw, w.ctypes.data_as(C.c_void_p), w.nbytes, 1) == 0
            engine.probe_response_dev(h, E.size, dE.value, dR.value, c.probes)
            engine.sync()
            assert not np.any(engine.last_info_dev(E.size))
            assert hip.hipMemcpy(R.ctypes.data_as(C.c_void_p), dR, R.nbytes, 2) == 0
            assert np.array_equal(R, engine.probe_response(h, E, c.probes))
            for run, host in ((lambda: engine.gless_int_probes_dev(h, 1, E.size, dE.value, dw.value, dout.value, c.probes),
                               lambda: engine.gless_int_probes(h, 1, E, w, c.probes)),
                              (lambda: engine.gless_int_probes_dev(h, None, E.size, dE.value, dw.value, dout.value, c.probes),
                               lambda: engine.gless_int_probes(h, None, E, w, c.probes)),
                              (lambda: engine.gr_int_probes_dev(h, E.size, dE.value, dw.value, dout.value, c.probes),
                               lambda: engine.gr_int_probes(h, E, w, c.probes))):
                run()
                engine.sync()
                assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), dout, out.nbytes, 2) == 0
                assert np.array_equal(out, host())
    finally:
        for p in ptrs:
            hip.hipFree(p)


def test_transmission_matrix_bits_are_the_parent_commits(engine):
    """check 12: negf_transmission_matrix on shapes (a) and (d) against tests/golden/dephase_tmat_parent.npz, captured on an
    MI355X from the commit before the probe set-up moved into a helper"""
    gold = np.load(GOLDEN)
    a = dr.shape_a()
    with _Const(engine, a) as h:
        assert np.array_equal(engine.transmission_matrix(h, a.energies, a.probes), gold["a"])
    for solver in ("fixed-point", "doubling"):
        h, g = dr.lower_d(engine, solver)
        got = engine.transmission_matrix(h, dr.D_ENERGIES, dr.shape_d()[4])
        assert np.array_equal(got, gold["d_" + solver.replace("-", "_")]), solver


# --------------------------------------------------------------------------- front ends
def test_front_ends(engine):
    from gaunegf_amd.density import bias_window_grid, densityGridProbesN
    from gaunegf_amd.integrate import GrIntProbes, GrLessIntProbes
    from gaunegf_amd.surfGTester import surfGTest
    from gaunegf_amd.transport import (SigmaCalculator, calculate_probe_occupations, calculate_probe_response,
                                       dephasing_probes, probeOccupations)
    c = dr.shape_a()
    N = c.n
    F, S = np.real(c.F), np.real(c.S)
    ci = [list(range(4)), list(range(N - 4, N))]
    g = surfGTest(F, S, ci, -0.25j)
    probes = dephasing_probes(S, [[6, 7], [7, 8, 9], [12]], [0.3, 0.5, 0.0])
    E = np.linspace(-1.0, 1.0, 5)
    w = _weights(E.size)
    engine.set_system(F, S)
    h = g._negf_lower(engine)
    for ind in (0, -1, None):
        assert np.array_equal(GrLessIntProbes(F, S, g, E, w, probes, ind), engine.gless_int_probes(h, ind, E, w, probes))
    assert np.array_equal(GrIntProbes(F, S, g, E + 0.1j, w, probes), engine.gr_int_probes(h, E + 0.1j, w, probes))
    grid, wts = bias_window_grid(-0.2, 0.3, 12, 0.0)
    den = densityGridProbesN(F, S, g, -0.2, 0.3, probes, ind=0, N=12, T=0.0)
    assert np.array_equal(den, engine.gless_int_probes(h, 0, grid, wts, probes) / (2 * np.pi))
    # the spin-diagonal split: the probes on the N orbitals of each block
    Z = np.zeros((N, N))
    Fb = F + 0.1 * np.diag(np.cos(np.arange(N)))
    F2 = np.block([[F, Z], [Z, Fb]]); S2 = np.block([[S, Z], [Z, S]])
    g2 = surfGTest(F2, S2, [ci[0] + [N + i for i in ci[0]], ci[1] + [N + i for i in ci[1]]], -0.25j)
    assert g2._negf_spin_split(N) is not None
    both = GrLessIntProbes(F2, S2, g2, E, w, probes, 0)
    gb = surfGTest(Fb, S, ci, -0.25j)
    assert _rel(both[:N, :N], GrLessIntProbes(F, S, g, E, w, probes, 0)) <= 1e-12
    assert _rel(both[N:, N:], GrLessIntProbes(Fb, S, gb, E, w, probes, 0)) <= 1e-12
    assert not np.any(both[:N, N:])

    class Foreign:
        def sigmaTot(self, E):
            return np.zeros((N, N), complex)
    with pytest.raises(NotImplementedError):
        GrLessIntProbes(F, S, Foreign(), E, w, probes)
    # responses and occupations
    sc = SigmaCalculator(g)
    R = calculate_probe_response(F, S, sc, E, probes)
    assert np.array_equal(R, engine.probe_response(g._negf_lower(engine), E, probes))
    assert not np.any(R[:, 2])                             # the gamma = 0 probe
    for T in (0.0, 300.0):
        occ = calculate_probe_occupations(F, S, sc, E, probes, 0.1, 0.4, T=T)
        assert occ.shape == (E.size, 3) and occ.min() >= 0 and occ.max() <= 1 + 1e-12
    inside = np.abs(E - 0.1) < 0.2                         # T = 0: f_L = 1, f_R = 0 inside the window, both 1 below it
    occ = calculate_probe_occupations(F, S, sc, E, probes, 0.1, 0.4, T=0.0)
    assert np.array_equal(occ[inside], R[inside][:, :, 0])
    assert np.abs(occ[E < -0.1][:, :2] - 1).max() <= 1e-10
    sig = c.contact_sigmas()
    st = SigmaCalculator(sig[0], sig[1])
    assert np.array_equal(probeOccupations(E, c.F, c.S, sig[0], sig[1], c.probes, 0.1, 0.4),
                          calculate_probe_occupations(c.F, c.S, st, E, c.probes, 0.1, 0.4))
    with pytest.raises(NotImplementedError):
        calculate_probe_response(np.kron(np.real(c.F), np.eye(2)), np.kron(np.real(c.S), np.eye(2)), st, E, None, spin='g')
