"""
The renormalisation-decimation ("doubling") solver of the 1-D chain surface Green's function on the GPU
(negf_sigma_chain1d_rd, k_chain1d_rd.hip), through the public Python API:
  * accuracy of g (identity-tau read-back) and Sigma against the extended-precision truth at the bar of
    tests/xprec_rd.py -- every size of the chain accuracy tests (both kernels), the leads L1 / L2 and their 2^+-64
    scalings at eta in {1e-4, 1e-6}, three energies each, free running and at 0, 1 and 3 steps;
  * step counts (the float64 restatement's +- 1), convergence flags, max_steps, NaN input;
  * bitwise scale equivariance;
  * agreement with the default solver where that one converges;
  * GrInt / GrLessInt / transmission / DOS / eigenchannels with solver='doubling' against the oracle integrals fed by
    a host provider that returns the float64 restatement's Sigma (the project's parity bar, 1e-8);
  * the g(E) cache never serves one solver's entry to the other; a hit equals its miss bit for bit;
  * the keyword itself.
Each line 'ACC ...' printed reports the worst ratio error / bar of one size.
"""
import functools

import numpy as np
import pytest

import oracle
import xprec
import xprec_chain as xc
import xprec_rd as xr
from helpers import chain_lead, random_system, rel_fro
from test_chain_accuracy_gpu import GLOBAL_SIZES, LDS_SIZES

pytestmark = pytest.mark.gpu

xprec.require_extended()

TOL = 1e-8
KS = (None,) + xr.K_FIXED


def _dev(lead, solver="doubling", K=None):
    from gaunegf_amd.surfG1D import surfG
    n = lead.n
    g = surfG(np.zeros((n, n)), np.eye(n), [list(range(n))], eta=lead.eta, solver=solver, **lead.kwargs())
    g.force_iters = -1 if K is None else K
    return g


@functools.lru_cache(maxsize=None)
def _table(n):
    """[(base lead, [(E, truth, {K: bar})])] of size n; the truths are built once per module, on xprec.pmap."""
    leads = xr.leads(n)
    flat = [(li, complex(E)) for li, lead in enumerate(leads) for E in lead.energies]
    built = xprec.pmap(lambda c: xr.build(leads[c[0]], c[1]), flat)
    out = [(lead, []) for lead in leads]
    for (li, E), (t, bars) in zip(flat, built):
        out[li][1].append((E, t, bars))
    return out


# --------------------------------------------------------------------------- #
# accuracy, step counts and flags
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n", LDS_SIZES + GLOBAL_SIZES)
def test_rd_accuracy_against_truth(engine, n):
    fails, worst = [], 0.0
    for base, rows in _table(n):
        for k in (0, 64, -64):
            lead = base if k == 0 else xc.scaled(base, k)
            f = 2.0 ** k
            Es = np.array([E * f for E, _, _ in rows])
            for K in KS:
                dev = _dev(lead, K=K)
                sig, its, cv = dev.sigma_batch(Es)
                for m, (E, t, bars) in enumerate(rows):
                    tv = t if k == 0 else xr.RdTruth.of(lead, t)
                    b = bars[K]
                    rg = b.g_ratio(dev.g(Es[m], 0), tv)
                    rs = b.sigma_ratio(sig[m], tv)
                    worst = max(worst, rg, rs)
                    tag = (lead.name, lead.eta, complex(Es[m]), K)
                    if not (rg <= 1.0 and rs <= 1.0):
                        fails.append(tag + (rg, rs))
                    if K is None:
                        if abs(int(its[m, 0]) - b.steps_numpy) > 1 or int(cv[m, 0]) != 1:
                            fails.append(tag + ("steps", int(its[m, 0]), b.steps_numpy, int(cv[m, 0])))
                    elif int(its[m, 0]) != K:
                        fails.append(tag + ("forced steps", int(its[m, 0])))
    print(f"ACC chain rd {'lds' if n <= 64 else 'global'} n={n}: worst ratio {worst:.3g}")
    assert not fails, fails[:10]


@pytest.mark.parametrize("n", (17, 50, 80))
def test_rd_max_steps_and_nan(engine, n):
    lead = xc.lead_l1(n)
    dev = _dev(lead)
    dev.doubling_max_steps = 3
    sig, its, cv = dev.sigma_batch([0.3])
    assert int(its[0, 0]) == 3 and int(cv[0, 0]) == 0 and np.all(np.isfinite(sig))
    # ... and that is the state after three steps
    ref = _dev(lead, K=3).sigma_batch([0.3])[0]
    assert np.array_equal(sig, ref)
    bad = xc.lead_l1(n)
    bad.alpha = bad.alpha.copy(); bad.alpha[1, 2] = np.nan
    sig, its, cv = _dev(bad).sigma_batch([0.3, 0.2 + 0.3j])
    assert np.all(np.isnan(sig.real) | np.isnan(sig.imag)) and np.all(cv == 0)


@pytest.mark.parametrize("n", (17, 50, 80))
def test_rd_scale_equivariance_bitwise(engine, n):
    """alpha, beta, tau, E, eta -> 2^k times themselves: exactly 2^-k g and 2^k Sigma, the same steps and flags."""
    for base in (xc.lead_l1(n), xc.lead_l2(n)):
        for K in KS:
            d0 = _dev(base, K=K)
            s0, i0, c0 = d0.sigma_batch(base.energies)
            g0 = [d0.g(E, 0) for E in base.energies]
            for k in (64, -64):
                lead = xc.scaled(base, k)
                d1 = _dev(lead, K=K)
                s1, i1, c1 = d1.sigma_batch(lead.energies)
                assert np.array_equal(s1, s0 * 2.0 ** k), (base.name, K, k)
                assert np.array_equal(i1, i0) and np.array_equal(c1, c0), (base.name, K, k)
                for m, E in enumerate(lead.energies):
                    assert np.array_equal(d1.g(E, 0), g0[m] * 2.0 ** -k), (base.name, K, k, m)


@pytest.mark.parametrize("n", (17, 50))
def test_rd_agrees_with_fixed_point_where_that_converges(engine, n):
    """Where the default solver reports converged = 1, || Sigma_fp - Sigma_rd || <= 2 x the distance of the float64
    oracle's fixed point (conv = 1e-5) from the truth at that energy."""
    checked = 0
    for eta in (1e-4, 1e-2):
        lead = xc.lead_l1(n, eta=eta)
        Es = np.concatenate([lead.energies, [0.2 + 0.05j, -0.4 + 0.1j, 0.9]])
        s_fp, _, c_fp = _dev(lead, solver="fixed-point").sigma_batch(Es)
        s_rd, _, c_rd = _dev(lead).sigma_batch(Es)
        assert np.all(c_rd == 1)
        for m, E in enumerate(Es):
            if int(c_fp[m, 0]) != 1:
                continue
            t = xr.RdTruth(lead, complex(E), ks=())
            g_or, _, _ = oracle.chain1d_g(complex(E), lead.alpha, lead.Salpha, lead.beta, lead.Sbeta, lead.eta)
            dist = t.sigma_err_abs(oracle.chain1d_sigma_block(complex(E), lead.tau, lead.Stau, g_or))
            diff = float(np.linalg.norm(s_fp[m] - s_rd[m]))
            print(f"RD vs fixed point n={n} eta={eta:g} E={complex(E):.3g}: {diff:.3g} against 2 x {dist:.3g}")
            assert diff <= 2.0 * dist, (eta, E, diff, dist)
            checked += 1
    assert checked >= 4


# --------------------------------------------------------------------------- #
# integrals
# --------------------------------------------------------------------------- #
class _HostRd:
    """Host provider with the reference's protocol whose Sigma is the float64 restatement's."""

    def __init__(self, F, leads, inds):
        self.F, self.leads, self.inds = F, leads, inds

    def sigma(self, E, i, conv=None):
        out = np.zeros(self.F.shape, dtype=complex)
        ix = self.inds[i]
        out[np.ix_(ix, ix)] += xr.rd64(self.leads[i], complex(E))[1]
        return out

    def sigmaTot(self, E, conv=None):
        return self.sigma(E, 0) + self.sigma(E, 1)


def test_rd_integrals_against_oracle(engine):
    from gaunegf_amd.integrate import GrInt, GrLessInt
    from gaunegf_amd.surfG1D import surfG
    from gaunegf_amd.transport import (SigmaCalculator, calculate_dos, calculate_transmission,
                                       calculate_transmission_channels)
    N, nc, eta = 120, 20, 1e-4
    F, S = random_system(N, 3)
    inds = [list(range(nc)), list(range(N - nc, N))]
    aL, aR = chain_lead(nc, 31), chain_lead(nc, 32)
    kw = dict(taus=[aL[2].copy(), aR[2].copy()], staus=[aL[3].copy(), aR[3].copy()], alphas=[aL[0], aR[0]],
              aOverlaps=[aL[1], aR[1]], betas=[aL[2], aR[2]], bOverlaps=[aL[3], aR[3]], eta=eta)
    g = surfG(F, S, inds, solver="doubling", **kw)
    ref = _HostRd(F, [xc.Lead("L", a[0], a[1], a[2], a[3], a[2], a[3], [], eta=eta) for a in (aL, aR)], inds)
    E, w = oracle.bias_window_grid(-0.3, 0.3, 24, 300.0)
    assert rel_fro(GrInt(F, S, g, E, w), oracle.GrInt(F, S, ref, E, w)) < TOL
    for ind in (None, 0):
        assert rel_fro(GrLessInt(F, S, g, E, w, ind), oracle.GrLessInt(F, S, ref, E, w, ind)) < TOL
    sc = SigmaCalculator(g)
    T = calculate_transmission(F, S, sc, E)
    dos, site = calculate_dos(F, S, sc, E)[:2]
    Tn = calculate_transmission_channels(F, S, sc, E)
    for k, e in enumerate(E):
        s0, s1 = ref.sigma(e, 0), ref.sigma(e, 1)
        st = s0 + s1
        Tr = oracle.transmission_restricted(e, F, S, st, 1j * (s0 - s0.conj().T), 1j * (s1 - s1.conj().T))
        assert abs(T[k] - Tr) < TOL * max(1.0, abs(Tr))
        assert abs(Tn[k].sum() - Tr) < TOL * max(1.0, abs(Tr))
        dr, sr = oracle.dos_kernel(e, F, S, st)
        assert abs(dos[k] - dr) < TOL * max(1.0, abs(dr))
        assert rel_fro(site[k], sr) < TOL
    assert np.all(np.abs(Tn.sum(axis=1) - T) <= 1e-11 * np.maximum(np.abs(T), 1e-3))
    sig, its, cv = g.sigma_batch(E)
    assert np.all(cv == 1) and its.max() <= 30


@pytest.mark.parametrize("ncL,ncR,M", [(50, 40, 5), (19, 9, 5), (64, 3, 5), (20, 12, 700), (80, 17, 5)])
def test_rd_unequal_contacts_and_more_units_than_slots(engine, ncL, ncR, M):
    """Contacts of unequal size share a launch (the padded workspace of a slot is re-zeroed when the size changes), and a
    launch with more units than resident slots (700 energies x 2 contacts) walks them slot by slot: Sigma of both contacts
    against the float64 restatement, step counts +- 1."""
    from gaunegf_amd.surfG1D import surfG
    N, eta = ncL + ncR + 7, 1e-4
    F, S = random_system(N, 5)
    inds = [list(range(ncL)), list(range(N - ncR, N))]
    aL, aR = chain_lead(ncL, 41), chain_lead(ncR, 42)
    kw = dict(taus=[aL[2].copy(), aR[2].copy()], staus=[aL[3].copy(), aR[3].copy()], alphas=[aL[0], aR[0]],
              aOverlaps=[aL[1], aR[1]], betas=[aL[2], aR[2]], bOverlaps=[aL[3], aR[3]], eta=eta)
    g = surfG(F, S, inds, solver="doubling", **kw)
    leads = [xc.Lead("L", a[0], a[1], a[2], a[3], a[2], a[3], [], eta=eta) for a in (aL, aR)]
    E = np.linspace(-1.5, 1.5, M)
    sample = range(M) if M <= 8 else (0, 1, M // 3, M // 2, M - 2, M - 1)
    for c in (0, 1):
        sig, its, cv = g.sigma_batch(E, c)
        assert np.all(cv == 1)
        for m in sample:
            ref, steps = xr.rd64(leads[c], complex(E[m]))[1:3]
            blk = sig[m][np.ix_(inds[c], inds[c])]
            assert rel_fro(blk, ref) < TOL, (c, m, rel_fro(blk, ref))
            assert abs(int(its[m, c]) - steps) <= 1
            rest = sig[m].copy(); rest[np.ix_(inds[c], inds[c])] = 0
            assert not rest.any()


# --------------------------------------------------------------------------- #
# cache and keyword
# --------------------------------------------------------------------------- #
@pytest.fixture
def cache(engine):
    engine.set_chain_cache(0)
    engine.set_chain_cache(512)
    yield engine
    engine.set_chain_cache(0)
    engine.set_chain_cache(512)


def test_rd_cache_is_keyed_on_the_solver(cache):
    lead = xc.lead_l1(33)
    E = np.linspace(-1.0, 1.0, 7) + 0.0j
    s = lambda: (cache.chain_cache_stats()["hits"], cache.chain_cache_stats()["misses"])
    h0, m0 = s()
    fp = _dev(lead, solver="fixed-point").sigma_batch(E)
    assert s() == (h0, m0 + 1)
    rd = _dev(lead).sigma_batch(E)
    assert s() == (h0, m0 + 2)                       # the fixed-point entry was not served to the doubling provider
    fp2 = _dev(lead, solver="fixed-point").sigma_batch(E)
    rd2 = _dev(lead).sigma_batch(E)
    assert s() == (h0 + 2, m0 + 2)                   # each finds its own
    for a, b in ((fp, fp2), (rd, rd2)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert not np.array_equal(fp[1], rd[1])          # (sweep counts against step counts)
    d3 = _dev(lead); d3.doubling_max_steps = 3
    d3.sigma_batch(E)
    assert s() == (h0 + 2, m0 + 3)                   # another max_steps: another entry
    dk = _dev(lead, K=2)
    dk.sigma_batch(E)
    assert s() == (h0 + 2, m0 + 4)                   # ... and another for a fixed step count


def test_rd_keyword(engine):
    from gaunegf_amd import config
    from gaunegf_amd.surfG1D import surfG
    lead = xc.lead_l1(17)
    n = lead.n
    args = (np.zeros((n, n)), np.eye(n), [list(range(n))])
    with pytest.raises(ValueError):
        surfG(*args, eta=lead.eta, solver="bogus", **lead.kwargs())
    g = surfG(*args, eta=lead.eta, **lead.kwargs())
    assert g.solver == config.SURFACE_GREEN_SOLVER == "fixed-point"
    with pytest.raises(ValueError):
        g.solver = "bogus"
    E = lead.energies
    s_default = g.sigma_batch(E)
    s_fp = surfG(*args, eta=lead.eta, solver="fixed-point", **lead.kwargs()).sigma_batch(E)
    for x, y in zip(s_default, s_fp):
        assert np.array_equal(x, y)
    g.solver = "doubling"                            # settable afterwards: a new lowering
    s_rd = g.sigma_batch(E)
    s_rd2 = surfG(*args, eta=lead.eta, solver="doubling", **lead.kwargs()).sigma_batch(E)
    for x, y in zip(s_rd, s_rd2):
        assert np.array_equal(x, y)
    assert s_rd[1].max() < 30 and not np.array_equal(s_rd[1], s_default[1])
    with pytest.raises(ValueError):
        engine.sigma_chain1d([list(range(n))], [lead.alpha], [lead.Salpha], [lead.beta], [lead.Sbeta], [lead.tau],
                             [lead.Stau], lead.eta, 1e-5, 0.1, solver="bogus")
