"""
The chain fixed point's extended-precision truth and first-order bar (tests/xprec_chain.py) on the CPU: the lead case
table is built exactly, the float64 oracle (oracle.chain1d_g / chain1d_sigma_block: LAPACK and BLAS) meets the bar
with half its constant, and planted defects of the chain kernels miss it by at least 10x: the stored P - E pivot row
with its +1 read-back, B g B^H summed in complex64, one sweep too few.  Lines 'CAL ...' / 'DEFECT ...' report the worst
ratios error / bar.

The first-order bound multiplies by (1 - r) + r ||h B||_2 ||B^H h||_2 per sweep.  On the real energies of these leads
(eta = 1e-4) that factor is 10 ... 300, so the bound grows past MAX_GROWTH = 1e3 after one to three sweeps and only those
K are checked there (xprec_chain.checked_k); the complex energy keeps K = 10.  Where it is checked the bar is loose by
orders of magnitude for errors that build up over sweeps, which is why the defects that a sweep cannot hide -- a
pivot row that loses its bits, a product in single precision -- are planted, and why the GPU module adds bitwise
scale equivariance.
"""
import functools

import numpy as np
import pytest

import oracle
import xprec
import xprec_chain as xc
from xprec import C_BAR

SIZES = (9, 50, 80)
KMAX = 10


def test_long_double_is_extended():
    xprec.require_extended()


@functools.lru_cache(maxsize=None)
def _leads(n):
    l1 = xc.lead_l1(n)
    return [l1, xc.lead_l2(n), xc.scaled(l1, 64), xc.scaled(l1, -64)]


@functools.lru_cache(maxsize=None)
def _truths(n):
    """{(lead name, energy index): (lead, truth)} at n; the L3 truths derived from L1's exactly."""
    out, base = {}, {}
    for lead in _leads(n):
        for m, E in enumerate(lead.energies):
            if lead.base is None:
                base[(lead.name, m)] = t = xc.ChainTruth(lead, E, KMAX)
            else:
                t = xc.ChainTruth.of(lead, base[(lead.base.name, m)])
            out[(lead.name, m)] = (lead, t)
    return out


def _ks(t):
    return xc.checked_k(t, KMAX)


def test_cases_are_exact():
    """The L3 inputs are bitwise 2^k times L1's (overlaps unchanged), so A, B and t are too, in float64."""
    for n in (9, 50):
        l1 = xc.lead_l1(n)
        for k in (64, -64):
            s = xc.scaled(l1, k)
            f = 2.0 ** k
            for a, b in ((s.alpha, l1.alpha), (s.beta, l1.beta), (s.tau, l1.tau)):
                assert np.array_equal(a, f * b) and np.array_equal(a / f, b)
            for a, b in ((s.Salpha, l1.Salpha), (s.Sbeta, l1.Sbeta), (s.Stau, l1.Stau)):
                assert np.array_equal(a, b)
            assert np.array_equal(s.energies, f * l1.energies) and s.eta == f * l1.eta
            for E0, E in zip(l1.energies, s.energies):
                assert np.array_equal(s.A64(E), f * l1.A64(E0))
                assert np.array_equal(s.B64(E), f * l1.B64(E0))
                assert np.array_equal(s.t64(E), f * l1.t64(E0))


def test_l2_core_levels_and_edge_energy():
    """L2 differs from L1 by the core levels only; the edge energy is a grid point of the 200-point grid."""
    l1, l2 = _leads(50)[:2]
    d = l2.alpha - l1.alpha
    core = np.arange(2, 50, 5)
    assert np.allclose(np.diag(d)[core], np.logspace(2, 4, core.size)) and np.count_nonzero(d) == core.size
    assert l1.energies[2].real in xc.EDGE_GRID


def test_truth_iterates_match_oracle_loosely():
    """The clongdouble iterates are the oracle's fixed point: chain1d_g at force_iters = K agrees to 1e-8."""
    lead, t = _truths(9)[("L1", 0)]
    for K in (0, 1, 5):
        g, _, _ = oracle.chain1d_g(t.E, lead.alpha, lead.Salpha, lead.beta, lead.Sbeta, lead.eta, force_iters=K)
        ref = t.g[K].astype(np.complex128)
        assert np.linalg.norm(g - ref) <= 1e-8 * np.linalg.norm(ref), K


@pytest.mark.parametrize("n", SIZES)
def test_calibration_oracle(n):
    """The float64 oracle meets the bar with c = C_BAR / 2 on every lead, energy and usable K, g and Sigma."""
    worst = {}
    for (name, m), (lead, t) in _truths(n).items():
        ks = _ks(t)
        assert ks and ks[0] == 0
        for K in ks:
            g, count, _ = oracle.chain1d_g(t.E, lead.alpha, lead.Salpha, lead.beta, lead.Sbeta, lead.eta, force_iters=K)
            assert count == K
            S = oracle.chain1d_sigma_block(t.E, lead.tau, lead.Stau, g)
            r = max(t.g_ratio(K, g), t.sigma_ratio(K, S)) * C_BAR / (C_BAR / 2)
            worst[name] = max(worst.get(name, 0.0), r)
        print(f"CAL oracle n={n} {name} E={t.E:.4g} usable K={ks[-1]} growth={t.growth[ks[-1]]:.3g}")
    for name, r in worst.items():
        print(f"CAL oracle n={n} {name}: worst ratio at c = C_BAR/2 {r:.3g}")
    assert max(worst.values()) <= 1.0, worst


def _defect_ratio(n, which):
    """{lead name: worst error / bar} of one planted defect over energies and usable K."""
    out = {}
    for (name, m), (lead, t) in _truths(n).items():
        for K in _ks(t):
            if which == "phat":
                g, S = xc.chain64(lead, t.E, K, inv=xc.gauss_jordan_phat)
            elif which == "c64":
                g, S = xc.chain64(lead, t.E, K, prod=xc.prod_c64)
            else:
                if K == 0:
                    continue
                g, S = xc.chain64(lead, t.E, K - 1)
            out[name] = max(out.get(name, 0.0), t.g_ratio(K, g), t.sigma_ratio(K, S))
    return out


@pytest.mark.parametrize("n", [9, 50])
def test_defect_phat_pivot_row_fails_on_l3(n):
    """The stored P - E pivot row (pivot row formed as q + (1/p - 1) q, read back as (x - 1) + 1) misses the bar by at
    least 10x on L1 x 2^64, whose pivots are ~2^64: 1/p - 1 rounds to -1 and the row cancels to nothing.  The same
    emulation on the unscaled leads stays within the bar -- the C3 leads lose 2-3 bits."""
    r = _defect_ratio(n, "phat")
    for name, v in r.items():
        print(f"DEFECT P-E pivot row n={n} {name}: worst ratio {v:.3g}")
    assert r["L1x2^64"] >= 10.0, r
    assert r["L1"] <= 1.0, r


@pytest.mark.parametrize("n", [9, 50])
def test_defect_complex64_product(n):
    """B g B^H summed in complex64 misses the bar by at least 10x."""
    r = _defect_ratio(n, "c64")
    for name, v in r.items():
        print(f"DEFECT complex64 B g B^H n={n} {name}: worst ratio {v:.3g}")
    assert max(r.values()) >= 10.0, r


@pytest.mark.parametrize("n", [9, 50])
def test_defect_one_sweep_short(n):
    """K - 1 sweeps against the truth of K misses the bar by at least 10x."""
    r = _defect_ratio(n, "short")
    for name, v in r.items():
        print(f"DEFECT one sweep too few n={n} {name}: worst ratio {v:.3g}")
    assert max(r.values()) >= 10.0, r


def test_phat_emulation_is_gauss_jordan_at_unit_scale():
    """The P - E emulation is an inverse (to 1e-12) at unit scale and loses the pivot rows at 2^64: the defect is the
    stored form, not the elimination."""
    rng = np.random.default_rng(3)
    A = rng.standard_normal((50, 50)) + 1j * rng.standard_normal((50, 50)) + 3 * np.eye(50)
    R = np.linalg.inv(A)
    assert np.linalg.norm(xc.gauss_jordan_phat(A) - R) <= 1e-12 * np.linalg.norm(R)
    G = xc.gauss_jordan_phat(A * 2.0 ** 64) * 2.0 ** 64
    assert np.linalg.norm(G - R) >= 0.1 * np.linalg.norm(R)
