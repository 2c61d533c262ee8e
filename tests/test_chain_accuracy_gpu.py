"""
Accuracy of the 1-D chain self-energy kernels (chain1d_rs_kernel for n_c <= 64, chain1d_kernel above or with
NEGF_CHAIN1D_ALGO=global) against extended-precision truths:
  * their inverse alone on the G1-G4 case table of tests/xprec.py (force_iters = 0, S_alpha = 0, alpha = -A: the kernel
    forms A = z 0 - alpha = A exactly and returns g_0 = A^-1), per column within the conditioning bar plus the
    read-back term xprec_chain.READBACK_U;
  * K sweeps of the fixed point on the leads L1 / L2 of tests/xprec_chain.py, g and Sigma within the propagated
    first-order bar (K where the bound's growth stays below 1e3, see test_chain_accuracy_host.py);
  * exact scale equivariance: alpha, beta, tau, E, eta -> 2^k times themselves give 2^-k g and 2^k Sigma bit for bit,
    at a fixed sweep count (k = +-64) and free running (k = +-8, the same sweep counts and flags).
Each line 'ACC ...' printed reports the worst ratio error / bar of one kernel x case.
"""
import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import xprec
import xprec_chain as xc
from xprec import LD, Truth

pytestmark = pytest.mark.gpu

xprec.require_extended()

LDS_SIZES = (9, 17, 33, 49, 50, 51, 63, 64)      # every pitch class of the LDS kernel and its remainder strips
GLOBAL_SIZES = (65, 80)
SWEEP_SIZES = (9, 33, 50, 64, 65, 80)
KMAX = 10


def _one_contact(n, lead_kw, eta, force_iters):
    from gaunegf_amd.surfG1D import surfG
    g = surfG(np.zeros((n, n)), np.eye(n), [list(range(n))], eta=eta, **lead_kw)
    g.force_iters = force_iters
    return g


def _report(what, ratios):
    print(f"ACC {what}: worst ratio {max(ratios):.3g}")


# --------------------------------------------------------------------------- #
# a. the chain kernels' inverse on the case table
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _inverse_truths(n):
    """{case name: (case, truth of the inverse of the float64 A64(E) the kernel is given)}."""
    out, base = {}, {}
    for c in xprec.case_table(n):
        if c.base is None:
            t = Truth.__new__(Truth)
            t.case, t.cols = c, np.arange(n)
            t.kappa = np.array([xprec.kappa2(c.A64(E)) for E in c.energies])
            res = xprec.refine([(c.A64(E).astype(LD), t.cols) for E in c.energies],
                               [max(1e-3 * xprec.bar(n, k, 1.0), 2.0 ** -58) for k in t.kappa])
            t.G = np.stack([r[0] for r in res])
            t.last_correction = np.array([r[1] for r in res])
            base[c.name] = t
        else:
            t = Truth.of(c, base[c.base.name])
        out[c.name] = (c, t)
    return out


def inverse_ratios(n):
    """{case name: worst column error / (C_BAR sqrt(n) u kappa_2 + READBACK_U)} of g_0 = A^-1 from the chain kernel."""
    zero = np.zeros((n, n))
    out = {}
    for name, (case, t) in _inverse_truths(n).items():
        ratios = []
        for m, E in enumerate(case.energies):
            A = case.A64(E)
            kw = dict(taus=[-np.eye(n)], staus=[zero], alphas=[-A], aOverlaps=[zero], betas=[zero], bOverlaps=[zero])
            g = _one_contact(n, kw, 1e-4, 0).g(0.0, 0)
            ratios.append(float(np.max(t.column_errors(m, g)) / (t.delta(m) + xc.READBACK_U)))
        out[name] = max(ratios)
    return out


@pytest.mark.parametrize("n", LDS_SIZES + GLOBAL_SIZES)
def test_chain_inverse_on_case_table(engine, n):
    """g_0 = A^-1 of the LDS kernel (n <= 64) and the global kernel (65, 80): every column within the bar."""
    r = inverse_ratios(n)
    kern = "lds" if n <= 64 else "global"
    for name, v in r.items():
        _report(f"chain inverse {kern} n={n} {name}", [v])
    assert max(r.values()) <= 1.0, r


def test_chain_inverse_forced_global(engine):
    """n = 17 and 50 through the global kernel (NEGF_CHAIN1D_ALGO=global is read once per process: a child)."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        from test_chain_accuracy_gpu import inverse_ratios
        worst = 0.0
        for n in (17, 50):
            for name, v in inverse_ratios(n).items():
                print(f"ACC chain inverse forced-global n={n} {name}: worst ratio {v:.3g}")
                worst = max(worst, v)
        print("ok" if worst <= 1.0 else "FAIL")
    """) % (os.path.dirname(here), here)
    env = dict(os.environ, NEGF_CHAIN1D_ALGO="global")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout, end="")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])


# --------------------------------------------------------------------------- #
# b. K sweeps against the propagated bar
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _leads(n):
    return [xc.lead_l1(n), xc.lead_l2(n)]


@pytest.mark.parametrize("n", SWEEP_SIZES)
def test_chain_sweeps_against_bar(engine, n):
    """g_K (read back through the identity-tau variant) and Sigma_K = t g_K t^H after K sweeps within the bar, for
    K in {1, 3, 10} and the last K <= 10 whose bound growth stays below MAX_GROWTH (fewer on the real energies)."""
    fails, worst = [], {}
    for lead in _leads(n):
        for E in lead.energies:
            t = xc.ChainTruth(lead, E, KMAX)
            ks = xc.checked_k(t, KMAX)
            for K in ks:
                dev = _one_contact(n, lead.kwargs(), lead.eta, K)
                rg = t.g_ratio(K, dev.g(E, 0), xc.READBACK_U)
                rs = t.sigma_ratio(K, dev.sigma(E, 0))
                worst[lead.name] = max(worst.get(lead.name, 0.0), rg, rs)
                if not (rg <= 1.0 and rs <= 1.0):
                    fails.append((lead.name, complex(E), K, rg, rs))
    kern = "lds" if n <= 64 else "global"
    for name, v in worst.items():
        _report(f"chain sweeps {kern} n={n} {name}", [v])
    assert not fails, fails


# --------------------------------------------------------------------------- #
# c. exact scale equivariance
# --------------------------------------------------------------------------- #
def _g_sigma(lead, force_iters):
    n = lead.n
    dev = _one_contact(n, lead.kwargs(), lead.eta, force_iters)
    g = np.stack([dev.g(E, 0) for E in lead.energies])
    sig, its, cv = dev.sigma_batch(lead.energies, 0)
    return g, sig, its, cv


@pytest.mark.parametrize("n", [17, 50, 80])
@pytest.mark.parametrize("force_iters", [0, 40])
@pytest.mark.parametrize("k", [64, -64])
def test_chain_scale_equivariance_fixed(engine, n, force_iters, k):
    """alpha, beta, tau, E, eta -> 2^k (...) (overlaps unchanged) maps A, B, t onto 2^k (A, B, t) exactly, so g -> 2^-k g
    and Sigma -> 2^k Sigma exactly: every operation of both kernels -- pivot keys, 1/p, the 3M products and updates,
    the mixing -- commutes with a power-of-two scale for normal numbers.  n = 17 and 50: the LDS kernel with a
    remainder strip; 80: the global kernel."""
    l1 = xc.lead_l1(n)
    g0, s0, _, _ = _g_sigma(l1, force_iters)
    gk, sk, _, _ = _g_sigma(xc.scaled(l1, k), force_iters)
    gb, sb = gk * 2.0 ** k, sk * 2.0 ** -k
    dg = np.abs(gb - g0).max() / np.abs(g0).max()
    ds = np.abs(sb - s0).max() / np.abs(s0).max()
    print(f"ACC chain scale n={n} K={force_iters} k={k}: max |2^k g_k - g| / max |g| = {dg:.3g}, Sigma {ds:.3g}")
    assert np.array_equal(gb, g0) and np.array_equal(sb, s0), (dg, ds)


@pytest.mark.parametrize("n", [17, 50, 80])
@pytest.mark.parametrize("k", [8, -8])
def test_chain_scale_equivariance_free_running(engine, n, k):
    """Free running (eta = 1e-3): the stopping test max |g_new - g| / max(|g_new|, 1e-12) is scale invariant while no
    |g_ij| comes near the 1e-12 floor, the reference's only absolute constant -- asserted first, with a margin of 2^9
    beyond the scale.  Then the sweep counts and convergence flags are identical and Sigma is bitwise 2^k times."""
    l1 = xc.lead_l1(n, eta=1e-3)
    g0, s0, i0, c0 = _g_sigma(l1, -1)
    lk = xc.scaled(l1, k)
    gk, sk, ik, ck = _g_sigma(lk, -1)
    assert min(np.abs(g0).min(), np.abs(gk).min()) > 1e-12 * 2.0 ** 9
    dg = np.abs(gk * 2.0 ** k - g0).max() / np.abs(g0).max()
    ds = np.abs(sk * 2.0 ** -k - s0).max() / np.abs(s0).max()
    print(f"ACC chain scale free n={n} k={k}: sweeps {i0.ravel().tolist()} / {ik.ravel().tolist()}, "
          f"g {dg:.3g}, Sigma {ds:.3g}")
    assert np.array_equal(i0, ik) and np.array_equal(c0, ck)
    assert np.array_equal(gk * 2.0 ** k, g0) and np.array_equal(sk * 2.0 ** -k, s0), (dg, ds)
