"""
The extended-precision reference of tests/xprec.py and its bar, on the CPU: the reference against mpmath, the
calibration of C_BAR on LAPACK and a textbook izamax Gauss-Jordan, and proof that the bar catches planted defects
(no row exchanges, |re|-only pivots, a reciprocal off by 1e-12, GrInt summed in float32) that the 1e-8 parity
tolerance lets through.  Lines 'CAL ...' / 'DEFECT ...' report the worst ratios error / bar.
"""
import functools

import numpy as np
import pytest

import oracle
import xprec
from xprec import C_BAR, Truth

SIZES = (17, 64, 200)


def test_long_double_is_extended():
    xprec.require_extended()


@functools.lru_cache(maxsize=None)
def _truths(n):
    """{case name: (case, truth)} over the case table at n."""
    out, base = {}, {}
    for c in xprec.case_table(n):
        if c.base is None:
            base[c.name] = Truth(c)
            out[c.name] = (c, base[c.name])
        else:
            out[c.name] = (c, Truth.of(c, base[c.base.name]))
    return out


def _worst(n, inverse, c=1.0):
    """{case name: worst column error / bar over its energies} for an fp64 inverse."""
    res = {}
    for name, (case, t) in _truths(n).items():
        res[name] = max(t.ratio(m, inverse(case.A64(E)), c) for m, E in enumerate(case.energies))
    return res


def test_case_table_transforms_are_exact():
    """G3 and G5 map A onto i A and 2^k A bitwise in float64, so their truths are the base truth times -i / 2^-k."""
    for n in (17, 64):
        for base in (xprec.ladder(n), xprec.bipartite(n)):
            for c in (xprec.rotated(base), xprec.scaled(base, 64), xprec.scaled(base, -64)):
                f = 1j if c.factor == -1j else 1.0 / c.factor
                for E0, E in zip(base.energies, c.energies):
                    assert np.array_equal(c.A64(E), f * base.A64(E0)), (c.name, E0)


def test_ladder_spans_the_conditioning_range():
    t = _truths(64)["G1"][1]
    assert t.kappa[0] < 1e3 and t.kappa[4] > 1e9, t.kappa


def test_reference_against_mpmath():
    """The clongdouble reference against a 40-digit inverse at n = 12 on G1 (kappa up to ~2e9) and G2: its error is at
    most 1e-2 times the smallest bar it is used for."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    n = 12
    worst = 0.0
    for case in (xprec.ladder(n), xprec.bipartite(n)):
        t = Truth(case)
        for m, E in enumerate(case.energies):
            Em = mpmath.mpc(E.real, E.imag)
            St = case.sig_tot
            A = mpmath.matrix(n, n)
            for i in range(n):
                for j in range(n):
                    A[i, j] = (Em * mpmath.mpf(float(case.S[i, j])) - mpmath.mpf(float(case.F[i, j]))
                               - mpmath.mpc(St[i, j].real, St[i, j].imag))
            Ginv = mpmath.inverse(A)
            G = t.G[m]
            for j in range(n):
                num = den = mpmath.mpf(0)
                for i in range(n):
                    x = G[i, j]
                    re = float(x.real); im = float(x.imag)
                    xm = mpmath.mpc(mpmath.mpf(re) + mpmath.mpf(float(x.real - re)),
                                    mpmath.mpf(im) + mpmath.mpf(float(x.imag - im)))
                    num += abs(xm - Ginv[i, j]) ** 2
                    den += abs(Ginv[i, j]) ** 2
                err = float(mpmath.sqrt(num / den))
                r = err / t.delta(m)
                worst = max(worst, r)
                assert r <= 1e-2, (case.name, m, j, err, t.delta(m))
    print(f"REF mpmath: worst reference error / bar {worst:.3g}")


@pytest.mark.parametrize("n", SIZES)
def test_calibration(n):
    """LAPACK (oracle.inv) and a textbook izamax Gauss-Jordan meet the bar with c = 1 at half of C_BAR or better on every
    case: C_BAR is the smallest power of two at least twice their worst ratio (measured 0.62: textbook GJ, G2 rotated,
    n = 64), and at most 16."""
    assert C_BAR <= 16
    lap = _worst(n, oracle.inv)
    gj = _worst(n, xprec.gauss_jordan)
    for name in lap:
        print(f"CAL n={n} {name}: lapack {lap[name]:.3g}  gj {gj[name]:.3g}")
    worst = max(max(lap.values()), max(gj.values()))
    assert 2 * worst <= C_BAR, (lap, gj)


def test_calibration_grint():
    """GrInt summed in float64 from LAPACK inverses meets its propagated per-column bar."""
    for n, name in [(n, name) for n in SIZES for name in ("G1", "G2", "G4")]:
        case, t = _truths(n)[name]
        w = np.random.default_rng(5).standard_normal(case.energies.size) * (1 + 1j)
        ref, bound = xprec.grint_truth_and_bound(t, w)
        P = sum(w[m] * oracle.inv(case.A64(E)) for m, E in enumerate(case.energies))
        err = np.linalg.norm((P[:, t.cols].astype(xprec.LD) - ref).astype(np.complex128), axis=0)
        print(f"CAL GrInt n={n} {name}: worst {np.max(err / bound):.3g}")
        assert np.all(err <= bound)


DEFECTS = {
    "no row exchanges": lambda A: xprec.gauss_jordan(A, pivot="none"),
    "|re|-only pivots": lambda A: xprec.gauss_jordan(A, pivot="re"),
    "reciprocal off by 1e-12": lambda A: xprec.gauss_jordan(A, recip_rel=1e-12),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_discrimination_inverse(defect):
    """Each planted defect exceeds the bar by >= 10x on at least one case."""
    worst = {}
    for n in SIZES:
        for name, r in _worst(n, DEFECTS[defect], C_BAR).items():
            worst[(n, name)] = r
    top = max(worst, key=worst.get)
    print(f"DEFECT {defect}: worst ratio {worst[top]:.3g} at n={top[0]} {top[1]}; "
          + ", ".join(f"{k[1]}@{k[0]} {v:.2g}" for k, v in worst.items()))
    assert worst[top] >= 10.0, worst


def test_discrimination_grint_float32():
    """GrInt accumulated in complex64 exceeds its propagated bar by >= 10x on at least one case (on the ladder the
    near-singular energy dominates both the sum and its bar; the well-conditioned cases expose it)."""
    worst = {}
    for n in SIZES:
        for name in ("G1", "G2", "G4"):
            case, t = _truths(n)[name]
            w = np.random.default_rng(5).standard_normal(case.energies.size) * (1 + 1j)
            ref, bound = xprec.grint_truth_and_bound(t, w)
            P = np.zeros((n, n), dtype=np.complex64)
            for m, E in enumerate(case.energies):
                P += (w[m] * xprec.gauss_jordan(case.A64(E))).astype(np.complex64)
            err = np.linalg.norm((P[:, t.cols].astype(xprec.LD) - ref).astype(np.complex128), axis=0)
            worst[(n, name)] = float(np.max(err / bound))
    top = max(worst, key=worst.get)
    print(f"DEFECT GrInt float32: worst ratio {worst[top]:.3g} at n={top[0]} {top[1]}; "
          + ", ".join(f"{k[1]}@{k[0]} {v:.2g}" for k, v in worst.items()))
    assert worst[top] >= 10.0, worst
