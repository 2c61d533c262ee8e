"""
Host checks of the yardstick the renormalisation-decimation kernel is held to (tests/xprec_rd.py): that the
extended-precision truth is fit to judge, how the bar is calibrated, and that planted defects miss it.

Case table: the leads L1 / L2 of xprec_chain at eta in {1e-4, 1e-6}, n_c in xprec_rd.HOST_SIZES, each lead's three
energies (in band, complex, near-edge): 36 cases.  (The scaled leads 2^+-64 derive truth, restatements and bar from
their base exactly -- a power of two commutes with every operation of the recursion -- so they add nothing here.)

  1. the algebraic identity: K steps of the clongdouble recursion against 2^K - 1 unrelaxed sweeps
     g <- inv(A - B g B^H) from inv(A), K in {1, 2, 3}: relative Frobenius difference no larger than the smaller float64
     error of the K-step restatements on that case;
  2. the fixed-point residual of the free-running truth is at most 1/100 of the smallest float64 error it judges;
  3. calibration: R_host, the worst ratio between the two float64 restatements' errors over the (free-running) table;
     C_RD must be 2 R_host rounded up to a power of two; each restatement inside the bar, free running and at fixed
     step counts; both stop after the same number of steps, within one of the truth's;
  4. planted defects (Q a dropped from the e update, products summed in complex64, b = B^T without the conjugate)
     miss the bar by >= 10x on every case.
"""
import functools

import numpy as np
import pytest

import xprec
import xprec_chain as xc
import xprec_rd as xr

xprec.require_extended()

KS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def _table():
    """[(lead, E, truth, {K: bar})] over the host case table; the truths are built on xprec.pmap."""
    cases = [c for n in xr.HOST_SIZES for c in xr.cases(n)]

    def make(c):
        lead, E = c
        t = xr.RdTruth(lead, E, ks=KS)
        return lead, E, t, {K: xr.RdBar(t, K) for K in (None,) + KS}
    return xprec.pmap(make, cases)


def _tag(lead, E):
    return f"{lead.name} n={lead.n} eta={lead.eta:g} E={E:.4g}"


def test_case_table_size():
    assert len(_table()) == 36


def test_recursion_is_the_unrelaxed_loop_doubled():
    """Step K of the recursion = iterate 2^K - 1 of the unrelaxed loop, both in clongdouble."""
    def check(row):
        lead, E, t, bars = row
        out = []
        for K in (1, 2, 3):
            gu = xr.unrelaxed_ld(lead, E, 2 ** K - 1)
            diff = xr._nf(t.gK[K] - gu) / xr._nf(gu)
            out.append((K, diff, min(bars[K].err_numpy, bars[K].err_gj)))
        return out
    worst, fails = 0.0, []
    for row, res in zip(_table(), xprec.pmap(check, _table())):
        for K, diff, floor in res:
            worst = max(worst, diff / floor)
            if not diff <= floor:
                fails.append((_tag(row[0], row[1]), K, diff, floor))
    print(f"RD identity: worst difference / smaller float64 error {worst:.3g}")
    assert not fails, fails


def test_truth_residual_is_small_enough_to_judge():
    worst, fails = 0.0, []
    for lead, E, t, bars in _table():
        floor = min(bars[None].err_numpy, bars[None].err_gj)
        worst = max(worst, t.residual / floor)
        if not t.residual <= 1e-2 * floor:
            fails.append((_tag(lead, E), t.residual, floor))
    print(f"RD truth residual: worst residual / smallest float64 error {worst:.3g} (allowed 1e-2)")
    assert not fails, fails


def test_calibration_of_the_bar():
    r_host, r_fixed, worst_err, worst_at, fails = 1.0, 1.0, 0.0, None, []
    for lead, E, t, bars in _table():
        for K, b in bars.items():
            r = max(b.err_numpy / b.err_gj, b.err_gj / b.err_numpy)
            if K is None:
                r_host = max(r_host, r)
            else:
                r_fixed = max(r_fixed, r)
            for e in (b.err_numpy, b.err_gj):
                if not e <= b.g_bar:
                    fails.append((_tag(lead, E), K, e, b.g_bar))
            if K is None:
                if max(b.err_numpy, b.err_gj) > worst_err:
                    worst_err, worst_at = max(b.err_numpy, b.err_gj), _tag(lead, E)
                if b.steps_numpy != b.steps_gj or not (b.conv_numpy and b.conv_gj):
                    fails.append((_tag(lead, E), "steps", b.steps_numpy, b.steps_gj))
    c_rd = 2.0 ** np.ceil(np.log2(2.0 * r_host))
    print(f"RD calibration: R_host {r_host:.3g} -> C_RD {c_rd:g} (xprec_rd.C_RD = {xr.C_RD:g}); "
          f"worst float64 error {worst_err:.3g} at {worst_at}; the same ratio at K in {KS} steps: {r_fixed:.3g}")
    assert not fails, fails
    assert c_rd == xr.C_RD, (r_host, c_rd, xr.C_RD)


def test_steps_of_the_restatements():
    """Both restatements stop where the truth does, +- 1 (the kernel is compared with these counts +- 1)."""
    counts = {}
    for lead, E, t, bars in _table():
        s = bars[None].steps_numpy
        counts.setdefault("complex" if abs(E.imag) > 0 else "real", []).append(s)
        assert abs(s - t.stop) <= 1 and s <= 25, (_tag(lead, E), s, t.stop)
    print("RD steps: " + ", ".join(f"{k} energies {min(v)}-{max(v)}" for k, v in sorted(counts.items())))


DEFECTS = {
    "no_qa": dict(defect="no_qa"),
    "c64_products": dict(prod=xr.prod_c64),
    "b_transposed": dict(defect="bT"),
}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_defects_miss_the_bar(name):
    least, fails = np.inf, []
    for lead, E, t, bars in _table():
        with np.errstate(all="ignore"):
            g, _, _, _ = xr.rd64(lead, E, **DEFECTS[name])
        ratio = bars[None].g_ratio(g)
        if not np.isfinite(ratio):
            ratio = np.inf
        least = min(least, ratio)
        if not ratio >= 10.0:
            fails.append((_tag(lead, E), ratio))
    print(f"RD planted defect {name}: least error / bar {least:.3g}")
    assert not fails, fails
