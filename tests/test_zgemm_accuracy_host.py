"""
The product kernels' truth, case table, bars and restatement of tests/xprec_zgemm.py on the CPU:
  * Z1 is what it claims: no zero entries, every partial sum of the 3M form below 2^33;
  * the int64 and the long-double truth agree with mpmath on two small cases;
  * the undefective restatement of both tiled kernels is bitwise exact on Z1, for every opB, and within the bars on Z2;
  * C_ZG equals what the calibration rule derives from the three float64 host implementations, and all three stay
    under the rigorous gamma_{K+4} ceiling;
  * every planted defect fails at least one Z1 case;
  * the Hermitian enumeration of negf_zgemm_plan visits every (by <= bx, b) exactly once and nothing else, for
    T = 1 ... 12 block columns and nb = 1 ... 9, with the block counts of both kernels;
  * the plan routes as launch_zgemm's rule says and demotes the Hermitian bit as launch_zgemm does.
Lines 'CAL zgemm ...' / 'DEFECT zgemm ...' report worst ratios and what caught each defect.
"""
import numpy as np
import pytest

import xprec
import xprec_zgemm as xz
from xprec import U


def test_long_double_is_extended():
    xprec.require_extended()


# --------------------------------------------------------------------------- #
# the case table
# --------------------------------------------------------------------------- #
def test_shape_table_holds_the_required_cases():
    have = {(s.M, s.N, s.K) for s in xz.SHAPES}
    for need in [(1, 1, 1), (16, 16, 4), (17, 15, 3), (64, 64, 16), (65, 63, 17), (16, 16, 0), (80, 130, 33),
                 (150, 12, 12), (150, 150, 12), (12, 40, 12), (12, 12, 40), (20, 150, 12), (330, 330, 40)]:
        assert need in have, need
    for n in (64, 100, 128, 130, 150, 200, 250, 330):
        assert any(s.M == s.N == n and s.nb == 1 for s in xz.SHAPES), n
    assert {s.nb for s in xz.SHAPES} >= {1, 3, 9}
    assert any(s.shareA for s in xz.SHAPES) and any(s.shareB for s in xz.SHAPES)
    # the block counts the square table promises, on the kernel each size is forced onto
    for n, T in ((64, 1), (100, 2), (128, 2), (150, 3), (250, 4), (330, 6)):
        assert xz.plan(n, n, n, 3, 1, 1)["blocks"] == (T, T)
    for n, T in ((130, 2), (200, 3), (330, 5)):
        assert xz.plan(n, n, n, 3, 1, 2)["blocks"] == (T, T)
    # batches: pairs of block columns times members that are and are not a multiple of 8 (even enumeration)
    pn = {((xz.plan(s.M, s.N, s.K, 3, s.nb, 1)["blocks"][1] + 1) // 2 * s.nb) % 8 == 0
          for s in xz.BATCHED if s.M == s.N and xz.plan(s.M, s.N, s.K, 3, s.nb, 1)["blocks"][1] % 2 == 0}
    assert pn == {True, False}


def test_z1_partial_sums_are_exact():
    """Integer parts in +-[1, 1024] without zeros, K <= 1024, and sum_k (|Ar| + |Ai|)(|Pr| + |Pi|) < 2^33: every
    partial sum of S1, S2, S3 and the recombination is an integer below 2^53 in any order."""
    for s in xz.SHAPES:
        for herm in ((False, True) if s.M == s.N else (False,)):
            A, P = xz.logical(s, "z1", herm)
            assert s.K <= 1024
            for X in (A, P):
                for part in (X.real, X.imag):
                    assert np.array_equal(part, np.rint(part))
                    if part.size:
                        assert 1 <= np.min(np.abs(part)) and np.max(np.abs(part)) <= 1024
            _, mim, _ = xz.magnitudes(s, "z1", herm)
            assert np.max(mim, initial=0.0) < 2.0 ** 33


def _mp_product(a, p):
    import mpmath
    mpmath.mp.dps = 40
    mp = mpmath
    am = mp.matrix([[mp.mpc(mp.mpf(float(v.real)), mp.mpf(float(v.imag))) for v in row] for row in a])
    pm = mp.matrix([[mp.mpc(mp.mpf(float(v.real)), mp.mpf(float(v.imag))) for v in row] for row in p])
    return mp, am * pm


def test_truth_against_mpmath():
    """(17, 15, 3) with graded entries in long double and (12, 12, 40) in int64 against 40-digit products: the int64
    truth exactly, the long-double truth to 2^-6 of the bar with C = 1 (it carries 11 bits more than float64)."""
    s = next(x for x in xz.SHAPES if (x.M, x.N, x.K) == (17, 15, 3))
    A, P = xz.logical(s, "graded")
    mp, T = _mp_product(A[0], P[0])
    tr, ti = xz.truth(s, "graded")
    mre, mim, _ = xz.magnitudes(s, "graded")
    f = 2.0 ** -6 * np.sqrt(s.K + 4.0) * U

    def ld(v):
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))
    for i in range(s.M):
        for j in range(s.N):
            assert abs(ld(tr[0, i, j]) - T[i, j].real) <= f * mre[0, i, j]
            assert abs(ld(ti[0, i, j]) - T[i, j].imag) <= f * mim[0, i, j]
    s = next(x for x in xz.SHAPES if (x.M, x.N, x.K) == (12, 12, 40))
    A, P = xz.logical(s, "z1")
    mp, T = _mp_product(A[0], P[0])
    tr, ti = xz.truth(s, "z1")
    for i in range(s.M):
        for j in range(s.N):
            assert int(tr[0, i, j]) == int(T[i, j].real) and int(ti[0, i, j]) == int(T[i, j].imag)


# --------------------------------------------------------------------------- #
# the restatement
# --------------------------------------------------------------------------- #
def _z1_launches():
    """(shape, opB, kernel) of every Z1 launch of the tiled kernels."""
    return [(s, opB, k) for s in xz.SHAPES for opB in xz.opbs(s) for k in (1, 2)]


def test_restatement_is_exact_on_z1():
    for s, opB, k in _z1_launches():
        ops = xz.operands(s, "z1", opB)
        want = ops.expected_flat(xz.truth_c128(s, "z1", bool(opB & 2)))
        assert xz.bitwise(xz.model(ops, k, kstep=16), want), (s, opB, k)
    # the vector-unit kernel's restatement (four products, the promise ignored)
    for s in xz.SHAPES[:8]:
        ops = xz.operands(s, "z1", 5)
        assert xz.bitwise(xz.model(ops, 3), ops.expected_flat(xz.truth_c128(s)))


def test_restatement_meets_the_bars_on_z2():
    worst = 0.0
    for s, kind, herm in xz.z2_table():
        if s.M * s.N * s.K > 150 ** 3:
            continue                                 # (the calibration runs the large products through three_m)
        for k in (1, 2):
            ops = xz.operands(s, kind, 3 if herm else 1)
            r, g = xz.ratios(ops.result(xz.model(ops, k)), s, kind, herm)
            assert r <= 1.0 and g <= 1.0, (s, kind, herm, k, r, g)
            worst = max(worst, r)
    print(f"CAL zgemm restatement: worst ratio {worst:.3g} of the bar with C_ZG = {xz.C_ZG:g}")


def test_calibration():
    """C_ZG is the smallest power of two at least twice the worst ratio of the three host implementations over the Z2
    table; each stays under the rigorous ceiling."""
    worst = {}
    for name, impl in xz.HOST_IMPLS.items():
        w = 0.0
        for s, kind, herm in xz.z2_table():
            r, g = xz.ratios(xz.host_product(s, kind, impl, herm), s, kind, herm, c=1.0)
            assert g <= 1.0, (name, s, kind, herm, g)
            w = max(w, r)
        worst[name] = w
        print(f"CAL zgemm {name}: worst ratio {w:.3g} (C = 1)")
    c = 2.0 ** np.ceil(np.log2(2.0 * max(worst.values())))
    assert c == xz.C_ZG, (worst, c)


def test_3m_cannot_meet_the_conventional_bound():
    """tinyim: |Ar||Pi| + |Ai||Pr| is 2e-9 of the 3M magnitude, so the 3M restatement exceeds the four-product form's
    componentwise bound by many orders while numpy's four-product matmul meets it."""
    s = next(x for x in xz.SHAPES if (x.M, x.N, x.K) == (80, 130, 33) and x.nb == 1)
    r3 = xz.conventional_ratio(xz.host_product(s, "tinyim", xz.HOST_IMPLS["3M k-step 4"]), s, "tinyim")
    r4 = xz.conventional_ratio(xz.host_product(s, "tinyim", xz.HOST_IMPLS["numpy matmul"]), s, "tinyim")
    print(f"CAL zgemm tinyim against the conventional bound: 3M {r3:.3g}, four products {r4:.3g}")
    assert r4 <= 1.0 and r3 > 1e4


# --------------------------------------------------------------------------- #
# planted defects
# --------------------------------------------------------------------------- #
def test_every_planted_defect_fails_a_z1_case():
    """Each defect changes the restatement's result on at least one Z1 launch of the table (a mismatch with the exact
    product is what the GPU test asserts bitwise); an unnoticed defect means the table is too weak."""
    launches = [l for l in _z1_launches() if l[0].M * l[0].N <= 150 * 150]     # (the larger squares add no mechanism)
    made = {}
    for d in xz.DEFECTS:
        caught = []
        for s, opB, k in launches:
            if (s, opB) not in made:
                ops = xz.operands(s, "z1", opB)
                made[s, opB] = ops, ops.expected_flat(xz.truth_c128(s, "z1", bool(opB & 2)))
            ops, want = made[s, opB]
            if not xz.bitwise(xz.model(ops, k, defect=d, kstep=16), want):
                caught.append((s.M, s.N, s.K, s.nb, opB, k))
        print(f"DEFECT zgemm {d}: caught by {len(caught)} of {len(launches)} launches, first {caught[:1]}")
        assert caught, d
        assert {c[5] for c in caught} == {1, 2}, (d, "not on both kernels")


# --------------------------------------------------------------------------- #
# the plan
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("kernel", [1, 2])
def test_hermitian_enumeration_visits_the_triangle_once(kernel):
    unit = 64 if kernel == 1 else 80
    for T in range(1, 13):
        n = unit * T
        for nb in range(1, 10):
            pl = xz.plan(n, n, 4, 3, nb, kernel)
            assert pl["kernel"] == kernel and pl["opB"] == 3 and pl["blocks"] == (T, T)
            dec = pl["decode"]
            assert dec.shape == (pl["grid"][0], 3) and pl["grid"][1:] == (1, 1)
            live = dec[dec[:, 0] >= 0]
            assert np.all(dec[dec[:, 0] < 0] == -1)
            want = sorted((by, bx, b) for b in range(nb) for bx in range(T) for by in range(bx + 1))
            assert sorted(map(tuple, live.tolist())) == want, (T, nb)


def test_plan_routes_as_the_rule_says():
    for M in list(range(1, 400, 7)) + [64, 128, 150, 330, 650, 720, 1000]:
        for N in (1, 12, 64, 100, 150, 330, M):
            pl = xz.plan(M, N)
            assert (pl["kernel"],) + pl["blocks"] == xz.rule(M, N), (M, N)
            assert pl["grid"] == (pl["blocks"][1], pl["blocks"][0], 1)
    for n, want in ((150, (2, 2, 2)), (330, (2, 5, 5)), (650, (1, 11, 11)), (720, (1, 12, 12))):
        pl = xz.plan(n, n, n, 3, 2)
        assert (pl["kernel"],) + pl["blocks"] == want
    assert xz.plan(100, 100, 1, 0, 5, 3)["grid"] == (4, 4, 5)              # the vector-unit kernel: 32 x 32 blocks


def test_plan_demotes_the_hermitian_bit_as_the_launcher_does():
    for opB in range(8):
        for M, N in ((100, 100), (100, 90)):
            eff = xz.plan(M, N, 8, opB, 1)["opB"]
            assert eff == (opB & ~2 if (opB & 2) and (M != N or opB & 4) else opB)
    from gaunegf_amd import _lib
    lib = _lib.load()
    bad = [(0, 4, 4, 0, 1, 0), (4, 0, 4, 0, 1, 0), (4, 4, -1, 0, 1, 0), (4, 4, 4, 8, 1, 0), (4, 4, 4, 0, 0, 0),
           (4, 4, 4, 0, 1, 4), (4, 4, 4, -1, 1, 0)]
    for a in bad:
        assert lib.negf_zgemm_plan(*a, None, None, None, None, None, 0) == _lib.NEGF_EINVAL, a
    import ctypes
    small = (ctypes.c_int * 3)()
    assert lib.negf_zgemm_plan(128, 128, 4, 3, 1, 1, None, None, None, None, small, 1) == _lib.NEGF_EINVAL
