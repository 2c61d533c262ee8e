"""
The Bethe-lattice truth, case table and bars of tests/xprec_bethe.py on the CPU:
  * the clongdouble truth agrees with an mpmath restatement (40 digits) to a small fraction of the bars;
  * the case table is what it claims: B1's energies lie below / in the sp / in the d band, B4's matrices are formed
    exactly by float64 arithmetic, B3 and the bipartite / weak B4 points exchange rows in a textbook Gauss-Jordan;
  * C_BETHE equals what the calibration rule derives from the two float64 references (LAPACK, izamax Gauss-Jordan), and
    both references meet the B4 inverse bars;
  * every planted defect (pivot key |re| only, no row exchanges, 1e-13 relative error in 1/p, Jacobi ordering in
    phase 1, Sigma_tot not frozen, +i eta, a surface update outside the plane) exceeds a bar on at least one case;
  * at most 10 % of the energies of each free-running grid are ambiguous for the stop rule.
Lines 'CAL ...' / 'DEFECT ...' report worst ratios error / bar.
"""
import functools

import numpy as np
import pytest

import oracle
import xprec
import xprec_bethe as xb
from xprec import LD, U

ATOM_NBS = ([3, 4, 5], [0, 9, -1, 3, 11])      # attached directions of the assembly checks: inside 0..8 and outside


def test_long_double_is_extended():
    xprec.require_extended()


# --------------------------------------------------------------------------- #
# the truth against mpmath
# --------------------------------------------------------------------------- #
def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def _to_mp(mp, X):
    X = np.asarray(X)
    return mp.matrix([[mp.mpc(mp.mpf(float(v.real)), mp.mpf(float(v.imag))) for v in row] for row in X])


def _ld_to_mp(mp, X):
    """clongdouble -> mpmath without loss: a float64 head and a float64 tail per component."""
    def one(v):
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))
    return mp.matrix([[mp.mpc(one(v.real), one(v.imag)) for v in row] for row in np.asarray(X)])


def _mp_rel(mp, A, B):
    """||A - B||_F / ||B||_F."""
    return float(mp.mnorm(A - B, 'f') / mp.mnorm(B, 'f'))


TRUTH_SHARE = 2.0 ** -6
"""The truth may err by this fraction of a bar at most: clongdouble carries 11 bits more than float64 (2^-11 of a bar
whose constant is 1), five of which are left to the constants of its own rounding-error growth."""


def test_truth_against_mpmath_sweeps():
    """Three bulk and three surface sweeps of a B1 case (Au, eta = 1e-6, the first band-edge point) restated in
    mpmath from the float64 inputs."""
    mp = _mp()
    lat = xb.b1_cases()[0]
    E = lat.energies[3]
    K = 3
    tr = xb.bulk(lat, E, K=K, keep={K})
    ts = xb.surface(lat, E, tr.at[K], K=K, keep={K})
    z = lat.z(E)
    zm = mp.mpc(mp.mpf(z.real), mp.mpf(z.imag))
    I9 = mp.eye(9)
    A = zm * I9 - _to_mp(mp, lat.H)
    B = [zm * _to_mp(mp, lat.S[k]) - _to_mp(mp, lat.V[k]) for k in range(12)]
    half = mp.mpf(0.5)
    sig = [mp.mpc(0, -1) * I9 for _ in range(12)]
    for _ in range(K):
        old = [s.copy() for s in sig]
        tot = sig[0].copy()
        for k in range(1, 12):
            tot = tot + sig[k]
        for k in range(12):
            g = mp.inverse(A - tot + sig[(k + 6) % 12])
            sig[k] = half * (B[k] * g * B[k].transpose_conj()) + half * old[k]
    for k in range(12):
        r = _mp_rel(mp, _ld_to_mp(mp, tr.at[K][k]), sig[k])
        assert r <= TRUTH_SHARE * U * tr.kappa[K - 1], (k, r)
    s = sig[:9]
    for _ in range(K):
        old = [x.copy() for x in s]
        tot = old[0].copy()
        for k in range(1, 9):
            tot = tot + old[k]
        g = mp.inverse(A - tot)
        for k in xb.PLANE:
            s[k] = half * (B[k] * g * B[k].transpose_conj()) + half * old[k]
    for k in range(9):
        r = _mp_rel(mp, _ld_to_mp(mp, ts.at[K][k]), s[k])
        assert r <= TRUTH_SHARE * U * ts.kappa[K - 1], (k, r)


def test_truth_against_mpmath_b4():
    """The ill-conditioned ladder point (x on the eigenvalue, kappa_2 ~ 1e9): g and G2 in mpmath."""
    mp = _mp()
    fam = xb.b4_families()[0]
    m = 4
    t = xb.b4_truth(0, m)
    assert t.kappa1 > 1e8
    x, d = fam.points[m]
    M = mp.mpc(mp.mpf(x), mp.mpf(d)) * mp.eye(9) - _to_mp(mp, fam.H)
    g = mp.inverse(M)
    G2 = mp.inverse(M + mp.mpc(0, 1) * mp.eye(9) + g)
    assert _mp_rel(mp, _ld_to_mp(mp, t.g), g) <= TRUTH_SHARE * xprec.bar(9, t.kappa1, 1.0)
    assert _mp_rel(mp, _ld_to_mp(mp, t.G2), G2) <= TRUTH_SHARE * xprec.bar(9, t.kappa2, 1.0)


# --------------------------------------------------------------------------- #
# the case table
# --------------------------------------------------------------------------- #
def test_b1_energies():
    """B1_FIXED: no density of states below the band, sp-dominated and d-dominated in the two band points; the edge
    points are interior grid points of the scan and distinct from the fixed energies."""
    for name, (deep, sp, d) in xb.B1_FIXED.items():
        lat = xb.shipped(name, 1e-4)
        dos = {}
        for E in (deep, sp, d):
            s, _, _ = oracle.bethe_sigmaK(E, lat.H, lat.S, lat.V, lat.eta, conv=1e-7)
            G = np.linalg.inv(lat.z(E) * np.eye(9) - lat.H - s.sum(0))
            w = np.abs(np.diag(G).imag) / np.pi
            dos[E] = (w[:4].sum(), w[4:].sum())
        assert sum(dos[deep]) < 1e-3, (name, dos)
        assert dos[sp][0] > 1.5 * dos[sp][1] and dos[sp][0] > 0.05, (name, dos)
        assert dos[d][1] > 2 * dos[d][0] and dos[d][1] > 0.5, (name, dos)
    for lat in xb.b1_cases():
        assert lat.energies.size == 7
        e1, e2 = lat.energies[3].real, lat.energies[4].real
        assert e1 in xb.EDGE_GRID and e2 in xb.EDGE_GRID and abs(e1 - e2) > 0.3
        print(f"CAL {lat.name}: band-edge points {e1:.2f}, {e2:.2f}")


def test_b2_b3_are_au_with_one_change():
    au, b2, b3 = xb.shipped("Au", 1e-6), xb.b2_case(), xb.b3_case()
    dH = b2.H - au.H
    assert np.count_nonzero(dH) == 2 and np.allclose(np.diag(dH)[[1, 5]], [1e3, 1e5], rtol=1e-12)
    assert np.array_equal(b2.V, au.V) and np.array_equal(b2.S, au.S)
    assert np.array_equal(b3.V, 32.0 * au.V) and np.array_equal(b3.H, au.H) and np.array_equal(b3.S, au.S)
    assert np.count_nonzero(au.H - np.diag(np.diag(au.H))) == 0          # nothing off-diagonal in H to scale


def test_b4_is_exact():
    """The float64 steps of the kernel that form the B4 matrices are exact: E's imaginary part, z, Sigma_tot = -12 i,
    (z I - H) - Sigma_tot + sigma_{k+6} = (x + i d) I - H, B_k = z 0 + I = I."""
    for fam in xb.b4_families():
        for m, (E, (x, d)) in enumerate(zip(fam.energies, fam.points)):
            assert LD(E.imag) == LD(xb.B4_ETA) - LD(11) + LD(d)
            z = fam.lat.z(E)
            assert LD(z.imag) == LD(d) - LD(11) and z.real == x
            A = z * np.eye(9) - fam.H                                    # float64, as the kernel and the oracle
            tot = np.sum(np.stack([-1j * np.eye(9)] * 12), axis=0)
            M = A - tot + (-1j * np.eye(9))
            assert np.array_equal(M.astype(LD), fam.matrix_ld(m)), (fam.name, m)
            assert np.array_equal(fam.matrix_ld(m).astype(np.complex128).astype(LD), fam.matrix_ld(m))
            B = z * fam.S[0] - fam.V[0]
            assert np.array_equal(B, np.eye(9))
        assert np.array_equal(fam.H, fam.H.T)


def test_b4_kappa_ladder():
    """The ladder spans kappa_2 ~ 10 ... 1e9."""
    k = [xb.b4_truth(0, m).kappa1 for m in range(5)]
    print("CAL B4 ladder kappa_2:", " ".join(f"{v:.3g}" for v in k))
    assert k[0] < 30 and 3e8 < k[4] < 1e10 and all(a < b for a, b in zip(k, k[1:]))


def _exchanges(A):
    """A textbook Gauss-Jordan with izamax pivoting exchanges a row on A: it then differs from the one without."""
    return not np.array_equal(xprec.gauss_jordan(A, "abs1"), xprec.gauss_jordan(A, "none"))


def test_row_exchanges():
    """B3: at least one matrix of sweep 1 needs a row exchange, at every energy; bipartite and weak B4 points too."""
    b3 = xb.b3_case()
    for E in b3.energies:
        mats = []
        xb.bulk(b3, E, K=1, inv=lambda A: (mats.append(A.copy()), np.linalg.inv(A))[1], ld=False)
        assert len(mats) == 12 and any(_exchanges(A) for A in mats), E
    fams = xb.b4_families()
    assert fams[1].name == "bipartite" and fams[2].name == "weak"
    assert _exchanges(xb.b4_truth(0, 6).M64) and xb.b4_truth(0, 6).kappa1 < 1e3
    for m, (x, d) in enumerate(fams[1].points):
        if d < 1.0:                                                      # (the contour point has a diagonal of 2i)
            assert _exchanges(xb.b4_truth(1, m).M64), m
    assert not _exchanges(xb.b4_truth(2, 0).M64)                         # weak: the diagonal i is the right pivot


# --------------------------------------------------------------------------- #
# float64 references, calibration
# --------------------------------------------------------------------------- #
def _ratios(ci, m, run):
    """Worst ratios of a float64 implementation `run(lat, E, K) -> (sigK, s9)` on one case and energy against the bars
    with c = 1: bulk, surface, cluster and atom assembly, over K_CHECKED."""
    lat = xb.sweep_cases()[ci]
    t = xb.sweep_truth(ci, m)
    worst = 0.0
    for K in xb.K_CHECKED:
        sigK, s9 = run(lat, t.E, K)
        r = [xb.sweep_ratio(sigK, t.bulk[K], t.kappa_bulk[K], 1.0),
             xb.sweep_ratio(s9, t.surf[K], t.kappa_surf[K], 1.0),
             xb.cluster_ratio(xb.cluster_blocks(sigK), t.bulk[K], t.kappa_bulk[K], 1.0)]
        for nbs in ATOM_NBS:
            true, used = xb.atom_sigma(t.surf[K], nbs)
            r.append(xb.sum_ratio(xb.atom_sigma(s9, nbs)[0], true, t.surf[K], used, t.kappa_surf[K], 1.0))
        worst = max(worst, *r)
    return worst


def _run_oracle(lat, E, K):
    sigK, count, _ = oracle.bethe_sigmaK(E, lat.H, lat.S, lat.V, lat.eta, force_iters=K)
    s9, cs, _, ck = oracle.bethe_sigma_surface(E, lat.H, lat.S, lat.V, lat.eta, force_iters=K)
    assert count == K and cs == K and ck == K
    return sigK, s9


def _run_loops(inv, surf_kw=None, **kw):
    def run(lat, E, K):
        sigK = xb.bulk(lat, E, K=K, inv=inv, ld=False, keep={K}, **kw).at[K]
        s9 = xb.surface(lat, E, sigK, K=K, inv=inv, ld=False, keep={K}, eta_sign=kw.get("eta_sign", -1.0),
                        **(surf_kw or {})).at[K]
        return sigK, s9
    return run


def _table(run):
    """{case name: worst ratio with c = 1} over the whole sweep table."""
    out = {}
    for ci, lat in enumerate(xb.sweep_cases()):
        out[lat.name] = max(_ratios(ci, m, run) for m in range(lat.energies.size))
    return out


def test_loops_restate_the_oracle():
    """The complex128 loops of xprec_bethe with LAPACK's inverse are oracle.bethe_sigmaK / bethe_sigma_surface (to
    rounding), and its assembly helpers are oracle.bethe_atom_sigma / bethe_cluster_sigma_total."""
    lat = xb.b1_cases()[0]
    for E in lat.energies[[1, 5]]:
        a, b = _run_oracle(lat, E, 10), _run_loops(np.linalg.inv)(lat, E, 10)
        for x, y in zip(a, b):
            assert np.linalg.norm(x - y) <= 1e-13 * np.linalg.norm(x)
        for nbs in ATOM_NBS:
            assert np.allclose(xb.atom_sigma(a[1], nbs)[0], oracle.bethe_atom_sigma(a[1], nbs), rtol=0, atol=1e-13)
        cl = oracle.bethe_cluster_sigma_total(E, lat.H, lat.S, lat.V, lat.eta, sigK=a[0])
        for k, blk in enumerate(xb.cluster_blocks(a[0])):
            assert np.allclose(cl[9 * k:9 * k + 9, 9 * k:9 * k + 9], blk, rtol=0, atol=1e-13)
    # free running: the oracle's sweep count is the truth's
    t = xb.free_truths(1e-5)[3]
    _, count, _ = oracle.bethe_sigmaK(t.E, t.lat.H, t.lat.S, t.lat.V, t.lat.eta, conv=1e-5)
    assert count == t.bulk.count


@functools.lru_cache(maxsize=None)
def _calibration():
    return _table(_run_oracle), _table(_run_loops(xprec.gauss_jordan))


def test_calibration():
    """C_BETHE is the smallest power of two at least twice the worst ratio error / (u kappa_max ||sigma_k||) of the two
    float64 references over the whole table."""
    lap, gj = _calibration()
    for name in lap:
        print(f"CAL bethe {name}: worst ratio at c = 1  LAPACK {lap[name]:.3g}  Gauss-Jordan {gj[name]:.3g}")
    worst = max(max(lap.values()), max(gj.values()))
    derived = 2.0 ** np.ceil(np.log2(2 * worst))
    print(f"CAL bethe: worst LAPACK {max(lap.values()):.3g}, worst Gauss-Jordan {max(gj.values()):.3g}, "
          f"derived C_BETHE {derived:g}")
    assert derived == xb.C_BETHE, (worst, derived)


def _b4_ratios(inv):
    """{family: worst ratio} of one sweep on the B4 points with the float64 inverse `inv` (k < 6 and k >= 6 blocks)."""
    out = {}
    for f, fam in enumerate(xb.b4_families()):
        r = 0.0
        for m in range(len(fam.points)):
            t = xb.b4_truth(f, m)
            g, G2 = xb.b4_reference(fam, m, inv)
            r = max(r, t.ratio_first(g), t.ratio_second(G2))
        out[fam.name] = r
    return out


def test_b4_references_meet_the_inverse_bar():
    """xprec.bar(9, kappa_2) with C_BAR, unchanged, holds both references with half its constant (the rule that set it)."""
    for what, inv in (("LAPACK", np.linalg.inv), ("Gauss-Jordan", xprec.gauss_jordan)):
        r = _b4_ratios(inv)
        for name, v in r.items():
            print(f"CAL bethe B4 {name} {what}: worst ratio {v:.3g}")
        assert max(r.values()) <= 0.5, (what, r)


# --------------------------------------------------------------------------- #
# planted defects
# --------------------------------------------------------------------------- #
def _gj(**kw):
    return functools.partial(xprec.gauss_jordan, **kw)


def _defect_report(what, table, b4=None):
    worst = max(table.values()) / xb.C_BETHE if table else 0.0
    for name, v in table.items():
        print(f"DEFECT {what} {name}: worst ratio {v / xb.C_BETHE:.3g}")
    for name, v in (b4 or {}).items():
        print(f"DEFECT {what} B4 {name}: worst ratio {v:.3g}")
    return max(worst, max((b4 or {"": 0.0}).values()))


def test_defect_pivot_key_real_part_only():
    """|re| as the pivot key: caught on the weak B4 family (a diagonal of i against real couplings of 1e-7)."""
    b4 = _b4_ratios(_gj(pivot="re"))
    assert _defect_report("pivot |re|", {}, b4) > 1.0
    assert b4["weak"] > 1.0, b4


def test_defect_no_row_exchanges():
    """No row exchanges: caught on the ladder's x = H_00 + 2^-30 point.  (The zero-diagonal bipartite points do not
    catch it: eliminating with their pivots of i d loses only the d-sized diagonal of the inverse, far below the
    column norms that the bar is relative to.)"""
    b4 = _b4_ratios(_gj(pivot="none"))
    tab = _table(_run_loops(_gj(pivot="none")))
    assert _defect_report("no exchanges", tab, b4) > 1.0
    assert b4["ladder"] > 1.0, b4


def test_defect_reciprocal():
    """A relative error of 1e-13 in 1/p."""
    tab = _table(_run_loops(_gj(recip_rel=1e-13)))
    b4 = _b4_ratios(_gj(recip_rel=1e-13))
    assert _defect_report("recip 1e-13", tab, b4) > 1.0


def test_defect_jacobi_ordering():
    tab = _table(_run_loops(np.linalg.inv, jacobi=True))
    assert _defect_report("Jacobi phase 1", tab) > 1.0
    assert min(tab.values()) / xb.C_BETHE > 1.0, tab


def test_defect_sigma_tot_not_frozen():
    tab = _table(_run_loops(np.linalg.inv, unfrozen=True))
    assert _defect_report("Sigma_tot not frozen", tab) > 1.0
    assert min(tab.values()) / xb.C_BETHE > 1.0, tab


def test_defect_eta_sign():
    tab = _table(_run_loops(np.linalg.inv, eta_sign=+1.0))
    assert _defect_report("+i eta", tab) > 1.0


def test_defect_surface_updates_outside_the_plane():
    tab = _table(_run_loops(np.linalg.inv, surf_kw=dict(plane=(0, 1, 2, 3, 6, 7, 8))))
    assert _defect_report("surface updates k = 3", tab) > 1.0
    assert min(tab.values()) / xb.C_BETHE > 1.0, tab


# --------------------------------------------------------------------------- #
# the stop rule
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("conv", xb.FREE_CONVS)
def test_ambiguity_cap(conv):
    """At most 10 % of a free-running grid is ambiguous (diff within a relative 1e-6 of conv at the stopping sweep or
    the one before), bulk or surface; and every point converges within max_iter."""
    ts = xb.free_truths(conv)
    amb = [t.ambiguous() for t in ts]
    counts = [(t.bulk.count, t.surf(t.bulk.count).count) for t in ts]
    print(f"CAL bethe free conv={conv:g}: counts {counts}, ambiguous {sum(amb)} of {len(ts)}")
    assert sum(amb) <= xb.AMBIGUOUS_CAP * len(ts)
    assert all(t.bulk.converged(conv) and t.surf(t.bulk.count).converged(conv) for t in ts)


@pytest.mark.parametrize("conv", xb.FREE_CONVS)
def test_free_running_oracle_meets_the_bar(conv):
    """The float64 loops (LAPACK inverse), free running, stop at the truth's counts and stay within the bar there.  The
    free grids are not part of the calibration table; the worst ratio sits at E = 5 (kappa_max 1.6, where the products'
    roundings and not the inverses set the error): 2.0 at c = 1, half the bar."""
    worst = 0.0
    for t in xb.free_truths(conv):
        tr = xb.bulk(t.lat, t.E, xb.FREE_MIX, conv=conv, inv=np.linalg.inv, ld=False, extra=0)
        assert tr.count == t.bulk.count, t.E
        c = tr.count
        ts = xb.surface(t.lat, t.E, tr.at[c], xb.FREE_MIX, conv=conv, inv=np.linalg.inv, ld=False, extra=0)
        su = t.surf(c)
        assert ts.count == su.count, t.E
        worst = max(worst, xb.sweep_ratio(tr.at[c], t.bulk.at[c], t.bulk.kappa[c - 1]),
                    xb.sweep_ratio(ts.at[ts.count], su.at[su.count], su.kappa[su.count - 1]))
    print(f"CAL bethe free conv={conv:g} LAPACK: worst ratio {worst:.3g}")
    assert worst <= 1.0
