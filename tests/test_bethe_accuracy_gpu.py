"""
Accuracy of the Bethe-lattice self-energy kernel (bethe_kernel: wave_inv9, the two-phase bulk sweep, the surface loop
and the atom assembly) against the extended-precision truth of tests/xprec_bethe.py:
  * B4, its inverse alone: every column of all twelve blocks of one sweep within the inverse bar of tests/xprec.py
    (k < 6: the six waves' own LDS slots on the same matrix; k >= 6: phase 1, with the first-order term of g's error);
  * B1-B3 at K in {1, 3, 10, 25} sweeps: sigmaK, sigma (K bulk and K surface sweeps), the cluster's sigmaTot and the
    assembled contacts of a surfGB, attached directions outside 0..8 included, within C_BETHE u kappa_max ||sigma_k||;
  * free running at conv = 1e-5 and 1e-8: the sweep counts are the truth's (one off only where the truth's diff sits
    on conv), the flags match and the result is within the bar of the truth at the device's own count;
  * launch geometry: a batch equals its energies one per call, and a two-contact surfGB with a different lattice per
    contact equals the raw single-atom launches, bit for bit;
  * containment: a non-finite energy gives a non-finite record flagged not converged and leaves the others alone.
Each line 'ACC bethe ...' reports the worst ratio error / bar of one case.
"""
import numpy as np
import pytest

import xprec
import xprec_bethe as xb
from helpers import random_system

pytestmark = pytest.mark.gpu

xprec.require_extended()


def _report(what, ratios):
    print(f"ACC bethe {what}: worst ratio {max(ratios):.3g}")


def _raw(engine, lat, E, which, K=-1, mix=0.5, conv=1e-5):
    out = engine.bethe_raw(lat.H, lat.S, lat.V, lat.eta, conv, np.atleast_1d(E), which, mix=mix,
                           max_iter=xb.MAX_ITER, force_iters=K)
    return out, engine.last_iters.copy(), engine.last_converged.copy()


# --------------------------------------------------------------------------- #
# B4: the inverse alone
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("f", range(4))
def test_b4_inverse(engine, f):
    """S_k = 0, V_k = -I, mix = 1, one sweep: sigma_k = g_k.  k < 6: ((x + i d) I - H)^-1 from each of the six waves;
    k >= 6: phase 1's (M + i I + g_hat)^-1."""
    fam = xb.b4_families()[f]
    out, its, _ = _raw(engine, fam.lat, fam.energies, 1, K=1, mix=1.0)
    assert np.all(its == 1)
    first, second, fails = [], [], []
    for m in range(len(fam.points)):
        t = xb.b4_truth(f, m)
        r1 = [t.ratio_first(out[m, k]) for k in range(6)]
        r2 = [t.ratio_second(out[m, k]) for k in range(6, 12)]
        print(f"ACC bethe B4 {fam.name} x={fam.points[m][0]:.6g} d={fam.points[m][1]:.3g} kappa={t.kappa1:.3g}/"
              f"{t.kappa2:.3g}: k<6 {max(r1):.3g}  k>=6 {max(r2):.3g}")
        first += r1; second += r2
        if not (max(r1) <= 1.0 and max(r2) <= 1.0):
            fails.append((m, r1, r2))
    _report(f"B4 {fam.name} k<6", first)
    _report(f"B4 {fam.name} k>=6", second)
    assert not fails, fails


# --------------------------------------------------------------------------- #
# B1-B3 at fixed sweep counts
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("ci", range(6))
def test_sweeps_against_bar(engine, ci):
    """sigmaK, sigma and the cluster's sigmaTot after K sweeps, every direction within the bar."""
    from gaunegf_amd.surfGBethe import surfGBAt
    lat = xb.sweep_cases()[ci]
    at = surfGBAt(lat.H, list(lat.S), list(lat.V), lat.eta)
    worst, fails = {"sigmaK": 0.0, "sigma": 0.0, "sigmaTot": 0.0}, []
    for K in xb.K_CHECKED:
        at.force_iters = K
        sK = at.sigmaK(lat.energies)
        assert np.all(at.last_iters == K)
        s9 = at.sigma(lat.energies)
        assert np.all(at.last_iters == K + (K << 16))
        for m, E in enumerate(lat.energies):
            t = xb.sweep_truth(ci, m)
            cl = at.sigmaTot(E)
            blocks = np.stack([cl[9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(12)])
            off = cl.copy()
            for k in range(12):
                off[9 * k:9 * k + 9, 9 * k:9 * k + 9] = 0
            assert not off.any()
            r = dict(sigmaK=xb.sweep_ratio(sK[m], t.bulk[K], t.kappa_bulk[K]),
                     sigma=xb.sweep_ratio(s9[m], t.surf[K], t.kappa_surf[K]),
                     sigmaTot=xb.cluster_ratio(blocks, t.bulk[K], t.kappa_bulk[K]))
            for what, v in r.items():
                worst[what] = max(worst[what], v)
                if not v <= 1.0:
                    fails.append((what, K, complex(E), v))
    for what, v in worst.items():
        _report(f"{lat.name} {what}", [v])
    assert not fails, fails


def _device(N=60):
    """Two contacts of three atoms x 9 orbitals at the ends of an N-orbital device (the geometry of the parity tests)."""
    coords = np.array([[0, 0, 0.0], [2.88, 0, 0], [1.44, 2.494, 0],
                       [0, 0, 20.0], [2.88, 0, 20.0], [1.44, 2.494, 20.0],
                       [1.44, 0.8, 10.0]])
    orbMap = np.concatenate([np.full(9, a + 1) for a in range(6)] + [np.full(N - 54, 7)])
    typ_one = np.array([0, 1001, 1002, 1003, 2001, 2002, 2003, 2004, 2005])
    orbTyp = np.concatenate([typ_one] * 6 + [np.zeros(N - 54, dtype=int)])
    return coords, orbMap, orbTyp


def _surfgb(eta, second=None, N=60):
    """A two-contact surfGB on the Au table; `second`: the table of the second contact's lattice, if another."""
    from gaunegf_amd.surfGBethe import construct_sk_matrix, read_bethe_params, surfGB, surfGBAt
    coords, orbMap, orbTyp = _device(N)
    F, S = random_system(N, 77)
    g = surfGB.from_arrays(F, S, [[1, 2, 3], [4, 5, 6]], orbMap, orbTyp, coords, latFile=xb.data_file("Au"), eta=eta,
                           fermi=0.0)
    assert g.Sdict['sss'] != 0                                   # no Xi products after the assembly
    if second is not None:
        _, _, Vd, Sd, H0 = read_bethe_params(xb.data_file(second))
        at = surfGBAt(H0, [construct_sk_matrix(Sd, d) for d in g.dirLists[1]],
                      [construct_sk_matrix(Vd, d) for d in g.dirLists[1]], eta)
        at.fermi = 0.0
        g.gList[1] = at
        g._version += 1
    return g


def _atom_blocks(g, i, sig):
    """The 9x9 blocks of the atoms of contact i in an assembled N x N matrix, and whether all else is zero."""
    rest = sig.copy()
    blocks = []
    for inds in g.indsLists[i]:
        blocks.append(sig[np.ix_(inds, inds)])
        rest[np.ix_(inds, inds)] = 0
    return blocks, not rest.any()


@pytest.mark.parametrize("K", [3, 25])
def test_assembled_contacts_against_bar(engine, K):
    """surfGB.sigma(E, i): every atom's block = sum of the nine surface blocks minus the attached ones, within the sum
    bar; with the directions found from the geometry and with directions outside 0..8 (wrapped, then clamped)."""
    g = _surfgb(1e-6)
    g.force_iters = K
    worst, fails = 0.0, []
    for variant in range(2):
        if variant == 1:
            g.nIndLists = [[[0, 9], [-1, 3, 11]] + [list(v) for v in g.nIndLists[0][2:]],
                           [[12, -9, 4]] + [list(v) for v in g.nIndLists[1][1:]]]
            g._version += 1
        for E in (-4.0, 0.5, -2.0 + 0.3j):
            for i in (0, 1):
                at = g.gList[i]
                lat = xb.Lattice("contact", at.H, np.stack(at.Slist), np.stack(at.Vlist), g.eta)
                t = xb.SweepTruth(lat, E, ks=(K,))
                blocks, rest_zero = _atom_blocks(g, i, g.sigma(E, i))
                assert rest_zero
                for a, nbs in enumerate(g.nIndLists[i]):
                    true, used = xb.atom_sigma(t.surf[K], nbs)
                    r = xb.sum_ratio(blocks[a], true, t.surf[K], used, t.kappa_surf[K])
                    worst = max(worst, r)
                    if not r <= 1.0:
                        fails.append((variant, complex(E), i, a, r))
    _report(f"assembled contacts K={K}", [worst])
    assert not fails, fails


# --------------------------------------------------------------------------- #
# free running
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("conv", xb.FREE_CONVS)
def test_free_running(engine, conv):
    """Sweep counts (bulk; surface in the upper half-word), flags and results of the free-running loops."""
    ts = xb.free_truths(conv)
    lat = ts[0].lat
    E = np.array([t.E for t in ts])
    sK, itK, cvK = _raw(engine, lat, E, 1, mix=xb.FREE_MIX, conv=conv)
    s9, it9, cv9 = _raw(engine, lat, E, 2, mix=xb.FREE_MIX, conv=conv)
    n_amb, rK, r9, fails = 0, [], [], []
    for m, t in enumerate(ts):
        cb, cs = int(it9[m]) & 0xFFFF, int(it9[m]) >> 16
        assert int(itK[m]) == cb, (m, itK[m], it9[m])             # the same bulk loop in both launches
        slack_b = 1 if t.bulk.ambiguous(conv) else 0
        if abs(cb - t.bulk.count) > slack_b:
            fails.append(("bulk count", m, cb, t.bulk.count))
            continue
        surf = t.surf(cb)
        slack_s = 1 if surf.ambiguous(conv) else 0
        n_amb += bool(slack_b or slack_s)
        if abs(cs - surf.count) > slack_s:
            fails.append(("surface count", m, cs, surf.count))
            continue
        flag_b = int(t.bulk.diffs[cb - 1] <= conv)
        flag_s = int(surf.diffs[cs - 1] <= conv)
        if not slack_b and (int(cvK[m]) != flag_b or (int(cv9[m]) & 1) != flag_b):
            fails.append(("bulk flag", m, int(cvK[m]), int(cv9[m]), flag_b))
        if not slack_s and (int(cv9[m]) >> 1) != flag_s:
            fails.append(("surface flag", m, int(cv9[m]), flag_s))
        rK.append(xb.sweep_ratio(sK[m], t.bulk.at[cb], t.bulk.kappa[cb - 1]))
        r9.append(xb.sweep_ratio(s9[m], surf.at[cs], surf.kappa[cs - 1]))
        if not (rK[-1] <= 1.0 and r9[-1] <= 1.0):
            fails.append(("bar", m, rK[-1], r9[-1]))
    print(f"ACC bethe free conv={conv:g}: counts {[(int(v) & 0xFFFF, int(v) >> 16) for v in it9]}, "
          f"ambiguous {n_amb} of {len(ts)}")
    _report(f"free conv={conv:g} sigmaK", rK or [np.inf])
    _report(f"free conv={conv:g} sigma", r9 or [np.inf])
    assert not fails, fails
    assert n_amb <= xb.AMBIGUOUS_CAP * len(ts)


# --------------------------------------------------------------------------- #
# launch geometry
# --------------------------------------------------------------------------- #
def test_batch_equals_single_launches(engine):
    """320 energies in one launch (blockIdx.y = energy) against one launch each, bit for bit: ten sweeps, and free
    running with the counts and flags."""
    lat = xb.shipped("Au", 1e-4)
    rng = np.random.default_rng(5)
    E = np.concatenate([np.linspace(-9.0, 7.0, 256), rng.uniform(-9, 7, 64) + 1j * rng.uniform(0.01, 3.0, 64)])
    for which in (1, 2):
        for K, conv in ((10, 1e-5), (-1, 1e-3)):
            out, its, cv = _raw(engine, lat, E, which, K=K, conv=conv)
            for m in range(E.size):
                o1, i1, c1 = _raw(engine, lat, E[m], which, K=K, conv=conv)
                assert np.array_equal(o1[0], out[m]) and i1[0] == its[m] and c1[0] == cv[m], (which, K, m)


def test_two_lattices_equal_raw_launches(engine):
    """A surfGB whose contacts carry different lattices (Au, Au2: blockIdx.x = contact and the strides of H, Slist and
    Vlist): every atom's block equals the raw single-atom launch of its contact's lattice, assembled on the host in the
    kernel's order, bit for bit."""
    g = _surfgb(1e-4, second="Au2")
    E = np.array([-4.0, 0.5, 2.5, -2.0 + 0.3j, 0.3 + 2.0j])
    for K in (7, -1):
        g.force_iters = K
        for at in g.gList:
            at.force_iters = K
        for i in (0, 1):
            got, its, cv = g.sigma_batch(E, i)
            raw = g.gList[i].sigma(E)
            assert np.array_equal(its[:, i], g.gList[i].last_iters) and np.array_equal(cv[:, i], g.gList[i].last_converged)
            for m in range(E.size):
                blocks, rest_zero = _atom_blocks(g, i, got[m])
                assert rest_zero
                for a, nbs in enumerate(g.nIndLists[i]):
                    assert np.array_equal(blocks[a], xb.atom_sigma(raw[m], nbs)[0]), (K, i, m, a)
        # the two lattices differ, and so do the contacts
        assert not np.array_equal(g.gList[0].sigma(E[:1]), g.gList[1].sigma(E[:1]))


# --------------------------------------------------------------------------- #
# containment
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("bad", [complex(np.nan, 0.0), complex(np.inf, 0.0), complex(0.5, np.nan)])
def test_non_finite_energy_is_contained(engine, bad):
    """One non-finite energy in a batch: its record is non-finite and flagged not converged (bulk and surface), every
    other record, count and flag is bitwise what it is without it.  (The loops end on a NaN diff: `diff > conv` is
    false for it, and the sweep count is bounded by max_iter in any case.)"""
    lat = xb.shipped("Au", 1e-4)
    E = np.array([-9.0, -4.0, 0.5, 2.5, -2.0 + 0.3j, 0.3 + 2.0j, 6.0, -1.0], dtype=np.complex128)
    Eb = E.copy()
    Eb[3] = bad
    keep = np.arange(E.size) != 3
    for which in (1, 2):
        for K in (5, -1):
            ref, it0, cv0 = _raw(engine, lat, E, which, K=K)
            out, its, cv = _raw(engine, lat, Eb, which, K=K)
            assert not np.isfinite(out[3]).all(), (which, K)
            assert cv[3] == 0, (which, K, int(cv[3]), int(its[3]))
            assert np.array_equal(out[keep], ref[keep]) and np.array_equal(its[keep], it0[keep])
            assert np.array_equal(cv[keep], cv0[keep])
            assert np.isfinite(ref).all()
