"""
Accuracy of the HIP Green's-function path against the extended-precision truth of tests/xprec.py, with bars that
follow from the condition number (||G_hat e_j - G e_j|| / ||G e_j|| <= C_BAR sqrt(n) u kappa_2(A), every sampled
column) instead of the 1e-8 parity tolerance: every inverse family forced onto the case table (ill-conditioned
ladder, zero-diagonal bipartite, rotated, graded), the derived quantities against their propagated bars, and exact
scale equivariance.  Each line 'ACC ...' printed reports the worst ratio error / bar of one family x case.
"""
import functools

import numpy as np
import pytest

import xprec
from xprec import C_BAR, Truth

pytestmark = pytest.mark.gpu

xprec.require_extended()


@functools.lru_cache(maxsize=None)
def _table(n):
    return {c.name: c for c in xprec.case_table(n)}


@functools.lru_cache(maxsize=None)
def _g2c(n):
    return xprec.bipartite(n, confined=True)


@pytest.fixture(scope="module")
def truth():
    """Truths computed once per (base case, n) for the whole module; rotated / scaled cases derive theirs exactly."""
    cache = {}

    def get(case):
        base = case.base or case
        key = (base.name, base.n)
        if key not in cache:
            cache[key] = Truth(base)
        return cache[key] if case.base is None else Truth.of(case, cache[key])
    return get


def _provider(case):
    """The production const provider for the formSigma cases (its matrices checked bitwise against the case's); the
    rotated and scaled cases go in through the precomputed-Sigma path as given."""
    if case.base is None and case.name in ("G1", "G2", "G4"):
        from gaunegf_amd.surfGTester import surfGTest
        g = surfGTest(case.F, case.S, case.inds, -1j * xprec.GAMMA)
        assert all(np.array_equal(a, b) for a, b in zip(g.sig, case.sigs))
        return g
    return xprec.ForeignConst(case)


def _force(engine, family):
    if family == "small0":
        engine.set_small_algo(0)
    elif family == "small1":
        engine.set_small_algo(1)
    elif family != "auto":
        engine.set_inverse_algo(int(family[-1]))


def _restore(engine):
    engine.set_inverse_algo(0)
    engine.set_small_algo(0)
    engine.set_gamma_algo(0)


def _report(what, ratios):
    print(f"ACC {what}: worst ratio {max(ratios):.3g}")


FAMILIES = ([("small0", n) for n in (2, 17, 33, 64, 65, 96)] + [("small1", n) for n in (2, 17, 33, 64, 65, 96)] +
            [("algo1", n) for n in (17, 100, 256)] + [("algo2", n) for n in (64, 200, 256)] +
            [("algo3", n) for n in (100, 209, 256, 333, 449, 513, 650)] +
            [("algo4", n) for n in (100, 209, 333, 513, 650)])


@pytest.mark.parametrize("family,n", FAMILIES)
def test_inverse_family_on_case_table(engine, truth, family, n):
    """Every sampled column of G(E) within the conditioning bar for every case of the table: small0 / small1 =
    negf_set_small_algo 0 (the fused n <= 96 kernel) / 1 (the kernel sequence of larger systems), algoK =
    negf_set_inverse_algo K (1 unblocked, 2 blocked MFMA, 3 register-strip windows, 4 team windows)."""
    from gaunegf_amd.integrate import GrBatch
    fails = []
    for name, case in _table(n).items():
        t = truth(case)
        _force(engine, family)
        try:
            G = GrBatch(case.F, case.S, _provider(case), case.energies)
        finally:
            _restore(engine)
        ratios = [t.ratio(m, G[m]) for m in range(case.energies.size)]
        _report(f"{family} n={n} {name}", ratios)
        fails += [(name, m, r) for m, r in enumerate(ratios) if not r <= 1.0]
    assert not fails, (family, n, fails)


def test_auto_large_batch_ladder_spread(engine, truth):
    """n = 300, M = 480 under the automatic choice: the six ladder energies sit first, last and either side of the
    multiples of 120 in a batch of well-conditioned points."""
    from gaunegf_amd.integrate import GrBatch
    case = _table(300)["G1"]
    t = truth(case)
    M = 480
    E = np.linspace(-2.5, 2.5, M) + 0.02j
    pos = [0, 119, 120, 240, 359, M - 1]
    E[pos] = case.energies
    G = GrBatch(case.F, case.S, _provider(case), E)
    ratios = [t.ratio(m, G[p]) for m, p in enumerate(pos)]
    _report("auto n=300 M=480 G1", ratios)
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_auto_1030_pairs(engine, truth, name):
    """n = 1030 in batches of two: the <8,4> class (four rows per lane, sub-panels of 8 columns, the team window kernel --
    there is no strip kernel beyond sub-panels of 16), one stream group, the windows one by one with fat updates."""
    from gaunegf_amd.integrate import GrBatch
    plan = engine.inverse_plan(1030, 2)
    assert plan["path"] == 2 and plan["cls"] == (8, 4) and [g["wk"] for g in plan["groups"]] == [9]
    assert [(g["pairs"], g["upd_full"]) for g in plan["groups"]] == [(0, 8)]
    case = _table(1030)[name]
    t = truth(case)
    g = _provider(case)
    ratios = []
    for a in range(0, case.energies.size, 2):
        G = GrBatch(case.F, case.S, g, case.energies[a:a + 2])
        ratios += [t.ratio(a + k, G[k]) for k in range(G.shape[0])]
    _report(f"auto n=1030 M=2 {name}", ratios)
    assert max(ratios) <= 1.0, ratios


# --------------------------------------------------------------------------- #
# derived quantities
# --------------------------------------------------------------------------- #
def _weights(M, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(M) + 1j * rng.standard_normal(M)


@pytest.mark.parametrize("n", [64, 200, 300])
def test_grint_ladder_against_bar(engine, truth, n):
    """GrInt = sum_m w_m G(E_m) at the ladder energies, per sampled column j:
    ||GrInt e_j - sum_m w_m G_m e_j|| <= sum_m |w_m| (delta_m + M u) ||G_m e_j||  (delta_m = C_BAR sqrt(n) u kappa_m).
    n = 64: the fused small kernel's partial sums; 200: the single-workgroup inverse; 300: the windowed inverse, whose
    weighted sum reads the un-gathered matrices through the pivot permutation."""
    from gaunegf_amd.integrate import GrInt
    case = _table(n)["G1"]
    t = truth(case)
    w = _weights(case.energies.size)
    ref, bound = xprec.grint_truth_and_bound(t, w)
    P = GrInt(case.F, case.S, _provider(case), case.energies, w)
    err = np.linalg.norm((P[:, t.cols].astype(xprec.LD) - ref).astype(np.complex128), axis=0)
    ratios = err / bound
    _report(f"GrInt n={n} G1", ratios)
    assert ratios.max() <= 1.0, (int(np.argmax(ratios)), ratios.max())


_GLESS_TRUTH = {}


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("name", ["G1", "G2c"])
@pytest.mark.parametrize("ind", [None, 0, -1])
@pytest.mark.parametrize("gamma_algo", [0, 1])
def test_grlessint_against_bar(engine, truth, n, name, ind, gamma_algo):
    """GrLessInt = sum_m w_m G_m Gamma G_m^H (Gamma of the total Sigma or of one contact), in Frobenius norm:
    ||dP||_F <= sum_m |w_m| [2 delta_m ||G_m||_F ||Gamma G_m^H||_2 + gamma_4n || |G_m| |Gamma| |G_m^H| ||_F]
               + M u sum_m |w_m| ||G_m Gamma G_m^H||_F
    (gamma_4n: two products of inner dimension n, doubled for the normwise bound of 3M complex products).  G1 carries
    formSigma's dense -1e-9 i S background (dense Gamma products); G2c's contacts are confined to their orbitals, so
    negf_set_gamma_algo 0 takes the compact products and 1 the dense ones."""
    from gaunegf_amd.integrate import GrLessInt
    case = _table(n)["G1"] if name == "G1" else _g2c(n)
    t = truth(case)
    w = _weights(case.energies.size, 7)
    key = (name, n, ind)
    if key not in _GLESS_TRUTH:
        _GLESS_TRUTH[key] = xprec.grless_truth_and_bound(t, w, ind)
    ref, bound = _GLESS_TRUTH[key]
    engine.set_gamma_algo(gamma_algo)
    try:
        P = GrLessInt(case.F, case.S, _provider(case), case.energies, w, ind)
    finally:
        _restore(engine)
    err = float(np.linalg.norm((P.astype(xprec.LD) - ref).astype(np.complex128)))
    _report(f"GrLessInt n={n} {name} ind={ind} gamma_algo={gamma_algo}", [err / bound])
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("name", ["G1", "G2c"])
def test_transmission_against_bar(engine, truth, n, name):
    """T(E) = Tr(Gamma_1 G Gamma_2 G^H) per energy:
    |dT| <= 2 delta ||G||_F ||Gamma_1 G Gamma_2||_F + gamma_4n Tr(|Gamma_1| |G| |Gamma_2| |G^H|)."""
    from gaunegf_amd.transport import SigmaCalculator, calculate_transmission
    case = _table(n)["G1"] if name == "G1" else _g2c(n)
    t = truth(case)
    ref, bound = xprec.transmission_truth_and_bound(t)
    T = calculate_transmission(case.F, case.S, SigmaCalculator(case.sigs[0], case.sigs[1]), case.energies)
    ratios = np.abs(np.asarray(T) - ref) / bound
    _report(f"transmission n={n} {name}", ratios)
    assert ratios.max() <= 1.0, (ratios, T, ref)


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_dos_against_bar(engine, truth, n, name):
    """DOS = -Im G_ii / pi per site and summed (every diagonal entry: n <= 256):
    |d dos_i| <= (delta ||G e_i|| + u |G_ii|) / pi,  |d dos| <= sum_i (delta ||G e_i|| + n u |G_ii|) / pi."""
    from gaunegf_amd.transport import SigmaCalculator, calculate_dos
    case = _table(n)[name]
    t = truth(case)
    tot_ref, site_ref, btot, bsite = xprec.dos_truth_and_bound(t)
    tot, site = calculate_dos(case.F, case.S, SigmaCalculator(case.sigs[0], case.sigs[1]), case.energies)
    r_site = np.abs(site - site_ref) / bsite
    r_tot = np.abs(tot - tot_ref) / btot
    _report(f"dos n={n} {name}", [r_site.max(), r_tot.max()])
    assert r_site.max() <= 1.0 and r_tot.max() <= 1.0, (r_site.max(), r_tot.max())


# --------------------------------------------------------------------------- #
# G5: exact scale equivariance
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("family,n", [("small0", 33), ("small1", 64), ("algo1", 100), ("algo2", 200), ("algo3", 100),
                                      ("algo3", 333), ("algo4", 333), ("auto", 300), ("auto", 1030)])
@pytest.mark.parametrize("k", [64, -64])
def test_scale_equivariance_bitwise(engine, family, n, k):
    """E, F, Sigma -> 2^k (E, F, Sigma) maps A -> 2^k A and G -> 2^-k G exactly.  Every operation of the inverse paths
    is equivariant under a power-of-two scale for normal numbers: pivot keys |re| + |im| (and their high words) keep
    their order, 1/p = conj(p) / |p|^2 (v_rcp_f64 plus Newton steps) scales by 2^-k, and the 3M products and updates
    only multiply and add.  So each path returns bitwise 2^-k times its unscaled result."""
    from gaunegf_amd.integrate import GrBatch
    base = _table(n)["G1"]
    sc = xprec.scaled(base, k)
    E = base.energies if n < 1000 else base.energies[4:6]
    Es = sc.energies if n < 1000 else sc.energies[4:6]
    _force(engine, family)
    try:
        G0 = GrBatch(base.F, base.S, xprec.ForeignConst(base), E)
        Gk = GrBatch(sc.F, sc.S, xprec.ForeignConst(sc), Es)
    finally:
        _restore(engine)
    back = Gk * 2.0 ** k
    diff = np.abs(back - G0).max() / np.abs(G0).max()
    print(f"ACC G5 {family} n={n} k={k}: max |2^k G_k - G_0| / max |G_0| = {diff:.3g}")
    assert np.array_equal(back, G0), diff
