"""
The inverse, product and chain kernels on the MI355X against extended-precision truth on inputs whose rows and columns
differ: the complex-Hermitian cases of tests/xprec_hermitian.py (G6, G6c, L4 and the layered case h).  Every other truth
case of the suite is complex symmetric, where G = G^T: a transposed write-back, a G^H conjugated but not transposed,
contact rows for contact columns and exchanged contacts pass there (test_hermitian_host.py measures it).
  a. every inverse family forced onto G6, through the const provider and through the precomputed-Sigma assemble
  b. four cells of the automatic launch rule (pairs, side streams, lean updates, the un-gathered read) with G6 in the
     ladder's place, residuals from both sides
  c. the classes (4,8) and (2,16), n = 2049 and 4097, by both residuals
  d. GrInt, GrLessInt, T in both orders of the contacts and the DOS on G6c against their propagated bars
  e. the stored-conjugate-transpose products at N = 200 ... 720 against float64 numpy
  f. the chain kernels: their inverse on G6, K sweeps on L4, two unequal Hermitian leads in one provider
  g. the layered path on case h
Lines 'ACC herm ...' report the worst ratio error / bar of one kernel x case.
"""
import functools

import numpy as np
import pytest

import rgf_ref as rr
import xprec
import xprec_chain as xc
import xprec_hermitian as xh
from helpers import rel_fro
from test_chain_accuracy_gpu import GLOBAL_SIZES, KMAX, LDS_SIZES, SWEEP_SIZES, _one_contact
from test_inverse_cells_gpu import CELLS, DOWNLOAD_MAX, _kern, _masks, _names, _one_hot, _place
from xprec import LD, Truth

pytestmark = pytest.mark.gpu

xprec.require_extended()

S256, S512, S1024, LA12, TEAM, SINGLE = 1, 5, 6, 8, 9, 10
TOL = 1e-8                           # the project's parity bar (test_gpu_parity.TOL)


def _report(what, ratios):
    print(f"ACC herm {what}: worst ratio {max(ratios):.3g}")


def _const(case):
    """The production CONST path: surfGTest with the case's matrices in place of formSigma's before first use."""
    from gaunegf_amd.surfGTester import surfGTest
    g = surfGTest(case.F, case.S, case.inds)
    g.sig = [np.ascontiguousarray(s) for s in case.sigs]
    return g


@functools.lru_cache(maxsize=None)
def _g6_case(n):
    case = xh.hermitian_ladder(n)
    return case, _const(case)


@functools.lru_cache(maxsize=None)
def _g6(n):
    """(case, truth, const provider) of G6 at dimension n, once per module."""
    case, g = _g6_case(n)
    return case, Truth(case), g


@functools.lru_cache(maxsize=None)
def _g6c(n):
    case = xh.hermitian_confined(n)
    return case, Truth(case), _const(case)


def _force(engine, family):
    if family == "small0":
        engine.set_small_algo(0)
    elif family == "small1":
        engine.set_small_algo(1)
    else:
        engine.set_inverse_algo(int(family[-1]))


def _restore(engine):
    engine.set_inverse_algo(0)
    engine.set_small_algo(0)
    engine.set_gamma_algo(0)


# --------------------------------------------------------------------------- #
# a. the inverse families on G6
# --------------------------------------------------------------------------- #
SPLIT_FROM = 1025                    # from here on one test per energy: the truth of six energies costs 10 s of CPU
FAMILIES = ([("small0", n, None) for n in (2, 17, 33, 64, 65, 96)] + [("small1", n, None) for n in (2, 17, 33, 64, 65, 96)] +
            [("algo1", n, None) for n in (17, 100)] + [("algo2", n, None) for n in (64, 200, 256)] +
            [("algo3", n, None) for n in (100, 257, 513)] + [("algo4", n, None) for n in (257, 513)] +
            [("algo4", 1025, m) for m in range(6)])
# (family, n >= 100) -> path, class, window kernel of the one group of six energies (none on the unblocked path)
PLANS = {("algo1", 100): (0, (0, 0), []), ("algo2", 200): (1, (0, 0), [SINGLE]), ("algo2", 256): (2, (16, 1), [S256]),
         ("algo3", 100): (2, (16, 1), [S256]), ("algo3", 257): (2, (16, 1), [S512]), ("algo3", 513): (2, (16, 2), [S1024]),
         ("algo4", 257): (2, (16, 1), [LA12]), ("algo4", 513): (2, (16, 2), [TEAM]), ("algo4", 1025): (2, (8, 4), [TEAM])}


@functools.lru_cache(maxsize=None)
def _g6_one(n, m):
    """(case, truth of energy m alone, const provider) of G6 at a dimension whose six truths are too much for one test."""
    case, g = _g6_case(n)
    one = xprec.Case(case.name, n, case.F, case.S, case.inds, case.sigs, case.energies[m:m + 1], resonant=case.resonant)
    return case, Truth(one), g


@pytest.mark.parametrize("family,n,only", FAMILIES, ids=[f"{f}-{n}" + ("" if m is None else f"-E{m}") for f, n, m in FAMILIES])
def test_inverse_family_on_g6(engine, family, n, only):
    """Every sampled column of G(E) within the conditioning bar, the six energies of G6 in one batch, as
    test_accuracy_gpu.test_inverse_family_on_case_table.  From n = 100 on the window kernel and the class are asserted
    through Engine.inverse_plan before the call and Engine.inverse_last after it.  n = 1025 runs the batch of six once
    per energy and checks that energy against its truth (`only`): the size stays, the truth's CPU time is split."""
    from gaunegf_amd.integrate import GrBatch
    assert (only is None) == (n < SPLIT_FROM)
    case, t, g = _g6(n) if only is None else _g6_one(n, only)
    M = case.energies.size
    providers = [("const", g)] + ([("precomputed", xprec.ForeignConst(case))] if n <= 96 else [])
    plan = None
    if n >= 100:
        plan = engine.inverse_plan(n, M, algo=int(family[-1]))
        got = (plan["path"], plan["cls"], [gr["wk"] for gr in plan["groups"]])
        assert got == PLANS[family, n], (family, n, got)
    fails = []
    for tag, prov in providers:
        _force(engine, family)
        try:
            G = GrBatch(case.F, case.S, prov, case.energies)
            last = engine.inverse_last()
        finally:
            _restore(engine)
        if plan is not None:
            assert last == {"path": plan["path"], "masks": _masks(plan)}, (family, n, last, _masks(plan))
        ratios = [t.ratio(m, G[m]) for m in range(M)] if only is None else [t.ratio(0, G[only])]
        _report(f"{family} n={n} G6 {tag}" + ("" if only is None else f" energy {only}"), ratios)
        fails += [(tag, m, r) for m, r in enumerate(ratios) if not r <= 1.0]
    assert not fails, (family, n, only, fails)


# --------------------------------------------------------------------------- #
# b. cells of the automatic rule
# --------------------------------------------------------------------------- #
HERM_CELLS = [c for c in CELLS if (c[0], c[1]) in ((100, 257), (257, 255), (257, 344), (513, 148))]


@pytest.mark.parametrize("n,nb,name,path,cls,cnt,wk,pairs,full,single", HERM_CELLS,
                         ids=[f"{c[0]}x{c[1]}" for c in HERM_CELLS])
def test_cell_on_g6(engine, n, nb, name, path, cls, cnt, wk, pairs, full, single):
    """test_inverse_cells_gpu.test_cell_against_the_conditioning_bar with G6 in the ladder's place: the ladder energies
    within the bar, the fillers' residuals from BOTH sides (||G A - I|| and ||A G - I||, over sqrt(n), below 1e-9: on G6
    the two differ), second copies bitwise."""
    from gaunegf_amd.integrate import GrBatch
    assert len(HERM_CELLS) == 4
    plan = engine.inverse_plan(n, nb)
    got = (plan["path"], plan["cls"], [g["count"] for g in plan["groups"]], [g["wk"] for g in plan["groups"]],
           [g["pairs"] for g in plan["groups"]], [g["upd_full"] for g in plan["groups"]],
           [g["upd_single"] for g in plan["groups"]])
    assert got == (path, cls, cnt, wk, pairs, full, single), (name, got)
    case, t, g = _g6(n)
    assign, gid = _place(plan, nb)
    assert set(assign.values()) == set(range(6)) and {gid(p) for p in assign} == set(range(len(cnt)))
    E = np.linspace(-2.5, 2.5, nb) + 0.02j
    for p, k in assign.items():
        E[p] = case.energies[k]
    rng = np.random.default_rng(1000 * n + nb)
    free = np.array([p for p in range(nb) if p not in assign])
    fillers = [int(p) for p in rng.choice(free, min(8, free.size), replace=False)]
    sig = case.sig_tot
    kern = lambda p: _kern(plan["groups"][gid(p)])
    forms = []
    if 16.0 * n * n * nb <= DOWNLOAD_MAX:
        forms.append("GrBatch")
    if 16.0 * n * n * nb > DOWNLOAD_MAX or (n, nb) == (257, 255):
        forms.append("GrInt")
    engine.set_batch(nb)
    try:
        for form in forms:
            if form == "GrBatch":
                G = GrBatch(case.F, case.S, g, E)
                last, want = engine.inverse_last(), plan
                get = lambda p: G[p]
            else:
                want = engine.inverse_plan(n, nb, defer=True)
                cache = {}
                def get(p, cache=cache):
                    if p not in cache:
                        cache[p] = _one_hot(case.F, case.S, g, E, p)
                    return cache[p]
                get(next(iter(assign)))
                last = engine.inverse_last()
            assert last == {"path": want["path"], "masks": _masks(want)}, (name, form, last, _masks(want))
            ratios = {p: t.ratio(k, get(p)) for p, k in assign.items()}
            left, right = [], []
            for p in fillers:
                A = E[p] * case.S - case.F - sig
                left.append(np.linalg.norm(get(p) @ A - np.eye(n)) / np.sqrt(n))
                right.append(np.linalg.norm(A @ get(p) - np.eye(n)) / np.sqrt(n))
            print(f"ACC herm cell n={n} nb={nb} [{name}] {form}: kernels {_names(engine, plan)} masks "
                  f"{[hex(m) for m in last['masks']]}; worst ratio {max(ratios.values()):.3g} (ladder index "
                  f"{assign[max(ratios, key=ratios.get)]}), worst filler residual G A {max(left):.3g}, A G {max(right):.3g}")
            bad = {p: r for p, r in ratios.items() if not r <= 1.0}
            assert not bad, (name, form, bad)
            assert all(r < 1e-9 for r in left + right), (name, form, left, right)
            twins = 0
            for k in range(6):
                ps = [p for p in assign if assign[p] == k]
                for q in ps[1:]:
                    if gid(q) != gid(ps[0]) and kern(q) == kern(ps[0]):
                        assert np.array_equal(get(q), get(ps[0])), (name, form, k, ps[0], q)
                        twins += 1
            assert twins >= 1 or len({kern(p) for p in assign}) == len(cnt), (name, "no second copy in a group of the same kernels")
    finally:
        engine.set_batch(0)


# --------------------------------------------------------------------------- #
# c. the classes (4,8) and (2,16)
# --------------------------------------------------------------------------- #
_BIG = {}


def _big(n):
    """G6's F, S and Sigma at a size beyond any truth; one size is kept at a time (a gigabyte at n = 4097)."""
    if n not in _BIG:
        _BIG.clear()
        F, S, inds, sigs, _, _ = xh.matrices(n)
        case = xprec.Case("G6", n, F, S, inds, sigs, [0.3 + 2j, -0.7 + 0.02j])
        _BIG[n] = (case, _const(case))
    return _BIG[n]


@pytest.mark.parametrize("m", [0, 1], ids=["0.3+2j", "-0.7+0.02j"])
@pytest.mark.parametrize("n,nb,cls", [(2049, 2, (4, 8)), (4097, 1, (2, 16))])
def test_largest_classes_by_both_residuals(engine, n, nb, cls, m):
    """No truth at these sizes: ||G A - I||_F / sqrt(n) and ||A G - I||_F / sqrt(n), formed in float64 on the host, both
    below 1e-9 -- the fillers' criterion; a transposition makes them O(1).  n = 2049 in batches of two (the energy under
    test and the other one), n = 4097 one energy at a time."""
    from gaunegf_amd.integrate import GrBatch
    plan = engine.inverse_plan(n, nb)
    assert plan["path"] == 2 and plan["cls"] == cls and [g["wk"] for g in plan["groups"]] == [TEAM]
    case, g = _big(n)
    E = case.energies if nb == 2 else case.energies[m:m + 1]
    engine.set_batch(nb)
    try:
        G = GrBatch(case.F, case.S, g, E)
        last = engine.inverse_last()
    finally:
        engine.set_batch(0)
    assert last == {"path": 2, "masks": _masks(plan)}, last
    assert np.all(np.asarray(engine.last_info[:nb]) == 0)
    Gm = G[m if nb == 2 else 0]
    del G
    A = case.A64(case.energies[m])
    assert xh.asymmetry(A) >= 0.5
    left = np.linalg.norm(Gm @ A - np.eye(n)) / np.sqrt(n)
    right = np.linalg.norm(A @ Gm - np.eye(n)) / np.sqrt(n)
    print(f"ACC herm class {cls} n={n} nb={nb} E={complex(case.energies[m]):.4g}: residual G A {left:.3g}, A G {right:.3g} "
          f"(bar 1e-9): worst ratio {max(left, right) / 1e-9:.3g}")
    assert left < 1e-9 and right < 1e-9, (left, right)
    if (n, m) == (4097, 1):
        _BIG.clear()


# --------------------------------------------------------------------------- #
# d. derived quantities
# --------------------------------------------------------------------------- #
def _weights(M, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(M) + 1j * rng.standard_normal(M)


@functools.lru_cache(maxsize=None)
def _g6_best(n):
    """G6 at its three best-conditioned energies."""
    case, t, _ = _g6(n)
    sub = xh.subset(t, np.sort(np.argsort(t.kappa)[:3]))
    return sub.case, sub, _const(sub.case)


def _derived(name, n):
    return _g6c(n) if name == "G6c" else _g6_best(n)


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("name", ["G6c", "G6"])
def test_grint_against_bar(engine, name, n):
    from gaunegf_amd.integrate import GrInt
    case, t, g = _derived(name, n)
    w = _weights(case.energies.size)
    ref, bound = xprec.grint_truth_and_bound(t, w)
    P = GrInt(case.F, case.S, g, case.energies, w)
    ratios = np.linalg.norm((P[:, t.cols].astype(LD) - ref).astype(np.complex128), axis=0) / bound
    _report(f"GrInt n={n} {name}", ratios)
    assert ratios.max() <= 1.0, (int(np.argmax(ratios)), ratios.max())


_GLESS_TRUTH = {}


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("ind", [None, 0, -1])
@pytest.mark.parametrize("gamma_algo", [0, 1])
def test_grlessint_against_bar(engine, n, ind, gamma_algo):
    """sum_m w_m G_m Gamma G_m^H on G6c within xprec.grless_truth_and_bound's Frobenius bound: negf_set_gamma_algo 0
    takes the compact products (contact COLUMNS of G), 1 the dense ones (the stored conjugate transpose)."""
    from gaunegf_amd.integrate import GrLessInt
    case, t, g = _g6c(n)
    w = _weights(case.energies.size, 7)
    if (n, ind) not in _GLESS_TRUTH:
        _GLESS_TRUTH[n, ind] = xprec.grless_truth_and_bound(t, w, ind)
    ref, bound = _GLESS_TRUTH[n, ind]
    engine.set_gamma_algo(gamma_algo)
    try:
        P = GrLessInt(case.F, case.S, g, case.energies, w, ind)
    finally:
        _restore(engine)
    err = float(np.linalg.norm((P.astype(LD) - ref).astype(np.complex128)))
    _report(f"GrLessInt n={n} G6c ind={ind} gamma_algo={gamma_algo}", [err / bound])
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("n", [64, 256])
def test_transmission_in_both_orders_against_bar(engine, n):
    """T asked as (0, 1) and as (1, 0), each against its own truth; at the complex energy the two truths differ by more
    than 1e-4 relative, so exchanged contacts cannot pass."""
    from gaunegf_amd.transport import SigmaCalculator, calculate_transmission
    case, t, _ = _g6c(n)
    tx = xh.truth_of_exchanged(t)
    ref, bound = xprec.transmission_truth_and_bound(t)
    refx, boundx = xprec.transmission_truth_and_bound(tx)
    m = int(np.argmax(np.abs(case.energies.imag)))
    assert case.energies[m].imag == 2.0 and abs(ref[m] - refx[m]) > 1e-4 * abs(ref[m]), (ref, refx)
    T = calculate_transmission(case.F, case.S, SigmaCalculator(case.sigs[0], case.sigs[1]), case.energies)
    Tx = calculate_transmission(case.F, case.S, SigmaCalculator(case.sigs[1], case.sigs[0]), case.energies)
    r, rx = np.abs(np.asarray(T) - ref) / bound, np.abs(np.asarray(Tx) - refx) / boundx
    _report(f"transmission (0, 1) n={n} G6c", r)
    _report(f"transmission (1, 0) n={n} G6c", rx)
    assert r.max() <= 1.0 and rx.max() <= 1.0, (r, rx, T, ref, Tx, refx)


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("name", ["G6c", "G6"])
def test_dos_against_bar(engine, name, n):
    from gaunegf_amd.transport import SigmaCalculator, calculate_dos
    case, t, _ = _derived(name, n)
    tot_ref, site_ref, btot, bsite = xprec.dos_truth_and_bound(t)
    tot, site = calculate_dos(case.F, case.S, SigmaCalculator(case.sigs[0], case.sigs[1]), case.energies)
    r_site, r_tot = np.abs(site - site_ref) / bsite, np.abs(tot - tot_ref) / btot
    _report(f"dos n={n} {name}", [r_site.max(), r_tot.max()])
    assert r_site.max() <= 1.0 and r_tot.max() <= 1.0, (r_site.max(), r_tot.max())


# --------------------------------------------------------------------------- #
# e. the stored-conjugate-transpose products
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("N", [200, 330, 650, 720])
def test_dense_hermitian_products_on_hermitian_systems(engine, N):
    """test_gpu_parity.test_dense_hermitian_products_read_a_stored_conjugate_transpose on G6c's matrices, where
    G^H is not conj(G): GrLessInt (ind None / 0 / -1) under negf_set_gamma_algo 1 and 0 against float64 numpy within the
    parity bar 1e-8 (loose on purpose: the defects give O(1)), Hermitian to 1e-13, and T for both algos."""
    from gaunegf_amd.integrate import GrLessInt
    case = xh.hermitian_confined(N)
    g = _const(case)
    F, S = case.F, case.S
    E = np.linspace(-2, 2, 6); w = np.full(6, 4.0 / 6) + 0j
    Gs = [np.linalg.inv(e * S - F - case.sig_tot) for e in E]
    worst = 0.0
    for ind in (None, 0, -1):
        Gam = xprec._gamma_of(case, ind)
        ref = sum(w[m] * Gs[m] @ Gam @ Gs[m].conj().T for m in range(6))
        for algo in (1, 0):
            engine.set_gamma_algo(algo)
            try:
                P = GrLessInt(F, S, g, E, w, ind)
            finally:
                engine.set_gamma_algo(0)
            err, herm = rel_fro(P, ref), rel_fro(P, P.conj().T)
            worst = max(worst, err / TOL, herm / 1e-13)
            assert err < TOL, (ind, algo, err)
            assert herm < 1e-13, (ind, algo, herm)
    g1, g2 = case.gammas()
    tref = np.array([np.sum((g1 @ G @ g2) * G.conj()).real for G in Gs])
    h = g._negf_lower(engine)
    engine.set_system(F, S)
    for algo in (1, 0):
        engine.set_gamma_algo(algo)
        try:
            T = engine.transmission(h, 0, 1, E + 0j)
        finally:
            engine.set_gamma_algo(0)
        errs = np.abs(T - tref) / (TOL * np.maximum(1.0, np.abs(tref)))
        worst = max(worst, errs.max())
        assert errs.max() < 1.0, (algo, T, tref)
    _report(f"dense products N={N} G6c (parity bar 1e-8, Hermitian to 1e-13)", [worst])


# --------------------------------------------------------------------------- #
# f. the chain kernels
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n", LDS_SIZES + GLOBAL_SIZES)
def test_chain_inverse_on_g6(engine, n):
    """test_chain_accuracy_gpu.test_chain_inverse_on_case_table's procedure on G6: alpha = -A64(E), S_alpha = 0,
    force_iters = 0 returns g_0 = A^-1; every column within the bar plus the read-back term."""
    case = xh.hermitian_ladder(n)
    t = Truth.__new__(Truth)
    t.case, t.cols = case, np.arange(n)
    t.kappa = np.array([xprec.kappa2(case.A64(E)) for E in case.energies])
    res = xprec.refine([(case.A64(E).astype(LD), t.cols) for E in case.energies],
                       [max(1e-3 * xprec.bar(n, k, 1.0), 2.0 ** -58) for k in t.kappa])
    t.G = np.stack([r[0] for r in res])
    zero = np.zeros((n, n))
    ratios = []
    for m, E in enumerate(case.energies):
        A = case.A64(E)
        kw = dict(taus=[-np.eye(n)], staus=[zero], alphas=[-A], aOverlaps=[zero], betas=[zero], bOverlaps=[zero])
        g = _one_contact(n, kw, 1e-4, 0).g(0.0, 0)
        ratios.append(float(np.max(t.column_errors(m, g)) / (t.delta(m) + xc.READBACK_U)))
    _report(f"chain inverse {'lds' if n <= 64 else 'global'} n={n} G6", ratios)
    assert max(ratios) <= 1.0, ratios


@functools.lru_cache(maxsize=None)
def _l4(n):
    return xh.hermitian_lead(n)


@pytest.mark.parametrize("m", [0, 1, 2], ids=["in-band", "complex", "edge"])
@pytest.mark.parametrize("n", SWEEP_SIZES)
def test_chain_sweeps_on_l4(engine, n, m):
    """test_chain_accuracy_gpu.test_chain_sweeps_against_bar's procedure on L4: g_K and Sigma_K within the propagated
    bar for every checked K (K = 0 included); one test per energy (the truth of ten sweeps at n = 80 costs a second)."""
    lead = _l4(n)
    E = lead.energies[m]
    t = xc.ChainTruth(lead, E, KMAX)
    fails, worst = [], 0.0
    for K in xc.checked_k(t, KMAX):
        dev = _one_contact(n, lead.kwargs(), lead.eta, K)
        rg = t.g_ratio(K, dev.g(E, 0), xc.READBACK_U)
        rs = t.sigma_ratio(K, dev.sigma(E, 0))
        worst = max(worst, rg, rs)
        if not (rg <= 1.0 and rs <= 1.0):
            fails.append((complex(E), K, rg, rs))
    _report(f"chain sweeps {'lds' if n <= 64 else 'global'} n={n} L4 E={complex(E):.4g}", [worst])
    assert not fails, fails


PAIR_K = 3
PAIR_ENERGIES = np.array([0.2 + 0.3j, -0.6 + 0.2j, 0.9 + 0.15j, -1.1 + 0.1j, 0.3 + 2j])


@pytest.mark.parametrize("ncL,ncR", [(19, 9), (50, 40)])
def test_two_unequal_hermitian_leads(engine, ncL, ncR):
    """One provider with two contacts of different Hermitian leads at K = 3 sweeps, five energies in one launch (ten
    fixed points); the smaller lead runs in the larger one's pitch class.  Each contact's g and Sigma against its own
    ChainTruth, with the round robin off and with 4 slots and a quantum of 2 sweeps (every fixed point is set aside
    and resumed), which may not change a bit."""
    from gaunegf_amd.surfG1D import surfG
    leads = [_l4(ncL), _l4(ncR)]
    N = ncL + ncR + 9
    F, S, _ = xh._system(N, 0)
    inds = [list(range(ncL)), list(range(N - ncR, N))]
    kw = {k: [leads[0].kwargs()[k][0], leads[1].kwargs()[k][0]] for k in leads[0].kwargs()}
    truths = [[xc.ChainTruth(lead, E, PAIR_K) for E in PAIR_ENERGIES] for lead in leads]
    assert all(t.usable(PAIR_K) for ts in truths for t in ts)
    out = {}
    engine.set_chain_cache(0)                      # every evaluation runs its fixed points
    try:
        for mode in ((0, 0), (2, 4)):
            engine.set_chain_round_robin(*mode)
            dev = surfG(F, S, inds, eta=leads[0].eta, **kw)
            dev.force_iters = PAIR_K
            eng = dev._engine()
            eng.set_system(F, S)
            hg = dev._negf_lower(eng, identity_tau=True)
            hs = dev._negf_lower(eng)
            out[mode] = [(eng.sigma_eval(hg, i, PAIR_ENERGIES, 2)[:, inds[i]][:, :, inds[i]],
                          eng.sigma_eval(hs, i, PAIR_ENERGIES, 2)) for i in (0, 1)]
    finally:
        engine.set_chain_round_robin(-1, 0)
        engine.set_chain_cache(512)
    for i, nc in enumerate((ncL, ncR)):
        g0, s0 = out[0, 0][i]
        g1, s1 = out[2, 4][i]
        assert np.array_equal(g0, g1) and np.array_equal(s0, s1), (i, "the round robin changed a bit")
        outside = np.ones((N, N), dtype=bool)
        outside[np.ix_(inds[i], inds[i])] = False
        assert not np.any(s0[:, outside])
        ratios = []
        for m, t in enumerate(truths[i]):
            ratios.append(t.g_ratio(PAIR_K, g0[m], xc.READBACK_U))
            ratios.append(t.sigma_ratio(PAIR_K, s0[m][np.ix_(inds[i], inds[i])]))
        _report(f"chain pair ({ncL}, {ncR}) contact {i} n={nc} L4 K={PAIR_K}", ratios)
        assert max(ratios) <= 1.0, (i, ratios)


# --------------------------------------------------------------------------- #
# g. the layered path
# --------------------------------------------------------------------------- #
def test_layered_case_h(engine):
    """Case h (Hermitian layers of 40, 100 and 33 orbitals: the single-workgroup blocked inverse, two layers at the foreign
    stride 100^2): T in both directions, dos, pdos and the blocks of each energy alone (one-hot weights) within
    rgf_ref's bar, C_RGF times the larger error of the two float64 sweeps."""
    c = xh.rgf_case()
    assert [engine.inverse_plan(n, 5)["path"] for n in c.sizes] == [1, 1, 1]
    fwd, back = xh.rgf_truth()
    E = xh.rgf_energies()
    assert abs(fwd["truth"]["T"][-1] - back["truth"]["T"][-1]) > 1e-4 * abs(fwd["truth"]["T"][-1])
    h = engine.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    try:
        tl = engine.layered_terminal_const(h, 0, c.left, c.sig_left)
        tr = engine.layered_terminal_const(h, len(c.sizes) - 1, c.right, c.sig_right)
        got = dict(T=engine.layered_transmission(h, tr, tl, E), T_back=engine.layered_transmission(h, tl, tr, E))
        _, got["dos"] = engine.layered_dos(h, E)
        _, got["pdos"] = engine.layered_dos(h, E, mulliken=True)
        single = []
        for j in range(E.size):
            w = np.zeros(E.size, dtype=complex)
            w[j] = 1.0
            d, u, l = engine.layered_gr_int(h, E, w)
            single.append(np.concatenate([b.ravel() for b in d + u + l]))
    finally:
        engine.layered_free(h)
    ratios = {k: rr.rel_err(got[k], fwd["truth"][k]) / rr.bar(fwd, k) for k in ("T", "dos", "pdos")}
    ratios["T into the left terminal"] = rr.rel_err(got["T_back"], back["truth"]["T"]) / rr.bar(back, "T")
    for j in range(E.size):
        ratios[f"blocks[{j}]"] = rr.rel_err(single[j], fwd["truth"]["single"][j]) / rr.bar_single(fwd, j)
    for k, v in ratios.items():
        print(f"ACC herm layered h {k}: worst ratio {v:.3g}")
    assert max(ratios.values()) <= 1.0, ratios
