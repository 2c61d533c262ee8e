"""
The dense path's sweeps under negf_set_batch on the MI355X: every entry point of include/negf.h that walks the n x n
workspace over a grid, with the grid REALLY cut (helpers.swept holds every call to the limit it ran under), against its own
result at the automatic batch -- one sweep.

What only runs from the second sweep on is index arithmetic: results and status at m0, operands at m0, the carries of the
sums whose bits the header promises, the per-sweep areas sized by the batch, the upper workspace half of the transmission,
the inverse plan that follows the number of energies in a sweep.

  per energy   m = 7 at E + 0.05j, b in (1, 3, 6, 7, 9): array_equal with b = 0, results, info and iteration counts
  promised     bond_int and gless_int_probes, m = 70, b in (1, 3, 31, 32, 33, 64): array_equal with b = 0 and, for
               gless_int_probes on dephase_ref's shapes (a), (b), (d), with the bits of the commit before the sum got
               its carry (tests/golden/gless_probes_parent.npz, scripts/gen_gless_probes_parent_fixture.py)
  per sweep    gless_int, gless_int_seg, gr_int_probes, gr_int_seg: their chunks are the sweep's, so their bits follow the
               sweeps; each entry within accumulate_ref's bar for the sweeps it ran, operands the device's own matrices
  singular     an exactly singular energy behind the first sweep: info and NaN there and nowhere else
  transitions  limits set, lowered, lifted and raised on one context
  kernels      n = 257, 344 energies against sweeps of 64: the windowed inverse takes other kernels, G differs in rounding;
               gr_batch and the per-site DOS under both within the conditioning bar of xprec

Systems: accumulate_ref.const_system (its non-symmetric contact block keeps G from being complex symmetric) at n = 130
(plain inverse above the fused path's 96) and n = 300 (windowed inverse, deferred gather).
"""
import ctypes
import hashlib
import os
import warnings

import numpy as np
import pytest

import accumulate_ref as R
import dephase_ref as dr
import tmatrix_ref as tr
from helpers import chain_lead, random_system, shrink_workspace, swept

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gless_probes_parent.npz")
M7, CUTS7 = 7, (9, 1, 6, 3, 7)                   # (in no order: every block starts from a workspace of one energy)
M70, CUTS70 = 70, (64, 1, 33, 3, 32, 31)
SIZES = (130, 300)


def _Engine():
    from gaunegf_amd.engine import Engine
    return Engine


class _Limit:
    """negf_set_batch(b) for a block, behind a workspace of one energy (helpers.shrink_workspace on `handle`: the block's
    first call builds the workspace to the limit whatever the order of the limits tried); ran(transmission) behind every
    call asserts the sweep (b > 0) and returns it"""

    def __init__(self, engine, b, m, handle):
        self.engine, self.b, self.m, self.handle = engine, b, m, handle

    def __enter__(self):
        if self.b:
            shrink_workspace(self.engine, self.handle, self.b)
        else:
            self.engine.set_batch(0)
        return self

    def __exit__(self, *exc):
        self.engine.set_batch(0)

    def ran(self, transmission=False):
        if self.b:
            return swept(self.engine, self.b, self.m, transmission)
        return min(self.engine.get_batch(), self.m)


class _Dev:
    """device buffers through the HIP runtime the library is linked to (as test_dephase_gpu.test_device_pointer_forms)"""

    def __init__(self):
        C = ctypes
        self.hip = C.CDLL("libamdhip64.so.7")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.ptrs = []

    def empty(self, nbytes):
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), max(int(nbytes), 8)) == 0
        self.ptrs.append(p)
        return p

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.empty(a.nbytes)
        assert self.hip.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p), a.nbytes, 1) == 0
        return p

    def down(self, p, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), p, out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


@pytest.fixture
def dev():
    d = _Dev()
    yield d
    d.free()


def _grid7(n):
    return np.linspace(-2.0, 2.0, M7) + 0.05j


def _same(ref, got, what):
    """every result of `got` equals its twin of `ref` bit for bit; the assertion names ALL that do not"""
    assert ref.keys() == got.keys()
    bad = [k for k in ref if not np.array_equal(ref[k], got[k], equal_nan=True)]
    assert not bad, (what, bad)


def _probes(n, wide):
    """probes on const_system(n) (contacts on the first / last n // 10 orbitals): three of 4 orbitals (with a contact fewer
    than n / 2 orbitals in all: the compact D) or eight of n // 14 (more: the n x n D)"""
    rng = np.random.default_rng(n + (1 if wide else 0))
    k, cnt = (n // 14, 8) if wide else (4, 3)
    start = n // 10 + 2
    return [(np.arange(start + q * (k + 1), start + q * (k + 1) + k), tr.sigma_block(k, rng)) for q in range(cnt)]


def _block_contacts(n, K):
    """(F, S, [Sigma_L, Sigma_R]) with Sigma confined to the first / last K orbitals (no -i 1e-9 S background as
    const_system has, which makes every orbital part of a contact's support): a damping of 0.1 plus a seeded non-symmetric
    block of a tenth of it.  K = n // 10: K_L + K_R <= n / 2, the compact coupling products (3 K_L K_R <= n^2) and at most 96
    eigenchannels; K = 0.6 n: the dense products."""
    F, S = random_system(n, 900 + n)
    rng = np.random.default_rng(n + K)
    sig = []
    for ix in (np.arange(K), np.arange(n - K, n)):
        V = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
        s_ = np.zeros((n, n), dtype=complex)
        s_[np.ix_(ix, ix)] = -0.1j * np.eye(K) + 0.01 * V / np.sqrt(K)
        sig.append(s_)
    return F, S, sig


def _contacts(n, which):
    """(F, S, Sigmas, K): 'everywhere' = accumulate_ref.const_system (support: all orbitals, the dense products, no
    eigenchannels), 'narrow' / 'wide' = _block_contacts with K = n // 10 / 0.6 n"""
    if which == "everywhere":
        return R.const_system(n, 500 + n) + (n,)
    K = n // 10 if which == "narrow" else (6 * n) // 10
    return _block_contacts(n, K) + (K,)


# =========================================================================== per-energy results, constant provider
def _per_energy_const(engine, h, E, lim, dev, n, channels):
    """every per-energy entry point once; lim.ran() behind each call"""
    m = E.size
    out = {}

    def keep(name, val, transmission=False):
        lim.ran(transmission)
        vals = val if isinstance(val, tuple) else (val,)
        for q, v in enumerate(vals):
            out[f"{name}[{q}]"] = np.array(v)
        out[name + " info"] = np.array(engine.last_info)

    keep("gr_batch", engine.gr_batch(h, E))
    keep("dos", engine.dos(h, E))
    keep("dos total", engine.dos(h, E, per_site=False))
    keep("sigma_eval 1", engine.sigma_eval(h, 1, E, 2))
    keep("sigma_eval tot", engine.sigma_eval(h, None, E, 2))
    keep("transmission", engine.transmission(h, 0, 1, E), True)
    keep("transmission spin", engine.transmission(h, 0, 1, E, spin_block=True), True)
    engine.set_gamma_algo(1)
    try:
        keep("transmission dense coupling", engine.transmission(h, 0, 1, E), True)
    finally:
        engine.set_gamma_algo(0)
    groups = np.arange(n) // 7
    keep("local_transmission", engine.local_transmission(h, 0, E))
    keep("local_transmission groups", engine.local_transmission(h, 1, E, groups))
    for op in ("S", "F"):
        for rows in (False, True):
            keep(f"population ret {op} rows={rows}", engine.population(h, _Engine().RETARDED, E, op, rows=rows))
            keep(f"population 0 {op} rows={rows}", engine.population(h, 0, E, op, groups, rows=rows))
    W = np.random.default_rng(n).standard_normal((3, n)) + 0j
    keep("projected_dos ret", engine.projected_dos(h, _Engine().RETARDED, E, W))
    keep("projected_dos 1", engine.projected_dos(h, 1, E, W))
    if channels:                                        # (at most 96 of them)
        keep("transmission_channels", engine.transmission_channels(h, 0, 1, E))
        keep("channel_states", engine.channel_states(h, 0, 1, E))
    for tag, pr in (("few", _probes(n, False)), ("many", _probes(n, True))):
        keep(f"transmission_matrix {tag}", engine.transmission_matrix(h, E, pr))
        keep(f"probe_response {tag}", engine.probe_response(h, E, pr))
    keep("transmission_matrix none", engine.transmission_matrix(h, E))
    # ---- the device-resident forms: grid and results in the caller's HBM
    dE = dev.up(E.astype(np.complex128))
    pr = _probes(n, False)
    C = 2 + len(pr)
    ng = int(groups.max()) + 1
    dW = dev.up(W)
    for name, shape, call, tm in (
            ("transmission_dev", (m,), lambda o: engine.transmission_dev(h, 0, 1, m, dE.value, o), True),
            ("local_transmission_dev", (m, ng, ng), lambda o: engine.local_transmission_dev(h, 0, m, dE.value, groups, o), False),
            ("population_dev", (m, ng), lambda o: engine.population_dev(h, 1, m, dE.value, o, 'F', groups, rows=True), False),
            ("projected_dos_dev", (m, 3), lambda o: engine.projected_dos_dev(h, 0, m, dE.value, 3, dW.value, o), False),
            ("transmission_matrix_dev", (m, C, C), lambda o: engine.transmission_matrix_dev(h, m, dE.value, o, pr), False),
            ("probe_response_dev", (m, len(pr), 2), lambda o: engine.probe_response_dev(h, m, dE.value, o, pr), False)):
        o = dev.empty(8 * int(np.prod(shape)))
        call(o.value)
        engine.sync()
        lim.ran(tm)
        out[name] = dev.down(o, shape, np.float64)
        out[name + " info"] = np.array(engine.last_info_dev(m))
    Ts = dev.empty(8 * 5 * m)
    engine.transmission_dev(h, 0, 1, m, dE.value, Ts.value, Ts.value + 8 * m, spin_block=True)
    engine.sync()
    lim.ran(True)
    out["transmission_dev spin"] = dev.down(Ts, (5 * m,), np.float64)[m:]
    if channels:
        nch = engine.channel_count(h, 0, 1)
        o = dev.empty(8 * m * nch)
        engine.transmission_channels_dev(h, 0, 1, m, dE.value, nch, o.value)
        engine.sync()
        lim.ran()
        out["transmission_channels_dev"] = dev.down(o, (m, nch), np.float64)
        ns = engine.channel_states_count(h, 0)
        o, ps = dev.empty(8 * m * ns), dev.empty(16 * m * ns * n)
        engine.channel_states_dev(h, 0, 1, m, dE.value, ns, o.value, ps.value)
        engine.sync()
        lim.ran()
        out["channel_states_dev T"] = dev.down(o, (m, ns), np.float64)
        out["channel_states_dev psi"] = dev.down(ps, (m, ns, n), np.complex128)
    return out


@pytest.mark.parametrize("contacts", ["everywhere", "narrow", "wide"])
@pytest.mark.parametrize("n", SIZES)
def test_per_energy_results_of_a_constant_provider(engine, dev, n, contacts):
    """everywhere: const_system, whose contacts' support is every orbital; narrow: contacts of n // 10 orbitals (K_L + K_R
    <= n / 2, 3 K_L K_R <= n^2: the compact transmission, the eigenchannels; few probes 2 K_U <= n, many above); wide:
    contacts of 0.6 n orbitals (the dense products by size).  Host and device forms agree at b = 0."""
    F, S, sig, K = _contacts(n, contacts)
    channels = K <= _Engine().EIG_KMAX
    E = _grid7(n)
    engine.set_system(F, S)
    h = engine.sigma_const(sig)
    try:
        with _Limit(engine, 0, M7, h) as lim:
            ref = _per_energy_const(engine, h, E, lim, dev, n, channels)
        assert all(np.all(np.isfinite(v)) for v in ref.values()) and not any(np.any(v) for k, v in ref.items() if k.endswith("info"))
        for host, device in (("transmission[0]", "transmission_dev"), ("transmission spin[1]", "transmission_dev spin"),
                             ("transmission_matrix few[0]", "transmission_matrix_dev"), ("probe_response few[0]", "probe_response_dev")):
            assert np.array_equal(ref[host].ravel(), ref[device].ravel()), (host, device)
        plans = {}
        for b in CUTS7:
            dev.free()
            with _Limit(engine, b, M7, h) as lim:
                got = _per_energy_const(engine, h, E, lim, dev, n, channels)
            plans[b] = _Engine().inverse_plan(n, min(b, M7))
            _same(ref, got, (n, contacts, b, plans[b]))
        print(f"CUT per-energy n={n} {contacts}: {len(ref)} results equal b=0 under b in {CUTS7}; inverse plans by sweep: "
              + "; ".join(f"{min(b, M7)}: path {p['path']} class {p.get('cls')}" for b, p in plans.items()))
    finally:
        engine.sigma_free(h)


# =========================================================================== per-energy results, the other providers
def _chain_provider(engine, n, solver):
    from gaunegf_amd.surfG1D import surfG
    ncs = (6, 20)
    F, S = random_system(n, 77)
    lead = [chain_lead(k, 50 + q) for q, k in enumerate(ncs)]
    ci = [list(range(ncs[0])), list(range(n - ncs[1], n))]
    rng = np.random.default_rng(77)
    g = surfG(F, S, ci, taus=[0.2 * rng.standard_normal((k, k)) for k in ncs], staus=[0.02 * rng.standard_normal((k, k)) for k in ncs],
              alphas=[l[0] for l in lead], aOverlaps=[l[1] for l in lead], betas=[l[2] for l in lead],
              bOverlaps=[l[3] for l in lead], eta=1e-3, solver=solver)
    engine.set_system(F, S)
    return g, g._negf_lower(engine)


def _bethe_provider(engine, n):
    from gaunegf_amd.surfGBethe import surfGB
    from test_gpu_parity import _bethe_device
    coords, orbMap, orbTyp = _bethe_device("Au", n)
    F, S = random_system(n, 79)
    lat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaunegf_amd", "data", "Au")
    g = surfGB.from_arrays(F, S, [[1, 2, 3], [4, 5, 6]], orbMap, orbTyp, coords, latFile=lat, eta=1e-6, fermi=0.0)
    g.force_iters = 30
    engine.set_system(F, S)
    return g, g._negf_lower(engine)


def _per_energy_blocks(engine, h, E, lim, nct):
    out = {}
    out["gr_batch"] = engine.gr_batch(h, E); lim.ran()
    out["gr_batch info"] = np.array(engine.last_info)
    for ct in (0, None):
        out[f"sigma_eval {ct}"] = engine.sigma_eval(h, ct, E, nct); lim.ran()
        out[f"sigma_eval {ct} iters"] = engine.last_iters.copy()
        out[f"sigma_eval {ct} converged"] = engine.last_converged.copy()
    out["transmission"] = engine.transmission(h, 0, 1, E); lim.ran(True)
    out["transmission info"] = np.array(engine.last_info)
    return out


@pytest.mark.parametrize("kind,rr,cache", [("chain1d", True, True), ("chain1d", False, True), ("chain1d", True, False),
                                            ("chain1d", False, False), ("chain1d_rd", True, True), ("chain1d_rd", False, True),
                                            ("chain1d_rd", True, False), ("chain1d_rd", False, False),
                                            ("bethe", True, True)])
def test_per_energy_results_of_block_providers(engine, kind, rr, cache):
    """chain leads of 6 and 20 orbitals (fixed point and renormalisation-decimation; the round-robin launch forced on five
    slots or off, the g(E) cache on or off) and Bethe leads (data/Au.bethe) at n = 130: G, Sigma with its sweep counts and
    flags, T.  Operands at m0: the energies, d_iters + m0 * n_contacts, the blocks of the sweep."""
    n = 130
    E = _grid7(n)
    g, h = _bethe_provider(engine, n) if kind == "bethe" else \
        _chain_provider(engine, n, "doubling" if kind == "chain1d_rd" else "fixed-point")
    engine.set_chain_cache(512 if cache else 0)
    engine.chain_cache_clear()
    engine.set_chain_round_robin(-1, 5) if rr else engine.set_chain_round_robin(0, 0)
    try:
        with _Limit(engine, 0, M7, h) as lim:
            ref = _per_energy_blocks(engine, h, E, lim, 2)
        assert np.all(np.isfinite(ref["gr_batch"])) and np.any(ref["sigma_eval 0 iters"] > 0)
        for b in CUTS7:
            with _Limit(engine, b, M7, h) as lim:
                _same(ref, _per_energy_blocks(engine, h, E, lim, 2), (kind, rr, cache, b))
    finally:
        engine.set_chain_round_robin(-1, 0)
        engine.set_chain_cache(512)
        g._release()


@pytest.mark.parametrize("gammas", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_per_energy_results_of_a_precomputed_provider(engine, n, gammas):
    """Sigma staged per energy (d_pre_tot + n^2 m0, d_pre_c at (m0 + b) n_c + c), different at every energy; with explicit,
    non-Hermitian coupling matrices the transmission takes the full product (opB = 1)."""
    F, S, sig = R.const_system(n, 500 + n)
    E = _grid7(n)
    rng = np.random.default_rng(n)
    scale = 1.0 + 0.1 * rng.standard_normal((M7, 1, 1))
    per_c = np.stack([np.stack([s * scale[k, 0, 0] * (1 + 0.05 * c) for c, s in enumerate(sig)]) for k in range(M7)])
    tot = per_c.sum(axis=1)
    gam = None
    if gammas:
        gam = 1j * (per_c - np.conj(np.swapaxes(per_c, 2, 3)))
        gam[:, :, : n // 10, : n // 10] += 0.01 * rng.standard_normal((M7, 2, n // 10, n // 10))     # not Hermitian
    engine.set_system(F, S)
    h = engine.sigma_precomputed(tot, None if gammas else per_c, gam)

    def everything(lim):
        out = {}
        out["gr_batch"] = engine.gr_batch(h, E); lim.ran()
        out["sigma_eval"] = engine.sigma_eval(h, None, E, 2); lim.ran()
        if not gammas:
            out["sigma_eval 1"] = engine.sigma_eval(h, 1, E, 2); lim.ran()
        out["transmission"] = engine.transmission(h, 0, 1, E); lim.ran(True)
        out["info"] = np.array(engine.last_info)
        return out
    try:
        with _Limit(engine, 0, M7, h) as lim:
            ref = everything(lim)
        assert np.array_equal(ref["sigma_eval"], tot) and np.all(np.isfinite(ref["transmission"]))
        for b in CUTS7:
            with _Limit(engine, b, M7, h) as lim:
                _same(ref, everything(lim), (n, gammas, b))
    finally:
        engine.sigma_free(h)


# =========================================================================== a singular energy behind the first sweep
@pytest.mark.parametrize("n", SIZES)
def test_singular_energy_behind_the_first_sweep(engine, n):
    """F = S, Sigma = 0 staged per energy: E S - F - Sigma is the zero matrix at E = 1, index 5 of 7 -- the second sweep of
    b = 3, the sixth of b = 1.  info is nonzero there and nowhere else, NaN at that energy (segment) only, every other
    energy equal to the b = 0 run: an error return, no fault."""
    at = 5
    _, S = random_system(n, 7)
    E = np.linspace(-1.5, 2.5, M7) + 0.1j
    E[at] = 1.0 + 0j
    one = np.ones(1, dtype=np.complex128)
    only = np.zeros(M7, dtype=bool); only[at] = True
    # the transmission matrix needs contacts on orbital lists, which a precomputed Sigma has not: constant contacts on the
    # first and the last orbital and F = S - Sigma_L - Sigma_R (exact: one entry each), so that F + Sigma = S again
    sL = np.zeros((n, n), complex); sL[0, 0] = -0.5j
    sR = np.zeros((n, n), complex); sR[n - 1, n - 1] = -0.25j
    Sc = S.astype(complex)
    engine.set_system(Sc - sL - sR, Sc)
    hc = engine.sigma_const([sL, sR])
    engine.set_system(S, S)
    hp = engine.sigma_precomputed(np.zeros((M7, n, n), dtype=complex), np.zeros((M7, 2, n, n), dtype=complex))

    def everything(lim):
        out = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out["gr_batch"] = engine.gr_batch(hp, E); lim.ran()
            out["gr_batch info"] = np.array(engine.last_info)
            out["transmission"] = engine.transmission(hp, 0, 1, E); lim.ran(True)
            out["transmission info"] = np.array(engine.last_info)
            out["gr_int_seg"] = np.stack(engine.gr_int_seg(hp, [(E[k:k + 1], one) for k in range(M7)])); lim.ran()
            out["gr_int_seg info"] = np.array(engine.last_info)
            engine.set_system(Sc - sL - sR, Sc)
            out["transmission_matrix"] = engine.transmission_matrix(hc, E); lim.ran()
            out["transmission_matrix info"] = np.array(engine.last_info)
            engine.set_system(S, S)
        return out
    try:
        with _Limit(engine, 0, M7, hp) as lim:
            ref = everything(lim)
        for b in (0, 1, 3):
            with _Limit(engine, b, M7, hp) as lim:
                got = everything(lim)
            for name in ("gr_batch", "transmission", "gr_int_seg", "transmission_matrix"):
                assert np.array_equal(got[name + " info"] != 0, only), (n, b, name, got[name + " info"])
                v = got[name].reshape(M7, -1)
                v = v.view(np.float64) if np.iscomplexobj(v) else v
                assert np.all(np.isnan(v[at])), (n, b, name)
                assert np.all(np.isfinite(v[~only])), (n, b, name)
                assert np.array_equal(got[name][~only], ref[name][~only]), (n, b, name)
    finally:
        engine.sigma_free(hp); engine.sigma_free(hc)


# =========================================================================== sums the header promises
def grid70(lo=-2.0, hi=2.0):
    k = np.arange(M70)
    return np.linspace(lo, hi, M70) + 0j, (np.cos(k) + 1.5) * (1 + 0.25j)


PROMISED = ("a", "b", "d")


def promised_system(engine, shape):
    """(handle, probes, contacts to sum for, grid, free): dephase_ref's shape (a), (b) or (d) resident on the engine"""
    if shape == "d":
        h, g = dr.lower_d(engine, "doubling")
        E, w = grid70(-1.0, 1.2)
        return h, dr.shape_d()[4], E, w, g._release
    c = dr.shape_a() if shape == "a" else dr.shape_b()
    engine.set_system(c.F, c.S)
    h = engine.sigma_const(c.contact_sigmas())
    E, w = grid70()
    return h, c.probes, E, w, lambda: engine.sigma_free(h)


def promised_sums(engine, h, probes, E, w, ran=lambda: None):
    """{tag: sum}: contact 0, contact 1 and the total, the probes floating and no probes at all"""
    out = {}
    for tag, pr in (("probes", probes), ("bare", [])):
        for ind in (0, 1, None):
            out[f"{tag} {ind}"] = engine.gless_int_probes(h, ind, E, w, pr); ran()
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


ROWS_D = (0, 5, 64, 129)                 # of shape (d)'s 130 x 130 sums the record keeps these rows and a digest of all


@pytest.mark.parametrize("shape", PROMISED)
def test_gless_int_probes_keeps_its_bits_under_every_cut(engine, shape):
    """(a) n = 24: the n x n D; (b) n = 40: the compact D; (d) n = 130, chain leads, ten probes.  70 energies: two full
    chunks of 32 and one of 6, cut below, at and above the chunk.  The one-sweep result is the parent commit's, bit for bit
    (one sweep IS launch_accumulate), and every cut gives the same bits (the carry)."""
    gold = np.load(GOLDEN)
    h, probes, E, w, free = promised_system(engine, shape)
    try:
        with _Limit(engine, 0, M70, h) as lim:
            ref = promised_sums(engine, h, probes, E, w, lim.ran)
        for tag, a in ref.items():
            key = f"{shape} {tag}"
            assert np.all(np.isfinite(a.view(np.float64))), key
            if shape == "d":
                assert digest(a) == str(gold[key + " sha256"]), key
                assert np.array_equal(a[list(ROWS_D)], gold[key + " rows"]), key
            else:
                assert np.array_equal(a, gold[key]), key
        for b in CUTS70:
            with _Limit(engine, b, M70, h) as lim:
                _same(ref, promised_sums(engine, h, probes, E, w, lim.ran), (shape, b))
    finally:
        free()


@pytest.mark.parametrize("contacts", ["everywhere", "narrow"])
@pytest.mark.parametrize("n", SIZES)
def test_promised_sums_on_the_asymmetric_systems(engine, dev, n, contacts):
    """bond_int (real weights) and gless_int_probes (no probes, few, many) on const_system(n) -- contacts on every orbital:
    the n x n D throughout -- and on contacts confined to n // 10 orbitals (few probes: 2 K_U <= n, the compact D; many: the
    n x n D), host and device forms: every cut equals one sweep."""
    F, S, sig, _ = _contacts(n, contacts)
    E, w = grid70()
    wr = np.ascontiguousarray(w.real)
    engine.set_system(F, S)
    h = engine.sigma_const(sig)
    dE, dw, dwr = dev.up(E), dev.up(w), dev.up(wr)
    oc, orl = dev.empty(16 * n * n), dev.empty(8 * n * n)
    few, many = _probes(n, False), _probes(n, True)

    def everything(lim):
        out = {}
        for ind in (0, None):
            out[f"bond_int {ind}"] = engine.bond_int(h, ind, E, wr); lim.ran()
        for tag, pr in (("few", few), ("many", many), ("none", [])):
            for ind in (0, 1, None):
                out[f"gless_int_probes {tag} {ind}"] = engine.gless_int_probes(h, ind, E, w, pr); lim.ran()
        engine.bond_int_dev(h, 1, M70, dE.value, dwr.value, orl.value); engine.sync(); lim.ran()
        out["bond_int_dev 1"] = dev.down(orl, (n, n), np.float64)
        engine.gless_int_probes_dev(h, 0, M70, dE.value, dw.value, oc.value, few); engine.sync(); lim.ran()
        out["gless_int_probes_dev few 0"] = dev.down(oc, (n, n), np.complex128)
        return out
    try:
        with _Limit(engine, 0, M70, h) as lim:
            ref = everything(lim)
        assert np.array_equal(ref["gless_int_probes_dev few 0"], ref["gless_int_probes few 0"])
        assert all(np.all(np.isfinite(v.view(np.float64))) for v in ref.values())
        for b in CUTS70:
            with _Limit(engine, b, M70, h) as lim:
                _same(ref, everything(lim), (n, contacts, b))
    finally:
        engine.sigma_free(h)


# =========================================================================== sums whose bits follow the sweeps
@pytest.mark.parametrize("n", SIZES)
def test_sums_that_follow_the_sweeps_stay_within_the_summation_bar(engine, n):
    """gless_int, gless_int_seg, gr_int_probes (n = 130) and gr_int_seg (n = 130: the gathered G; n = 300: the deferred form,
    read through the permutation) add chunk by chunk OF THE SWEEP: each entry against the extended-precision sum of the
    device's own per-energy matrices (the same call over the single energy k with weight 1) at accumulate_ref's bar,
    k_of(the shares of the sweeps run).  Two bridges make the operands sound: a one-energy gr_int is gr_batch's matrix bit
    for bit, and gr_batch does not depend on the limit."""
    F, S, sig = R.const_system(n, 500 + n)
    E, w = R.grid(M70, 1000 * n + M70)
    one = np.ones(1, dtype=np.complex128)
    sizes = [5, 27, 1, 33, 4]                                              # segments cut by chunk and sweep edges
    ends = list(np.cumsum(sizes))
    assert ends[-1] == M70
    segs = [(E[e - k:e], w[e - k:e]) for k, e in zip(sizes, ends)]
    pr = _probes(n, False)
    lesser = n == 130
    engine.set_system(F, S)
    h = engine.sigma_const(sig)

    def per_segment(got, X, shares):
        return max(R.ratio(got[s], w[e - k:e], X[e - k:e], R.k_of(shares[s])) for s, (k, e) in enumerate(zip(sizes, ends)))
    try:
        with _Limit(engine, 0, M70, h) as lim:
            G = engine.gr_batch(h, E); lim.ran()
            for k in (0, 31, 32, 69):
                assert np.array_equal(engine.gr_int(h, E[k:k + 1], one), G[k]), (n, k)
            if lesser:
                A = np.stack([engine.gless_int(h, 0, E[k:k + 1], one) for k in range(M70)])
                Gp = np.stack([engine.gr_int_probes(h, E[k:k + 1], one, pr) for k in range(M70)])
        for b in CUTS7:
            with _Limit(engine, b, M7, h) as lim:
                Gb = engine.gr_batch(h, E[:M7]); lim.ran()
            assert np.array_equal(Gb, G[:M7]), (n, b)
        worst = {}
        for b in (0,) + CUTS70:
            with _Limit(engine, b, M70, h) as lim:
                Gb = engine.gr_batch(h, E); sweep = lim.ran()
                assert np.array_equal(Gb, G), (n, b)
                k_all = R.k_of(R.shares_of([M70], M70, sweep)[0])
                shares = R.shares_of(ends, M70, sweep)
                r = {}
                got = engine.gr_int_seg(h, segs); lim.ran()
                r["gr_int_seg"] = per_segment(got, G, shares)
                if lesser:
                    got = engine.gless_int(h, 0, E, w); lim.ran()
                    r["gless_int"] = R.ratio(got, w, A, k_all)
                    got = engine.gr_int_probes(h, E, w, pr); lim.ran()
                    r["gr_int_probes"] = R.ratio(got, w, Gp, k_all)
                    got = engine.gless_int_seg(h, 0, segs); lim.ran()
                    r["gless_int_seg"] = per_segment(got, A, shares)
            print(f"CUT sums n={n} b={b} sweep={sweep} k={k_all}: worst ratio " + ", ".join(f"{a} {v:.3f}" for a, v in r.items()))
            worst[b] = r
        for b, r in worst.items():
            for a, v in r.items():
                assert v <= 1.0, (n, b, a, v)
    finally:
        engine.sigma_free(h)


# =========================================================================== a cut that changes the inverse's kernels
def test_a_cut_that_changes_the_window_kernel_stays_within_the_conditioning_bar(engine):
    """n = 257, 344 energies (test_inverse_cells_gpu's cell "pairs on side streams"): in one sweep the windowed inverse runs
    four stream groups of 86 with one window kernel and windows in pairs; cut into sweeps of 64 (and a last one of 24) it
    runs groups of 16 (6) with another kernel, one window at a time.  The two kernels round differently, so here the bits
    of G(E) DO follow negf_set_batch (negf.h at negf_set_batch states the condition).  What holds, and is held: under
    b = 0 and under b = 64 alike, G at the six ladder energies of xprec.ladder(257) -- placed first, last, on either side
    of every group boundary of the one-sweep plan and of two sweep boundaries -- is within the conditioning bar
    C_BAR sqrt(n) u kappa_2 of its extended-precision truth on every sampled column; the per-site DOS of those columns
    within xprec.dos_truth_and_bound's bar (delta ||G e_i|| + u |G_ii|) / pi; eight seeded fillers satisfy
    ||G A - 1|| / sqrt(n) < 1e-9; info is clean.  The difference between the two runs is printed per ladder energy as a
    multiple of the bar; two results within delta of one truth are within 2 delta of each other, which is asserted."""
    import xprec
    import test_inverse_cells_gpu as cells
    n, m, b = 257, 344, 64
    Eng = _Engine()
    whole = Eng.inverse_plan(n, m)
    parts = [Eng.inverse_plan(n, nb) for nb in sorted({nb for _, nb in R.sweeps_of(m, b)})]
    k_whole = {cells._kern(g) for g in whole["groups"]}
    k_parts = {cells._kern(g) for p in parts for g in p["groups"]}
    assert whole["path"] == 2 and all(p["path"] == 2 for p in parts)
    assert k_whole.isdisjoint(k_parts), (k_whole, k_parts)                 # no kernel in common: every energy changes route
    case, t, g = cells._ladder(n)
    assign, gid = cells._place(whole, m)
    for q, p in enumerate((b - 1, b, 5 * b - 1, 5 * b)):                   # either side of the first and of the last cut
        assign.setdefault(p, (4, 3, 2, 4)[q])
    E = np.linspace(-2.5, 2.5, m) + 0.02j
    for p, k in assign.items():
        E[p] = case.energies[k]
    rng = np.random.default_rng(1000 * n + m)
    free = np.array([p for p in range(m) if p not in assign])
    fillers = [int(p) for p in rng.choice(free, 8, replace=False)]
    keep = sorted(assign) + fillers
    cols = t.cols
    engine.set_system(case.F, case.S)
    h = g._negf_lower(engine)
    runs = {}
    for limit in (0, b):
        with _Limit(engine, limit, m, h) as lim:
            G = engine.gr_batch(h, E); sweep = lim.ran()
            info = np.array(engine.last_info)
            last = engine.inverse_last()
            _, site = engine.dos(h, E); lim.ran()
        assert sweep == (b if limit else m) and not np.any(info), (limit, sweep, info)
        want = whole if not limit else Eng.inverse_plan(n, m % b)
        assert last == {"path": 2, "masks": [gr["mask"] for gr in want["groups"]]}, (limit, last)
        runs[limit] = ({p: G[p].copy() for p in keep}, site[sorted(assign)][:, cols].copy())
        del G
    worst = {}
    for limit, (G, site) in runs.items():
        ratios = {p: t.ratio(k, G[p]) for p, k in assign.items()}
        res = [np.linalg.norm(G[p] @ (E[p] * case.S - case.F - case.sig_tot) - np.eye(n)) / np.sqrt(n) for p in fillers]
        dos = 0.0
        for row, p in enumerate(sorted(assign)):
            k = assign[p]
            T = t.G[k]                                                     # [n, sampled columns] in extended precision
            d = T[cols, np.arange(cols.size)]
            ref = (-d.imag / np.longdouble(np.pi)).astype(np.float64)
            bound = (t.delta(k) * np.linalg.norm(T.astype(np.complex128), axis=0) + xprec.U * np.abs(d.astype(np.complex128))) / np.pi
            dos = max(dos, float(np.max(np.abs(site[row] - ref) / bound)))
        worst[limit] = (max(ratios.values()), dos, max(res))
        print(f"CUT kernels n={n} m={m} b={limit}: worst G ratio {worst[limit][0]:.3g} (ladder index "
              f"{assign[max(ratios, key=ratios.get)]}), worst per-site DOS ratio {dos:.3g}, worst filler residual {max(res):.3g}")
        assert all(r <= 1.0 for r in ratios.values()), (limit, ratios)
        assert dos <= 1.0, (limit, dos)
        assert all(r < 1e-9 for r in res), (limit, res)
    differ, between = 0, {}
    for p, k in assign.items():
        a, c = runs[0][0][p], runs[b][0][p]
        differ += not np.array_equal(a, c)
        D = (a[:, cols] - c[:, cols])
        rel = np.linalg.norm(D, axis=0) / np.linalg.norm(t.G[k].astype(np.complex128), axis=0)
        between[p] = float(np.max(rel) / t.delta(k))
    print(f"CUT kernels n={n} m={m}: b=0 against b={b}: {differ} of {len(assign)} ladder positions differ in bits; the difference "
          f"as a multiple of the bar, by ladder index: " + ", ".join(f"{assign[p]}: {v:.3g}" for p, v in sorted(between.items())))
    assert all(v <= 2.0 for v in between.values()), between


# =========================================================================== transitions on one context
def test_limits_set_lowered_lifted_and_raised(engine):
    """b = 0 over 12 energies, then 5, then 2 through the transmission, then 0 again, then 40 over 7 energies: after every
    call negf_get_batch is what the rules of negf_set_batch give, negf_workspace_bytes is that workspace, and the results
    equal the first call's."""
    n = 130
    F, S, sig = R.const_system(n, 500 + n)
    E12 = np.linspace(-2.0, 2.0, 12) + 0.05j
    engine.set_system(np.eye(2), np.eye(2))                               # (drops the workspace: the automatic size is built anew)
    engine.set_system(F, S)
    h = engine.sigma_const(sig)

    def bytes_of(batch):
        return 3 * (n * n * batch + 64) * 16

    def check(batch):
        assert engine.get_batch() == batch, (engine.get_batch(), batch)
        assert engine.workspace_bytes()[0] == bytes_of(batch)
    try:
        G = engine.gr_batch(h, E12)
        auto = engine.get_batch()
        assert auto in (12, 24)                                           # (twice the grid once a transmission has run on the context)
        check(auto)
        T = engine.transmission(h, 0, 1, E12)
        check(24)
        engine.set_batch(5)
        assert np.array_equal(engine.gr_batch(h, E12), G)
        check(5)                                                          # released and rebuilt at the limit
        engine.set_batch(2)
        assert np.array_equal(engine.transmission(h, 0, 1, E12), T)
        check(2)                                                          # sweeps of one energy, the other half scratch
        engine.set_batch(1)
        assert np.array_equal(engine.transmission(h, 0, 1, E12), T)
        check(2)                                                          # the transmission's two energies win
        assert np.array_equal(engine.gr_batch(h, E12), G)
        check(1)
        engine.set_batch(0)
        assert np.array_equal(engine.gr_batch(h, E12), G)
        check(24)                                                         # no limit: the automatic size again
        engine.set_batch(40)
        assert np.array_equal(engine.gr_batch(h, E12[:7]), G[:7])
        check(24)                                                         # not above the limit: kept
        engine.set_batch(6)
        assert np.array_equal(engine.transmission(h, 0, 1, E12), T)
        check(6)                                                          # sweeps of 3
        engine.set_batch(40)
        assert np.array_equal(engine.gr_batch(h, E12), G)
        check(12)                                                         # grown as ever: min(limit, grid)
    finally:
        engine.set_batch(0)
        engine.sigma_free(h)
