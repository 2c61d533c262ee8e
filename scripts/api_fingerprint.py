"""
Bitwise fingerprint of the C ABI: every numeric entry point of libnegf_hip.so is called through gaunegf_amd._lib on
fixed seeded inputs, and one line per call is printed -- return code, sha256 of the raw bytes of every output, and
info / iters / converged where the call has them.  Two builds that print the same report compute the same bits through
every orchestration path of negf_api.hip; run it before and after a change of that file and diff the reports.

    python scripts/api_fingerprint.py [--sizes 24,130,300] [> report.txt]

The report is some 1300 lines in groups (one per context and provider, headed by a "# group" line).  --digest prints one
line per group instead -- the number of its lines and one sha256 over them --, the form kept under profiles/;
--digest-of REPORT turns a full report into that form (no GPU needed): two reports agree line by line exactly when their
digests agree, and a digest line that differs names the group whose full lines are to be compared.

Needs a GPU and torch (device buffers of the *_dev forms); reads nothing but the package, writes nothing but stdout.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaunegf_amd import _lib  # noqa: E402
from gaunegf_amd._lib import NEGF_IND_TOTAL, NEGF_SPIN_BLOCK, NEGF_SPIN_RESTRICTED  # noqa: E402

L = torch = None                         # the library and torch: loaded by main() when there is something to run
LINES, QUIET = [], False                 # every report line; QUIET: keep them for the digest instead of printing
TOT = NEGF_IND_TOTAL
M = 45                                   # grid points: 7-energy batches cut the segments and the 32-energy bond chunks
SEG = [0, 1, 1, 10, 33, 45]              # an empty segment, a single point, an empty one again, three ordinary ones


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def emit(line):
    LINES.append(line)
    if not QUIET:
        print(line, flush=True)


def group(name):
    emit("# " + name)


def print_digest(lines):
    groups = []
    for ln in lines:
        if ln.startswith("# "):
            groups.append((ln[2:], []))
        elif groups and ln != "done":
            groups[-1][1].append(ln)
    for name, body in groups:
        print(f"{name}: lines={len(body)} sha256={hashlib.sha256(chr(10).join(body).encode()).hexdigest()}")
    print(f"all: groups={len(groups)} lines={sum(len(b) for _, b in groups)}")


def rec(label, rc, **outs):
    emit(" ".join([f"{label}: rc={rc}"] + [f"{k}={sha(v)}" for k, v in outs.items()]))


def c128(a):
    return np.ascontiguousarray(a, dtype=np.complex128)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class Dev:
    """A device copy of a host array (torch owns the memory); .host() brings it back after negf_sync."""
    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.dtype, self.shape = a.dtype, a.shape
        self.t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        self.p = C.c_void_p(self.t.data_ptr())

    def host(self):
        return self.t.cpu().numpy().view(self.dtype).reshape(self.shape)


def system(n, seed):
    r = np.random.default_rng(seed)
    a = r.standard_normal((n, n)); b = r.standard_normal((n, n))
    F = (a + a.T) / np.sqrt(2 * n) * 2
    S = np.eye(n) + 0.1 * (b + b.T) / np.sqrt(2 * n)
    return c128(F), c128(S)


def grid(m, seed, real=False):
    r = np.random.default_rng(seed)
    E = np.sort(r.uniform(-0.9, 0.9, m)) + (0.0 if real else 1j * r.uniform(0.01, 0.2, m))
    w = r.standard_normal(m) + 1j * r.standard_normal(m)
    return c128(E), c128(w)


def lead(nl, seed):
    r = np.random.default_rng(seed)
    a = r.standard_normal((nl, nl)); b = r.standard_normal((nl, nl)) * 0.2; s = r.standard_normal((nl, nl))
    return ((a + a.T) * 0.25, np.eye(nl) + 0.05 * (s + s.T) * 0.5 / np.sqrt(nl), b,
            0.05 * r.standard_normal((nl, nl)) / np.sqrt(nl))


class Ctx:
    def __init__(self, n=0, seed=0, batch=0):
        self.c = C.c_void_p()
        assert L.negf_create(C.byref(self.c), 0) == 0
        self.n = n
        if n:
            self.F, self.S = system(n, seed)
            assert L.negf_set_system(self.c, n, ptr(self.F), ptr(self.S)) == 0
        assert L.negf_set_batch(self.c, batch) == 0

    def close(self):
        L.negf_destroy(self.c)

    # ---- providers -> handle
    def const(self, sig):
        sig = c128(sig); h = C.c_int(-1)
        assert L.negf_sigma_const(self.c, sig.shape[0], ptr(sig), C.byref(h)) == 0
        return h.value

    def chain(self, ncs, solver):
        n = self.n
        inds = i32(list(range(ncs[0])) + list(range(n - ncs[1], n)))
        ld = [lead(k, 11 + i) for i, k in enumerate(ncs)]
        cat = lambda j: c128(np.concatenate([c128(x[j]).ravel() for x in ld]))
        a, Sa, b, Sb = cat(0), cat(1), cat(2), cat(3)
        h = C.c_int(-1)
        if solver == "rd":
            rc = L.negf_sigma_chain1d_rd(self.c, 2, ptr(i32(ncs)), ptr(inds), ptr(a), ptr(Sa), ptr(b), ptr(Sb), ptr(b), ptr(Sb),
                                         1e-3, 2.0 ** -52, 64, -1, C.byref(h))
        else:
            rc = L.negf_sigma_chain1d(self.c, 2, ptr(i32(ncs)), ptr(inds), ptr(a), ptr(Sa), ptr(b), ptr(Sb), ptr(b), ptr(Sb),
                                      1e-3, 1e-5, 0.1, 2000, -1, C.byref(h))
        assert rc == 0
        return h.value

    def bethe(self):
        from gaunegf_amd.surfGBethe import read_bethe_params, construct_sk_matrix, gen_neighbors
        here = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "data", "Au")
        ne, Ed, Vd, Sd, H0 = read_bethe_params(here)
        dirs = gen_neighbors(np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.2, 0.0]))
        Sl = np.array([construct_sk_matrix(Sd, d) for d in dirs]); Vl = np.array([construct_sk_matrix(Vd, d) for d in dirs])
        n = self.n
        Hc = np.ascontiguousarray(np.stack([H0, H0]), dtype=np.float64)
        Sc = np.ascontiguousarray(np.stack([Sl, Sl]), dtype=np.float64); Vc = np.ascontiguousarray(np.stack([Vl, Vl]), dtype=np.float64)
        orbs = i32(list(range(9)) + list(range(n - 9, n)))
        h = C.c_int(-1)
        rc = L.negf_sigma_bethe(self.c, 2, ptr(i32([1, 1])), ptr(orbs), ptr(i32([3, 3])), ptr(i32([0, 1, 2, 6, 7, 8])),
                                ptr(Hc), ptr(Sc), ptr(Vc), None, 1e-4, 1e-8, 0.5, 1000, -1, C.byref(h))
        assert rc == 0
        self.bethe_raw_args = (np.ascontiguousarray(H0, dtype=np.float64), Sc[0].copy(), Vc[0].copy())
        return h.value

    def precomputed(self, E, sig, gammas):
        n = self.n
        f = (1.0 + 0.1 * E)[:, None, None, None]
        sc = c128(f * c128(sig)[None])                                   # [m][2][n][n]
        st = c128(sc.sum(axis=1))
        if gammas:
            sc = c128(1j * (sc - np.conj(np.swapaxes(sc, 2, 3))) + 0.01 * np.arange(n)[None, None, None, :])   # not Hermitian
        h = C.c_int(-1)
        assert L.negf_sigma_precomputed(self.c, E.size, ptr(st), -2 if gammas else 2, ptr(sc), C.byref(h)) == 0
        return h.value


def sig_test(n, k, V=None):
    """what surfGTest hands negf_sigma_const: V = None, its default -0.05j on the contact orbitals alone (compact
    coupling matrices); V given, formSigma's matrices with the -1e-9j S background on every orbital (dense ones)"""
    from gaunegf_amd.surfGTester import surfGTest
    F, S = system(n, 1)
    return [c128(s) for s in surfGTest(F, S, [list(range(k)), list(range(n - k, n))], V).sig]


def run_provider(x, tag, h, E, w, *, blocks, contacts=True, gammas=False, chan=False, real_E=None):
    """every entry point that takes a provider, host and device forms"""
    group(tag)
    c, n, m = x.c, x.n, E.size
    n2 = n * n
    seg = i32(SEG)
    info = np.full(m, -7, dtype=np.int32)
    Ed, wd = Dev(E), Dev(w)
    it = np.full((m, 2), -7, dtype=np.int32); cv = it.copy()

    def iters(label):
        a, b = it.copy(), cv.copy()
        rc = L.negf_last_iters(c, h, m, ptr(a), ptr(b))
        li = np.full(m, -7, dtype=np.int32)
        rc2 = L.negf_last_info(c, m, ptr(li))
        emit(f"{tag} {label}: last_iters rc={rc} iters={a.ravel().tolist()} converged={b.ravel().tolist()} last_info rc={rc2} {li.tolist()}")

    out = np.zeros((n, n), dtype=np.complex128)
    rc = L.negf_gr_int(c, h, m, ptr(E), ptr(w), ptr(out), ptr(info)); rec(f"{tag} gr_int", rc, out=out, info=info)
    iters("gr_int")
    if blocks:
        rc = L.negf_gr_int(c, h, m, ptr(E), ptr(w), ptr(out), ptr(info)); rec(f"{tag} gr_int again", rc, out=out, info=info)
        iters("gr_int again")
        st = [C.c_longlong(0) for _ in range(4)]
        L.negf_chain_cache_stats(c, *[C.byref(v) for v in st])
        emit(f"{tag} chain cache: hits={st[0].value} misses={st[1].value} entries={st[2].value}")
    od = Dev(out * 0)
    rc = L.negf_gr_int_dev(c, h, m, Ed.p, wd.p, od.p); L.negf_sync(c); rec(f"{tag} gr_int_dev", rc, out=od.host())
    so = np.zeros((len(SEG), n, n), dtype=np.complex128)
    rc = L.negf_gr_int_seg(c, h, m, ptr(E), ptr(w), len(SEG), ptr(seg), ptr(so), ptr(info)); rec(f"{tag} gr_int_seg", rc, out=so, info=info)
    sd = Dev(so * 0)
    rc = L.negf_gr_int_seg_dev(c, h, m, Ed.p, wd.p, len(SEG), ptr(seg), sd.p); L.negf_sync(c); rec(f"{tag} gr_int_seg_dev", rc, out=sd.host())
    for ind in ((0, -1, TOT) if contacts else (TOT,)):
        if gammas and ind == TOT:
            continue
        rc = L.negf_gless_int(c, h, ind, m, ptr(E), ptr(w), ptr(out), ptr(info)); rec(f"{tag} gless_int ind={ind}", rc, out=out, info=info)
        rc = L.negf_gless_int_seg(c, h, ind, m, ptr(E), ptr(w), len(SEG), ptr(seg), ptr(so), ptr(info))
        rec(f"{tag} gless_int_seg ind={ind}", rc, out=so, info=info)
    ind = 0 if contacts else TOT
    od = Dev(out * 0)
    rc = L.negf_gless_int_dev(c, h, ind, m, Ed.p, wd.p, od.p); L.negf_sync(c); rec(f"{tag} gless_int_dev", rc, out=od.host())
    sd = Dev(so * 0)
    rc = L.negf_gless_int_seg_dev(c, h, ind, m, Ed.p, wd.p, len(SEG), ptr(seg), sd.p); L.negf_sync(c); rec(f"{tag} gless_int_seg_dev", rc, out=sd.host())
    mb = 9
    G = np.zeros((mb, n, n), dtype=np.complex128)
    rc = L.negf_gr_batch(c, h, mb, ptr(E), ptr(G), ptr(info[:mb].copy())); rec(f"{tag} gr_batch", rc, G=G)
    ds, dsite = np.zeros(m), np.zeros((m, n))
    rc = L.negf_dos(c, h, m, ptr(E), ptr(ds), ptr(dsite), ptr(info)); rec(f"{tag} dos site", rc, dos=ds, site=dsite, info=info)
    rc = L.negf_dos(c, h, m, ptr(E), ptr(ds), None, None); rec(f"{tag} dos", rc, dos=ds)
    sg = np.zeros((mb, n, n), dtype=np.complex128)
    for ct in ((0, TOT) if contacts and not gammas else (TOT,)):
        a, b = it[:mb].copy(), cv[:mb].copy()
        rc = L.negf_sigma_eval(c, h, ct, mb, ptr(E), ptr(sg), ptr(a), ptr(b))
        emit(f"{tag} sigma_eval ct={ct}: rc={rc} out={sha(sg)} iters={a.ravel().tolist()} converged={b.ravel().tolist()}")
    if contacts:
        T, Ts = np.zeros(m), np.zeros((m, 4))
        rc = L.negf_transmission(c, h, 0, 1, NEGF_SPIN_RESTRICTED, m, ptr(E), ptr(T), None, ptr(info)); rec(f"{tag} transmission", rc, T=T, info=info)
        rc = L.negf_transmission(c, h, 0, -1, NEGF_SPIN_BLOCK, m, ptr(E), ptr(T), ptr(Ts), ptr(info)); rec(f"{tag} transmission spin", rc, T=T, Ts=Ts, info=info)
        Td, Tsd = Dev(T * 0), Dev(Ts * 0)
        rc = L.negf_transmission_dev(c, h, 1, 0, NEGF_SPIN_BLOCK, m, Ed.p, Td.p, Tsd.p); L.negf_sync(c); rec(f"{tag} transmission_dev spin", rc, Ts=Tsd.host())
        # (the workspace is now sized for twice the grid: the integrals once more through it)
        rc = L.negf_gr_int(c, h, m, ptr(E), ptr(w), ptr(out), ptr(info)); rec(f"{tag} gr_int after transmission", rc, out=out, info=info)
    if chan:
        k = C.c_int(-1)
        for cl, cr in ((0, 1), (1, 0)):
            rc = L.negf_channel_count(c, h, cl, cr, C.byref(k))
            Tc = np.zeros((m, max(k.value, 1) + 2))
            rc2 = L.negf_transmission_channels(c, h, cl, cr, m, ptr(E), Tc.shape[1], ptr(Tc), ptr(info))
            rec(f"{tag} channels L={cl} R={cr} count rc={rc} k={k.value}", rc2, T=Tc, info=info)
        Tcd = Dev(Tc * 0)
        rc = L.negf_transmission_channels_dev(c, h, 0, 1, m, Ed.p, Tc.shape[1], Tcd.p); L.negf_sync(c); rec(f"{tag} channels_dev", rc, T=Tcd.host())
    if contacts:
        Er = real_E if real_E is not None else E
        wr = np.ascontiguousarray(w.real)
        ng = 5
        grp = i32(np.arange(n) * ng // n)
        tab = np.zeros((m, ng, ng))
        rc = L.negf_local_transmission(c, h, 0, m, ptr(Er), ng, ptr(grp), ptr(tab), ptr(info)); rec(f"{tag} local_transmission groups", rc, out=tab, info=info)
        mo = 5
        tab = np.zeros((mo, n, n))
        rc = L.negf_local_transmission(c, h, -1, mo, ptr(Er), n, None, ptr(tab), None); rec(f"{tag} local_transmission orbitals", rc, out=tab)
        Erd, td = Dev(Er), Dev(np.zeros((m, ng, ng)))
        rc = L.negf_local_transmission_dev(c, h, 1, m, Erd.p, ng, ptr(grp), td.p); L.negf_sync(c); rec(f"{tag} local_transmission_dev", rc, out=td.host())
        bo = np.zeros((n, n))
        rc = L.negf_bond_int(c, h, 0, m, ptr(Er), ptr(wr), ptr(bo), ptr(info)); rec(f"{tag} bond_int", rc, out=bo, info=info)
        wrd, bd = Dev(wr), Dev(bo * 0)
        rc = L.negf_bond_int_dev(c, h, TOT, m, Erd.p, wrd.p, bd.p); L.negf_sync(c); rec(f"{tag} bond_int_dev total", rc, out=bd.host())


def run_refine(x, tag, h, E, w):
    """two adaptive integrations of two levels each, the second continued from P_in"""
    c, n = x.c, x.n
    m = 16
    nlev, seg = i32([2, 2]), i32([2, 8, 10, 16])
    ratio = np.array([np.nan, 1.0 / 3.0, 0.5, 1.0 / 3.0])
    r = np.random.default_rng(9)
    P_in = c128(r.standard_normal((2, n, n)) + 1j * r.standard_normal((2, n, n)))
    for tol in (1e-30, 1e3):
        P = np.zeros((2, n, n), dtype=np.complex128); lev = np.full(2, -7, dtype=np.int32); mdp = np.zeros(4)
        info = np.full(m, -7, dtype=np.int32)
        rc = L.negf_gr_int_refine(c, h, m, ptr(E), ptr(w), 2, ptr(nlev), ptr(seg), ptr(ratio), tol, ptr(P_in), ptr(P), ptr(lev), ptr(mdp), ptr(info))
        emit(f"{tag} gr_int_refine tol={tol:g}: rc={rc} P={sha(P)} maxdp={sha(mdp)} level={lev.tolist()} info={sha(info)}")


def run_size(n, batch):
    x = Ctx(n, 1, batch)
    tag0 = f"n={n} batch={batch or 'auto'}"
    E, w = grid(M, 3)
    Er, _ = grid(M, 4, real=True)
    k = 6 if n < 64 else 18
    sig = sig_test(n, k)
    h = x.const(sig)
    run_provider(x, f"{tag0} surfGTest", h, E, w, blocks=False, chan=True, real_E=Er)
    run_refine(x, f"{tag0} surfGTest", h, E, w)
    h = x.const(sig_test(n, k, -0.1j))
    run_provider(x, f"{tag0} CONST formSigma", h, E, w, blocks=False, real_E=Er)
    for solver in ("fp", "rd"):
        L.negf_chain_cache_clear(x.c)
        h = x.chain((k, k - 4), solver)
        run_provider(x, f"{tag0} chain {solver}", h, Er, w, blocks=True, chan=True)
        run_refine(x, f"{tag0} chain {solver}", h, Er, w)
    h = x.bethe()
    Eb = c128(Er - 3.2)
    run_provider(x, f"{tag0} bethe", h, Eb, w, blocks=True, chan=True)
    for gam in (False, True):
        h = x.precomputed(E, sig, gam)
        run_provider(x, f"{tag0} precomputed{' gammas' if gam else ''}", h, E, w, blocks=False, gammas=gam, real_E=E)
    x.close()


def run_misc():
    group("misc")
    x = Ctx(24, 1)
    x.bethe()
    H0, Sl, Vl = x.bethe_raw_args
    E = c128(np.linspace(-3.8, -2.6, 5))
    for which, nd in ((1, 12), (2, 9)):
        out = np.zeros((5, nd, 9, 9), dtype=np.complex128); it = np.zeros(5, dtype=np.int32); cv = it.copy()
        rc = L.negf_bethe_raw(x.c, ptr(H0), ptr(Sl), ptr(Vl), 1e-4, 1e-8, 0.5, 1000, -1, which, 5, ptr(E), ptr(out), ptr(it), ptr(cv))
        emit(f"bethe_raw which={which}: rc={rc} out={sha(out)} iters={it.tolist()} converged={cv.tolist()}")
    r = np.random.default_rng(2)
    for K in (5, 40):
        a = r.standard_normal((6, K, K)) + 1j * r.standard_normal((6, K, K))
        A = c128(a + np.conj(np.swapaxes(a, 1, 2)))
        wv = np.zeros((6, K)); info = np.full(6, -7, dtype=np.int32)
        rc = L.negf_eigvalsh_batched(x.c, K, 6, ptr(A), ptr(wv), ptr(info)); rec(f"eigvalsh K={K}", rc, w=wv, info=info)
    buf = r.standard_normal(1 << 19)
    emit(f"hash_bytes: {L.negf_hash_bytes(ptr(buf), buf.nbytes):016x} {L.negf_hash_bytes(ptr(buf), 100):016x}")
    x.close()


def run_singular():
    group("singular")
    n = 24
    x = Ctx()
    F = c128(np.diag(np.arange(1.0, n + 1))); S = c128(np.eye(n))
    assert L.negf_set_system(x.c, n, ptr(F), ptr(S)) == 0
    x.n = n
    h = x.const(np.zeros((2, n, n)))
    E = c128([0.5, 3.0, 2.5, 7.0]); w = c128([1, 1, 1, 1])
    for algo in (0, 1):
        L.negf_set_small_algo(x.c, algo)
        out = np.zeros((n, n), dtype=np.complex128); info = np.full(4, -7, dtype=np.int32)
        rc = L.negf_gr_int(x.c, h, 4, ptr(E), ptr(w), ptr(out), ptr(info))
        emit(f"singular small_algo={algo} gr_int: rc={rc} info={info.tolist()} out={sha(out)}")
        so = np.zeros((2, n, n), dtype=np.complex128); seg = i32([1, 4])
        rc = L.negf_gr_int_seg(x.c, h, 4, ptr(E), ptr(w), 2, ptr(seg), ptr(so), ptr(info))
        emit(f"singular small_algo={algo} gr_int_seg: rc={rc} info={info.tolist()} out={sha(so)}")
        T = np.zeros(4)
        rc = L.negf_transmission(x.c, h, 0, 1, NEGF_SPIN_RESTRICTED, 4, ptr(E), ptr(T), None, ptr(info))
        emit(f"singular small_algo={algo} transmission: rc={rc} info={info.tolist()} T={sha(T)}")
        ds = np.zeros(4)
        rc = L.negf_dos(x.c, h, 4, ptr(E), ptr(ds), None, None)
        emit(f"singular small_algo={algo} dos without info: rc={rc} dos={sha(ds)}")
    x.close()


def run_invalid():
    group("invalid")
    n, m = 25, 4
    x = Ctx(n, 1)
    E, w = grid(m, 3)
    out = np.zeros((2, n, n), dtype=np.complex128); T = np.zeros(m); Ts = np.zeros((m, 4)); info = np.zeros(m, dtype=np.int32)
    h = x.const(sig_test(n, 6))
    hp = x.precomputed(E, sig_test(n, 6), True)
    seg_ok, seg_bad = i32([2, 4]), i32([3, 2])
    k = C.c_int(0)
    grp_bad = i32([9] * n)
    fresh = Ctx()
    calls = [
        ("gr_int stale handle", lambda: L.negf_gr_int(x.c, 99, m, ptr(E), ptr(w), ptr(out), None)),
        ("gr_int negative handle", lambda: L.negf_gr_int(x.c, -1, m, ptr(E), ptr(w), ptr(out), None)),
        ("gr_int no system", lambda: L.negf_gr_int(fresh.c, 0, m, ptr(E), ptr(w), ptr(out), None)),
        ("gr_int null context", lambda: L.negf_gr_int(None, 0, m, ptr(E), ptr(w), ptr(out), None)),
        ("gr_int null out", lambda: L.negf_gr_int(x.c, h, m, ptr(E), ptr(w), None, None)),
        ("gr_int null w", lambda: L.negf_gr_int(x.c, h, m, ptr(E), None, ptr(out), None)),
        ("gr_int m < 0", lambda: L.negf_gr_int(x.c, h, -1, ptr(E), ptr(w), ptr(out), None)),
        ("gr_int m = 0", lambda: L.negf_gr_int(x.c, h, 0, None, None, ptr(out), None)),
        ("gr_int precomputed m > m_pre", lambda: L.negf_gr_int(x.c, hp, m + 1, ptr(E), ptr(w), ptr(out), None)),
        ("gr_int_dev null out", lambda: L.negf_gr_int_dev(x.c, h, m, ptr(E), ptr(w), None)),
        ("gless_int contact 5", lambda: L.negf_gless_int(x.c, h, 5, m, ptr(E), ptr(w), ptr(out), None)),
        ("gless_int contact -3", lambda: L.negf_gless_int(x.c, h, -3, m, ptr(E), ptr(w), ptr(out), None)),
        ("gless_int_dev contact 5 and null out", lambda: L.negf_gless_int_dev(x.c, h, 5, m, ptr(E), ptr(w), None)),
        ("gr_int_seg bad segments", lambda: L.negf_gr_int_seg(x.c, h, m, ptr(E), ptr(w), 2, ptr(seg_bad), ptr(out), None)),
        ("gr_int_seg nseg = 0", lambda: L.negf_gr_int_seg(x.c, h, m, ptr(E), ptr(w), 0, ptr(seg_ok), ptr(out), None)),
        ("gr_int_seg_dev null segments", lambda: L.negf_gr_int_seg_dev(x.c, h, m, ptr(E), ptr(w), 2, None, ptr(out))),
        ("gless_int_seg contact 2", lambda: L.negf_gless_int_seg(x.c, h, 2, m, ptr(E), ptr(w), 2, ptr(seg_ok), ptr(out), None)),
        ("gless_int_seg_dev stale handle", lambda: L.negf_gless_int_seg_dev(x.c, 99, 0, m, ptr(E), ptr(w), 2, ptr(seg_ok), ptr(out))),
        ("gr_int_refine nint = 0", lambda: L.negf_gr_int_refine(x.c, h, m, ptr(E), ptr(w), 0, ptr(seg_ok), ptr(seg_ok), ptr(T), 1e-3, None,
                                                                 ptr(out), ptr(info), ptr(Ts), None)),
        ("gr_int_refine continued without P_in", lambda: L.negf_gr_int_refine(x.c, h, m, ptr(E), ptr(w), 1, ptr(i32([2])), ptr(seg_ok),
                                                                               ptr(np.array([0.5, 0.5])), 1e-3, None, ptr(out), ptr(info), ptr(Ts), None)),
        ("gr_batch null out", lambda: L.negf_gr_batch(x.c, h, m, ptr(E), None, None)),
        ("transmission spin block, odd n", lambda: L.negf_transmission(x.c, h, 0, 1, NEGF_SPIN_BLOCK, m, ptr(E), ptr(T), ptr(Ts), None)),
        ("transmission spin block, null Tspin", lambda: L.negf_transmission(x.c, h, 0, 1, NEGF_SPIN_BLOCK, m, ptr(E), ptr(T), None, None)),
        ("transmission contact 7", lambda: L.negf_transmission(x.c, h, 0, 7, NEGF_SPIN_RESTRICTED, m, ptr(E), ptr(T), None, None)),
        ("transmission_dev spin mode 3", lambda: L.negf_transmission_dev(x.c, h, 0, 1, 3, m, ptr(E), ptr(T), None)),
        ("dos null out", lambda: L.negf_dos(x.c, h, m, ptr(E), None, None, None)),
        ("sigma_eval contact 9", lambda: L.negf_sigma_eval(x.c, h, 9, m, ptr(E), ptr(out), None, None)),
        ("sigma_free stale handle", lambda: L.negf_sigma_free(x.c, 99)),
        ("channel_count total contact", lambda: L.negf_channel_count(x.c, h, TOT, 1, C.byref(k))),
        ("channel_count precomputed", lambda: L.negf_channel_count(x.c, hp, 0, 1, C.byref(k))),
        ("channels nchan = 0", lambda: L.negf_transmission_channels(x.c, h, 0, 1, m, ptr(E), 0, ptr(Ts), None)),
        ("channels precomputed", lambda: L.negf_transmission_channels(x.c, hp, 0, 1, m, ptr(E), 4, ptr(Ts), None)),
        ("channels_dev no system", lambda: L.negf_transmission_channels_dev(fresh.c, 0, 0, 1, m, ptr(E), 4, ptr(Ts))),
        ("local_transmission caller's gammas", lambda: L.negf_local_transmission(x.c, hp, 0, m, ptr(E), n, None, ptr(out), None)),
        ("local_transmission bad group", lambda: L.negf_local_transmission(x.c, h, 0, m, ptr(E), 3, ptr(grp_bad), ptr(out), None)),
        ("local_transmission n_groups = 0", lambda: L.negf_local_transmission(x.c, h, 0, m, ptr(E), 0, ptr(grp_bad), ptr(out), None)),
        ("local_transmission_dev contact 4", lambda: L.negf_local_transmission_dev(x.c, h, 4, m, ptr(E), n, None, ptr(out))),
        ("bond_int caller's gammas", lambda: L.negf_bond_int(x.c, hp, 0, m, ptr(E), ptr(T), ptr(out), None)),
        ("bond_int null w", lambda: L.negf_bond_int(x.c, h, 0, m, ptr(E), None, ptr(out), None)),
        ("bond_int_dev no system", lambda: L.negf_bond_int_dev(fresh.c, 0, 0, m, ptr(E), ptr(T), ptr(out))),
        ("last_iters stale handle", lambda: L.negf_last_iters(x.c, 99, 1, None, None)),
        ("last_info m above the grid", lambda: L.negf_last_info(x.c, 1 << 20, ptr(info))),
        ("eigvalsh K = 0", lambda: L.negf_eigvalsh_batched(x.c, 0, 1, ptr(out), ptr(T), None)),
        ("set_batch -1", lambda: L.negf_set_batch(x.c, -1)),
    ]
    for name, f in calls:
        emit(f"invalid {name}: rc={f()}")
    fresh.close()
    x.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="24,130,300", help="matrix dimensions: fused small path, blocked, windowed inverse")
    ap.add_argument("--digest", action="store_true", help="print one line per group (line count, sha256 of its lines) instead of the report")
    ap.add_argument("--digest-of", metavar="REPORT", help="print the digest of a full report written earlier; runs nothing")
    a = ap.parse_args()
    if a.digest_of:
        print_digest(open(a.digest_of).read().splitlines())
        return
    global L, torch, QUIET
    import torch
    L = _lib.load()
    QUIET = a.digest
    run_invalid()
    run_singular()
    run_misc()
    for n in (int(s) for s in a.sizes.split(",")):
        for batch in (0, 7):
            run_size(n, batch)
    if a.digest:
        print_digest(LINES)
    else:
        print("done", flush=True)


if __name__ == "__main__":
    main()
