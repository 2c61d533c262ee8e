"""
Bitwise fingerprint of the C ABI: every numeric entry point of libnegf_hip.so is called through gaunegf_amd._lib on
fixed seeded inputs, and one line per call is printed -- return code, sha256 of the raw bytes of every output, and
info / iters / converged where the call has them.  Two builds that print the same report compute the same bits through
every orchestration path of negf_api.hip; run it before and after a change of that file and diff the reports.

    python scripts/api_fingerprint.py [--sizes 24,130,300] [> report.txt]

The report is some 5200 lines in 93 groups (per context and provider one for the integrals and transport calls, one
"later" group for channel states, populations, the transmission matrix and the probes, one per context for a layered
system; each headed by a "# group" line).  --digest prints one
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


def probes(n):
    """two probes in the middle of the orbitals that share one orbital; blocks that are not anti-Hermitian"""
    r = np.random.default_rng(21)
    c = n // 2
    nk = i32([3, 2])
    inds = i32([c, c + 1, c + 3, c + 1, c + 5])
    blocks = []
    for k in nk:
        a = 0.02 * r.standard_normal((k, k))
        blocks.append((a + a.T - 0.05j * np.eye(k) + 0.01j * r.standard_normal((k, k))).ravel())
    return nk, inds, c128(np.concatenate(blocks))


def run_later(x, tag, h, E, w, *, chan, gammas):
    """the entry points added after the first fold: channel states, populations and projected DOS, the transmission
    matrix and the floating probes; host and device forms, and every one of them on an empty grid"""
    group(tag + " later")
    c, n, m = x.c, x.n, E.size
    RET = _lib.NEGF_IND_RETARDED
    info = np.full(m, -7, dtype=np.int32)
    Ed, wd = Dev(E), Dev(w)

    def last(label, mm=m):
        li = np.full(max(mm, 1), -7, dtype=np.int32)
        rc = L.negf_last_info(c, mm, ptr(li))
        emit(f"{tag} {label}: last_info rc={rc} {li[:mm].tolist()}")

    # ---- channel states: nchan below and above the count, both directions
    k = C.c_int(-1)
    rc = L.negf_channel_states_count(c, h, 0, C.byref(k))
    emit(f"{tag} channel_states_count: rc={rc} k={k.value}")
    ks = max(k.value, 1)
    for src, dst in ((0, 1), (1, 0)):
        for nchan in (max(ks - 2, 1), ks + 2):
            T = np.zeros((m, nchan)); psi = np.zeros((m, nchan, n), dtype=np.complex128); info[:] = -7
            rc = L.negf_channel_states(c, h, src, dst, m, ptr(E), nchan, ptr(T), ptr(psi), ptr(info))
            rec(f"{tag} channel_states src={src} dst={dst} nchan={nchan}", rc, T=T, psi=psi, info=info)
    nchan = ks + 1
    Td, pd = Dev(np.zeros((m, nchan))), Dev(np.zeros((m, nchan, n), dtype=np.complex128))
    rc = L.negf_channel_states_dev(c, h, -1, 0, m, Ed.p, nchan, Td.p, pd.p); L.negf_sync(c)
    rec(f"{tag} channel_states_dev", rc, T=Td.host(), psi=pd.host()); last("channel_states_dev")
    T = np.full((1, nchan), 7.0); psi = np.full((1, nchan, n), 7.0 + 0j)
    rc = L.negf_channel_states(c, h, 0, 1, 0, None, nchan, ptr(T), ptr(psi), None); rec(f"{tag} channel_states m=0", rc, T=T, psi=psi)
    rc = L.negf_channel_states_dev(c, h, 0, 1, 0, None, nchan, Td.p, pd.p); L.negf_sync(c)
    rec(f"{tag} channel_states_dev m=0", rc, T=Td.host(), psi=pd.host()); last("channel_states_dev m=0", 0)
    if chan:
        Tc = np.full((1, 3), 7.0)
        rc = L.negf_transmission_channels(c, h, 0, 1, 0, None, 3, ptr(Tc), None); rec(f"{tag} channels m=0", rc, T=Tc)

    # ---- populations: retarded and contact forms, S and F, tables and rows, identity and mapped groups
    ng = 5
    grp = i32(np.arange(n) * ng // n)
    for ind, op, rows, mapped, mm in ((RET, 0, 0, True, m), (RET, 1, 1, False, m), (0, 0, 1, True, m), (0, 1, 0, False, 5),
                                      (TOT, 0, 0, True, m), (-1, 1, 1, True, m), (RET, 0, 0, False, 5)):
        g = ng if mapped else n
        out = np.zeros((mm, g) if rows else (mm, g, g)); info[:] = -7
        rc = L.negf_population(c, h, ind, op, rows, mm, ptr(E), g, ptr(grp) if mapped else None, ptr(out), ptr(info))
        rec(f"{tag} population ind={ind} op={op} rows_only={rows} mapped={int(mapped)} m={mm}", rc, out=out, info=info[:mm])
    od = Dev(np.zeros((m, ng)))
    rc = L.negf_population_dev(c, h, RET, 0, 1, m, Ed.p, ng, ptr(grp), od.p); L.negf_sync(c)
    rec(f"{tag} population_dev retarded rows", rc, out=od.host()); last("population_dev retarded rows")
    od = Dev(np.zeros((m, ng, ng)))
    rc = L.negf_population_dev(c, h, -1, 1, 0, m, Ed.p, ng, ptr(grp), od.p); L.negf_sync(c)
    rec(f"{tag} population_dev contact table", rc, out=od.host()); last("population_dev contact table")
    out = np.full((1, ng, ng), 7.0)
    rc = L.negf_population(c, h, RET, 0, 0, 0, None, ng, ptr(grp), ptr(out), None); rec(f"{tag} population m=0", rc, out=out)
    rc = L.negf_population_dev(c, h, 0, 0, 0, 0, None, ng, ptr(grp), od.p); L.negf_sync(c)
    rec(f"{tag} population_dev m=0", rc, out=od.host()); last("population_dev m=0", 0)

    # ---- projected DOS on three vectors
    kv = 3
    r = np.random.default_rng(17)
    Wv = c128(r.standard_normal((kv, n)) + 1j * r.standard_normal((kv, n)))
    Wd = Dev(Wv)
    for ind in (RET, 0, TOT):
        out = np.zeros((m, kv)); info[:] = -7
        rc = L.negf_projected_dos(c, h, ind, m, ptr(E), kv, ptr(Wv), ptr(out), ptr(info)); rec(f"{tag} projected_dos ind={ind}", rc, out=out, info=info)
    for ind in (RET, 1):
        od = Dev(np.zeros((m, kv)))
        rc = L.negf_projected_dos_dev(c, h, ind, m, Ed.p, kv, Wd.p, od.p); L.negf_sync(c)
        rec(f"{tag} projected_dos_dev ind={ind}", rc, out=od.host()); last(f"projected_dos_dev ind={ind}")
    out = np.full((1, kv), 7.0)
    rc = L.negf_projected_dos(c, h, RET, 0, None, kv, ptr(Wv), ptr(out), None); rec(f"{tag} projected_dos m=0", rc, out=out)
    rc = L.negf_projected_dos_dev(c, h, 0, 0, None, kv, Wd.p, od.p); L.negf_sync(c)
    rec(f"{tag} projected_dos_dev m=0", rc, out=od.host()); last("projected_dos_dev m=0", 0)

    # ---- the transmission matrix and the floating probes, without probes and with two
    nk, pin, psg = probes(n)
    nc = 2
    out = np.zeros((n, n), dtype=np.complex128)
    for P in (0, 2):
        a = (ptr(nk), ptr(pin), ptr(psg)) if P else (None, None, None)
        Cn = nc + P
        T = np.zeros((m, Cn, Cn)); info[:] = -7
        rc = L.negf_transmission_matrix(c, h, P, *a, m, ptr(E), ptr(T), ptr(info)); rec(f"{tag} transmission_matrix P={P}", rc, T=T, info=info)
        Td = Dev(T * 0)
        rc = L.negf_transmission_matrix_dev(c, h, P, *a, m, Ed.p, Td.p); L.negf_sync(c)
        rec(f"{tag} transmission_matrix_dev P={P}", rc, T=Td.host()); last(f"transmission_matrix_dev P={P}")
        R = np.zeros((m, max(P, 1), nc)); info[:] = -7
        rc = L.negf_probe_response(c, h, P, *a, m, ptr(E), ptr(R), ptr(info)); rec(f"{tag} probe_response P={P}", rc, R=R, info=info)
        Rd = Dev(R * 0)
        rc = L.negf_probe_response_dev(c, h, P, *a, m, Ed.p, Rd.p); L.negf_sync(c)
        rec(f"{tag} probe_response_dev P={P}", rc, R=Rd.host()); last(f"probe_response_dev P={P}")
        for ind in (0, TOT):
            if gammas and ind == TOT:
                continue
            info[:] = -7
            rc = L.negf_gless_int_probes(c, h, ind, P, *a, m, ptr(E), ptr(w), ptr(out), ptr(info))
            rec(f"{tag} gless_int_probes ind={ind} P={P}", rc, out=out, info=info)
        od = Dev(out * 0)
        rc = L.negf_gless_int_probes_dev(c, h, -1, P, *a, m, Ed.p, wd.p, od.p); L.negf_sync(c)
        rec(f"{tag} gless_int_probes_dev P={P}", rc, out=od.host()); last(f"gless_int_probes_dev P={P}")
        info[:] = -7
        rc = L.negf_gr_int_probes(c, h, P, *a, m, ptr(E), ptr(w), ptr(out), ptr(info)); rec(f"{tag} gr_int_probes P={P}", rc, out=out, info=info)
        od = Dev(out * 0)
        rc = L.negf_gr_int_probes_dev(c, h, P, *a, m, Ed.p, wd.p, od.p); L.negf_sync(c)
        rec(f"{tag} gr_int_probes_dev P={P}", rc, out=od.host()); last(f"gr_int_probes_dev P={P}")
    a = (ptr(nk), ptr(pin), ptr(psg))
    T = np.full((1, 4, 4), 7.0); R = np.full((1, 2, 2), 7.0); out[:] = 7.0
    Td, Rd, od = Dev(T), Dev(R), Dev(out)
    rc = L.negf_transmission_matrix(c, h, 2, *a, 0, None, ptr(T), None); rec(f"{tag} transmission_matrix m=0", rc, T=T)
    rc = L.negf_transmission_matrix_dev(c, h, 2, *a, 0, None, Td.p); L.negf_sync(c)
    rec(f"{tag} transmission_matrix_dev m=0", rc, T=Td.host()); last("transmission_matrix_dev m=0", 0)
    rc = L.negf_probe_response(c, h, 2, *a, 0, None, ptr(R), None); rec(f"{tag} probe_response m=0", rc, R=R)
    rc = L.negf_probe_response_dev(c, h, 2, *a, 0, None, Rd.p); L.negf_sync(c)
    rec(f"{tag} probe_response_dev m=0", rc, R=Rd.host()); last("probe_response_dev m=0", 0)
    rc = L.negf_gless_int_probes(c, h, 0, 2, *a, 0, None, None, ptr(out), None); rec(f"{tag} gless_int_probes m=0", rc, out=out)
    rc = L.negf_gless_int_probes_dev(c, h, 0, 2, *a, 0, None, None, od.p); L.negf_sync(c)
    rec(f"{tag} gless_int_probes_dev m=0", rc, out=od.host()); last("gless_int_probes_dev m=0", 0)
    out[:] = 7.0; od = Dev(out)
    rc = L.negf_gr_int_probes(c, h, 2, *a, 0, None, None, ptr(out), None); rec(f"{tag} gr_int_probes m=0", rc, out=out)
    rc = L.negf_gr_int_probes_dev(c, h, 2, *a, 0, None, None, od.p); L.negf_sync(c)
    rec(f"{tag} gr_int_probes_dev m=0", rc, out=od.host()); last("gr_int_probes_dev m=0", 0)


def layer_sizes(n):
    return [n // 3, n - n // 3 - n // 4, n // 4]


class Layered:
    """three layers of unequal size cut out of system(n): a constant terminal on layer 0, a chain terminal on the last
    layer; the probes of the transmission matrix sit on the middle layer"""
    def __init__(self, x, n, F=None, S=None, tail=None):
        self.c = x.c
        self.sizes = sz = layer_sizes(n)
        self.N = n
        if F is None:
            F, S = system(n, 5)
        o = np.concatenate([[0], np.cumsum(sz)])
        self.off = o
        cat = lambda A, up: c128(np.concatenate([A[o[i]:o[i + 1], o[i + up]:o[i + 1 + up]].ravel() for i in range(3 - up)]))
        self.blocks = (cat(F, 0), cat(F, 1), cat(S, 0), cat(S, 1))
        self.h = C.c_int(-1)
        rc = L.negf_layered_create(self.c, 3, ptr(i32(sz)), *[ptr(b) for b in self.blocks], C.byref(self.h))
        assert rc == 0, rc
        self.h = self.h.value
        self.pattern = sum(s * s for s in sz) + 2 * sum(sz[i] * sz[i + 1] for i in range(2))
        K0 = min(4, sz[0])
        self.inds0 = i32(np.arange(K0) + (sz[0] - K0 if tail else 0))
        t = C.c_int(-1)
        sig = c128(-0.05j * np.eye(K0) + 0.01 * np.ones((K0, K0)))
        assert L.negf_layered_terminal_const(self.c, self.h, 0, K0, ptr(self.inds0), ptr(sig), C.byref(t)) == 0
        K1 = min(5, sz[2])
        self.K1 = K1
        a, Sa, b, Sb = [c128(v) for v in lead(K1, 31)]
        inds1 = i32(np.arange(sz[2] - K1, sz[2]))
        rc = L.negf_layered_terminal_chain(self.c, self.h, 2, K1, ptr(inds1), ptr(a), ptr(Sa), ptr(b), ptr(Sb), ptr(b), ptr(Sb),
                                           1e-3, 2.0 ** -52, 0.1, 64, -1, 1, C.byref(t))
        assert rc == 0 and t.value == 1, (rc, t.value)
        mid = int(o[1])
        r = np.random.default_rng(23)
        a = 0.02 * r.standard_normal((2, 2))
        self.probe = (i32([2]), i32([mid + 1, mid + 3]), c128(a + a.T - 0.05j * np.eye(2)))

    def close(self):
        L.negf_layered_free(self.c, self.h)


def run_layered_calls(ls, tag, E, w, mm):
    """every numeric negf_layered_* entry point on mm energies, host and device forms"""
    c, h, N, sz = ls.c, ls.h, ls.N, ls.sizes
    E, w = E[:mm], w[:mm]
    wr = np.ascontiguousarray(w.real)
    Ed, wd, wrd = Dev(E if mm else E0), Dev(w if mm else E0), Dev(wr if mm else np.zeros(1))
    m1 = max(mm, 1)
    info = np.full(m1, -7, dtype=np.int32)
    e = lambda a: ptr(a) if mm else None

    def last(label):
        li = np.full(m1, -7, dtype=np.int32)
        rc = L.negf_last_info(c, mm, ptr(li))
        emit(f"{tag} {label}: last_info rc={rc} {li[:mm].tolist()}")

    sg = np.full((m1, ls.K1, ls.K1), 7.0 + 0j)
    rc = L.negf_layered_terminal_sigma(c, h, 1, mm, e(E), ptr(sg)); rec(f"{tag} terminal_sigma", rc, out=sg)
    for ta, tb in ((1, 0), (0, 1)):
        T = np.full(m1, 7.0); info[:] = -7
        rc = L.negf_layered_transmission(c, h, ta, tb, mm, e(E), ptr(T), ptr(info)); rec(f"{tag} transmission a={ta} b={tb}", rc, T=T, info=info)
    Td = Dev(np.full(m1, 7.0))
    rc = L.negf_layered_transmission_dev(c, h, 1, 0, mm, Ed.p, Td.p); L.negf_sync(c)
    rec(f"{tag} transmission_dev", rc, T=Td.host()); last("transmission_dev")
    for form in (0, 1):
        ds, dsite = np.full(m1, 7.0), np.full((m1, N), 7.0); info[:] = -7
        rc = L.negf_layered_dos(c, h, form, mm, e(E), ptr(ds), ptr(dsite), ptr(info)); rec(f"{tag} dos form={form}", rc, dos=ds, site=dsite, info=info)
        rc = L.negf_layered_dos(c, h, form, mm, e(E), ptr(ds), None, None); rec(f"{tag} dos form={form} total only", rc, dos=ds)
    dd, dsd = Dev(np.full(m1, 7.0)), Dev(np.full((m1, N), 7.0))
    rc = L.negf_layered_dos_dev(c, h, 1, mm, Ed.p, dd.p, dsd.p); L.negf_sync(c)
    rec(f"{tag} dos_dev", rc, dos=dd.host(), site=dsd.host()); last("dos_dev")
    out = np.full(ls.pattern, 7.0 + 0j); info[:] = -7
    rc = L.negf_layered_gr_int(c, h, mm, e(E), e(w), ptr(out), ptr(info)); rec(f"{tag} gr_int", rc, out=out, info=info)
    od = Dev(np.full(ls.pattern, 7.0 + 0j))
    rc = L.negf_layered_gr_int_dev(c, h, mm, Ed.p, wd.p, od.p); L.negf_sync(c); rec(f"{tag} gr_int_dev", rc, out=od.host()); last("gr_int_dev")
    for ind in (0, -1, TOT):
        out[:] = 7.0; info[:] = -7
        rc = L.negf_layered_gless_int(c, h, ind, mm, e(E), e(w), ptr(out), ptr(info)); rec(f"{tag} gless_int ind={ind}", rc, out=out, info=info)
        ds, dsite = np.full(m1, 7.0), np.full((m1, N), 7.0); info[:] = -7
        rc = L.negf_layered_contact_dos(c, h, ind, mm, e(E), ptr(ds), ptr(dsite), ptr(info))
        rec(f"{tag} contact_dos ind={ind}", rc, dos=ds, site=dsite, info=info)
    od = Dev(np.full(ls.pattern, 7.0 + 0j))
    rc = L.negf_layered_gless_int_dev(c, h, 1, mm, Ed.p, wd.p, od.p); L.negf_sync(c); rec(f"{tag} gless_int_dev", rc, out=od.host()); last("gless_int_dev")
    dd, dsd = Dev(np.full(m1, 7.0)), Dev(np.full((m1, N), 7.0))
    rc = L.negf_layered_contact_dos_dev(c, h, TOT, mm, Ed.p, dd.p, dsd.p); L.negf_sync(c)
    rec(f"{tag} contact_dos_dev", rc, dos=dd.host(), site=dsd.host()); last("contact_dos_dev")
    for P in (0, 1):
        a = [ptr(v) for v in ls.probe] if P else [None] * 3
        Cn = 2 + P
        T = np.full((m1, Cn, Cn), 7.0); info[:] = -7
        rc = L.negf_layered_transmission_matrix(c, h, P, *a, mm, e(E), ptr(T), ptr(info)); rec(f"{tag} transmission_matrix P={P}", rc, T=T, info=info)
        Td = Dev(np.full((m1, Cn, Cn), 7.0))
        rc = L.negf_layered_transmission_matrix_dev(c, h, P, *a, mm, Ed.p, Td.p); L.negf_sync(c)
        rec(f"{tag} transmission_matrix_dev P={P}", rc, T=Td.host()); last(f"transmission_matrix_dev P={P}")
    gpl = i32([2, 3, 1])
    gof = i32(np.concatenate([np.arange(s) * g // s for s, g in zip(sz, gpl)]))
    gsz = sum(int(g) ** 2 for g in gpl) + 2 * sum(int(gpl[i]) * int(gpl[i + 1]) for i in range(2))
    mo = min(mm, 5)
    for ind, grouped, mq in ((0, True, mm), (1, False, mo), (TOT, True, mm)):
        per = gsz if grouped else ls.pattern
        tab = np.full((max(mq, 1), per), 7.0); info[:] = -7
        rc = L.negf_layered_local_transmission(c, h, ind, mq, e(E), ptr(gpl) if grouped else None, ptr(gof) if grouped else None, ptr(tab), ptr(info))
        rec(f"{tag} local_transmission ind={ind} grouped={int(grouped)} m={mq}", rc, out=tab, info=info[:mq])
    td = Dev(np.full((m1, gsz), 7.0))
    rc = L.negf_layered_local_transmission_dev(c, h, 1, mm, Ed.p, ptr(gpl), ptr(gof), td.p); L.negf_sync(c)
    rec(f"{tag} local_transmission_dev", rc, out=td.host()); last("local_transmission_dev")
    for ind in (0, TOT):
        bo = np.full(ls.pattern, 7.0); info[:] = -7
        rc = L.negf_layered_bond_int(c, h, ind, mm, e(E), e(wr), ptr(bo), ptr(info)); rec(f"{tag} bond_int ind={ind}", rc, out=bo, info=info)
    bd = Dev(np.full(ls.pattern, 7.0))
    rc = L.negf_layered_bond_int_dev(c, h, 1, mm, Ed.p, wrd.p, bd.p); L.negf_sync(c); rec(f"{tag} bond_int_dev", rc, out=bd.host()); last("bond_int_dev")
    wb = C.c_longlong(-1)
    rc = L.negf_layered_workspace_bytes(c, h, C.byref(wb)); emit(f"{tag} workspace_bytes: rc={rc} {wb.value}")


E0 = np.zeros(1, dtype=np.complex128)


def run_layered(x, tag, E, Er, w):
    group(tag)
    ls = Layered(x, x.n)
    run_layered_calls(ls, tag + " complex E", E, w, E.size)
    run_layered_calls(ls, tag + " real E", Er, w, Er.size)
    run_layered_calls(ls, tag + " m=0", Er, w, 0)
    ls.close()


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
    run_later(x, f"{tag0} surfGTest", h, E, w, chan=True, gammas=False)
    h = x.const(sig_test(n, k, -0.1j))
    run_provider(x, f"{tag0} CONST formSigma", h, E, w, blocks=False, real_E=Er)
    run_later(x, f"{tag0} CONST formSigma", h, Er, w, chan=False, gammas=False)
    for solver in ("fp", "rd"):
        L.negf_chain_cache_clear(x.c)
        h = x.chain((k, k - 4), solver)
        run_provider(x, f"{tag0} chain {solver}", h, Er, w, blocks=True, chan=True)
        run_refine(x, f"{tag0} chain {solver}", h, Er, w)
        run_later(x, f"{tag0} chain {solver}", h, Er, w, chan=True, gammas=False)
    h = x.bethe()
    Eb = c128(Er - 3.2)
    run_provider(x, f"{tag0} bethe", h, Eb, w, blocks=True, chan=True)
    run_later(x, f"{tag0} bethe", h, Eb, w, chan=True, gammas=False)
    for gam in (False, True):
        h = x.precomputed(E, sig, gam)
        run_provider(x, f"{tag0} precomputed{' gammas' if gam else ''}", h, E, w, blocks=False, gammas=gam, real_E=E)
        run_later(x, f"{tag0} precomputed{' gammas' if gam else ''}", h, E, w, chan=False, gammas=gam)
    run_layered(x, f"{tag0} layered", E, Er, w)
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
        wv = np.zeros((6, K)); V = np.zeros((6, K, K), dtype=np.complex128); info = np.full(6, -7, dtype=np.int32)
        rc = L.negf_eigh_batched(x.c, K, 6, ptr(A), ptr(wv), ptr(V), ptr(info)); rec(f"eigh K={K}", rc, w=wv, V=V, info=info)
        A[2, 1, 0] = np.nan                                                  # a non-finite input: a NaN row, info 1
        rc = L.negf_eigh_batched(x.c, K, 6, ptr(A), ptr(wv), ptr(V), ptr(info)); rec(f"eigh K={K} nan", rc, w=wv, V=V, info=info)
        rc = L.negf_eigh_batched(x.c, K, 6, ptr(A), ptr(wv), ptr(V), None); rec(f"eigh K={K} nan, no info", rc, w=wv, V=V)
        wv[:] = 7.0; V[:] = 7.0
        rc = L.negf_eigh_batched(x.c, K, 0, None, ptr(wv), ptr(V), None); rec(f"eigh K={K} m=0", rc, w=wv, V=V)
        rc = L.negf_eigvalsh_batched(x.c, K, 0, None, ptr(wv), None); rec(f"eigvalsh K={K} m=0", rc, w=wv)
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
    # the later entry points: contacts on orbitals 8..11 and 20..23, so that E = 3 still meets its zero pivot (orbital 2)
    # in the middle of the batch; the probes sit on orbitals 12..17
    sig = np.zeros((2, n, n), dtype=np.complex128)
    for k, o in enumerate((8, 20)):
        sig[k, o:o + 4, o:o + 4] = -0.05j * np.eye(4) + 0.01
    h = x.const(sig)
    RET = _lib.NEGF_IND_RETARDED
    nk, pin, psg = probes(n)
    a = (ptr(nk), ptr(pin), ptr(psg))
    grp = i32(np.arange(n) // 6)
    Wv = c128(np.eye(n)[:2] + 0.5j)
    for algo in (0, 1):
        L.negf_set_small_algo(x.c, algo)
        tag = f"singular small_algo={algo}"
        info = np.full(4, -7, dtype=np.int32)
        T = np.zeros((4, 3)); psi = np.zeros((4, 3, n), dtype=np.complex128)
        rc = L.negf_channel_states(x.c, h, 0, 1, 4, ptr(E), 3, ptr(T), ptr(psi), ptr(info)); rec(f"{tag} channel_states info={info.tolist()}", rc, T=T, psi=psi)
        rc = L.negf_transmission_channels(x.c, h, 0, 1, 4, ptr(E), 3, ptr(T), ptr(info)); rec(f"{tag} channels info={info.tolist()}", rc, T=T)
        for ind in (RET, 0):
            out = np.zeros((4, 4, 4))
            rc = L.negf_population(x.c, h, ind, 0, 0, 4, ptr(E), 4, ptr(grp), ptr(out), ptr(info)); rec(f"{tag} population ind={ind} info={info.tolist()}", rc, out=out)
            out = np.zeros((4, 2))
            rc = L.negf_projected_dos(x.c, h, ind, 4, ptr(E), 2, ptr(Wv), ptr(out), ptr(info)); rec(f"{tag} projected_dos ind={ind} info={info.tolist()}", rc, out=out)
        T = np.zeros((4, 4, 4))
        rc = L.negf_transmission_matrix(x.c, h, 2, *a, 4, ptr(E), ptr(T), ptr(info)); rec(f"{tag} transmission_matrix info={info.tolist()}", rc, T=T)
        R = np.zeros((4, 2, 2))
        rc = L.negf_probe_response(x.c, h, 2, *a, 4, ptr(E), ptr(R), ptr(info)); rec(f"{tag} probe_response info={info.tolist()}", rc, R=R)
        out = np.zeros((n, n), dtype=np.complex128)
        rc = L.negf_gless_int_probes(x.c, h, 0, 2, *a, 4, ptr(E), ptr(w), ptr(out), ptr(info)); rec(f"{tag} gless_int_probes info={info.tolist()}", rc, out=out)
        rc = L.negf_gr_int_probes(x.c, h, 2, *a, 4, ptr(E), ptr(w), ptr(out), ptr(info)); rec(f"{tag} gr_int_probes info={info.tolist()}", rc, out=out)
        Ed, Td = Dev(E), Dev(T * 0)
        rc = L.negf_transmission_matrix_dev(x.c, h, 2, *a, 4, Ed.p, Td.p); L.negf_sync(x.c)
        li = np.full(4, -7, dtype=np.int32); rc2 = L.negf_last_info(x.c, 4, ptr(li))
        rec(f"{tag} transmission_matrix_dev last_info rc={rc2} {li.tolist()}", rc, T=Td.host())
    L.negf_set_small_algo(x.c, 0)
    # a layered system of uncoupled layers with the same diagonal: layer 0 is singular at E = 3
    ls = Layered(x, n, F, S, tail=True)
    run_layered_calls(ls, "singular layered", E, w, 4)
    ls.close()
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
    RET = _lib.NEGF_IND_RETARDED
    nk, pin, psg = probes(n)
    pin_twice, pin_out, nk_zero = i32([3, 3, 5, 4, 6]), i32([3, 4, n, 4, 6]), i32([0, 2])
    big = np.zeros((m, n, n), dtype=np.complex128)
    ls = Layered(x, 24)
    lp = ls.probe
    span = i32([int(ls.off[1]) - 1, int(ls.off[1])])                          # a probe across two layers
    calls += [
        ("channel_states_count total contact", lambda: L.negf_channel_states_count(x.c, h, TOT, C.byref(k))),
        ("channel_states_count precomputed", lambda: L.negf_channel_states_count(x.c, hp, 0, C.byref(k))),
        ("channel_states nchan = 0", lambda: L.negf_channel_states(x.c, h, 0, 1, m, ptr(E), 0, ptr(Ts), ptr(big), None)),
        ("channel_states null psi", lambda: L.negf_channel_states(x.c, h, 0, 1, m, ptr(E), 2, ptr(Ts), None, None)),
        ("channel_states contact 3", lambda: L.negf_channel_states(x.c, h, 0, 3, m, ptr(E), 2, ptr(Ts), ptr(big), None)),
        ("channel_states_dev precomputed", lambda: L.negf_channel_states_dev(x.c, hp, 0, 1, m, ptr(E), 2, ptr(Ts), ptr(big))),
        ("channel_states_dev no system", lambda: L.negf_channel_states_dev(fresh.c, 0, 0, 1, m, ptr(E), 2, ptr(Ts), ptr(big))),
        ("eigh K = 97", lambda: L.negf_eigh_batched(x.c, 97, 1, ptr(big), ptr(T), ptr(big), None)),
        ("eigh null V", lambda: L.negf_eigh_batched(x.c, 4, 1, ptr(big), ptr(T), None, None)),
        ("eigh null context", lambda: L.negf_eigh_batched(None, 4, 1, ptr(big), ptr(T), ptr(big), None)),
        ("population op = 2", lambda: L.negf_population(x.c, h, RET, 2, 0, m, ptr(E), n, None, ptr(big), None)),
        ("population rows_only = 2", lambda: L.negf_population(x.c, h, RET, 0, 2, m, ptr(E), n, None, ptr(big), None)),
        ("population bad group", lambda: L.negf_population(x.c, h, 0, 0, 0, m, ptr(E), 3, ptr(grp_bad), ptr(big), None)),
        ("population n_groups above n", lambda: L.negf_population(x.c, h, 0, 0, 0, m, ptr(E), n + 1, None, ptr(big), None)),
        ("population caller's gammas, contact form", lambda: L.negf_population(x.c, hp, 0, 0, 0, m, ptr(E), n, None, ptr(big), None)),
        ("gless_int retarded selector", lambda: L.negf_gless_int(x.c, h, RET, m, ptr(E), ptr(w), ptr(out), None)),
        ("population_dev null out", lambda: L.negf_population_dev(x.c, h, RET, 0, 0, m, ptr(E), n, None, None)),
        ("population_dev op = -1", lambda: L.negf_population_dev(x.c, h, 0, -1, 0, m, ptr(E), n, None, ptr(big))),
        ("projected_dos k = 0", lambda: L.negf_projected_dos(x.c, h, RET, m, ptr(E), 0, ptr(big), ptr(Ts), None)),
        ("projected_dos k above n", lambda: L.negf_projected_dos(x.c, h, RET, m, ptr(E), n + 1, ptr(big), ptr(Ts), None)),
        ("projected_dos null W", lambda: L.negf_projected_dos(x.c, h, 0, m, ptr(E), 2, None, ptr(Ts), None)),
        ("projected_dos_dev contact 6", lambda: L.negf_projected_dos_dev(x.c, h, 6, m, ptr(E), 2, ptr(big), ptr(Ts))),
        ("transmission_matrix n_probes = -1", lambda: L.negf_transmission_matrix(x.c, h, -1, ptr(nk), ptr(pin), ptr(psg), m, ptr(E), ptr(big), None)),
        ("transmission_matrix too many terminals", lambda: L.negf_transmission_matrix(x.c, h, 1023, ptr(nk), ptr(pin), ptr(psg), m, ptr(E), ptr(big), None)),
        ("transmission_matrix null probe arrays", lambda: L.negf_transmission_matrix(x.c, h, 2, None, None, None, m, ptr(E), ptr(big), None)),
        ("transmission_matrix orbital named twice", lambda: L.negf_transmission_matrix(x.c, h, 2, ptr(nk), ptr(pin_twice), ptr(psg), m, ptr(E), ptr(big), None)),
        ("transmission_matrix orbital outside", lambda: L.negf_transmission_matrix(x.c, h, 2, ptr(nk), ptr(pin_out), ptr(psg), m, ptr(E), ptr(big), None)),
        ("transmission_matrix empty probe", lambda: L.negf_transmission_matrix(x.c, h, 2, ptr(nk_zero), ptr(pin), ptr(psg), m, ptr(E), ptr(big), None)),
        ("transmission_matrix precomputed", lambda: L.negf_transmission_matrix(x.c, hp, 0, None, None, None, m, ptr(E), ptr(big), None)),
        ("transmission_matrix_dev null T", lambda: L.negf_transmission_matrix_dev(x.c, h, 0, None, None, None, m, ptr(E), None)),
        ("transmission_matrix_dev too many terminals", lambda: L.negf_transmission_matrix_dev(x.c, h, 1023, ptr(nk), ptr(pin), ptr(psg), m, ptr(E), ptr(big))),
        ("probe_response n_probes = -1", lambda: L.negf_probe_response(x.c, h, -1, ptr(nk), ptr(pin), ptr(psg), m, ptr(E), ptr(big), None)),
        ("probe_response null R", lambda: L.negf_probe_response(x.c, h, 2, ptr(nk), ptr(pin), ptr(psg), m, ptr(E), None, None)),
        ("probe_response_dev too many terminals", lambda: L.negf_probe_response_dev(x.c, h, 1023, ptr(nk), ptr(pin), ptr(psg), m, ptr(E), ptr(big))),
        ("probe_response_dev orbital named twice", lambda: L.negf_probe_response_dev(x.c, h, 2, ptr(nk), ptr(pin_twice), ptr(psg), m, ptr(E), ptr(big))),
        ("gless_int_probes contact 5", lambda: L.negf_gless_int_probes(x.c, h, 5, 2, ptr(nk), ptr(pin), ptr(psg), m, ptr(E), ptr(w), ptr(out), None)),
        ("gless_int_probes too many terminals", lambda: L.negf_gless_int_probes(x.c, h, 0, 1023, ptr(nk), ptr(pin), ptr(psg), m, ptr(E), ptr(w), ptr(out), None)),
        ("gless_int_probes null w", lambda: L.negf_gless_int_probes(x.c, h, 0, 2, ptr(nk), ptr(pin), ptr(psg), m, ptr(E), None, ptr(out), None)),
        ("gless_int_probes_dev precomputed", lambda: L.negf_gless_int_probes_dev(x.c, hp, 0, 0, None, None, None, m, ptr(E), ptr(w), ptr(out))),
        ("gr_int_probes n_probes = -1", lambda: L.negf_gr_int_probes(x.c, h, -1, None, None, None, m, ptr(E), ptr(w), ptr(out), None)),
        ("gr_int_probes null out", lambda: L.negf_gr_int_probes(x.c, h, 2, ptr(nk), ptr(pin), ptr(psg), m, ptr(E), ptr(w), None, None)),
        ("gr_int_probes_dev orbital outside", lambda: L.negf_gr_int_probes_dev(x.c, h, 2, ptr(nk), ptr(pin_out), ptr(psg), m, ptr(E), ptr(w), ptr(out))),
        ("layered_create one layer", lambda: L.negf_layered_create(x.c, 1, ptr(i32([4])), ptr(big), ptr(big), ptr(big), ptr(big), C.byref(k))),
        ("layered_create empty layer", lambda: L.negf_layered_create(x.c, 2, ptr(i32([4, 0])), ptr(big), ptr(big), ptr(big), ptr(big), C.byref(k))),
        ("layered_terminal_const interior layer", lambda: L.negf_layered_terminal_const(x.c, ls.h, 1, 2, ptr(i32([0, 1])), ptr(big), C.byref(k))),
        ("layered_terminal_const orbital named twice", lambda: L.negf_layered_terminal_const(x.c, ls.h, 0, 2, ptr(i32([1, 1])), ptr(big), C.byref(k))),
        ("layered_terminal_sigma unknown terminal", lambda: L.negf_layered_terminal_sigma(x.c, ls.h, 5, m, ptr(E), ptr(big))),
        ("layered_transmission same end", lambda: L.negf_layered_transmission(x.c, ls.h, 0, 0, m, ptr(E), ptr(T), None)),
        ("layered_transmission unknown handle", lambda: L.negf_layered_transmission(x.c, 77, 1, 0, m, ptr(E), ptr(T), None)),
        ("layered_transmission_dev null T", lambda: L.negf_layered_transmission_dev(x.c, ls.h, 1, 0, m, ptr(E), None)),
        ("layered_dos form 2", lambda: L.negf_layered_dos(x.c, ls.h, 2, m, ptr(E), ptr(T), None, None)),
        ("layered_dos_dev null site", lambda: L.negf_layered_dos_dev(x.c, ls.h, 0, m, ptr(E), ptr(T), None)),
        ("layered_gr_int null w", lambda: L.negf_layered_gr_int(x.c, ls.h, m, ptr(E), None, ptr(big), None)),
        ("layered_gr_int_dev m < 0", lambda: L.negf_layered_gr_int_dev(x.c, ls.h, -1, ptr(E), ptr(w), ptr(big))),
        ("layered_gless_int terminal 2", lambda: L.negf_layered_gless_int(x.c, ls.h, 2, m, ptr(E), ptr(w), ptr(big), None)),
        ("layered_gless_int_dev terminal -3", lambda: L.negf_layered_gless_int_dev(x.c, ls.h, -3, m, ptr(E), ptr(w), ptr(big))),
        ("layered_contact_dos terminal 2", lambda: L.negf_layered_contact_dos(x.c, ls.h, 2, m, ptr(E), ptr(T), None, None)),
        ("layered_contact_dos_dev null site", lambda: L.negf_layered_contact_dos_dev(x.c, ls.h, 0, m, ptr(E), ptr(T), None)),
        ("layered_transmission_matrix probe across layers", lambda: L.negf_layered_transmission_matrix(x.c, ls.h, 1, ptr(lp[0]), ptr(span), ptr(lp[2]), m, ptr(E), ptr(big), None)),
        ("layered_transmission_matrix n_probes = -1", lambda: L.negf_layered_transmission_matrix(x.c, ls.h, -1, ptr(lp[0]), ptr(lp[1]), ptr(lp[2]), m, ptr(E), ptr(big), None)),
        ("layered_transmission_matrix too many terminals", lambda: L.negf_layered_transmission_matrix(x.c, ls.h, 1023, ptr(lp[0]), ptr(lp[1]), ptr(lp[2]), m, ptr(E), ptr(big), None)),
        ("layered_transmission_matrix_dev orbital named twice", lambda: L.negf_layered_transmission_matrix_dev(x.c, ls.h, 1, ptr(lp[0]), ptr(i32([9, 9])), ptr(lp[2]), m, ptr(E), ptr(big))),
        ("layered_local_transmission one group pointer", lambda: L.negf_layered_local_transmission(x.c, ls.h, 0, m, ptr(E), ptr(i32([1, 1, 1])), None, ptr(big), None)),
        ("layered_local_transmission bad group", lambda: L.negf_layered_local_transmission(x.c, ls.h, 0, m, ptr(E), ptr(i32([1, 1, 1])), ptr(i32([3] * 24)), ptr(big), None)),
        ("layered_local_transmission_dev terminal 4", lambda: L.negf_layered_local_transmission_dev(x.c, ls.h, 4, m, ptr(E), None, None, ptr(big))),
        ("layered_bond_int null w", lambda: L.negf_layered_bond_int(x.c, ls.h, 0, m, ptr(E), None, ptr(big), None)),
        ("layered_bond_int_dev unknown handle", lambda: L.negf_layered_bond_int_dev(x.c, 77, 0, m, ptr(E), ptr(T), ptr(big))),
        ("layered_workspace_bytes unknown handle", lambda: L.negf_layered_workspace_bytes(x.c, 77, C.byref(C.c_longlong(0)))),
        ("layered_free unknown handle", lambda: L.negf_layered_free(x.c, 77)),
    ]
    for name, f in calls:
        emit(f"invalid {name}: rc={f()}")
    ls.close()
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
