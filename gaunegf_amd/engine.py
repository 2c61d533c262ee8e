"""
Engine: thin Python owner of one ``negf_ctx`` (one process, one GPU).

All O(N^3) M work happens in libnegf_hip.so; this class only converts numpy
arrays to the C ABI's layout (C-contiguous complex128) and keeps handles alive.
PyTorch is not needed here; the *_dev methods accept raw device pointers
(``tensor.data_ptr()``) so that a torch-managed buffer can be all-reduced with
RCCL afterwards (distributed.py).
"""
import ctypes as C
import os
import warnings

import numpy as np

from . import _lib
from ._lib import NEGF_IND_RETARDED, NEGF_IND_TOTAL, NEGF_SPIN_BLOCK, NEGF_SPIN_RESTRICTED, check
from .config import SURFACE_DOUBLING_MAX_STEPS, SURFACE_DOUBLING_TOL

_engines = {}


def _c128(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a), dtype=np.complex128)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


_FP_LIB = None


def fingerprint(a):
    """Checksum of an array's bytes, for "has the caller changed this array since the last call" tests of cached
    device-side providers and spin-block splits: the library's negf_hash_bytes (host code, eight threads on large
    buffers: a per-GPU share of BASELINE C5 checks 10 arrays of 16 ... 64 MB per step -- 9 of its 123 ms with a
    single-threaded xxh3).  (Values are only ever compared with values of this same function in this process.)"""
    global _FP_LIB
    b = np.ascontiguousarray(a)
    if _FP_LIB is None:
        _FP_LIB = _lib.load()
    return int(_FP_LIB.negf_hash_bytes(b.ctypes.data_as(C.c_void_p), C.c_ulonglong(b.nbytes)))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_p = C.c_void_p                                   # a raw device address (``tensor.data_ptr()``) as the *_dev calls take it


def _ind(ind):
    return NEGF_IND_TOTAL if ind is None else int(ind)


def _first_bad(bad):
    return f"{bad[:8].tolist()}{'...' if bad.size > 8 else ''}"


class Engine:
    def __init__(self, device=None):
        self._lib = _lib.load()
        ndev = self._lib.negf_device_count()
        if ndev <= 0:
            raise RuntimeError(
                "gaunegf_amd: no HIP device visible.  The NEGF engine is GPU-only "
                "(hand-written gfx950 kernels); there is no CPU fallback.")
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0")) % ndev
        self.device = int(device)
        ctx = C.c_void_p()
        check(self._lib.negf_create(C.byref(ctx), self.device), "negf_create")
        self._ctx = ctx
        self.n = 0
        self._F = None
        self._S = None
        self.last_info = None
        self.last_iters = None
        self.last_converged = None
        # calls into the hot path and energy points they carried, since the object was made (bench.py --config scf)
        self.counters = {"calls": 0, "points": 0}

    # ------------------------------------------------- the way into the library
    # Every wrapper below is one of three shapes.  A new entry point of negf.h gets one ``def`` on the helper that fits,
    # with the C function's name written once, and one scenario in tests/test_engine_calls_host.py.
    def _call(self, name, *args, refused=None):
        """Return code (>= 0) of the library's ``name`` on this context; a negative one raises (_failed).  Array arguments
        stay referenced by ``args`` until the call is back."""
        rc = getattr(self._lib, name)(self._ctx, *args)
        return rc if rc >= 0 else self._failed(rc, name, refused)

    def _failed(self, rc, name, refused):
        """Negative codes raise NegfError under the C function's name, except NEGF_EINVAL where the call has a refusal
        rule: of a ``negf_layered_*`` call it is the caller's ValueError (invalid arguments, before anything was launched);
        with ``refused`` (a text) it is NotImplementedError(refused), the dense feature calls' "this provider is not
        served"."""
        if rc == _lib.NEGF_EINVAL and name.startswith("negf_layered_"):
            raise ValueError(f"{name}: invalid argument (layer sizes, index lists, terminal layers and numbers or the "
                             "number of energies of a 'blocks' terminal)")
        if rc == _lib.NEGF_EINVAL and refused is not None:
            raise NotImplementedError(refused)
        return check(rc, name)

    def _counted(self, m):
        """Count a device-resident call over ``m`` energies and hand back ``_call``.  Written ``self._counted(m)(name, ...)``:
        the call is counted before its arguments are coerced and before it is made, so a call with an invalid argument
        and a call the library refuses are counted too."""
        self.counters["calls"] += 1; self.counters["points"] += int(m)
        return self._call

    def _host(self, where, m, *args, refused=None, raw=False):
        """The host form ``negf_<where>`` over ``m`` energies: ``args`` and the per-energy info array as the last argument.
        Sets ``last_info``, warns about singular energies under the public name ``where`` and returns info[:m];
        ``raw``: returns it untouched instead (the channel calls sort its signs out themselves)."""
        name, info = "negf_" + where, np.zeros(max(m, 1), dtype=np.int32)
        rc = getattr(self._lib, name)(self._ctx, *args, _ptr(info))
        if rc < 0:
            self._failed(rc, name, refused)
        info = info[:m]
        if not raw:
            self._numerical(rc, info, where)
        return info

    def _table(self, name):
        """a host-side dict per handle, made on first use (an Engine built without __init__ has it too)"""
        return self.__dict__.setdefault(name, {})

    # ------------------------------------------------------------- lifetime
    # (close, sigma_free, layered_free and get_batch call the library directly: they ignore or hand back the return code)
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.negf_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        """Launch everything on this hipStream_t (``torch.cuda.Stream().cuda_stream``; 0 / None: the default stream).
        The new stream is ordered behind the old one on the device -- work queued before the switch finishes before
        anything queued after it starts; the host does not wait -- and setting the stream already set is free.
        The ``*_dev`` methods then follow the stream contract of include/negf.h: inputs are read in stream order,
        the output buffers are overwritten (never accumulated into, no need to zero them), results are valid in stream
        order on that stream or after ``sync()``.  A warm call returns without waiting, except with a 1-D chain
        provider while the g(E) cache is on (one download of the grid per launch), with host tables to upload (probes,
        groups, ``layered_gless_int_dev`` / ``layered_contact_dos_dev``), and whenever a buffer has to grow."""
        self._call("negf_set_stream", _p(stream_ptr or 0))

    def set_batch(self, batch):
        self._call("negf_set_batch", int(batch))

    def get_batch(self):
        return self._lib.negf_get_batch(self._ctx)

    def set_inverse_algo(self, algo):
        self._call("negf_set_inverse_algo", int(algo))

    def set_small_algo(self, algo):
        """0: systems of n <= 96 take the single-kernel path (default), 1: the kernel sequence of larger systems."""
        self._call("negf_set_small_algo", int(algo))

    def set_chain_round_robin(self, quantum=-1, slots=0):
        """Round-robin execution of chain launches with more fixed points than resident slots: a fixed point runs
        `quantum` sweeps, then makes room for a waiting one (-1: default, 0: off); `slots` > 0 caps the slots (tests)."""
        self._call("negf_set_chain_round_robin", int(quantum), int(slots))

    def set_gamma_algo(self, algo):
        """0: compact Gamma products where the provider allows (default), 1: dense n x n products."""
        self._call("negf_set_gamma_algo", int(algo))

    def sync(self):
        self._call("negf_sync")

    CHAIN_CACHE_DEFAULT = 512

    def set_chain_cache(self, max_grids=None, max_bytes=None):
        """g(E) cache of the 1-D chain providers: number of evaluated grids kept in HBM (default 512, 0 = off) and
        their total size in bytes (default 8 GB)."""
        if max_grids is not None:
            self._call("negf_set_chain_cache", int(max_grids))
        if max_bytes is not None:
            self._call("negf_set_chain_cache_bytes", int(max_bytes))

    def chain_cache_clear(self):
        self._call("negf_chain_cache_clear")

    def chain_cache_stats(self):
        """dict(hits, misses, entries, bytes)."""
        v = [C.c_longlong(0) for _ in range(4)]
        self._call("negf_chain_cache_stats", *[C.byref(x) for x in v])
        return dict(zip(("hits", "misses", "entries", "bytes"), (int(x.value) for x in v)))

    # --------------------------------------------------------------- system
    def set_system(self, F, S):
        """Make F, S the resident system.  The library keeps the last two systems on the device and recognises them
        bitwise (negf_set_system): calls that repeat a system, or alternate between two -- the spin blocks of a
        blockdiag(alpha, beta) Fock matrix -- upload nothing.  Matrices that reach the library as this engine's own
        private complex copies (``_c128_keyed``) carry a key and are recognised without the comparison."""
        F, kF = self._c128_keyed(F)
        S, kS = self._c128_keyed(S)
        assert F.shape == S.shape, "F and S must have the same shape"
        assert F.ndim == 2 and F.shape[0] == F.shape[1], "F and S must be square matrices"
        n_changed = F.shape[0] != self.n
        key = (kF << 32) | kS if kF and kS else 0
        # (not through _call: an error of the keyed function is reported under the name callers know, negf_set_system)
        check(self._lib.negf_set_system_keyed(self._ctx, F.shape[0], _ptr(F), _ptr(S), C.c_ulonglong(key)), "negf_set_system")
        self.n = F.shape[0]
        if n_changed:
            self.generation = getattr(self, "generation", 0) + 1   # provider handles died
        return True

    def _c128_cached(self, a):
        return self._c128_keyed(a)[0]

    def _c128_keyed(self, a):
        """(complex128 C-contiguous form of a system matrix, its serial number or 0).  An SCF step hands the same REAL F and
        S to every one of its ~30 integrals; converting 2 x 5 MB to complex at N = 800 each time is 2 ms per call.  The
        conversions of the last four matrices are kept together with a snapshot of their source: the same array object
        with the same content (compared element by element -- a caller may have changed it in place; an owned read-only
        array cannot change and is not compared) gets its conversion back.  A kept conversion is private to the engine and
        never changes: it carries a serial number (never reused) by which the library recognises a resident system
        without comparing bytes (negf_set_system_keyed).  Arrays handed in as complex128 already are passed through
        (serial 0: the library compares) unless they are frozen."""
        a = np.asarray(a)
        frozen = (not a.flags.writeable) and a.base is None       # an owned read-only array (integrate._split_blocks): cannot change
        ready = a.dtype == np.complex128 and a.flags.c_contiguous
        if ready and not frozen:
            return a, 0                                           # (nothing to convert, nothing known about its future)
        cache = self.__dict__.setdefault("_sys_conv", [])
        for k, (src, snap, conv, serial) in enumerate(cache):
            if src is a and (snap is None or (snap.shape == a.shape and snap.dtype == a.dtype and np.array_equal(a, snap))):
                cache.append(cache.pop(k))
                return conv, serial
        conv = a if ready else _c128(a)
        if 128 * 128 <= a.size and a.nbytes <= (64 << 20):        # (small: the conversion costs less than the comparison; large: not worth the host memory)
            serial = self.__dict__["_sys_serial"] = self.__dict__.get("_sys_serial", 0) + 1
            if serial >= (1 << 32):
                return conv, 0
            cache.append((a, None if frozen else a.copy(), conv, serial))
            del cache[:-4]
            return conv, serial
        return conv, 0

    # ------------------------------------------------------------ providers
    def _provider(self, name, n_contacts, *args):
        """Make a provider with ``name``; remember how many contacts the one behind the new handle has
        (transmission_matrix sizes its result by it)."""
        h = C.c_int(-1)
        self._call(name, *args, C.byref(h))
        self._table("_n_contacts")[int(h.value)] = int(n_contacts)
        return h.value

    def sigma_const(self, sigmas):
        sig = _c128(np.stack([np.asarray(s) for s in sigmas]))
        assert sig.shape[1:] == (self.n, self.n), "sigma shape must match F"
        return self._provider("negf_sigma_const", sig.shape[0], sig.shape[0], _ptr(sig))

    def sigma_chain1d(self, inds_list, alphas, Salphas, betas, Sbetas, taus, Staus,
                      eta, conv, relFactor, max_iter=2000, force_iters=-1, solver='fixed-point',
                      tol=SURFACE_DOUBLING_TOL, max_steps=SURFACE_DOUBLING_MAX_STEPS):
        """CHAIN1D provider.  solver='fixed-point': the reference's relaxed loop (conv, relFactor, max_iter);
        solver='doubling': renormalisation-decimation (tol, max_steps; conv / relFactor / max_iter are ignored and
        force_iters counts doubling steps)."""
        if solver not in ('fixed-point', 'doubling'):
            raise ValueError(f"solver must be 'fixed-point' or 'doubling', got {solver!r}")
        nc = np.array([len(i) for i in inds_list], dtype=np.int32)
        inds = np.ascontiguousarray(np.concatenate([np.asarray(i).ravel() for i in inds_list]), dtype=np.int32)

        def cat(mats):
            out = []
            for k, m in enumerate(mats):
                m = _c128(m)
                if m.shape != (nc[k], nc[k]):
                    raise ValueError(f"contact {k}: expected {nc[k]}x{nc[k]} matrix, got {m.shape}")
                out.append(m.ravel())
            return np.ascontiguousarray(np.concatenate(out))
        lead = [_ptr(cat(x)) for x in (alphas, Salphas, betas, Sbetas, taus, Staus)]
        if solver == 'doubling':
            return self._provider("negf_sigma_chain1d_rd", len(nc), len(nc), _ptr(nc), _ptr(inds), *lead, float(eta),
                                  float(tol), int(max_steps), int(force_iters))
        return self._provider("negf_sigma_chain1d", len(nc), len(nc), _ptr(nc), _ptr(inds), *lead, float(eta),
                              float(conv), float(relFactor), int(max_iter), int(force_iters))

    def sigma_bethe(self, atom_orbs, atom_nbs, H, Slist, Vlist, xi, eta, conv, mix=0.5,
                    max_iter=1000, force_iters=-1):
        """atom_orbs[c][a] = 9 orbital indices; atom_nbs[c][a] = attached directions;
        H[c] 9x9; Slist[c], Vlist[c] 12x9x9."""
        n_atoms = np.array([len(c) for c in atom_orbs], dtype=np.int32)
        orbs = np.ascontiguousarray(
            np.concatenate([np.asarray(a, dtype=np.int32).ravel() for c in atom_orbs for a in c]), dtype=np.int32)
        n_nb = np.array([len(a) for c in atom_nbs for a in c], dtype=np.int32)
        flat = [int(v) for c in atom_nbs for a in c for v in a]
        nb = np.array(flat if flat else [0], dtype=np.int32)
        Hc = np.ascontiguousarray(np.stack([np.asarray(h, dtype=np.float64) for h in H]))
        Sc = np.ascontiguousarray(np.stack([np.asarray(s, dtype=np.float64) for s in Slist]))
        Vc = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.float64) for v in Vlist]))
        assert Hc.shape[1:] == (9, 9) and Sc.shape[1:] == (12, 9, 9) and Vc.shape[1:] == (12, 9, 9)
        xi_c = None if xi is None else _c128(xi, (self.n, self.n))
        return self._provider("negf_sigma_bethe", len(n_atoms), len(n_atoms), _ptr(n_atoms), _ptr(orbs), _ptr(n_nb),
                              _ptr(nb), _ptr(Hc), _ptr(Sc), _ptr(Vc), _ptr(xi_c), float(eta), float(conv), float(mix),
                              int(max_iter), int(force_iters))

    def bethe_raw(self, H, Slist, Vlist, eta, conv, E, which, mix=0.5, max_iter=1000, force_iters=-1):
        """surfGBAt.sigmaK (which=1 -> [m,12,9,9]) / surfGBAt.sigma (which=2 -> [m,9,9,9])."""
        E, _ = self._grid(E)
        Hc = np.ascontiguousarray(H, dtype=np.float64)
        Sc = np.ascontiguousarray(np.stack([np.asarray(s, dtype=np.float64) for s in Slist]))
        Vc = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.float64) for v in Vlist]))
        assert Hc.shape == (9, 9) and Sc.shape == (12, 9, 9) and Vc.shape == (12, 9, 9)
        nd = 12 if which == 1 else 9
        out = np.zeros((E.size, nd, 9, 9), dtype=np.complex128)
        iters = np.zeros(max(E.size, 1), dtype=np.int32)
        conv_f = np.zeros(max(E.size, 1), dtype=np.int32)
        self._call("negf_bethe_raw", _ptr(Hc), _ptr(Sc), _ptr(Vc), float(eta), float(conv), float(mix), int(max_iter),
                   int(force_iters), int(which), E.size, _ptr(E), _ptr(out), _ptr(iters), _ptr(conv_f))
        self.last_iters = iters[:E.size]
        self.last_converged = conv_f[:E.size]
        return out

    def sigma_precomputed(self, sigma_tot, sigma_c=None, gammas=None):
        """sigma_tot [m,n,n]; sigma_c [m,n,n] or [m,k,n,n]; gammas [m,k,n,n] are used
        as coupling matrices directly (mutually exclusive with sigma_c)."""
        st = _c128(sigma_tot)
        m = st.shape[0]
        assert st.shape[1:] == (self.n, self.n)
        ncc, sc = 0, None
        if gammas is not None:
            sc = _c128(gammas)
            assert sc.ndim == 4 and sc.shape[0] == m
            ncc = -sc.shape[1]
        elif sigma_c is not None:
            sc = _c128(sigma_c)
            if sc.ndim == 3:
                sc = sc[:, None]
            assert sc.shape[0] == m
            ncc = sc.shape[1]
            sc = np.ascontiguousarray(sc)
        return self._provider("negf_sigma_precomputed", max(abs(ncc), 1), m, _ptr(st), ncc, _ptr(sc))

    def sigma_free(self, handle):
        if getattr(self, "_ctx", None):
            self._lib.negf_sigma_free(self._ctx, int(handle))

    # -------------------------------------------------------------- hot path
    def _grid(self, E, w=None):
        E = np.ascontiguousarray(np.asarray(E).ravel(), dtype=np.complex128)
        self.counters["calls"] += 1; self.counters["points"] += E.size
        if w is None:
            return E, None
        w = np.ascontiguousarray(np.asarray(w).ravel(), dtype=np.complex128)
        assert E.size == w.size, "Elist and weights must have the same length"
        return E, w

    def _numerical(self, rc, info, where, grid_index=None):
        self.last_info = info
        if rc == _lib.NEGF_ESINGULAR:
            bad = np.nonzero(info)[0]
            if grid_index is not None:                  # positions in a shard -> indices of the caller's grid
                bad = np.asarray(grid_index)[bad]
            warnings.warn(f"{where}: exactly singular E*S-F-Sigma at energy indices {_first_bad(bad)}", RuntimeWarning)

    def gr_int(self, handle, E, w):
        E, w = self._grid(E, w)
        out = np.zeros((self.n, self.n), dtype=np.complex128)
        self._host("gr_int", E.size, int(handle), E.size, _ptr(E), _ptr(w), _ptr(out))
        return out

    def _segments(self, segments, none_ok=False):
        """(E, w, ends) of a list of (E, w): the grids one after the other, ``ends`` the index one past each.  An empty list
        is an empty grid for gr_int_seg (``none_ok``); for gless_int_seg it is numpy's ValueError, before anything is counted."""
        Es = [np.asarray(E).ravel() for E, _ in segments]
        ws = [np.asarray(w).ravel() for _, w in segments]
        E, w = self._grid(np.concatenate(Es) if Es or not none_ok else np.zeros(0),
                          np.concatenate(ws) if Es or not none_ok else np.zeros(0))
        return E, w, np.ascontiguousarray(np.cumsum([e.size for e in Es]), dtype=np.int32)

    def gr_int_seg(self, handle, segments):
        """[sum_m w_m G(E_m) for (E, w) in segments] from ONE pass over all the energies (negf_gr_int_seg)."""
        E, w, ends = self._segments(segments, none_ok=True)
        out = np.zeros((len(segments), self.n, self.n), dtype=np.complex128)
        self._host("gr_int_seg", E.size, int(handle), E.size, _ptr(E), _ptr(w), len(segments), _ptr(ends), _ptr(out))
        return [out[k] for k in range(len(segments))]

    REFINE_MAX_N = 4096                                           # negf_gr_int_refine up to here (n <= 512: one workgroup walks an integral's levels; above: a launch per level); beyond, the running values alone are GBs
    REFINE_MAX_INTEGRALS, REFINE_MAX_LEVELS = 64, 2048

    def gr_int_refine(self, handle, requests, tol):
        """Nested adaptive refinement on the device (negf_gr_int_refine).  ``requests`` = [(E, w, counts, ratios, P_in)] per
        integral: ``E``, ``w`` the NEW nodes of consecutive levels of the nested rule, one after the other (``counts`` nodes
        per level), ``ratios`` the nested-weight ratio of each level (None for the first level of a fresh integration) and
        ``P_in`` the running value of an integration that continues (None otherwise).
        Returns [(P, converged, maxdps)]: the value at the converged level (``converged`` = its index among the levels
        handed in) or after the last level (``converged`` = -1), and the maxDP of every level consumed (NaN for a first level)."""
        Es, ws, ends, rats, nlev, off = [], [], [], [], [], 0
        for E, w, counts, ratios, P_in in requests:
            E = np.asarray(E).ravel(); w = np.asarray(w).ravel()
            assert E.size == w.size == sum(counts) and len(counts) == len(ratios), "levels do not add up to the grid"
            assert all((r is None) == (j == 0 and P_in is None) for j, r in enumerate(ratios)), \
                "only the first level of a fresh integration has no ratio"
            Es.append(E); ws.append(w); nlev.append(len(counts))
            for c, r in zip(counts, ratios):
                off += int(c)
                ends.append(off); rats.append(np.nan if r is None else float(r))
        E, w = self._grid(np.concatenate(Es), np.concatenate(ws))
        nint = len(requests)
        ends = np.ascontiguousarray(ends, dtype=np.int32)
        nlev = np.ascontiguousarray(nlev, dtype=np.int32)
        rats = np.ascontiguousarray(rats, dtype=np.float64)
        P_in = None
        if any(r[4] is not None for r in requests):
            P_in = np.zeros((nint, self.n, self.n), dtype=np.complex128)
            for k, r in enumerate(requests):
                if r[4] is not None:
                    P_in[k] = r[4]
        out = np.empty((nint, self.n, self.n), dtype=np.complex128)
        level = np.zeros(nint, dtype=np.int32)
        maxdp = np.zeros(ends.size, dtype=np.float64)
        self._host("gr_int_refine", E.size, int(handle), E.size, _ptr(E), _ptr(w), nint, _ptr(nlev), _ptr(ends), _ptr(rats),
                   C.c_double(tol), _ptr(P_in), _ptr(out), _ptr(level), _ptr(maxdp))
        res, s0 = [], 0
        for k in range(nint):
            res.append((out[k], int(level[k]), maxdp[s0:s0 + nlev[k]].copy()))
            s0 += int(nlev[k])
        return res

    def gless_int_seg(self, handle, ind, segments):
        """[sum_m w_m G Gamma G^H for (E, w) in segments] from ONE pass over all the energies (negf_gless_int_seg)."""
        E, w, ends = self._segments(segments)
        out = np.zeros((len(segments), self.n, self.n), dtype=np.complex128)
        self._host("gless_int_seg", E.size, int(handle), _ind(ind), E.size, _ptr(E), _ptr(w), len(segments), _ptr(ends),
                   _ptr(out))
        return [out[k] for k in range(len(segments))]

    def gless_int(self, handle, ind, E, w):
        E, w = self._grid(E, w)
        out = np.zeros((self.n, self.n), dtype=np.complex128)
        self._host("gless_int", E.size, int(handle), _ind(ind), E.size, _ptr(E), _ptr(w), _ptr(out))
        return out

    def gr_batch(self, handle, E):
        E, _ = self._grid(E)
        out = np.zeros((E.size, self.n, self.n), dtype=np.complex128)
        self._host("gr_batch", E.size, int(handle), E.size, _ptr(E), _ptr(out))
        return out

    def transmission(self, handle, contact_L, contact_R, E, spin_block=False):
        E, _ = self._grid(E)
        T = np.zeros(E.size, dtype=np.float64)
        Ts = np.zeros((E.size, 4), dtype=np.float64) if spin_block else None
        mode = NEGF_SPIN_BLOCK if spin_block else NEGF_SPIN_RESTRICTED
        self._host("transmission", E.size, int(handle), int(contact_L), int(contact_R), mode, E.size, _ptr(E), _ptr(T),
                   _ptr(Ts))
        return (T, Ts) if spin_block else T

    # ------------------------------------------------------ eigenchannels
    EIG_KMAX = 96

    def _eig(self, where, A, vectors):
        """(w [m, K], V [m, K, K] or None, whether A was one matrix) behind eigvalsh / eigh"""
        A = np.asarray(A)
        single = A.ndim == 2
        A = _c128(A[None] if single else A)
        if A.ndim != 3 or A.shape[1] != A.shape[2]:
            raise ValueError(f"{where}: expected [m, K, K] Hermitian matrices, got shape {A.shape}")
        m, K = A.shape[0], A.shape[1]
        if not 1 <= K <= self.EIG_KMAX:
            raise ValueError(f"{where}: K = {K} outside 1 .. {self.EIG_KMAX} (the matrix is held in one compute unit's LDS)")
        w = np.zeros((m, K), dtype=np.float64)
        V = np.zeros((m, K, K), dtype=np.complex128) if vectors else None
        info = np.zeros(max(m, 1), dtype=np.int32)
        if vectors:
            rc = self._call("negf_eigh_batched", K, m, _ptr(A), _ptr(w), _ptr(V), _ptr(info))
        else:
            rc = self._call("negf_eigvalsh_batched", K, m, _ptr(A), _ptr(w), _ptr(info))
        self.last_info = info[:m]
        if rc == _lib.NEGF_ESINGULAR:
            warnings.warn(f"{where}: non-finite input or no convergence for matrices {_first_bad(np.nonzero(info[:m])[0])}",
                          RuntimeWarning)
        return w, V, single

    def eigvalsh(self, A):
        """Ascending eigenvalues [m, K] of the Hermitian matrices A [m, K, K] (or one [K, K] -> [K]), K <= 96, read from
        their lower triangles like numpy.linalg.eigvalsh: batched complex Jacobi on the GPU (negf_eigvalsh_batched).
        A row whose input is not finite is NaN; ``last_info`` holds the per-matrix flags (1 non-finite, 2 not converged)."""
        w, _, single = self._eig("eigvalsh", A, False)
        return w[0] if single else w

    _CHAN_REFUSED = ("transmission eigenchannels need a self-energy provider whose couplings live on known contact orbital "
                     "lists (constant Sigma with a nonzero support per contact, 1-D chain leads, Bethe leads without the "
                     f"Xi Sigma Xi transform) and at most {EIG_KMAX} channels; this provider / contact pair is not served")

    def channel_count(self, handle, contact_L, contact_R):
        """min(K_L, K_R): the number of transmission eigenchannels of (contact_L, contact_R).  NotImplementedError for
        providers whose couplings are not confined to an orbital list, and for more than 96 channels."""
        nc = C.c_int(0)
        self._call("negf_channel_count", int(handle), int(contact_L), int(contact_R), C.byref(nc), refused=self._CHAN_REFUSED)
        return nc.value

    def _channels(self, where, count, nchan, E, n_psi, refused, *pair):
        """(T [m, nchan], psi [m, nchan, n_psi] or None with n_psi = 0) of the channel call ``negf_<where>`` on the contact
        ``pair``; ``count``: the number of channels a None ``nchan`` stands for (its call counts nothing)."""
        nchan = count if nchan is None else int(nchan)
        if nchan < 1:
            raise ValueError("nchan must be at least 1")
        E, _ = self._grid(E)
        T = np.zeros((E.size, nchan), dtype=np.float64)
        psi = np.zeros((E.size, nchan, n_psi), dtype=np.complex128) if n_psi else None
        outs = (_ptr(T), _ptr(psi)) if n_psi else (_ptr(T),)
        info = self._host(where, E.size, *pair, E.size, _ptr(E), nchan, *outs, refused=refused, raw=True)
        # info > 0: singular E S - F - Sigma (LAPACK pivot column); < 0: the eigensolver's flags on H (-1 non-finite,
        # -2 not converged) -- reported apart
        self._numerical(_lib.NEGF_ESINGULAR if np.any(info > 0) else 0, np.where(info > 0, info, 0), where)
        self.last_info = info
        bad = np.nonzero(info < 0)[0]
        if bad.size:
            what = {-1: "non-finite H", -2: "Jacobi not converged within its sweep limit"}
            kinds = sorted({what.get(int(v), str(int(v))) for v in info[bad]})
            warnings.warn(f"{where}: eigensolver flags ({', '.join(kinds)}) at energy indices {_first_bad(bad)}",
                          RuntimeWarning)
        return T, psi

    def transmission_channels(self, handle, contact_L, contact_R, E, nchan=None):
        """Transmission eigenchannels T_n(E) [m, nchan], descending per energy (negf_transmission_channels); nchan
        defaults to channel_count().  Rows of singular energies are NaN (with a warning, as transmission)."""
        count = self.channel_count(handle, contact_L, contact_R)
        return self._channels("transmission_channels", count, nchan, E, 0, None, int(handle), int(contact_L),
                              int(contact_R))[0]

    def workspace_bytes(self):
        """(work, blocks): device bytes of the three n x n work areas per energy in flight and of the Sigma block staging
        of chain / Bethe providers (negf_workspace_bytes)."""
        w = C.c_longlong(0); b = C.c_longlong(0)
        self._call("negf_workspace_bytes", C.byref(w), C.byref(b))
        return w.value, b.value

    def transmission_channels_dev(self, handle, contact_L, contact_R, m, E_ptr, nchan, T_ptr):
        self._counted(m)("negf_transmission_channels_dev", int(handle), int(contact_L), int(contact_R), int(m),
                         _p(E_ptr), int(nchan), _p(T_ptr))

    # ------------------------------------------ eigenchannel scattering states
    def eigh(self, A):
        """(w, V) of the Hermitian matrices A [m, K, K] (or one [K, K]), K <= 96, as numpy.linalg.eigh: w ascending and
        bitwise equal to ``eigvalsh(A)`` (the same Jacobi rotations), V[..., :, j] the eigenvector of w[..., j]
        (negf_eigh_batched).  A matrix whose input is not finite gives NaN in w and V; ``last_info`` as eigvalsh."""
        w, V, single = self._eig("eigh", A, True)
        return (w[0], V[0]) if single else (w, V)

    _STATES_REFUSED = ("eigenchannel scattering states need a self-energy provider whose couplings live on known contact "
                       "orbital lists (constant Sigma with a nonzero support per contact, 1-D chain leads, Bethe leads "
                       "without the Xi Sigma Xi transform) and a source contact of at most 96 orbitals; this provider / "
                       "contact pair is not served")

    def channel_states_count(self, handle, contact_src):
        """K_s: the number of scattering states contact_src injects (negf_channel_states_count).  NotImplementedError
        for providers whose couplings are not confined to an orbital list, and for K_s > 96."""
        nc = C.c_int(0)
        self._call("negf_channel_states_count", int(handle), int(contact_src), C.byref(nc), refused=self._STATES_REFUSED)
        return nc.value

    def channel_states(self, handle, contact_src, contact_dst, E, nchan=None):
        """(T [m, nchan], psi [m, nchan, n]): the eigenchannels of the current injected by contact_src and collected by
        contact_dst, T descending, and their scattering states psi_n = G[:, I_s] L u_n (negf_channel_states); nchan
        defaults to channel_states_count().  Each state's largest component is real positive; columns beyond the rank
        of Gamma_src are exact zeros; rows of singular energies are NaN (with a warning, as transmission_channels)."""
        count = self.channel_states_count(handle, contact_src)
        return self._channels("channel_states", count, nchan, E, self.n, self._STATES_REFUSED, int(handle),
                              int(contact_src), int(contact_dst))

    def channel_states_dev(self, handle, contact_src, contact_dst, m, E_ptr, nchan, T_ptr, psi_ptr):
        """negf_channel_states_dev: the grid, T [m, nchan] and psi [m, nchan, n] stay in HBM; asynchronous."""
        self._counted(m)("negf_channel_states_dev", int(handle), int(contact_src), int(contact_dst), int(m), _p(E_ptr),
                         int(nchan), _p(T_ptr), _p(psi_ptr), refused=self._STATES_REFUSED)

    # ------------------------------------------- local (bond) transmission
    BOND_MAX_N = 8192

    _BOND_REFUSED = ("local transmission reads A_ji as conj(A_ij), A = G Gamma_c G^H: coupling matrices handed in by the "
                     "caller (sigma_precomputed(gammas=...)) need not be Hermitian and are not served, nor are systems of "
                     "more than 8192 orbitals; an invalid contact index is refused the same way")

    def _groups(self, groups, n_groups=None):
        """(n_groups, int32 map or None) of an orbital -> group map of length n (None: every orbital its own group)."""
        if groups is None:
            if n_groups not in (None, self.n):
                raise ValueError(f"without a group map there are n = {self.n} groups, not {n_groups}")
            return self.n, None
        g = np.asarray(groups).ravel()
        if g.size != self.n:
            raise ValueError(f"groups must map each of the {self.n} orbitals to a group, got {g.size} entries")
        if not np.issubdtype(g.dtype, np.integer):
            raise ValueError("groups must be integers")
        ng = int(g.max()) + 1 if n_groups is None else int(n_groups)
        if g.min() < 0 or g.max() >= ng or ng > self.n:
            raise ValueError(f"group labels must lie in [0, n_groups) with n_groups <= n; got {int(g.min())} .. {int(g.max())}, n_groups = {ng}")
        return ng, np.ascontiguousarray(g, dtype=np.int32)

    @staticmethod
    def _real_weights(w, where):
        """float64 weights of a bond integral; complex ones are taken if their imaginary parts are all zero"""
        w = np.asarray(w).ravel()
        if np.iscomplexobj(w):
            if np.any(w.imag != 0):
                raise ValueError(f"{where} takes real weights")
            w = w.real
        return np.ascontiguousarray(w, dtype=np.float64)

    def local_transmission(self, handle, ind, E, groups=None, n_groups=None):
        """Local (bond) transmission tables [m, n_g, n_g] of the current injected by contact ``ind``
        (negf_local_transmission): entry [k, a, b] = sum_{i in a, j in b} 2 Im[(E_k S - F)_ij (G Gamma G^H)_ji].
        ``groups``: orbital -> group labels (length n), None = per orbital pair.  Tables of singular energies are NaN
        (with a warning, as transmission)."""
        ng, g = self._groups(groups, n_groups)
        E, _ = self._grid(E)
        out = np.zeros((E.size, ng, ng), dtype=np.float64)
        self._host("local_transmission", E.size, int(handle), _ind(ind), E.size, _ptr(E), ng, _ptr(g), _ptr(out),
                   refused=self._BOND_REFUSED)
        return out

    def local_transmission_dev(self, handle, ind, m, E_ptr, groups, out_ptr, n_groups=None):
        """negf_local_transmission_dev: grid and the [m, n_g, n_g] result in HBM; ``groups`` stays a host array (or None)."""
        ng, g = self._groups(groups, n_groups)
        self._counted(m)("negf_local_transmission_dev", int(handle), _ind(ind), int(m), _p(E_ptr), ng, _ptr(g),
                         _p(out_ptr), refused=self._BOND_REFUSED)

    def bond_int(self, handle, ind, E, w):
        """sum_k w_k flow(E_k) [n, n] float64 with REAL weights, one pass (negf_bond_int)."""
        w = self._real_weights(w, "bond_int")
        E, _ = self._grid(E)
        assert E.size == w.size, "Elist and weights must have the same length"
        out = np.zeros((self.n, self.n), dtype=np.float64)
        self._host("bond_int", E.size, int(handle), _ind(ind), E.size, _ptr(E), _ptr(w), _ptr(out),
                   refused=self._BOND_REFUSED)
        return out

    def bond_int_dev(self, handle, ind, m, E_ptr, w_ptr, out_ptr):
        """negf_bond_int_dev: E complex128 [m], w float64 [m] and out float64 [n, n] in HBM."""
        self._counted(m)("negf_bond_int_dev", int(handle), _ind(ind), int(m), _p(E_ptr), _p(w_ptr), _p(out_ptr),
                         refused=self._BOND_REFUSED)

    # ------------------------------------------- populations and projected DOS
    RETARDED = NEGF_IND_RETARDED                  # ``ind`` of the retarded form of population / projected_dos

    _POP_REFUSED = ("the contact form of population / projected_dos reads A = G Gamma_c G^H as Hermitian: coupling matrices "
                    "handed in by the caller (sigma_precomputed(gammas=...)) are not served (the retarded form, "
                    "ind = Engine.RETARDED, is), nor are systems of more than 8192 orbitals; an invalid contact index, op, "
                    "or number of vectors is refused the same way")
    _POP_OPS = {'S': 0, 'F': 1, 0: 0, 1: 1}

    def _pop_op(self, op):
        if not isinstance(op, (str, int)) or op not in self._POP_OPS:
            raise ValueError(f"op must be 'S' (overlap population) or 'F' (Hamilton population), got {op!r}")
        return self._POP_OPS[op]

    def _pop_ind(self, ind):
        return NEGF_IND_RETARDED if ind == 'retarded' else _ind(ind)

    def population(self, handle, ind, E, op='S', groups=None, n_groups=None, rows=False):
        """Overlap (``op='S'``, COOP) or Hamilton (``op='F'``, COHP) populations per energy (negf_population).
        ``ind = Engine.RETARDED``: pop[i, j] = -(1/pi) Im[G_ij conj(X_ij)]; a contact index or None (all contacts):
        that contact's share (1/2pi) Re[(G Gamma_c G^H)_ij conj(X_ij)].  Returns the tables [m, n_g, n_g] summed over
        ``groups`` (orbital -> group labels, None = per orbital pair), or with ``rows=True`` their row sums [m, n_g] --
        for ``op='S'`` the projected DOS of each orbital / atom / fragment, -Im (G S)_ii / pi summed over the group --
        in one pass, without the table.  Singular energies give NaN (with a warning, as transmission)."""
        op = self._pop_op(op)
        ng, g = self._groups(groups, n_groups)
        E, _ = self._grid(E)
        out = np.zeros((E.size, ng) if rows else (E.size, ng, ng), dtype=np.float64)
        self._host("population", E.size, int(handle), self._pop_ind(ind), op, int(bool(rows)), E.size, _ptr(E), ng, _ptr(g),
                   _ptr(out), refused=self._POP_REFUSED)
        return out

    def population_dev(self, handle, ind, m, E_ptr, out_ptr, op='S', groups=None, n_groups=None, rows=False):
        """negf_population_dev: grid and the [m, n_g, n_g] / [m, n_g] result in HBM; ``groups`` stays a host array."""
        op = self._pop_op(op)
        ng, g = self._groups(groups, n_groups)
        self._counted(m)("negf_population_dev", int(handle), self._pop_ind(ind), op, int(bool(rows)), int(m), _p(E_ptr),
                         ng, _ptr(g), _p(out_ptr), refused=self._POP_REFUSED)

    def projected_dos(self, handle, ind, E, W):
        """Projection on the vectors W [k, n] (negf_projected_dos): p[m, a] = -(1/pi) Im[w_a^H G w_a] for
        ``ind = Engine.RETARDED``, (1/2pi) Re[w_a^H G Gamma_c G^H w_a] for a contact.  For orbitals with coefficients c
        in a non-orthogonal basis pass w = S c."""
        W = np.ascontiguousarray(np.atleast_2d(np.asarray(W)), dtype=np.complex128)
        if W.ndim != 2 or W.shape[1] != self.n:
            raise ValueError(f"W must be [k, n] with n = {self.n}, got {W.shape}")
        E, _ = self._grid(E)
        k = W.shape[0]
        out = np.zeros((E.size, k), dtype=np.float64)
        self._host("projected_dos", E.size, int(handle), self._pop_ind(ind), E.size, _ptr(E), k, _ptr(W), _ptr(out),
                   refused=self._POP_REFUSED)
        return out

    def projected_dos_dev(self, handle, ind, m, E_ptr, k, W_ptr, out_ptr):
        """negf_projected_dos_dev: E complex128 [m], W complex128 [k, n] and out float64 [m, k] in HBM."""
        self._counted(m)("negf_projected_dos_dev", int(handle), self._pop_ind(ind), int(m), _p(E_ptr), int(k),
                         _p(W_ptr), _p(out_ptr), refused=self._POP_REFUSED)

    # ------------------------------------------------ multi-terminal transmission matrix
    _TMAT_REFUSED = ("the transmission matrix needs a self-energy provider whose couplings live on known contact orbital "
                     "lists (constant Sigma with a nonzero support per contact, 1-D chain leads, Bethe leads without the "
                     "Xi Sigma Xi transform) and at most 1024 terminals; this provider is not served")

    def _probes(self, probes, n=None):
        """The four arguments (n_probes, sizes int32, concatenated indices int32, concatenated blocks complex128) of a list
        of (indices, block); ValueError for an invalid list.  ``n``: the number of orbitals (None: the dense system's)."""
        if not probes:
            return 0, None, None, None
        n = self.n if n is None else n
        nk, inds, blocks = [], [], []
        for q, (idx, blk) in enumerate(probes):
            idx = np.asarray(idx).ravel()
            if idx.size < 1 or not np.issubdtype(idx.dtype, np.integer):
                raise ValueError(f"probe {q}: the orbital list must be a non-empty list of integers")
            if idx.min() < 0 or idx.max() >= n or np.unique(idx).size != idx.size:
                raise ValueError(f"probe {q}: orbital indices must be distinct and lie in [0, {n})")
            blk = np.asarray(blk)
            if blk.shape != (idx.size, idx.size):
                raise ValueError(f"probe {q}: expected a {idx.size}x{idx.size} block, got {blk.shape}")
            nk.append(idx.size); inds.append(idx.astype(np.int32)); blocks.append(_c128(blk).ravel())
        return (len(nk), _ptr(np.array(nk, dtype=np.int32)), _ptr(np.ascontiguousarray(np.concatenate(inds))),
                _ptr(np.ascontiguousarray(np.concatenate(blocks))))

    def terminal_count(self, handle, probes=None):
        """C = the provider's contacts + the probes: the size of transmission_matrix's result."""
        nc = self._table("_n_contacts").get(int(handle))
        if nc is None:
            raise ValueError(f"handle {handle} was not created by this engine")
        return nc + (len(probes) if probes else 0)

    def transmission_matrix(self, handle, E, probes=None):
        """T [m, C, C] between all terminals of the junction from one inverse per energy (negf_transmission_matrix):
        T[k, a, b] = Re Tr[Gamma_a G Gamma_b G^H](E_k), the transmission from b into a; the terminals are the provider's
        contacts followed by ``probes``, a list of (orbital indices, K x K complex block Sigma_p) -- fictitious,
        energy-independent contacts whose blocks are subtracted from E S - F - Sigma on their orbitals.  Matrices of
        singular energies are NaN (with a warning, as transmission).  NotImplementedError for providers without
        contact orbital lists."""
        pr = self._probes(probes)
        Cn = self.terminal_count(handle, probes)
        E, _ = self._grid(E)
        T = np.zeros((E.size, Cn, Cn), dtype=np.float64)
        self._host("transmission_matrix", E.size, int(handle), *pr, E.size, _ptr(E), _ptr(T), refused=self._TMAT_REFUSED)
        return T

    def transmission_matrix_dev(self, handle, m, E_ptr, T_ptr, probes=None):
        """negf_transmission_matrix_dev: grid and the [m, C, C] result in HBM; ``probes`` stays a host list (or None)."""
        pr = self._probes(probes)
        self._counted(m)("negf_transmission_matrix_dev", int(handle), *pr, int(m), _p(E_ptr), _p(T_ptr),
                         refused=self._TMAT_REFUSED)

    # ------------------------------------------------ floating dephasing probes
    # negf_common.h's DEPH_LDS_MAX_P / DEPH_LDS_MAX_RHS (test_dephase_host.test_size_class_constants_agree holds the copies together)
    DEPH_LDS_MAX_P = 80                           # the response kernel solves in LDS up to this many probes, above in HBM
    DEPH_LDS_MAX_RHS = 16                         # ... for providers of at most this many contacts

    _DEPH_REFUSED = ("floating probes need a self-energy provider whose couplings live on known contact orbital lists "
                     "(constant Sigma with a nonzero support per contact, 1-D chain leads, Bethe leads without the "
                     "Xi Sigma Xi transform) and at most 1024 terminals; this provider is not served")

    def _response(self, where, ends, n_ends, handle, pr, E, refused=None):
        """R [m, P, n_ends] of the probe-response call ``negf_<where>``; ``ends``: what its columns are called
        ("contact" / "terminal") where probes that reach none of them are reported"""
        E, _ = self._grid(E)
        R = np.zeros((E.size, pr[0], n_ends), dtype=np.float64)
        info = self._host(where, E.size, int(handle), *pr, E.size, _ptr(E), _ptr(R), refused=refused)
        lost = np.nonzero(np.isnan(R).any(axis=(1, 2)) & (info == 0))[0]      # (nothing where R has no rows or no columns)
        if lost.size:
            warnings.warn(f"{where}: probes without a path to any {ends} (singular W, undefined occupations) at "
                          f"energy indices {_first_bad(lost)}", RuntimeWarning)
        return R

    def probe_response(self, handle, E, probes):
        """R [m, P, n_c]: the response of the floating ``probes`` to the provider's contacts (negf_probe_response), solved
        on the device from the transmission matrices of Engine.transmission_matrix: probe p's occupation at E_k is
        sum_c R[k, p, c] f_c(E_k).  Rows of decoupled probes are exact zeros; the other rows sum to 1.  Singular energies
        give NaN (with a warning, as transmission_matrix)."""
        pr = self._probes(probes)
        return self._response("probe_response", "contact", self.terminal_count(handle), handle, pr, E, self._DEPH_REFUSED)

    def probe_response_dev(self, handle, m, E_ptr, R_ptr, probes):
        """negf_probe_response_dev: grid and the [m, P, n_c] result in HBM; ``probes`` stays a host list."""
        pr = self._probes(probes)
        self._counted(m)("negf_probe_response_dev", int(handle), *pr, int(m), _p(E_ptr), _p(R_ptr),
                         refused=self._DEPH_REFUSED)

    def _deph_ind(self, handle, ind, where):
        """an out-of-range contact index is the error gless_int raises for it, not a refused provider"""
        nc = self.terminal_count(handle)
        if ind is not None and not -nc <= int(ind) < nc:
            check(_lib.NEGF_EINVAL, f"negf_{where}: contact index {ind} outside [-{nc}, {nc})")
        return _ind(ind)

    def gless_int_probes(self, handle, ind, E, w, probes):
        """sum_k w_k G D_s G^H [n, n] with the ``probes`` floating (negf_gless_int_probes): D_s = Gamma_s + sum_p R_ps Gamma_p,
        G the inverse of the matrix that carries the probes; ``ind`` as gless_int (None: all terminals, no solve)."""
        where = "gless_int_probes"
        pr = self._probes(probes)
        E, w = self._grid(E, w)
        out = np.zeros((self.n, self.n), dtype=np.complex128)
        self._host(where, E.size, int(handle), self._deph_ind(handle, ind, where), *pr, E.size, _ptr(E), _ptr(w), _ptr(out),
                   refused=self._DEPH_REFUSED)
        return out

    def gless_int_probes_dev(self, handle, ind, m, E_ptr, w_ptr, out_ptr, probes):
        where = "gless_int_probes_dev"
        pr = self._probes(probes)
        self._counted(m)("negf_" + where, int(handle), self._deph_ind(handle, ind, where), *pr, int(m), _p(E_ptr),
                         _p(w_ptr), _p(out_ptr), refused=self._DEPH_REFUSED)

    def gr_int_probes(self, handle, E, w, probes):
        """sum_k w_k G(E_k) [n, n] with the ``probes`` in E S - F - Sigma (negf_gr_int_probes)."""
        pr = self._probes(probes)
        E, w = self._grid(E, w)
        out = np.zeros((self.n, self.n), dtype=np.complex128)
        self._host("gr_int_probes", E.size, int(handle), *pr, E.size, _ptr(E), _ptr(w), _ptr(out),
                   refused=self._DEPH_REFUSED)
        return out

    def gr_int_probes_dev(self, handle, m, E_ptr, w_ptr, out_ptr, probes):
        pr = self._probes(probes)
        self._counted(m)("negf_gr_int_probes_dev", int(handle), *pr, int(m), _p(E_ptr), _p(w_ptr), _p(out_ptr),
                         refused=self._DEPH_REFUSED)

    def _dos(self, where, E, n_site, per_site, *head):
        """(total [m], per site [m, n_site]) or the total alone of the DOS call ``negf_<where>``; ``head``: its arguments in
        front of the grid"""
        tot = np.zeros(E.size, dtype=np.float64)
        site = np.zeros((E.size, n_site), dtype=np.float64) if per_site else None
        self._host(where, E.size, *head, E.size, _ptr(E), _ptr(tot), _ptr(site))
        return (tot, site) if per_site else tot

    def dos(self, handle, E, per_site=True):
        """negf_dos: -Im diag G / pi, the reference's _dos_kernel -- it ignores the overlap matrix.  In a non-orthogonal
        basis the population is ``population(handle, Engine.RETARDED, E, rows=True)``."""
        E, _ = self._grid(E)
        return self._dos("dos", E, self.n, per_site, int(handle))

    def sigma_eval(self, handle, contact, E, n_contacts=1):
        E, _ = self._grid(E)
        out = np.zeros((E.size, self.n, self.n), dtype=np.complex128)
        iters = np.zeros((max(E.size, 1), max(n_contacts, 1)), dtype=np.int32)
        conv = np.zeros((max(E.size, 1), max(n_contacts, 1)), dtype=np.int32)
        self._call("negf_sigma_eval", int(handle), _ind(contact), E.size, _ptr(E), _ptr(out), _ptr(iters), _ptr(conv))
        self.last_iters = iters[:E.size]
        self.last_converged = conv[:E.size]
        return out

    # ------------------------------------------------------ layered devices
    # The recursive Green's function path (negf_layered_*): a layered system is an object of its own inside the context;
    # nothing here touches the dense system, its providers or ``self.n``.  Invalid arguments of these calls are the
    # caller's: ValueError, before anything was launched (_call).
    def layered_create(self, F_diag, F_up, S_diag, S_up):
        """Blocks of a layered system: L diagonal blocks n_i x n_i and L - 1 upper blocks n_i x n_{i+1} of F and S."""
        Fd = [_c128(b) for b in F_diag]; Sd = [_c128(b) for b in S_diag]
        Fu = [_c128(b) for b in F_up]; Su = [_c128(b) for b in S_up]
        L = len(Fd)
        if L < 2 or len(Sd) != L or len(Fu) != L - 1 or len(Su) != L - 1:
            raise ValueError("a layered system has L >= 2 diagonal blocks and L - 1 upper blocks of F and of S")
        sizes = []
        for i, b in enumerate(Fd):
            if b.ndim != 2 or b.shape[0] != b.shape[1] or b.shape[0] < 1 or Sd[i].shape != b.shape:
                raise ValueError(f"diagonal block {i}: F {b.shape}, S {Sd[i].shape}")
            sizes.append(b.shape[0])
        for i in range(L - 1):
            if Fu[i].shape != (sizes[i], sizes[i + 1]) or Su[i].shape != Fu[i].shape:
                raise ValueError(f"upper block {i}: expected {(sizes[i], sizes[i + 1])}, got F {Fu[i].shape}, S {Su[i].shape}")

        def cat(bl):
            return np.ascontiguousarray(np.concatenate([b.ravel() for b in bl])) if bl else np.zeros(0, np.complex128)
        sz = np.ascontiguousarray(sizes, dtype=np.int32)
        h = C.c_int(-1)
        self._call("negf_layered_create", L, _ptr(sz), _ptr(cat(Fd)), _ptr(cat(Fu)), _ptr(cat(Sd)), _ptr(cat(Su)), C.byref(h))
        self._table("_layered_sizes")[h.value] = tuple(sizes)
        self._table("_layered_nterm")[h.value] = 0
        return h.value

    def layered_free(self, handle):
        if getattr(self, "_ctx", None):
            self._lib.negf_layered_free(self._ctx, int(handle))
            self._table("_layered_sizes").pop(int(handle), None)
            self._table("_layered_nterm").pop(int(handle), None)

    def _lsizes(self, handle):
        try:
            return self._table("_layered_sizes")[int(handle)]
        except KeyError:
            raise ValueError(f"no layered system with handle {handle}") from None

    def _lprobes(self, handle, probes):
        """_probes for a layered system: the indices are numbered in the whole system in layer order"""
        return self._probes(probes, sum(self._lsizes(handle)))

    @staticmethod
    def _linds(inds):
        return np.ascontiguousarray(np.asarray(inds).ravel(), dtype=np.int32)

    def _lterminal(self, name, handle, *args):
        """Make an end terminal with ``name``; the system then has one more than the new terminal's number."""
        t = C.c_int(-1)
        self._call(name, int(handle), *args, C.byref(t))
        self._table("_layered_nterm")[int(handle)] = t.value + 1
        return t.value

    def layered_terminal_const(self, handle, layer, inds, sigma):
        inds = self._linds(inds)
        sig = _c128(sigma, (inds.size, inds.size))
        return self._lterminal("negf_layered_terminal_const", handle, int(layer), inds.size, _ptr(inds), _ptr(sig))

    def layered_terminal_chain(self, handle, layer, inds, alpha, Salpha, beta, Sbeta, tau, Stau, eta, conv=1e-5,
                               relFactor=0.1, max_iter=2000, force_iters=-1, solver='fixed-point',
                               tol=SURFACE_DOUBLING_TOL, max_steps=SURFACE_DOUBLING_MAX_STEPS):
        """A 1-D chain lead on ``inds`` of an end layer; arguments as sigma_chain1d's for one contact."""
        if solver not in ('fixed-point', 'doubling'):
            raise ValueError(f"solver must be 'fixed-point' or 'doubling', got {solver!r}")
        inds = self._linds(inds)
        k = inds.size
        mats = [_c128(x, (k, k)) for x in (alpha, Salpha, beta, Sbeta, tau, Stau)]
        rd = solver == 'doubling'
        return self._lterminal("negf_layered_terminal_chain", handle, int(layer), k, _ptr(inds), *[_ptr(x) for x in mats],
                               float(eta), float(tol if rd else conv), float(relFactor),
                               int(max_steps if rd else max_iter), int(force_iters), 1 if rd else 0)

    def layered_terminal_blocks(self, handle, layer, inds, sigma):
        """Self-energy blocks [m, K, K] supplied per energy: block k serves energy k of every later call."""
        inds = self._linds(inds)
        sig = _c128(sigma)
        if sig.ndim != 3 or sig.shape[1:] != (inds.size, inds.size) or sig.shape[0] < 1:
            raise ValueError(f"expected [m, {inds.size}, {inds.size}] blocks, got {sig.shape}")
        return self._lterminal("negf_layered_terminal_blocks", handle, int(layer), inds.size, _ptr(inds), sig.shape[0],
                               _ptr(sig))

    def layered_terminal_sigma(self, handle, terminal, E, K):
        """Sigma_t(E) [m, K, K] of a terminal with K orbitals."""
        E, _ = self._grid(E)
        out = np.zeros((E.size, int(K), int(K)), dtype=np.complex128)
        self._call("negf_layered_terminal_sigma", int(handle), int(terminal), E.size, _ptr(E), _ptr(out))
        return out

    def layered_transmission(self, handle, term_a, term_b, E):
        """T_ab(E) [m] between terminals on opposite end layers (the transmission from b into a)."""
        E, _ = self._grid(E)
        T = np.zeros(E.size, dtype=np.float64)
        self._host("layered_transmission", E.size, int(handle), int(term_a), int(term_b), E.size, _ptr(E), _ptr(T))
        return T

    def layered_dos(self, handle, E, mulliken=False, per_site=True):
        """(dos_total [m], dos_site [m, N]): -Im diag G / pi, or with ``mulliken`` -Im diag(G S) / pi."""
        E, _ = self._grid(E)
        return self._dos("layered_dos", E, sum(self._lsizes(handle)), per_site, int(handle), 1 if mulliken else 0)

    def _lsplit(self, handle, flat):
        """one pattern's values -> (diag, upper, lower) block lists: _lsplit_tables without the energy axis"""
        return tuple([t[0] for t in blocks] for blocks in self._lsplit_tables(self._lsizes(handle), flat[None]))

    def layered_pattern_size(self, handle):
        return self.layered_table_size(self._lsizes(handle))

    def _lpattern(self, where, handle, m, dtype, *args):
        """(diagonal, upper, lower) block lists of the integral ``negf_layered_<where>`` on the pattern of S; ``args``: all
        its arguments in front of the result"""
        flat = np.zeros(self.layered_pattern_size(handle), dtype=dtype)
        self._host(where, m, int(handle), *args, _ptr(flat))
        return self._lsplit(handle, flat)

    def layered_gr_int(self, handle, E, w):
        """sum_m w_m G(E_m) on the pattern of S: (diagonal blocks, upper blocks G_{i,i+1}, lower blocks G_{i+1,i})."""
        E, w = self._grid(E, w)
        return self._lpattern("layered_gr_int", handle, E.size, np.complex128, E.size, _ptr(E), _ptr(w))

    def layered_gless_int(self, handle, ind, E, w):
        """sum_m w_m G Gamma G^H on the pattern of S for terminal ``ind`` (None: all terminals), as gless_int: (diagonal
        blocks, upper blocks A_{i,i+1}, lower blocks sum_m w_m A_{i,i+1}(E_m)^H)."""
        E, w = self._grid(E, w)
        return self._lpattern("layered_gless_int", handle, E.size, np.complex128, _ind(ind), E.size, _ptr(E), _ptr(w))

    def layered_contact_dos(self, handle, ind, E, per_site=True):
        """(total [m], site [m, N]): terminal ``ind``'s share of the Mulliken DOS, (1/2pi) Re sum_j (G Gamma G^H)_ij conj(S_ij)
        (None: all terminals) -- population(h, ind, E, rows=True) of the dense engine."""
        E, _ = self._grid(E)
        return self._dos("layered_contact_dos", E, sum(self._lsizes(handle)), per_site, int(handle), _ind(ind))

    def layered_gless_int_dev(self, handle, ind, m, E_ptr, w_ptr, out_ptr):
        """out: layered_pattern_size(handle) complex values, diagonal | upper | lower blocks."""
        self._counted(m)("negf_layered_gless_int_dev", int(handle), _ind(ind), int(m), _p(E_ptr), _p(w_ptr),
                         _p(out_ptr))

    def layered_contact_dos_dev(self, handle, ind, m, E_ptr, tot_ptr, site_ptr):
        self._counted(m)("negf_layered_contact_dos_dev", int(handle), _ind(ind), int(m), _p(E_ptr), _p(tot_ptr),
                         _p(site_ptr))

    def layered_transmission_dev(self, handle, term_a, term_b, m, E_ptr, T_ptr):
        self._counted(m)("negf_layered_transmission_dev", int(handle), int(term_a), int(term_b), int(m), _p(E_ptr),
                         _p(T_ptr))

    def layered_dos_dev(self, handle, m, E_ptr, tot_ptr, site_ptr, mulliken=False):
        self._counted(m)("negf_layered_dos_dev", int(handle), 1 if mulliken else 0, int(m), _p(E_ptr), _p(tot_ptr),
                         _p(site_ptr))

    def layered_gr_int_dev(self, handle, m, E_ptr, w_ptr, out_ptr):
        """out: layered_pattern_size(handle) complex values, diagonal | upper | lower blocks."""
        self._counted(m)("negf_layered_gr_int_dev", int(handle), int(m), _p(E_ptr), _p(w_ptr), _p(out_ptr))

    def layered_terminal_count(self, handle, probes=None):
        """C = the system's end terminals + the probes: the size of layered_transmission_matrix's result."""
        self._lsizes(handle)
        return self._table("_layered_nterm")[int(handle)] + (len(probes) if probes else 0)

    def layered_transmission_matrix(self, handle, E, probes=None):
        """T [m, C, C] between ALL terminals of a layered system (negf_layered_transmission_matrix): T[k, a, b] =
        Re Tr[Gamma_a G Gamma_b G^H](E_k), the transmission from b into a, as transmission_matrix defines it.  The terminals
        are the end terminals in the order they were made, then ``probes``: a list of (orbital indices, K x K complex block
        Sigma_p) as transmission_matrix takes, the indices numbered in the whole system in layer order and each probe
        inside ONE layer -- any layer.  Without probes: the matrix over the end terminals, same-end pairs included.
        ValueError for a probe that spans layers, repeats or leaves the system, and for more than 1024 terminals; matrices
        of singular energies are NaN (with a warning, as layered_transmission)."""
        pr = self._lprobes(handle, probes)
        Cn = self.layered_terminal_count(handle, probes)
        E, _ = self._grid(E)
        T = np.zeros((E.size, Cn, Cn), dtype=np.float64)
        self._host("layered_transmission_matrix", E.size, int(handle), *pr, E.size, _ptr(E), _ptr(T))
        return T

    def layered_transmission_matrix_dev(self, handle, m, E_ptr, T_ptr, probes=None):
        """negf_layered_transmission_matrix_dev: grid and the [m, C, C] result in HBM; ``probes`` stays a host list."""
        pr = self._lprobes(handle, probes)
        self._counted(m)("negf_layered_transmission_matrix_dev", int(handle), *pr, int(m), _p(E_ptr), _p(T_ptr))

    # ------------------------------------------------ floating dephasing probes on a layered system
    def layered_probe_response(self, handle, E, probes):
        """R [m, P, n_t]: the response of the floating ``probes`` (layered_transmission_matrix's lists, any layer) to the
        system's end terminals (negf_layered_probe_response), as probe_response: probe p's occupation at E_k is
        sum_c R[k, p, c] f_c(E_k); rows of decoupled probes are exact zeros, the others sum to 1.  Singular energies and
        energies whose probes reach no end terminal give NaN (with a warning, as probe_response)."""
        pr = self._lprobes(handle, probes)
        return self._response("layered_probe_response", "terminal", self.layered_terminal_count(handle), handle, pr, E)

    def layered_probe_response_dev(self, handle, m, E_ptr, R_ptr, probes):
        """negf_layered_probe_response_dev: grid and the [m, P, n_t] result in HBM; ``probes`` stays a host list."""
        pr = self._lprobes(handle, probes)
        self._counted(m)("negf_layered_probe_response_dev", int(handle), *pr, int(m), _p(E_ptr), _p(R_ptr))

    def layered_gless_int_probes(self, handle, ind, E, w, probes):
        """sum_k w_k G D_s G^H on the pattern of S with the ``probes`` floating (negf_layered_gless_int_probes): D_s = Gamma_s +
        sum_p R_ps Gamma_p, G the inverse of the matrix that carries the probes; ``ind`` as layered_gless_int (None: all
        terminals, no solve).  Returns layered_gless_int's (diagonal, upper, lower) block lists."""
        pr = self._lprobes(handle, probes)
        E, w = self._grid(E, w)
        return self._lpattern("layered_gless_int_probes", handle, E.size, np.complex128, _ind(ind), *pr, E.size, _ptr(E),
                              _ptr(w))

    def layered_gless_int_probes_dev(self, handle, ind, m, E_ptr, w_ptr, out_ptr, probes):
        """out: layered_pattern_size(handle) complex values, diagonal | upper | lower blocks; ``probes`` stays a host list."""
        pr = self._lprobes(handle, probes)
        self._counted(m)("negf_layered_gless_int_probes_dev", int(handle), _ind(ind), *pr, int(m), _p(E_ptr), _p(w_ptr),
                         _p(out_ptr))

    def layered_gr_int_probes(self, handle, E, w, probes):
        """sum_k w_k G(E_k) on the pattern of S with the ``probes`` in E S - F - Sigma (negf_layered_gr_int_probes):
        layered_gr_int's (diagonal, upper, lower) block lists."""
        pr = self._lprobes(handle, probes)
        E, w = self._grid(E, w)
        return self._lpattern("layered_gr_int_probes", handle, E.size, np.complex128, *pr, E.size, _ptr(E), _ptr(w))

    def layered_gr_int_probes_dev(self, handle, m, E_ptr, w_ptr, out_ptr, probes):
        """out: layered_pattern_size(handle) complex values, diagonal | upper | lower blocks; ``probes`` stays a host list."""
        pr = self._lprobes(handle, probes)
        self._counted(m)("negf_layered_gr_int_probes_dev", int(handle), *pr, int(m), _p(E_ptr), _p(w_ptr), _p(out_ptr))

    def _lgroups(self, handle, groups_per_layer, group_of):
        """(g [L] sizes of the tables, the two host arrays or None) of a bond-table call; only the lengths are checked
        here -- the library must not read past an array -- everything else is the library's NEGF_EINVAL."""
        sizes = self._lsizes(handle)
        gpl = go = None
        if groups_per_layer is not None:
            gpl = np.ascontiguousarray(np.asarray(groups_per_layer).ravel(), dtype=np.int32)
            if gpl.size != len(sizes):
                raise ValueError(f"groups_per_layer must have one entry per layer ({len(sizes)}), got {gpl.size}")
        if group_of is not None:
            go = np.ascontiguousarray(np.asarray(group_of).ravel(), dtype=np.int32)
            if go.size != sum(sizes):
                raise ValueError(f"group_of must map each of the {sum(sizes)} orbitals to a group of its layer, got {go.size} entries")
        g = tuple(int(x) for x in gpl) if gpl is not None and go is not None else sizes
        return g, gpl, go

    @staticmethod
    def _lsplit_tables(g, flat):
        """[m, table] -> (diag, upper, lower) block lists [m, g_i, g_j], negf_layered_gr_int's order with g in place of n"""
        m = flat.shape[0]
        diag, up, low, o = [], [], [], 0
        for n in g:
            diag.append(flat[:, o:o + n * n].reshape(m, n, n)); o += n * n
        for a, b in zip(g[:-1], g[1:]):
            up.append(flat[:, o:o + a * b].reshape(m, a, b)); o += a * b
        for a, b in zip(g[:-1], g[1:]):
            low.append(flat[:, o:o + a * b].reshape(m, b, a)); o += a * b
        return diag, up, low

    @staticmethod
    def layered_table_size(g):
        return sum(n * n for n in g) + 2 * sum(a * b for a, b in zip(g[:-1], g[1:]))

    def layered_local_transmission(self, handle, ind, E, groups_per_layer=None, group_of=None):
        """Local (bond) transmission of the current injected by terminal ``ind`` (None: all) on the pattern of S
        (negf_layered_local_transmission): (diag, upper, lower) block lists, entry [k, a, b] of a block =
        sum_{r in a, c in b} 2 Im[(E_k S - F)_rc (G Gamma G^H)_cr].  ``groups_per_layer`` [L] and ``group_of`` [N] (for each
        orbital its group inside its own layer) reduce the blocks to [m, g_i, g_j]; both None: per orbital pair.  Tables of
        singular energies are NaN (with a warning, as layered_transmission)."""
        g, gpl, go = self._lgroups(handle, groups_per_layer, group_of)
        E, _ = self._grid(E)
        flat = np.zeros((E.size, self.layered_table_size(g)), dtype=np.float64)
        self._host("layered_local_transmission", E.size, int(handle), _ind(ind), E.size, _ptr(E), _ptr(gpl), _ptr(go),
                   _ptr(flat))
        return self._lsplit_tables(g, flat)

    def layered_local_transmission_dev(self, handle, ind, m, E_ptr, out_ptr, groups_per_layer=None, group_of=None):
        """negf_layered_local_transmission_dev: grid and the [m, layered_table_size(g)] result in HBM; the groups stay
        host arrays (or None)."""
        _, gpl, go = self._lgroups(handle, groups_per_layer, group_of)
        self._counted(m)("negf_layered_local_transmission_dev", int(handle), _ind(ind), int(m), _p(E_ptr), _ptr(gpl),
                         _ptr(go), _p(out_ptr))

    def layered_bond_int(self, handle, ind, E, w):
        """sum_k w_k flow(E_k) at orbital level with REAL weights, one pass (negf_layered_bond_int): (diagonal blocks,
        upper blocks, lower blocks) of float64."""
        w = self._real_weights(w, "layered_bond_int")
        E, _ = self._grid(E)
        assert E.size == w.size, "Elist and weights must have the same length"
        return self._lpattern("layered_bond_int", handle, E.size, np.float64, _ind(ind), E.size, _ptr(E), _ptr(w))

    def layered_bond_int_dev(self, handle, ind, m, E_ptr, w_ptr, out_ptr):
        """negf_layered_bond_int_dev: E complex128 [m], w float64 [m] and out float64 [layered_pattern_size] in HBM."""
        self._counted(m)("negf_layered_bond_int_dev", int(handle), _ind(ind), int(m), _p(E_ptr), _p(w_ptr), _p(out_ptr))

    def layered_workspace_bytes(self, handle):
        v = C.c_longlong(0)
        self._call("negf_layered_workspace_bytes", int(handle), C.byref(v))
        return int(v.value)

    # -------------------------------------------------- device-resident calls
    def gr_int_dev(self, handle, m, E_ptr, w_ptr, out_ptr):
        self._counted(m)("negf_gr_int_dev", int(handle), int(m), _p(E_ptr), _p(w_ptr), _p(out_ptr))

    def gless_int_dev(self, handle, ind, m, E_ptr, w_ptr, out_ptr):
        self._counted(m)("negf_gless_int_dev", int(handle), _ind(ind), int(m), _p(E_ptr), _p(w_ptr), _p(out_ptr))

    def gr_int_seg_dev(self, handle, m, E_ptr, w_ptr, ends, out_ptr):
        """negf_gr_int_seg_dev: ``ends`` (host, int32) = index one past each segment; out [len(ends)][n][n] on the device."""
        ends = np.ascontiguousarray(ends, dtype=np.int32)
        self._counted(m)("negf_gr_int_seg_dev", int(handle), int(m), _p(E_ptr), _p(w_ptr), int(ends.size), _ptr(ends),
                         _p(out_ptr))

    def gless_int_seg_dev(self, handle, ind, m, E_ptr, w_ptr, ends, out_ptr):
        ends = np.ascontiguousarray(ends, dtype=np.int32)
        self._counted(m)("negf_gless_int_seg_dev", int(handle), _ind(ind), int(m), _p(E_ptr), _p(w_ptr), int(ends.size),
                         _ptr(ends), _p(out_ptr))

    def transmission_dev(self, handle, contact_L, contact_R, m, E_ptr, T_ptr, Tspin_ptr=0, spin_block=False):
        mode = NEGF_SPIN_BLOCK if spin_block else NEGF_SPIN_RESTRICTED
        self._counted(m)("negf_transmission_dev", int(handle), int(contact_L), int(contact_R), mode, int(m), _p(E_ptr),
                         _p(T_ptr), _p(Tspin_ptr or 0))

    def last_info_dev(self, m):
        info = np.zeros(max(m, 1), dtype=np.int32)
        self._call("negf_last_info", int(m), _ptr(info))
        return info[:m]

    def warn_if_singular_dev(self, m, where, grid_index=None):
        """The *_dev entry points return no per-energy info: fetch it and warn like the host variants
        (``grid_index``: the grid indices of the m energies when they are a shard of a larger grid)."""
        info = self.last_info_dev(m)
        self._numerical(_lib.NEGF_ESINGULAR if np.any(info) else 0, info, where, grid_index)

    def last_iters_dev(self, handle, m, n_contacts):
        """(sweeps, converged) [m, n_contacts] of the fixed points run by the last call."""
        it = np.zeros((max(m, 1), max(n_contacts, 1)), dtype=np.int32)
        cv = np.zeros((max(m, 1), max(n_contacts, 1)), dtype=np.int32)
        self._call("negf_last_iters", int(handle), int(m), _ptr(it), _ptr(cv))
        return it[:m], cv[:m]

    # ---------------------------------------------------------- diagnostics
    def profile(self, on=True):
        self._call("negf_profile_enable", 1 if on else 0)

    def profile_reset(self):
        self._call("negf_profile_reset")

    def profile_read(self, family):
        ms = C.c_double(0.0)
        n = C.c_int(0)
        self._call("negf_profile_read", family.encode(), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def profile_read_flops(self, family):
        """(algorithmic flops, flops issued to the matrix cores) of the family's launches since profile_reset."""
        a = C.c_double(0.0); m = C.c_double(0.0)
        self._call("negf_profile_read_flops", family.encode(), C.byref(a), C.byref(m))
        return a.value, m.value

    def selftest_mfma(self):
        err = C.c_double(-1.0)
        self._call("negf_selftest_mfma", C.byref(err))
        return err.value

    def zgemm(self, M, N, K, nb, A, lda, strideA, B, ldb, strideB, opB, C_in, ldc, strideC, kernel=0):
        """The batched product kernels on flat complex128 arrays with explicit leading dimensions and batch strides
        (negf_zgemm_batched, a diagnostic call; include/negf.h has the layout, opB and kernel).  ``C_in`` is what the
        device result array holds before the launch; the whole array comes back, so the caller sees what was written."""
        A, B = _c128(A).ravel(), _c128(B).ravel()
        out = np.array(C_in, dtype=np.complex128).ravel()             # a copy: C_in stays as it is
        rows_b, rows_c = (N if opB & 1 else K), (N if opB & 4 else M)
        need = ((strideA * nb if strideA else M * lda), (strideB * nb if strideB else rows_b * ldb), strideC * nb)
        if A.size < need[0] or B.size < need[1] or out.size < need[2] or strideC < rows_c * ldc:
            raise ValueError(f"zgemm: arrays of {A.size}, {B.size}, {out.size} elements, the layout needs {need}")
        self._call("negf_zgemm_batched", int(M), int(N), int(K), int(nb), _ptr(A), int(lda), int(strideA), _ptr(B), int(ldb),
                   int(strideB), int(opB), _ptr(out), int(ldc), int(strideC), int(kernel))
        return out

    # (zgemm_plan and inverse_plan take no context and no engine: they call the loaded library directly)
    @staticmethod
    def zgemm_plan(M, N, K=1, opB=0, nb=1, kernel=0):
        """What ``zgemm`` does with a shape (negf_zgemm_plan; needs no GPU): a dict with ``kernel`` (1 = 64 x 64 blocks,
        2 = flexible blocks, 3 = vector unit), ``opB`` after the demotion of the Hermitian bit, ``blocks`` (rows,
        columns), ``grid`` (x, y, z) and, for a Hermitian launch of kernel 1 or 2, ``decode``: int32 [grid x, 3], the
        (block row, block column, batch member) of every workgroup, -1 for one that returns at once (else None)."""
        lib = _lib.load()
        ku, oe = C.c_int(0), C.c_int(0)
        blocks, grid = (C.c_int * 2)(), (C.c_int * 3)()
        args = (int(M), int(N), int(K), int(opB), int(nb), int(kernel), C.byref(ku), C.byref(oe), blocks, grid)
        check(lib.negf_zgemm_plan(*args, None, 0), "negf_zgemm_plan")
        decode = None
        if (oe.value & 2) and ku.value != 3:
            decode = np.zeros((grid[0], 3), dtype=np.int32)
            check(lib.negf_zgemm_plan(*args, decode.ctypes.data_as(C.POINTER(C.c_int)), int(grid[0])), "negf_zgemm_plan")
        return {"kernel": ku.value, "opB": oe.value, "blocks": (blocks[0], blocks[1]),
                "grid": (grid[0], grid[1], grid[2]), "decode": decode}

    INVERSE_WINDOW_KERNELS = {0: "none", 1: "strip<1,32,4,2,4>", 5: "strip<2,16,4,2,1>", 6: "strip<2,16,8,1,2>",
                              7: "la<16,4,6>", 8: "la<16,8,12>", 9: "team", 10: "single"}    # (2, 3, 4: retired, unused)

    @staticmethod
    def inverse_plan(n, nb, algo=0, defer=False):
        """What the inverse of ``nb`` matrices of dimension ``n`` launches (negf_inverse_plan; needs no GPU): a dict
        with ``path`` (0 unblocked, 1 single workgroup, 2 windowed), ``cls`` = (NBI, RPT), ``nblk``, ``gather``,
        ``deferred`` and ``groups``: a list of dicts ``first``, ``count``, ``wk`` (window kernel id, named by
        INVERSE_WINDOW_KERNELS), ``pairs``, ``upd_full`` / ``upd_single`` (4 lean, 8 fat, 0 none) and ``mask``."""
        lib = _lib.load()
        v = [C.c_int(0) for _ in range(7)]
        tab = (C.c_int * 28)()
        check(lib.negf_inverse_plan(int(n), int(nb), int(algo), int(bool(defer)), C.byref(v[0]), C.byref(v[1]),
                                    C.byref(v[2]), C.byref(v[3]), C.byref(v[4]), tab, C.byref(v[5]), C.byref(v[6])),
              "negf_inverse_plan")
        keys = ("first", "count", "wk", "pairs", "upd_full", "upd_single", "mask")
        groups = [dict(zip(keys, tab[7 * g:7 * g + 7])) for g in range(v[4].value)]
        return {"path": v[0].value, "cls": (v[1].value, v[2].value), "nblk": v[3].value, "groups": groups,
                "gather": bool(v[5].value), "deferred": bool(v[6].value)}

    def inverse_last(self):
        """What this engine's last inverse launched (negf_inverse_last): ``path`` and ``masks``, the launch mask of
        every group -- equal to ``[g["mask"] for g in inverse_plan(...)["groups"]]`` when the launch followed the plan."""
        path, groups = C.c_int(0), C.c_int(0)
        masks = (C.c_int * 4)()
        self._call("negf_inverse_last", C.byref(path), C.byref(groups), masks)
        return {"path": path.value, "masks": [masks[g] for g in range(groups.value)]}


def get_engine(device=None):
    """Process-wide engine for ``device`` (default: LOCAL_RANK, else 0)."""
    key = device
    if key not in _engines:
        _engines[key] = Engine(device)
    return _engines[key]


def reset_engines():
    for e in _engines.values():
        e.close()
    _engines.clear()
