"""
Energy-grid integration of Green's functions -- drop-in for gauNEGF/integrate.py.

    GrInt(F, S, g, Elist, weights)            -> sum_m w_m G^r(E_m)          (integrate.py:146-173)
    GrLessInt(F, S, g, Elist, weights, ind)   -> sum_m w_m G Gamma_c G^H     (integrate.py:177-208)

The reference vmaps a per-energy closure and, above 5 GB of [M,N,N] temporaries,
falls back to scan-over-batches (integrate.py:97-142).  Here the whole grid goes to
libnegf_hip.so in one call: the library streams the energies through a fixed
workspace (assemble -> blocked Gauss-Jordan inverse -> products -> weighted
accumulate) and never materialises [M,N,N].

How ``g`` reaches the device:
  * provider objects of this package (surfGTest, surfG, surfGB) lower themselves to
    a device-side provider (``_negf_lower``): Sigma(E) is produced on the GPU;
  * any other object with ``sigmaTot(E)`` / ``sigma(E, i)`` (the reference's duck
    typed protocol, integrate.py:169,203-204) is called on the host once per energy
    and its matrices are shipped as a PRECOMPUTED provider, chunked so the staged
    Sigma stays below ``CALLBACK_STAGE_BYTES``.
"""
import numpy as np

from . import distributed as _dist
from .engine import get_engine

CALLBACK_STAGE_BYTES = 1.0e9      # host-evaluated Sigma staged per chunk


def _check(F, S, Elist, weights):
    # same assertions, same messages as integrate.py:85-87
    assert Elist.size == weights.size, "Elist and weights must have the same length"
    assert F.shape == S.shape, "F and S must have the same shape"
    assert F.shape[0] == F.shape[1], "F and S must be square matrices"


def _callback_chunks(n, m, per_energy_mats):
    per = 16.0 * n * n * per_energy_mats
    step = max(1, int(CALLBACK_STAGE_BYTES // per))
    return [(a, min(a + step, m)) for a in range(0, m, step)]


def _sigma_tot_stack(g, E):
    """[m,n,n] host-evaluated Sigma_tot; providers may offer a vectorised ``sigmaTot_batch``
    (one GPU launch for all energies, e.g. surfGBAt) instead of one call per energy."""
    if hasattr(g, "sigmaTot_batch"):
        return np.asarray(g.sigmaTot_batch(E))
    return np.stack([np.asarray(g.sigmaTot(e)) for e in E])


def _partial_gr(engine, g, E, w):
    """sum over the given energies on this process's GPU."""
    if E.size == 0:
        return np.zeros((engine.n, engine.n), dtype=np.complex128)
    if hasattr(g, "_negf_lower"):
        return engine.gr_int(g._negf_lower(engine), E, w)
    acc = np.zeros((engine.n, engine.n), dtype=np.complex128)
    for a, b in _callback_chunks(engine.n, E.size, 1):
        sig = _sigma_tot_stack(g, E[a:b])
        h = engine.sigma_precomputed(sig)
        try:
            acc += engine.gr_int(h, E[a:b], w[a:b])
        finally:
            engine.sigma_free(h)
    return acc


def _partial_gless(engine, g, E, w, ind):
    if E.size == 0:
        return np.zeros((engine.n, engine.n), dtype=np.complex128)
    if hasattr(g, "_negf_lower"):
        return engine.gless_int(g._negf_lower(engine), ind, E, w)
    acc = np.zeros((engine.n, engine.n), dtype=np.complex128)
    for a, b in _callback_chunks(engine.n, E.size, 1 if ind is None else 2):
        sig = _sigma_tot_stack(g, E[a:b])
        sig_c = None if ind is None else np.stack([np.asarray(g.sigma(e, ind)) for e in E[a:b]])
        h = engine.sigma_precomputed(sig, sig_c)
        try:
            # the staged provider holds exactly one contact matrix (index 0)
            acc += engine.gless_int(h, None if ind is None else 0, E[a:b], w[a:b])
        finally:
            engine.sigma_free(h)
    return acc


# --------------------------------------------------------------------------- #
# spin-polarised systems without spin mixing: blockdiag(alpha, beta) (scf.py:177-180)
# --------------------------------------------------------------------------- #
SPIN_BLOCK_SPLIT = True      # False: always work on the full 2N x 2N matrices, as the reference does


class _NotBlockDiagonal(Exception):
    pass


class _SpinBlockView:
    """One diagonal N x N block of a foreign 2N x 2N provider (reference protocol, host evaluated): every
    matrix it hands out is checked to vanish outside the diagonal blocks."""
    def __init__(self, g, N, sl, cache):
        self.g, self.N, self.sl, self.cache = g, N, sl, cache

    def _block(self, key, fn):
        if key not in self.cache:
            if len(self.cache) > 64:
                self.cache.clear()
            full = np.asarray(fn())
            N = self.N
            if full.shape != (2 * N, 2 * N) or np.any(full[:N, N:]) or np.any(full[N:, :N]):
                raise _NotBlockDiagonal()
            self.cache[key] = full
        return self.cache[key][self.sl, self.sl]

    def sigmaTot(self, E):
        return self._block(("t", complex(E)), lambda: self.g.sigmaTot(E))

    def sigma(self, E, i):
        return self._block(("c", complex(E), i), lambda: self.g.sigma(E, i))


_SPLIT_BLOCKS = {}        # the blocks of the last block-diagonal system: key (id, shape, dtype, fingerprint) of F and S


def _split_blocks(F, S, N):
    """(F_aa, S_aa, F_bb, S_bb) as contiguous READ-ONLY copies when F, S are exactly block diagonal, else None.  A front-end
    that alternates between two entry points on one system (GrLessInt, calculate_transmission, ...) hands the same 2N x 2N
    arrays over again and again: scanning the off-diagonal blocks, copying the diagonal ones and converting them to
    complex was 20 ms per entry point at N = 1000 (38 of the 148 ms of a per-GPU share of BASELINE C5).  The answer is kept
    for the last system, recognised by object identity AND a checksum of its bytes (a caller may have changed it in place);
    the blocks are read-only, so the engine keeps their complex conversions without comparing contents."""
    from .engine import fingerprint
    key = None
    if F.flags.c_contiguous and S.flags.c_contiguous:
        key = (id(F), id(S), F.shape, F.dtype.str, S.dtype.str, fingerprint(F), fingerprint(S))
        hit = _SPLIT_BLOCKS.get("last")
        if hit is not None and hit[0] == key:
            return hit[1]
    n2 = F.shape[0]
    blocks = None
    if not any(np.any(M[:N, N:]) or np.any(M[N:, :N]) for M in (F, S)):
        blocks = tuple(np.ascontiguousarray(M[sl, sl]) for sl in (slice(0, N), slice(N, n2)) for M in (F, S))
        for b in blocks:
            b.setflags(write=False)
    if key is not None:
        _SPLIT_BLOCKS["last"] = (key, blocks)
    return blocks


def _spin_split(F, S, g):
    """[(slice, F_block, S_block, g_block)] * 2 when F, S are exactly block diagonal 2N x 2N matrices and
    the provider can serve the blocks separately; None otherwise.  Two N-sized solves then replace the
    2N-sized one (a quarter of the flops); the result is the same up to rounding -- and exactly zero
    between the blocks."""
    n2 = F.shape[0]
    if not SPIN_BLOCK_SPLIT or n2 % 2 or n2 < 4:
        return None
    N = n2 // 2
    sls = (slice(0, N), slice(N, n2))
    if hasattr(g, "_negf_spin_split"):
        pass
    elif hasattr(g, "_negf_lower"):
        return None                                   # device-side provider defined on the 2N space
    blocks = _split_blocks(F, S, N)
    if blocks is None:
        return None
    if hasattr(g, "_negf_spin_split"):
        halves = g._negf_spin_split(N)
        if halves is None:
            return None
    else:
        cache = {}
        halves = [_SpinBlockView(g, N, sl, cache) for sl in sls]
    return [(sls[0], blocks[0], blocks[1], halves[0]), (sls[1], blocks[2], blocks[3], halves[1])]


_split_depth = 0          # > 0 while the blocks of a split system are being integrated: split once, not recursively


def _blockwise(F, S, g, call):
    global _split_depth
    if _split_depth:          # a spin block that happens to be block diagonal itself (e.g. diagonal F, S = I)
        return None
    parts = _spin_split(F, S, g)
    if parts is None:
        return None
    out = np.zeros(F.shape, dtype=np.complex128)
    _split_depth += 1
    try:
        for sl, Fb, Sb, gb in parts:
            out[sl, sl] = call(np.ascontiguousarray(Fb), np.ascontiguousarray(Sb), gb)
    except _NotBlockDiagonal:
        return None
    finally:
        _split_depth -= 1
    return out


def _as_grid(Elist, weights):
    E = np.asarray(Elist)
    w = np.asarray(weights)
    return E, w


def GrInt(F, S, g, Elist, weights):
    """Integrated retarded Green's function, N x N complex (integrate.py:146-173)."""
    F = np.asarray(F)
    S = np.asarray(S)
    E, w = _as_grid(Elist, weights)
    _check(F, S, E, w)
    split = _blockwise(F, S, g, lambda Fb, Sb, gb: GrInt(Fb, Sb, gb, E, w))
    if split is not None:
        return split
    engine = get_engine()
    engine.set_system(F, S)
    E = np.ascontiguousarray(E.ravel(), dtype=np.complex128)
    w = np.ascontiguousarray(w.ravel(), dtype=np.complex128)
    if _dist.is_active() and hasattr(g, "_negf_lower"):
        # N > 1: the partial sum never leaves HBM before the (single) all-reduce
        h = g._negf_lower(engine)
        return _dist.sharded_device_sum(engine, lambda m, Ep, wp, op: engine.gr_int_dev(h, m, Ep, wp, op), E, w)
    return _dist.sharded_sum(lambda idx: _partial_gr(engine, g, E[idx], w[idx]), E.size)


def can_fuse_segments(F, S, g):
    """True when GrIntSegments / GrLessIntSegments evaluate several integrals of this system in ONE pass of the engine
    (per spin block, and per rank when the energy grid is sharded -- then with ONE all-reduce for all of them): ``g``
    lowers to a device-side provider, directly or block by block.  Everything else (foreign providers evaluated on the
    host) falls back to one GrInt per segment -- callers that evaluate levels AHEAD of a convergence test
    (density._speculation_budget) must not speculate then: every speculated level would be a launch of its own."""
    if hasattr(g, "_negf_lower") and not hasattr(g, "_negf_spin_split"):
        return True
    if _split_depth:
        return hasattr(g, "_negf_lower")
    parts = _spin_split(np.asarray(F), np.asarray(S), g)
    if parts is None:
        return hasattr(g, "_negf_lower")
    return all(hasattr(gb, "_negf_lower") for _, _, _, gb in parts)


def _blockwise_segments(F, S, g, nseg, call):
    """The spin blocks of a block-diagonal system, each through ``call(F_block, S_block, g_block) -> [nseg sums]``."""
    global _split_depth
    if _split_depth:
        return None
    parts = _spin_split(F, S, g)
    if parts is None:
        return None
    outs = [np.zeros(F.shape, dtype=np.complex128) for _ in range(nseg)]
    _split_depth += 1
    try:
        for sl, Fb, Sb, gb in parts:
            for o, v in zip(outs, call(Fb, Sb, gb)):
                o[sl, sl] = v
    except _NotBlockDiagonal:
        return None
    finally:
        _split_depth -= 1
    return outs


def _c128_segments(segs):
    return [(np.ascontiguousarray(E.ravel(), dtype=np.complex128), np.ascontiguousarray(w.ravel(), dtype=np.complex128))
            for E, w in segs]


def GrIntSegments(F, S, g, segments):
    """``[GrInt(F, S, g, E, w) for (E, w) in segments]`` from ONE pass of the engine over all the energies
    (negf_gr_int_seg; under energy sharding negf_gr_int_seg_dev on the rank's share of all the segments and ONE
    all-reduce of the stacked sums; a block-diagonal spin system block by block) when ``g`` lives on the device; a
    plain loop of GrInt otherwise (foreign providers).  The adaptive integrations of density.py hand the levels they
    are about to visit over together -- a level of 2 ... 36 points alone in a launch is latency, not work -- and a density
    step its contour and real-axis grids (scfE.py:316-328)."""
    F = np.asarray(F)
    S = np.asarray(S)
    segs = [(np.asarray(E), np.asarray(w)) for E, w in segments]
    for E, w in segs:
        _check(F, S, E, w)
    if len(segs) < 2:
        return [GrInt(F, S, g, E, w) for E, w in segs]
    split = _blockwise_segments(F, S, g, len(segs), lambda Fb, Sb, gb: GrIntSegments(Fb, Sb, gb, segs))
    if split is not None:
        return split
    if not hasattr(g, "_negf_lower"):
        return [GrInt(F, S, g, E, w) for E, w in segs]
    engine = get_engine()
    engine.set_system(F, S)
    h = g._negf_lower(engine)
    if _dist.is_active():
        return _dist.sharded_device_seg_sums(
            engine, lambda m, Ep, wp, ends, op: engine.gr_int_seg_dev(h, m, Ep, wp, ends, op), _c128_segments(segs))
    return engine.gr_int_seg(h, segs)


def GrIntRefiner(F, S, g):
    """``refine(requests, tol)`` -- the nested adaptive refinement of one or several GrInt integrals of this system with the
    update and the stopping test ON THE DEVICE (Engine.gr_int_refine / negf_gr_int_refine: the level sums never leave HBM,
    only the refined value comes back) -- or None where that form does not apply: a provider evaluated on the host, an
    energy-sharded run (the level sums are all-reduced, the host refines), a spin-block system, more than 4096 orbitals."""
    from .engine import Engine
    F = np.asarray(F)
    S = np.asarray(S)
    if not hasattr(g, "_negf_lower") or _dist.is_active() or _split_depth or F.shape[0] > Engine.REFINE_MAX_N:
        return None
    if _spin_split(F, S, g) is not None:
        return None

    def refine(requests, tol):
        assert len(requests) <= Engine.REFINE_MAX_INTEGRALS and sum(len(r[2]) for r in requests) <= Engine.REFINE_MAX_LEVELS
        for E, w, *_ in requests:
            _check(F, S, np.asarray(E), np.asarray(w))
        engine = get_engine()
        engine.set_system(F, S)
        return engine.gr_int_refine(g._negf_lower(engine), requests, tol)
    return refine


def GrLessIntSegments(F, S, g, segments, ind=None):
    """``[GrLessInt(F, S, g, E, w, ind) for (E, w) in segments]`` from one pass of the engine (negf_gless_int_seg /
    negf_gless_int_seg_dev); a plain loop under the same conditions as GrIntSegments."""
    F = np.asarray(F)
    S = np.asarray(S)
    segs = [(np.asarray(E), np.asarray(w)) for E, w in segments]
    for E, w in segs:
        _check(F, S, E, w)
    if len(segs) < 2:
        return [GrLessInt(F, S, g, E, w, ind) for E, w in segs]
    split = _blockwise_segments(F, S, g, len(segs), lambda Fb, Sb, gb: GrLessIntSegments(Fb, Sb, gb, segs, ind))
    if split is not None:
        return split
    if not hasattr(g, "_negf_lower"):
        return [GrLessInt(F, S, g, E, w, ind) for E, w in segs]
    engine = get_engine()
    engine.set_system(F, S)
    h = g._negf_lower(engine)
    if _dist.is_active():
        return _dist.sharded_device_seg_sums(
            engine, lambda m, Ep, wp, ends, op: engine.gless_int_seg_dev(h, ind, m, Ep, wp, ends, op), _c128_segments(segs))
    return engine.gless_int_seg(h, ind, segs)


def GrLessInt(F, S, g, Elist, weights, ind=None):
    """Integrated lesser Green's function, N x N complex (integrate.py:177-208).
    ``ind`` is None (total Sigma) or a contact index (0, -1, ...)."""
    F = np.asarray(F)
    S = np.asarray(S)
    E, w = _as_grid(Elist, weights)
    _check(F, S, E, w)
    split = _blockwise(F, S, g, lambda Fb, Sb, gb: GrLessInt(Fb, Sb, gb, E, w, ind))
    if split is not None:
        return split
    engine = get_engine()
    engine.set_system(F, S)
    E = np.ascontiguousarray(E.ravel(), dtype=np.complex128)
    w = np.ascontiguousarray(w.ravel(), dtype=np.complex128)
    if _dist.is_active() and hasattr(g, "_negf_lower"):
        h = g._negf_lower(engine)
        return _dist.sharded_device_sum(
            engine, lambda m, Ep, wp, op: engine.gless_int_dev(h, ind, m, Ep, wp, op), E, w)
    return _dist.sharded_sum(lambda idx: _partial_gless(engine, g, E[idx], w[idx], ind), E.size)


_PROBES_REFUSED = ("floating probes need a self-energy object the engine lowers itself (surfGTest, surfG, surfGB or a "
                   "constant provider with _negf_lower); this one is evaluated on the host and has no contact orbital lists")


def _probes_integral(F, S, g, Elist, weights, again, host, dev):
    """What GrLessIntProbes and GrIntProbes share: GrLessInt's checks, the spin-diagonal split (the probes on the N
    orbitals of a block), and the energy sharding -- device resident when the ranks are active, else a host sum."""
    F = np.asarray(F)
    S = np.asarray(S)
    E, w = _as_grid(Elist, weights)
    _check(F, S, E, w)
    split = _blockwise(F, S, g, lambda Fb, Sb, gb: again(Fb, Sb, gb, E, w))
    if split is not None:
        return split
    if not hasattr(g, "_negf_lower"):
        raise NotImplementedError(_PROBES_REFUSED)
    engine = get_engine()
    engine.set_system(F, S)
    E = np.ascontiguousarray(E.ravel(), dtype=np.complex128)
    w = np.ascontiguousarray(w.ravel(), dtype=np.complex128)
    h = g._negf_lower(engine)
    if _dist.is_active() and getattr(engine, "device", None) is not None:
        return _dist.sharded_device_sum(engine, lambda m, Ep, wp, op: dev(engine, h, m, Ep, wp, op), E, w)
    zero = lambda: np.zeros((engine.n, engine.n), dtype=np.complex128)
    # (a host-only engine -- the stub of the sharding test -- takes the host sum under active ranks as well)
    return _dist.sharded_sum(lambda idx: host(engine, h, E[idx], w[idx]) if E[idx].size else zero(), E.size)


def GrLessIntProbes(F, S, g, Elist, weights, probes, ind=None):
    """Integrated lesser Green's function with floating dephasing probes, N x N complex: sum_k w_k G D_s G^H with
    D_s = Gamma_s + sum_p R_ps(E_k) Gamma_p and the ``probes`` (a list of (indices, block), see
    transport.dephasing_probes) in E S - F - Sigma (Engine.gless_int_probes).  ``ind`` as GrLessInt: None (all
    terminals) or a contact index.  The reference has no such function."""
    return _probes_integral(F, S, g, Elist, weights,
                            lambda Fb, Sb, gb, E, w: GrLessIntProbes(Fb, Sb, gb, E, w, probes, ind),
                            lambda eng, h, E, w: eng.gless_int_probes(h, ind, E, w, probes),
                            lambda eng, h, m, Ep, wp, op: eng.gless_int_probes_dev(h, ind, m, Ep, wp, op, probes))


def GrIntProbes(F, S, g, Elist, weights, probes):
    """Integrated retarded Green's function with the ``probes`` in E S - F - Sigma (Engine.gr_int_probes): what completes
    a density with decoherence next to GrLessIntProbes.  The probes do not depend on E: contour grids stay valid."""
    return _probes_integral(F, S, g, Elist, weights,
                            lambda Fb, Sb, gb, E, w: GrIntProbes(Fb, Sb, gb, E, w, probes),
                            lambda eng, h, E, w: eng.gr_int_probes(h, E, w, probes),
                            lambda eng, h, m, Ep, wp, op: eng.gr_int_probes_dev(h, m, Ep, wp, op, probes))


def GrBatch(F, S, g, Elist):
    """[M,N,N] stack of G^r(E_m) (not in the reference API; used by parity tests and
    by callers that need G(E) itself, _gr_matrix_ops integrate.py:67-71)."""
    F = np.asarray(F)
    S = np.asarray(S)
    E = np.ascontiguousarray(np.asarray(Elist).ravel(), dtype=np.complex128)
    engine = get_engine()
    engine.set_system(F, S)
    if hasattr(g, "_negf_lower"):
        return engine.gr_batch(g._negf_lower(engine), E)
    out = np.zeros((E.size, engine.n, engine.n), dtype=np.complex128)
    for a, b in _callback_chunks(engine.n, E.size, 1):
        sig = _sigma_tot_stack(g, E[a:b])
        h = engine.sigma_precomputed(sig)
        try:
            out[a:b] = engine.gr_batch(h, E[a:b])
        finally:
            engine.sigma_free(h)
    return out
