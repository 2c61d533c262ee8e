"""Cases and runners of the layered entry points whose results are held bit for bit against a record of an earlier build
(tests/golden/layered_parent.npz, written by scripts/gen_layered_parent_fixture.py, read by test_rgf_parent_gpu.py).

Every runner returns {key: array}: the outputs of the engine's calls with their `info`, on rgf_ref.cases() (a - d, const
terminals), rgf_ref.contour() and rgf_tmat_ref.cases() (a - d), with the batch automatic ("b0") and set to 3 ("b3").
  green      layered_transmission in both directions, layered_dos in both forms, layered_gr_int
  less       layered_gless_int and layered_contact_dos for every way of naming the terminals, also with a second terminal
             on layer 0 (the union list differs from either terminal's list)
  tmat       the transmission matrix with and without probes, and with all terminals on ONE layer (a single pass)
  kinds      case b with `blocks` terminals and with chain terminals under both solvers, the terminals' Sigma
  singular   one energy singular in layer 1: info and the outputs of gr_int, gless_int and the matrix
  workspace  layered_workspace_bytes after each kind of call on case b
  counts     launches per profile family of one call of each entry point (host and device-resident) on case d, and of
             the matrix on tmat case b -- a run of its own, with the profile switched on
"""
import hashlib
import warnings

import numpy as np

import rgf_ref as rr
import rgf_tmat_ref as tm
from helpers import chain_lead

BATCHES = (0, 3)
FAMILIES = ("rgf", "zgemm", "inverse", "gamma", "accumulate", "tmat", "trace")
GROUPS = ("green", "less", "tmat", "kinds", "singular", "workspace", "counts")
FULL_CASE = "a"                      # the record keeps this case's arrays in full, of the others the digests


def digest(x):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest(), np.uint8)


def kept_in_full(key, x):
    return np.issubdtype(np.asarray(x).dtype, np.integer) or f"/{FULL_CASE}/" in key


def _flat(blocks):
    return np.concatenate([np.asarray(b).ravel() for part in blocks for b in part])


def _weights(m):
    k = np.arange(m)
    return (0.3 + 0.1 * k) * np.exp(0.4j * k)


def _create(eng, c):
    return eng.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)


def _bind(eng, c):
    h = _create(eng, c)
    return h, eng.layered_terminal_const(h, 0, c.left, c.sig_left), eng.layered_terminal_const(h, len(c.sizes) - 1, c.right, c.sig_right)


def _bind_tm(eng, c):
    h = _create(eng, c.base)
    for lay, idx, blk in c.leads:
        eng.layered_terminal_const(h, lay, idx, blk)
    return h


def _batched(eng, fn):
    """fn(tag) under each batch setting"""
    try:
        for nb in BATCHES:
            eng.set_batch(nb)
            fn(f"b{nb}")
    finally:
        eng.set_batch(0)


def _green_calls(eng, h, tl, tr, E, Eg, w, out, pre):
    def put(name, *vals):
        for k, v in enumerate(vals):
            out[f"{pre}/{name}/{k}"] = np.asarray(v)
        out[f"{pre}/{name}/info"] = eng.last_info.copy()
    put("T_rl", eng.layered_transmission(h, tr, tl, E))
    put("T_lr", eng.layered_transmission(h, tl, tr, E))
    put("dos", *eng.layered_dos(h, E, mulliken=False))
    put("pdos", *eng.layered_dos(h, E, mulliken=True))
    put("gr_int", _flat(eng.layered_gr_int(h, Eg, w)))


def _less_calls(eng, h, inds, E, w, out, pre):
    for ind in inds:
        out[f"{pre}/gless_int/{ind}"] = _flat(eng.layered_gless_int(h, ind, E, w))
        out[f"{pre}/gless_int/{ind}/info"] = eng.last_info.copy()
        tot, site = eng.layered_contact_dos(h, ind, E)
        out[f"{pre}/contact_dos/{ind}/tot"], out[f"{pre}/contact_dos/{ind}/site"] = tot, site
        out[f"{pre}/contact_dos/{ind}/info"] = eng.last_info.copy()


def run_green(eng):
    out = {}
    cb, Ec, wc = rr.contour()
    for c in rr.cases():
        E = np.asarray(c.energies)
        Eg, w = (Ec, wc) if c is cb else (E, _weights(E.size))
        h, tl, tr = _bind(eng, c)
        try:
            _batched(eng, lambda tag: _green_calls(eng, h, tl, tr, E, Eg, w, out, f"green/{c.name}/{tag}"))
        finally:
            eng.layered_free(h)
    return out


def run_less(eng):
    out = {}
    for c in rr.cases():
        E = np.asarray(c.energies)
        h, tl, tr = _bind(eng, c)
        try:
            _batched(eng, lambda tag: _less_calls(eng, h, (tl, tr, -1, None), E, _weights(E.size), out, f"less/{c.name}/{tag}"))
        finally:
            eng.layered_free(h)
    c = tm.cases()[1]                              # left, right and a second terminal on layer 0 that shares an orbital
    E = np.asarray(c.base.energies)
    h = _bind_tm(eng, c)
    try:
        _batched(eng, lambda tag: _less_calls(eng, h, (0, 1, 2, -1, None), E, _weights(E.size), out, f"less/b-two-left/{tag}"))
    finally:
        eng.layered_free(h)
    return out


def single_layer_case():
    """(rgf_ref case a, its left terminal alone, two probes on layer 0): every terminal on one layer"""
    c = rr.cases()[0]
    probes = [(np.array([0, 2]), np.array([[-0.2j, 0.01], [0.01, -0.3j]])), (np.array([1]), np.array([[-0.15j]]))]
    return c, probes


def run_tmat(eng):
    out = {}

    def matrix(h, E, probes, pre):
        out[pre] = eng.layered_transmission_matrix(h, E, probes)
        out[pre + "/info"] = eng.last_info.copy()
    for c in tm.cases():
        E = np.asarray(c.energies)
        h = _bind_tm(eng, c)
        try:
            def both(tag):
                matrix(h, E, c.global_terms(c.probes), f"tmat/{c.name}/{tag}/probes")
                matrix(h, E, None, f"tmat/{c.name}/{tag}/bare")
            _batched(eng, both)
        finally:
            eng.layered_free(h)
    c, probes = single_layer_case()
    h = _create(eng, c)
    try:
        eng.layered_terminal_const(h, 0, c.left, c.sig_left)
        _batched(eng, lambda tag: matrix(h, np.asarray(c.energies), probes, f"tmat/a-one-layer/{tag}/probes"))
    finally:
        eng.layered_free(h)
    return out


def _kinds_calls(eng, h, ts, K, E, w, probes, out, pre):
    _green_calls(eng, h, ts[0], ts[1], E, E, w, out, pre)
    _less_calls(eng, h, (None,), E, w, out, pre)
    out[f"{pre}/tmat"] = eng.layered_transmission_matrix(h, E, probes)
    out[f"{pre}/tmat/info"] = eng.last_info.copy()
    for t, k in zip(ts, K):
        out[f"{pre}/sigma/{t}"] = eng.layered_terminal_sigma(h, t, E, k)


def run_kinds(eng):
    out = {}
    c = rr.cases()[1]
    last = len(c.sizes) - 1
    E = np.asarray(c.energies)
    w = _weights(E.size)
    probes = tm.cases()[1].global_terms(tm.cases()[1].probes)
    K = (c.left.size, c.right.size)
    scale = (1.0 + 0.1 * np.arange(E.size))[:, None, None]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        h = _create(eng, c)
        try:
            ts = (eng.layered_terminal_blocks(h, 0, c.left, scale * c.sig_left),
                  eng.layered_terminal_blocks(h, last, c.right, scale * c.sig_right))
            _batched(eng, lambda tag: _kinds_calls(eng, h, ts, K, E, w, probes, out, f"kinds/blocks/{tag}"))
        finally:
            eng.layered_free(h)
        eta, conv, rel = 1e-4, 1e-7, 0.1
        for solver in ("fixed-point", "doubling"):
            h = _create(eng, c)
            try:
                ts = []
                for layer, idx, seed in ((0, c.left, 41), (last, c.right, 42)):
                    a, Sa, b, Sb = chain_lead(idx.size, seed)
                    ts.append(eng.layered_terminal_chain(h, layer, idx, a, Sa, b, Sb, b, Sb, eta, conv, rel, solver=solver))
                _batched(eng, lambda tag: _kinds_calls(eng, h, ts, K, E, w, probes, out, f"kinds/chain-{solver}/{tag}"))
            finally:
                eng.layered_free(h)
    return out


def run_singular(eng):
    """layer 1 of case a decoupled with F_11 = 0, S_11 = 1: singular at E = 0"""
    out = {}
    c = rr.cases()[0]
    Fd = [c.F_diag[0], np.zeros_like(c.F_diag[1])]
    Sd = [c.S_diag[0], np.eye(c.sizes[1])]
    Fu = [np.zeros_like(c.F_up[0])]
    probes = [([1, 2], np.array([[-0.2j, 0.01], [0.01, -0.3j]])), ([3, 4], np.array([[-0.1j, 0.0], [0.0, -0.1j]]))]
    E = np.array([0.3, 0.0, -0.2])
    h = eng.layered_create(Fd, Fu, Sd, Fu)
    try:
        eng.layered_terminal_const(h, 0, c.left, c.sig_left)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out["singular/a/gr_int"] = _flat(eng.layered_gr_int(h, E, np.ones(3)))
            out["singular/a/gr_int/info"] = eng.last_info.copy()
            out["singular/a/gless_int"] = _flat(eng.layered_gless_int(h, None, E, np.ones(3)))
            out["singular/a/gless_int/info"] = eng.last_info.copy()
            out["singular/a/tmat"] = eng.layered_transmission_matrix(h, E, probes)
            out["singular/a/tmat/info"] = eng.last_info.copy()
    finally:
        eng.layered_free(h)
    assert out["singular/a/gr_int/info"][1] != 0 and np.all(np.isnan(out["singular/a/tmat"][1]))
    return out


def run_workspace(eng):
    c = tm.cases()[1]
    E = np.asarray(c.base.energies)
    w = _weights(E.size)
    h = _bind_tm(eng, c)
    calls = (("transmission", lambda: eng.layered_transmission(h, 1, 0, E)),
             ("dos", lambda: eng.layered_dos(h, E)),
             ("gr_int", lambda: eng.layered_gr_int(h, E, w)),
             ("gless_int", lambda: eng.layered_gless_int(h, None, E, w)),
             ("contact_dos", lambda: eng.layered_contact_dos(h, 0, E)),
             ("tmat", lambda: eng.layered_transmission_matrix(h, E, c.global_terms(c.probes))),
             ("tmat-bare", lambda: eng.layered_transmission_matrix(h, E)))
    work = []
    try:
        for _, fn in calls:
            fn()
            work.append(eng.layered_workspace_bytes(h))
    finally:
        eng.layered_free(h)
    return {"workspace/b": np.array(work, dtype=np.int64)}


def run_counts(eng):
    """[call, family] launches; the device-resident forms on buffers of the HIP runtime the library is linked against"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    c = rr.cases()[3]
    m, N = len(c.energies), c.N
    E = np.ascontiguousarray(c.energies, dtype=np.complex128)
    w = np.ascontiguousarray(_weights(m), dtype=np.complex128)
    h, tl, tr = _bind(eng, c)
    ct = tm.cases()[1]
    ht = _bind_tm(eng, ct)
    bufs = []

    def dev(nbytes, src=None):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        bufs.append(p)
        if src is not None:
            assert hip.hipMemcpy(p, src.ctypes.data_as(C.c_void_p), nbytes, 1) == 0      # host -> device
        return p.value
    counts = np.zeros((11, len(FAMILIES)), dtype=np.int64)
    try:
        dE, dw = dev(E.nbytes, E), dev(w.nbytes, w)
        tot, site, pat = dev(8 * m), dev(8 * m * N), dev(16 * eng.layered_pattern_size(h))
        calls = (lambda: eng.layered_transmission(h, tr, tl, E),
                 lambda: eng.layered_dos(h, E, mulliken=True),
                 lambda: eng.layered_gr_int(h, E, w),
                 lambda: eng.layered_gless_int(h, None, E, w),
                 lambda: eng.layered_contact_dos(h, tl, E),
                 lambda: eng.layered_transmission_dev(h, tr, tl, m, dE, tot),
                 lambda: eng.layered_dos_dev(h, m, dE, tot, site, mulliken=True),
                 lambda: eng.layered_gr_int_dev(h, m, dE, dw, pat),
                 lambda: eng.layered_gless_int_dev(h, None, m, dE, dw, pat),
                 lambda: eng.layered_contact_dos_dev(h, tl, m, dE, tot, site),
                 lambda: eng.layered_transmission_matrix(ht, np.asarray(ct.energies), ct.global_terms(ct.probes)))
        eng.profile(True)
        for k, fn in enumerate(calls):
            eng.profile_reset()
            fn()
            eng.sync()
            counts[k] = [eng.profile_read(f)[1] for f in FAMILIES]
    finally:
        eng.profile(False)
        eng.sync()
        eng.layered_free(h)
        eng.layered_free(ht)
        for p in bufs:
            hip.hipFree(p)
    return {"counts/d": counts}


RUNNERS = dict(green=run_green, less=run_less, tmat=run_tmat, kinds=run_kinds, singular=run_singular,
               workspace=run_workspace, counts=run_counts)
