"""
The binding of Engine to the library, held on the CPU: every public method of ``Engine`` that reaches libnegf_hip.so is
driven against a recording stand-in of the library, and the transcript -- the library calls with every argument, what
the method returned or raised, the warnings, the counters and the ``last_*`` attributes -- must equal the committed one,
tests/golden/engine_calls_parent.txt, line by line.  The stand-in checks every call against ``_lib.SIGNATURES`` the way
ctypes would (argument count, ``from_param`` of every argtype), so a wrapper that disagrees with the declared signature
fails here and not first on the GPU machine.

The committed transcript is written by this module run as a script (``python tests/test_engine_calls_host.py --write
FILE COMMIT``) in a checkout of COMMIT, the commit named in its first line, with only this file added; written twice
there, the two files are equal.  No library, no GPU.  One line per scenario: ``== method [label] rc=code``, the library
calls (``lib same``: those of the sweep's first scenario, argument for argument), ``ret`` or ``exc``, the warnings, what the
scenario added to the counters and what it set of ``last_info`` / ``last_iters`` / ``last_converged`` / the generation.

A wrapper for a new entry point gets one scenario in ``script()`` below.  Every line stands on its own (counters as what the
scenario added, ``last_*`` cleared before it, ``lib same`` inside one sweep only), so the transcript is then extended by the
lines of that scenario and no other line moves (``--write`` and compare).  (A further sweep of a library function that has
one already, put in front of it, takes the four codes over from it: the codes go with the first sweep that reaches a function.)
"""
import ctypes as C
import hashlib
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gaunegf_amd import _lib                                   # noqa: E402
from gaunegf_amd.engine import Engine                          # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_calls_parent.txt")

# names of SIGNATURES that no scenario has to reach: those of Engine's constructor and close(), of NegfError's text and of
# the module-level fingerprint(), and one that Engine has no method for
NOT_REACHED = {
    "negf_device_count", "negf_create", "negf_destroy", "negf_strerror", "negf_version", "negf_hash_bytes",
    "negf_set_system",        # superseded by negf_set_system_keyed (key 0 = compare the bytes); kept in the C API for C callers
}
# public names of Engine that make no library call (tables kept on the host side)
NO_LIBRARY = {"terminal_count", "layered_terminal_count", "layered_pattern_size", "layered_table_size"}

# number of trailing output arrays of the calls that fill host arrays (None arguments among them are skipped) ...
_TRAILING_OUT = {
    "negf_bethe_raw": 3, "negf_sigma_eval": 3, "negf_gr_int": 2, "negf_gr_int_seg": 2, "negf_gless_int_seg": 2,
    "negf_gr_int_refine": 4, "negf_gless_int": 2, "negf_gr_batch": 2, "negf_transmission": 3, "negf_dos": 3,
    "negf_eigvalsh_batched": 2, "negf_transmission_channels": 2, "negf_eigh_batched": 3, "negf_channel_states": 3,
    "negf_local_transmission": 2, "negf_bond_int": 2, "negf_population": 2, "negf_projected_dos": 2,
    "negf_transmission_matrix": 2, "negf_probe_response": 2, "negf_gless_int_probes": 2, "negf_gr_int_probes": 2,
    "negf_layered_terminal_sigma": 1, "negf_layered_transmission": 2, "negf_layered_dos": 3, "negf_layered_gr_int": 2,
    "negf_layered_gless_int": 2, "negf_layered_contact_dos": 3, "negf_layered_transmission_matrix": 2,
    "negf_layered_probe_response": 2, "negf_layered_gless_int_probes": 2, "negf_layered_gr_int_probes": 2,
    "negf_layered_local_transmission": 2, "negf_layered_bond_int": 2, "negf_last_info": 1, "negf_last_iters": 2,
}
# ... whose last one is not the per-energy info array
_NO_INFO = {"negf_bethe_raw", "negf_sigma_eval", "negf_layered_terminal_sigma", "negf_last_iters"}
# outputs that are not trailing: position among the arguments (the context is argument 0)
_OUT_AT = {"negf_zgemm_batched": (11,), "negf_zgemm_plan": (10,)}

_CARG = type(C.byref(C.c_int()))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:10]


def _arr(a):
    return f"<{a.dtype.str[1:]} {list(a.shape)} {_sha(a)}>"


def _pattern(a, k):
    """a fixed non-trivial content for output array ``a``, different per argument position k"""
    i = np.arange(a.size)
    v = ((i * 7 + k * 3) % 11 - 3) * 0.25
    if a.dtype.kind == "c":
        v = v + 1j * (((i * 5 + k) % 7 - 2) * 0.5)
    return v.astype(a.dtype).reshape(a.shape)


def describe(v):
    """what a method returned: arrays by dtype (c16, f8, i4), shape and sha256 (its first 10 digits), containers element by element"""
    if isinstance(v, np.ndarray):
        return _arr(v)
    if isinstance(v, (tuple, list)):
        o, c = "()" if isinstance(v, tuple) else "[]"
        return o + ", ".join(describe(x) for x in v) + c
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {describe(x)}" for k, x in sorted(v.items())) + "}"
    if isinstance(v, (bool, np.bool_)):
        return str(bool(v))
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    return repr(v)


class Recorder:
    """Stand-in of the loaded library: any name of SIGNATURES is a callable that checks the call like ctypes, records
    it, fills the outputs and returns the code chosen for it."""

    def __init__(self):
        self.lines = []
        self.called = set()
        self.ctx = C.c_void_p(0xC0FFEE)
        self.reset()

    def reset(self):
        self.rc = {}             # name -> return code (others: rc_all)
        self.rc_all = 0
        self.info = None         # what the info array of a host form receives (cyclically), None: zeros
        self.byref = []          # values of the next byref outputs, in order (then the defaults)
        self.nan_row = None      # row of the first output array to fill with NaN

    def negf_strerror(self, code):
        return f"error {code}".encode()

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        res, argtypes = _lib.SIGNATURES[name]
        if len(args) != len(argtypes):
            raise TypeError(f"{name}: {len(args)} arguments, the signature has {len(argtypes)}")
        for a, t in zip(args, argtypes):
            t.from_param(a)                                    # ctypes.ArgumentError / TypeError as under ctypes
        out_at = _OUT_AT.get(name, tuple(range(len(args) - _TRAILING_OUT.get(name, 0), len(args))))
        info_at = len(args) - 1 if name in _TRAILING_OUT and name not in _NO_INFO else -1
        said, first = [], True
        for k, a in enumerate(args):
            arr = getattr(a, "_arr", None)
            if a is None:
                said.append("NULL")
            elif arr is not None:                              # a pointer made by ndarray.ctypes.data_as keeps its array
                # (an output is overwritten: what it held before -- zeros, or np.empty's leftovers -- is not part of the call)
                said.append(f"<{arr.dtype.str[1:]} {list(arr.shape)} out>" if k in out_at else _arr(arr))
                if k in out_at:
                    if k == info_at:
                        arr[...] = 0 if self.info is None else np.resize(np.asarray(self.info, dtype=arr.dtype), arr.shape)
                    else:
                        arr[...] = _pattern(arr, k)
                        if first and self.nan_row is not None and arr.size:
                            arr.reshape(arr.shape[0], -1)[self.nan_row] = np.nan
                        first = False
            elif isinstance(a, _CARG):
                obj = a._obj
                said.append(f"byref({type(obj).__name__})")
                default = {C.c_int: 2, C.c_longlong: 1000 + k, C.c_double: 0.5 + k, C.c_void_p: 0xABC}[type(obj)]
                obj.value = self.byref.pop(0) if self.byref else default
            elif isinstance(a, C.Array):
                said.append(f"{type(a).__name__}")
                for j in range(len(a)):
                    a[j] = (j * 3 + k) % 5 + 1
            elif isinstance(a, C.c_void_p):
                said.append("ctx" if a is self.ctx else f"ptr({a.value})")
            elif isinstance(a, C._SimpleCData):
                said.append(f"{type(a).__name__}({a.value!r})")
            elif isinstance(a, (bool, int)):
                said.append(str(int(a)))                       # (int(handle) and handle are the same value)
            else:
                said.append(repr(a))
        self.lines.append(f"lib {name}({', '.join(said)})")
        self.called.add(name)
        return self.rc.get(name, self.rc_all)


# --------------------------------------------------------------------------- #
# inputs: exactly representable, so that their bytes are the same everywhere
# --------------------------------------------------------------------------- #
def cm(shape, k=1):
    i = np.arange(int(np.prod(shape)))
    return (((i * (2 * k + 1)) % 17 - 8) / 4 + 1j * ((i * (k + 3)) % 13 - 6) / 8).reshape(shape)


def rm(shape, k=1):
    return cm(shape, k).real.copy()


N = 6
E3 = np.array([0.5 + 0.125j, -0.25 + 0.125j, 1.0 + 0.125j])
W3 = np.array([0.25 + 0.5j, 0.5 - 0.25j, 0.125 + 0j])
E0 = np.zeros(0, dtype=complex)
EINVAL, ESING, EHIP = _lib.NEGF_EINVAL, _lib.NEGF_ESINGULAR, _lib.NEGF_EHIP
P1 = [([1, 3], cm((2, 2), 4))]
P2 = [([0, 2], cm((2, 2), 5)), ([5], cm((1, 1), 6))]
SIZES = (2, 3, 2)


class Run:
    def __init__(self):
        self.lib = Recorder()
        eng = self.eng = object.__new__(Engine)
        eng._lib, eng._ctx, eng.n = self.lib, self.lib.ctx, N
        eng.counters = {"calls": 0, "points": 0}
        eng.last_info = eng.last_iters = eng.last_converged = None
        self.exercised, self.reaching, self.swept = set(), set(), set()

    def one(self, label, method, *args, rc=0, rcs=None, info=None, byref=(), nan_row=None, same=None, **kw):
        """One scenario: call Engine.<method>(*args, **kw) with the stand-in prepared as asked and record everything in one
        line that stands on its own -- the counters as what the scenario added, ``last_*`` as what it set (they are cleared
        first).  ``same``: the library calls of the scenario in front of it in a sweep; equal ones are written "lib same"."""
        lib, eng = self.lib, self.eng
        lib.reset()
        lib.rc_all, lib.rc, lib.info, lib.byref, lib.nan_row = rc, dict(rcs or {}), info, list(byref), nan_row
        head, before = f"== {method} [{label}] rc={rc}", len(lib.lines)
        self.exercised.add(method)
        eng.last_info = eng.last_iters = eng.last_converged = None
        c0, p0, g0 = eng.counters["calls"], eng.counters["points"], getattr(eng, "generation", 0)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                end = ["ret " + describe(getattr(eng, method)(*args, **kw))]
            except Exception as e:                             # the type and the full text are the record
                end = [f"exc {type(e).__name__}: {e}"]
        calls = lib.lines[before:]
        del lib.lines[before:]
        if calls:
            self.reaching.add(method)
        end += [f"warn {wn.category.__name__}: {wn.message}" for wn in caught]
        state = f"calls+{eng.counters['calls'] - c0} points+{eng.counters['points'] - p0}"
        for k, v in (("info", eng.last_info), ("iters", eng.last_iters), ("conv", eng.last_converged)):
            if v is not None:
                state += f" {k}={describe(v)}"
        if getattr(eng, "generation", 0) != g0:
            state += f" generation+{eng.generation - g0}"
        lib.lines.append(" | ".join([head] + (["lib same"] if calls and calls == same else calls) + end + [state]))
        return calls

    def sweep(self, label, method, *args, ok=(), sing_info=(0, 3, 1), **kw):
        """the scenario with every kind of return code: 0, NEGF_EINVAL, NEGF_ESINGULAR with a non-zero info, NEGF_EHIP,
        the first time it reaches a library function (its variants after that run with code 0);
        ``ok``: library functions that keep returning 0 (the count call in front of a channel call)"""
        rcs = {name: 0 for name in ok}
        calls = self.one(label, method, *args, rcs=rcs, **kw)
        reached = {line.split("(")[0].split()[1] for line in calls} - set(ok)
        if reached <= self.swept:                              # (a variant of a call whose codes were all seen: code 0 will do)
            return
        self.swept |= reached
        self.one(label, method, *args, rc=EINVAL, rcs=rcs, same=calls, **kw)
        self.one(label, method, *args, rc=ESING, rcs=rcs, info=sing_info, same=calls, **kw)
        self.one(label, method, *args, rc=EHIP, rcs=rcs, same=calls, **kw)


def script(r):
    one, sweep, eng = r.one, r.sweep, r.eng
    H, LH = 2, 5                                               # the dense provider's and the layered system's handles

    # ---- context settings
    sweep("stream", "set_stream", 0x7000)
    one("default", "set_stream", None)
    sweep("", "set_batch", 8)
    one("", "get_batch", rc=16)
    sweep("", "set_inverse_algo", 1)
    sweep("", "set_small_algo", 1)
    sweep("defaults", "set_chain_round_robin")
    one("given", "set_chain_round_robin", 4, slots=2)
    sweep("", "set_gamma_algo", 1)
    sweep("", "sync")
    one("nothing", "set_chain_cache")
    sweep("grids", "set_chain_cache", 16)
    sweep("bytes", "set_chain_cache", max_bytes=1 << 33)
    one("both", "set_chain_cache", 0, 1 << 20)
    sweep("", "chain_cache_clear")
    sweep("", "chain_cache_stats", byref=[5, 6, 7, 8])
    sweep("", "workspace_bytes")

    # ---- system
    big_F, big_S = rm((128, 128), 1), rm((128, 128), 2)        # large enough for the keyed conversion cache
    one("real large: keyed", "set_system", big_F, big_S)
    one("same arrays: same key", "set_system", big_F, big_S)
    one("complex: passed through", "set_system", cm((N, N), 1), cm((N, N), 2))
    sweep("real small", "set_system", rm((N, N), 1), rm((N, N), 2))
    one("shapes differ", "set_system", rm((N, N), 1), rm((5, 5), 2))
    one("not square", "set_system", rm((N, 5), 1), rm((N, 5), 2))

    # ---- providers
    sweep("two contacts", "sigma_const", [cm((N, N), 1), cm((N, N), 2)], byref=[H])
    one("wrong shape", "sigma_const", [cm((5, 5), 1)])
    il = [[0, 1], [4, 5]]
    mats = [[cm((2, 2), k), cm((2, 2), k + 1)] for k in range(1, 7)]
    sweep("fixed-point", "sigma_chain1d", il, *mats, 1e-4, 1e-6, 0.5, byref=[3])
    sweep("doubling", "sigma_chain1d", il, *mats, 1e-4, 1e-6, 0.5, max_iter=50, force_iters=3, solver='doubling',
          tol=1e-9, max_steps=40, byref=[3])
    one("bad solver", "sigma_chain1d", il, *mats, 1e-4, 1e-6, 0.5, solver='newton')
    one("bad block", "sigma_chain1d", il, [cm((2, 2), 1), cm((3, 3), 2)], *mats[1:], 1e-4, 1e-6, 0.5)
    orbs = [[list(range(9))], [list(range(9, 18)), list(range(18, 27))]]
    nbs = [[[0, 1, 2]], [[3], []]]
    H9, S12, V12 = [rm((9, 9), 1), rm((9, 9), 2)], [rm((12, 9, 9), 3), rm((12, 9, 9), 4)], [rm((12, 9, 9), 5), rm((12, 9, 9), 6)]
    sweep("xi", "sigma_bethe", orbs, nbs, H9, S12, V12, cm((N, N), 7), 1e-4, 1e-6, byref=[4])
    one("no xi, no neighbours", "sigma_bethe", [[list(range(9))]], [[[]]], H9[:1], S12[:1], V12[:1], None, 1e-4, 1e-6,
        mix=0.25, max_iter=10, force_iters=2, byref=[4])
    one("bad xi", "sigma_bethe", orbs, nbs, H9, S12, V12, cm((5, 5), 7), 1e-4, 1e-6)
    sweep("sigmaK", "bethe_raw", H9[0], list(S12[0]), list(V12[0]), 1e-4, 1e-6, E3, 1)
    one("sigma", "bethe_raw", H9[0], list(S12[0]), list(V12[0]), 1e-4, 1e-6, E3, 2, mix=0.25, max_iter=7, force_iters=1)
    one("m = 0", "bethe_raw", H9[0], list(S12[0]), list(V12[0]), 1e-4, 1e-6, E0, 1)
    sweep("total only", "sigma_precomputed", cm((3, N, N), 1), byref=[6])
    one("one contact", "sigma_precomputed", cm((3, N, N), 1), cm((3, N, N), 2), byref=[6])
    one("two contacts", "sigma_precomputed", cm((3, N, N), 1), cm((3, 2, N, N), 2), byref=[7])
    one("gammas", "sigma_precomputed", cm((3, N, N), 1), gammas=cm((3, 2, N, N), 3), byref=[8])
    one("wrong shape", "sigma_precomputed", cm((3, 5, 5), 1))
    sweep("", "sigma_eval", H, 1, E3, 2)
    one("total, m = 0", "sigma_eval", H, None, E0)

    # ---- hot path, host forms
    sweep("", "gr_int", H, E3, W3)
    one("m = 0", "gr_int", H, E0, E0)
    one("lengths differ", "gr_int", H, E3, W3[:2])
    segs = [(E3[:1], W3[:1]), (E3[1:], W3[1:])]
    sweep("", "gr_int_seg", H, segs)
    one("no segments", "gr_int_seg", H, [])
    for ind in (None, 0, -1):
        sweep(f"ind={ind}", "gless_int_seg", H, ind, segs)
        sweep(f"ind={ind}", "gless_int", H, ind, E3, W3)
    one("m = 0", "gless_int", H, 0, E0, E0)
    one("no segments", "gless_int_seg", H, 0, [])
    one("ind is no number", "gless_int", H, 'x', E3, W3)
    req = [(E3, W3, [1, 2], [None, 0.5], None), (E3[:2], W3[:2], [2], [0.25], cm((N, N), 9))]
    sweep("fresh + continued", "gr_int_refine", H, req, 1e-6)
    one("fresh only", "gr_int_refine", H, req[:1], 1e-6)
    one("levels do not add up", "gr_int_refine", H, [(E3, W3, [1, 1], [None, 0.5], None)], 1e-6)
    one("ratio missing", "gr_int_refine", H, [(E3, W3, [1, 2], [None, None], None)], 1e-6)
    sweep("", "gr_batch", H, E3)
    one("m = 0", "gr_batch", H, E0)
    for sb in (False, True):
        sweep(f"spin_block={sb}", "transmission", H, 0, 1, E3, spin_block=sb)
        sweep(f"per_site={sb}", "dos", H, E3, per_site=sb)
    one("m = 0", "transmission", H, 0, 1, E0, True)
    one("m = 0", "dos", H, E0)

    # ---- eigensolvers and eigenchannels
    for f in ("eigvalsh", "eigh"):
        sweep("batch", f, cm((3, 2, 2), 2))
        sweep("single", f, cm((2, 2), 2), sing_info=(2,))
        one("m = 0", f, cm((0, 2, 2), 2))
        one("not square", f, cm((3, 2, 3), 2))
        one("one dimension", f, cm((4,), 2))
        one("K too large", f, np.zeros((1, 97, 97)))
    sweep("", "channel_count", H, 0, 1, byref=[3])
    sweep("", "channel_states_count", H, 0, byref=[3])
    both = (2, -2, -1)
    for f, cnt in (("transmission_channels", "negf_channel_count"), ("channel_states", "negf_channel_states_count")):
        sweep("nchan from the count", f, H, 0, 1, E3, ok=(cnt,), sing_info=both, byref=[2])
        sweep("nchan given", f, H, 0, 1, E3, 1, ok=(cnt,), sing_info=both)
        one("info negative only", f, H, 0, 1, E3, info=(0, -2, -7))
        one("info positive only", f, H, 0, 1, E3, info=(0, 4, 0))
        one("the count refuses", f, H, 0, 1, E3, rcs={cnt: EINVAL})
        one("the count fails", f, H, 0, 1, E3, rcs={cnt: EHIP})
        one("nchan = 0", f, H, 0, 1, E3, 0)
        one("m = 0", f, H, 0, 1, E0, 2)
    sweep("", "transmission_channels_dev", H, 0, 1, 3, 0x1000, 2, 0x2000)
    sweep("", "channel_states_dev", H, 0, 1, 3, 0x1000, 2, 0x2000, 0x3000)

    # ---- bond currents, populations, projected DOS
    G3 = [0, 0, 1, 1, 2, 2]
    for ind in (None, 0, -1):
        sweep(f"ind={ind}", "local_transmission", H, ind, E3)
    sweep("groups", "local_transmission", H, 0, E3, G3)
    one("groups, n_groups", "local_transmission", H, 0, E3, np.array(G3), 4)
    one("n_groups = n", "local_transmission", H, 0, E3, None, N)
    one("m = 0", "local_transmission", H, 0, E0, G3)
    one("n_groups without groups", "local_transmission", H, 0, E3, None, 3)
    one("groups: wrong length", "local_transmission", H, 0, E3, [0, 1])
    one("groups: not integers", "local_transmission", H, 0, E3, [0.0] * N)
    one("groups: out of range", "local_transmission", H, 0, E3, G3, 2)
    one("groups: negative", "local_transmission", H, 0, E3, [-1, 0, 0, 0, 0, 0])
    sweep("", "local_transmission_dev", H, None, 3, 0x1000, None, 0x2000)
    sweep("groups", "local_transmission_dev", H, 1, 3, 0x1000, G3, 0x2000, n_groups=3)
    one("groups: wrong length", "local_transmission_dev", H, 1, 3, 0x1000, [0], 0x2000)
    Wr = np.array([0.25, 0.5, 0.125])
    sweep("real weights", "bond_int", H, 0, E3, Wr)
    sweep("complex weights, zero imaginary part", "bond_int", H, None, E3, Wr + 0j)
    one("complex weights", "bond_int", H, 0, E3, W3)
    one("lengths differ", "bond_int", H, 0, E3, Wr[:2])
    one("m = 0", "bond_int", H, -1, E0, np.zeros(0))
    sweep("", "bond_int_dev", H, 0, 3, 0x1000, 0x2000, 0x3000)
    one("total", "bond_int_dev", H, None, 3, 0x1000, 0x2000, 0x3000)
    for ind in (None, 0, -1, Engine.RETARDED, 'retarded'):
        sweep(f"ind={ind}", "population", H, ind, E3)
        one(f"ind={ind}", "population_dev", H, ind, 3, 0x1000, 0x2000)
        one(f"ind={ind}", "projected_dos", H, ind, E3, cm((2, N), 3))
        one(f"ind={ind}", "projected_dos_dev", H, ind, 3, 0x1000, 2, 0x2000, 0x3000)
    for rows in (False, True):
        sweep(f"F, groups, rows={rows}", "population", H, 0, E3, 'F', G3, None, rows)
        sweep(f"op 1, groups, rows={rows}", "population_dev", H, 0, 3, 0x1000, 0x2000, 1, G3, 3, rows)
    one("m = 0", "population", H, 0, E0, rows=True)
    one("bad op", "population", H, 0, E3, 'X')
    one("bad op before bad groups", "population", H, 0, E3, 2, [0])
    one("bad groups", "population", H, 0, E3, 'S', [0])
    one("bad op", "population_dev", H, 0, 3, 0x1000, 0x2000, None)
    one("bad groups", "population_dev", H, 0, 3, 0x1000, 0x2000, 'S', [0])
    sweep("", "projected_dos", H, 0, E3, cm((2, N), 3))
    one("one vector", "projected_dos", H, 0, E3, cm((N,), 3))
    one("m = 0", "projected_dos", H, 0, E0, cm((2, N), 3))
    one("wrong n", "projected_dos", H, 0, E3, cm((2, 5), 3))
    sweep("", "projected_dos_dev", H, 0, 3, 0x1000, 2, 0x2000, 0x3000)

    # ---- transmission matrix, floating probes
    one("", "terminal_count", H)
    one("probes", "terminal_count", H, P2)
    one("unknown handle", "terminal_count", 77)
    bad_probes = [("empty list", [([], cm((0, 0)))]), ("not integers", [([0.5], cm((1, 1)))]),
                  ("out of range", [([N], cm((1, 1)))]), ("repeated", [([1, 1], cm((2, 2)))]),
                  ("wrong block", P1 + [([0, 2], cm((3, 3)))])]
    for pr, name in ((None, "none"), (P1, "one"), (P2, "two")):
        sweep(f"probes: {name}", "transmission_matrix", H, E3, pr)
        sweep(f"probes: {name}", "transmission_matrix_dev", H, 3, 0x1000, 0x2000, pr)
        sweep(f"probes: {name}", "probe_response", H, E3, pr)
        sweep(f"probes: {name}", "probe_response_dev", H, 3, 0x1000, 0x2000, pr)
        sweep(f"probes: {name}", "gr_int_probes", H, E3, W3, pr)
        sweep(f"probes: {name}", "gr_int_probes_dev", H, 3, 0x1000, 0x2000, 0x3000, pr)
        for ind in (None, 0, -1) if pr is P1 else (0,):
            sweep(f"ind={ind}, probes: {name}", "gless_int_probes", H, ind, E3, W3, pr)
            sweep(f"ind={ind}, probes: {name}", "gless_int_probes_dev", H, ind, 3, 0x1000, 0x2000, 0x3000, pr)
    one("m = 0", "transmission_matrix", H, E0, P1)
    one("m = 0", "probe_response", H, E0, P1)
    one("m = 0", "gr_int_probes", H, E0, E0, P1)
    one("m = 0", "gless_int_probes", H, 0, E0, E0, P1)
    one("unknown handle", "transmission_matrix", 77, E3, P1)
    one("unknown handle", "probe_response", 77, E3, P1)
    one("unknown handle", "gless_int_probes", 77, 0, E3, W3, P1)
    one("unknown handle", "gless_int_probes_dev", 77, 0, 3, 0x1000, 0x2000, 0x3000, P1)
    one("lengths differ", "gr_int_probes", H, E3, W3[:2], P1)
    one("lengths differ", "gless_int_probes", H, 0, E3, W3[:2], P1)
    one("a lost probe", "probe_response", H, E3, P2, nan_row=1)
    one("a lost probe at a singular energy", "probe_response", H, E3, P2, nan_row=1, rc=ESING, info=(0, 3, 0))
    one("NaN without probes", "probe_response", H, E3, None, nan_row=1)
    for ind in (2, -3):
        one(f"contact {ind} out of range", "gless_int_probes", H, ind, E3, W3, P1)
        one(f"contact {ind} out of range", "gless_int_probes_dev", H, ind, 3, 0x1000, 0x2000, 0x3000, P1)
    for label, pr in bad_probes:
        one(f"probes: {label}", "transmission_matrix", H, E3, pr)
    f_probes = [("transmission_matrix_dev", (H, 3, 0x1000, 0x2000)), ("probe_response", (H, E3)),
                ("probe_response_dev", (H, 3, 0x1000, 0x2000)), ("gr_int_probes", (H, E3, W3)),
                ("gr_int_probes_dev", (H, 3, 0x1000, 0x2000, 0x3000)), ("gless_int_probes", (H, 0, E3, W3)),
                ("gless_int_probes_dev", (H, 0, 3, 0x1000, 0x2000, 0x3000))]
    for f, a in f_probes:
        one("probes: out of range", f, *a, bad_probes[2][1])

    # ---- layered devices
    Fd, Sd = [cm((s, s), 1 + i) for i, s in enumerate(SIZES)], [cm((s, s), 4 + i) for i, s in enumerate(SIZES)]
    Fu = [cm((a, b), 7 + i) for i, (a, b) in enumerate(zip(SIZES[:-1], SIZES[1:]))]
    Su = [cm((a, b), 9 + i) for i, (a, b) in enumerate(zip(SIZES[:-1], SIZES[1:]))]
    one("no system yet", "layered_pattern_size", LH)
    one("no system yet", "layered_gr_int", LH, E3, W3)
    one("refused", "layered_create", Fd, Fu, Sd, Su, rc=EINVAL, byref=[LH])
    one("fails", "layered_create", Fd, Fu, Sd, Su, rc=EHIP, byref=[LH])
    one("", "layered_create", Fd, Fu, Sd, Su, byref=[LH])
    one("a second one", "layered_create", Fd[:2], Fu[:1], Sd[:2], Su[:1], rc=ESING, byref=[LH + 1])
    one("one layer", "layered_create", Fd[:1], [], Sd[:1], [])
    one("block counts", "layered_create", Fd, Fu[:1], Sd, Su)
    one("diagonal block", "layered_create", Fd, Fu, [Sd[0], cm((2, 2)), Sd[2]], Su)
    one("upper block", "layered_create", Fd, [Fu[1], Fu[0]], Sd, Su)
    one("", "layered_pattern_size", LH)
    one("", "layered_table_size", (1, 2, 1))
    one("", "layered_terminal_count", LH)
    sweep("", "layered_terminal_const", LH, 0, [0, 1], cm((2, 2), 3), byref=[0])
    one("wrong block", "layered_terminal_const", LH, 0, [0, 1], cm((3, 3), 3))
    one("after one terminal", "layered_terminal_count", LH, P2)
    lm = [cm((2, 2), k) for k in range(1, 7)]
    sweep("fixed-point", "layered_terminal_chain", LH, 2, [0, 1], *lm, 1e-4, byref=[1])
    sweep("doubling", "layered_terminal_chain", LH, 2, [0, 1], *lm, 1e-4, 1e-6, 0.5, 50, 3, 'doubling', 1e-9, 40, byref=[1])
    one("bad solver", "layered_terminal_chain", LH, 2, [0, 1], *lm, 1e-4, solver='newton')
    one("wrong block", "layered_terminal_chain", LH, 2, [0, 1], cm((3, 3)), *lm[1:], 1e-4)
    sweep("", "layered_terminal_blocks", LH, 2, [1], cm((3, 1, 1), 2), byref=[2])
    one("wrong shape", "layered_terminal_blocks", LH, 2, [1], cm((3, 2, 2), 2))
    one("no energies", "layered_terminal_blocks", LH, 2, [1], cm((0, 1, 1), 2))
    one("after three terminals", "layered_terminal_count", LH)
    one("unknown handle", "layered_terminal_count", 77)
    sweep("", "layered_terminal_sigma", LH, 0, E3, 2)
    one("m = 0", "layered_terminal_sigma", LH, 0, E0, 2)
    sweep("", "layered_transmission", LH, 0, 1, E3)
    sweep("", "layered_transmission_dev", LH, 0, 1, 3, 0x1000, 0x2000)
    for flag in (False, True):
        sweep(f"mulliken={flag}, per_site={not flag}", "layered_dos", LH, E3, flag, not flag)
        sweep(f"mulliken={flag}", "layered_dos_dev", LH, 3, 0x1000, 0x2000, 0x3000, flag)
        sweep(f"per_site={flag}", "layered_contact_dos", LH, 0, E3, flag)
    one("all terminals", "layered_contact_dos", LH, None, E3)
    sweep("", "layered_contact_dos_dev", LH, None, 3, 0x1000, 0x2000, 0x3000)
    sweep("", "layered_gr_int", LH, E3, W3)
    sweep("", "layered_gr_int_dev", LH, 3, 0x1000, 0x2000, 0x3000)
    for ind in (None, 0, -1):
        sweep(f"ind={ind}", "layered_gless_int", LH, ind, E3, W3)
        sweep(f"ind={ind}", "layered_gless_int_dev", LH, ind, 3, 0x1000, 0x2000, 0x3000)
        sweep(f"ind={ind}", "layered_local_transmission", LH, ind, E3)
        sweep(f"ind={ind}", "layered_bond_int", LH, ind, E3, Wr)
    gpl, gof = [1, 2, 1], [0, 0, 0, 1, 1, 0, 0]
    sweep("groups", "layered_local_transmission", LH, 0, E3, gpl, gof)
    one("groups_per_layer alone", "layered_local_transmission", LH, 0, E3, gpl)
    one("group_of alone", "layered_local_transmission", LH, 0, E3, None, gof)
    one("groups_per_layer: wrong length", "layered_local_transmission", LH, 0, E3, [1, 2], gof)
    one("group_of: wrong length", "layered_local_transmission", LH, 0, E3, gpl, gof[:5])
    sweep("", "layered_local_transmission_dev", LH, None, 3, 0x1000, 0x2000)
    sweep("groups", "layered_local_transmission_dev", LH, 0, 3, 0x1000, 0x2000, gpl, gof)
    one("group_of: wrong length", "layered_local_transmission_dev", LH, 0, 3, 0x1000, 0x2000, gpl, gof[:5])
    sweep("complex weights, zero imaginary part", "layered_bond_int", LH, 0, E3, Wr + 0j)
    one("complex weights", "layered_bond_int", LH, 0, E3, W3)
    one("lengths differ", "layered_bond_int", LH, 0, E3, Wr[:2])
    sweep("", "layered_bond_int_dev", LH, 0, 3, 0x1000, 0x2000, 0x3000)
    LP1, LP2 = [([2, 4], cm((2, 2), 4))], [([0, 1], cm((2, 2), 5)), ([6], cm((1, 1), 6))]
    for pr, name in ((None, "none"), (LP1, "one"), (LP2, "two")):
        sweep(f"probes: {name}", "layered_transmission_matrix", LH, E3, pr)
        sweep(f"probes: {name}", "layered_transmission_matrix_dev", LH, 3, 0x1000, 0x2000, pr)
        sweep(f"probes: {name}", "layered_probe_response", LH, E3, pr)
        sweep(f"probes: {name}", "layered_probe_response_dev", LH, 3, 0x1000, 0x2000, pr)
        sweep(f"probes: {name}", "layered_gr_int_probes", LH, E3, W3, pr)
        sweep(f"probes: {name}", "layered_gr_int_probes_dev", LH, 3, 0x1000, 0x2000, 0x3000, pr)
        for ind in (None, 0, -1) if pr is LP1 else (0,):
            sweep(f"ind={ind}, probes: {name}", "layered_gless_int_probes", LH, ind, E3, W3, pr)
            sweep(f"ind={ind}, probes: {name}", "layered_gless_int_probes_dev", LH, ind, 3, 0x1000, 0x2000, 0x3000, pr)
    one("a lost probe", "layered_probe_response", LH, E3, LP2, nan_row=2)
    one("a lost probe at a singular energy", "layered_probe_response", LH, E3, LP2, nan_row=2, rc=ESING, info=(0, 0, 5))
    one("NaN without probes", "layered_probe_response", LH, E3, None, nan_row=0)
    one("no terminals", "layered_probe_response", LH + 1, E3, [([0], cm((1, 1)))], nan_row=0)
    lf_probes = [("layered_transmission_matrix", (LH, E3)), ("layered_transmission_matrix_dev", (LH, 3, 0x1000, 0x2000)),
                 ("layered_probe_response", (LH, E3)), ("layered_probe_response_dev", (LH, 3, 0x1000, 0x2000)),
                 ("layered_gr_int_probes", (LH, E3, W3)), ("layered_gr_int_probes_dev", (LH, 3, 0x1000, 0x2000, 0x3000)),
                 ("layered_gless_int_probes", (LH, 0, E3, W3)),
                 ("layered_gless_int_probes_dev", (LH, 0, 3, 0x1000, 0x2000, 0x3000))]
    for f, a in lf_probes:
        one("probes: past the system", f, *a, [([7], cm((1, 1)))])
        one("unknown handle", f, 77, *a[1:], LP1)
    one("m = 0", "layered_transmission_matrix", LH, E0, LP1)
    one("m = 0", "layered_probe_response", LH, E0, LP1)
    one("m = 0", "layered_gr_int_probes", LH, E0, E0, LP1)
    one("m = 0", "layered_gless_int_probes", LH, 0, E0, E0, LP1)
    one("m = 0", "layered_gr_int", LH, E0, E0)
    one("m = 0", "layered_dos", LH, E0)
    one("m = 0", "layered_local_transmission", LH, 0, E0, gpl, gof)
    one("lengths differ", "layered_gr_int", LH, E3, W3[:2])
    for f, a in (("layered_transmission", (0, 1, E3)), ("layered_dos", (E3,)), ("layered_contact_dos", (0, E3)),
                 ("layered_gless_int", (0, E3, W3)), ("layered_local_transmission", (0, E3)),
                 ("layered_local_transmission_dev", (0, 3, 0x1000, 0x2000)), ("layered_bond_int", (0, E3, Wr)),
                 ("layered_workspace_bytes", ())):
        one("unknown handle", f, 77, *a)
    sweep("", "layered_workspace_bytes", LH)

    # ---- device-resident forms of the dense hot path, what the last call left behind
    sweep("", "gr_int_dev", H, 3, 0x1000, 0x2000, 0x3000)
    one("m = 0", "gr_int_dev", H, 0, 0x1000, 0x2000, 0x3000)
    # what a device form cannot coerce is found after the call was counted
    one("an address is no number", "gr_int_dev", H, 3, 'x', 0x2000, 0x3000)
    one("ind is no number", "gless_int_dev", H, 'x', 3, 0x1000, 0x2000, 0x3000)
    one("ind is no number", "population_dev", H, 'foo', 3, 0x1000, 0x2000)
    one("ind is no number", "layered_gless_int_probes_dev", LH, 'x', 3, 0x1000, 0x2000, 0x3000, None)
    one("m is no number", "gr_int_dev", H, None, 0x1000, 0x2000, 0x3000)
    for ind in (None, 0, -1):
        sweep(f"ind={ind}", "gless_int_dev", H, ind, 3, 0x1000, 0x2000, 0x3000)
        sweep(f"ind={ind}", "gless_int_seg_dev", H, ind, 3, 0x1000, 0x2000, [1, 3], 0x3000)
    sweep("", "gr_int_seg_dev", H, 3, 0x1000, 0x2000, np.array([1, 3]), 0x3000)
    sweep("restricted", "transmission_dev", H, 0, 1, 3, 0x1000, 0x2000)
    sweep("spin blocks", "transmission_dev", H, 0, 1, 3, 0x1000, 0x2000, 0x3000, True)
    one("Tspin_ptr None", "transmission_dev", H, 0, 1, 3, 0x1000, 0x2000, None)
    sweep("", "last_info_dev", 3)
    one("m = 0", "last_info_dev", 0)
    one("clean", "warn_if_singular_dev", 3, "GrInt")
    one("singular", "warn_if_singular_dev", 3, "GrInt", info=(0, 2, 1))
    one("singular, a shard", "warn_if_singular_dev", 3, "GrInt", [10, 11, 12], info=(0, 2, 1))
    one("many", "warn_if_singular_dev", 12, "GrInt", info=(1,))
    one("fails", "warn_if_singular_dev", 3, "GrInt", rc=EHIP)
    sweep("", "last_iters_dev", H, 3, 2)
    one("m = 0", "last_iters_dev", H, 0, 0)

    # ---- diagnostics
    sweep("on", "profile")
    one("off", "profile", False)
    sweep("", "profile_reset")
    sweep("", "profile_read", "inverse", byref=[1.5, 4])
    sweep("", "profile_read_flops", "zgemm", byref=[2e9, 1e9])
    sweep("", "selftest_mfma", byref=[1e-15])
    sweep("", "zgemm", 2, 2, 2, 1, cm((2, 2), 1), 2, 0, cm((2, 2), 2), 2, 0, 0, cm((2, 2), 3), 2, 4)
    one("batch, kernel", "zgemm", 2, 2, 2, 2, cm((8,), 1), 2, 4, cm((8,), 2), 2, 4, 5, cm((8,), 3), 2, 4, kernel=2)
    one("arrays too short", "zgemm", 2, 2, 2, 2, cm((4,), 1), 2, 4, cm((8,), 2), 2, 4, 0, cm((8,), 3), 2, 4)
    sweep("no decode", "zgemm_plan", 64, 64, 8, byref=[1, 0])
    sweep("decode", "zgemm_plan", 64, 64, 8, 2, 3, 1, byref=[1, 2, 1, 2])
    one("vector unit", "zgemm_plan", 4, 4, byref=[3, 2])
    sweep("", "inverse_plan", 200, 8, byref=[2, 16, 4, 13, 2, 1, 0])
    one("deferred", "inverse_plan", 200, 8, 1, True, byref=[2, 16, 4, 13, 3, 0, 1])
    sweep("", "inverse_last", byref=[2, 3])

    # ---- handles and the context go
    one("", "sigma_free", H, rc=EINVAL)
    one("", "layered_free", LH, rc=EINVAL)
    one("gone", "layered_pattern_size", LH)
    one("gone", "layered_terminal_count", LH)
    one("", "close")
    one("twice", "close")
    one("after close", "sigma_free", H)
    one("after close", "layered_free", LH + 1)


def transcript():
    """(lines, the Run): the stand-in takes the place of the loaded library for the static methods and NegfError too"""
    run = Run()
    saved, _lib._lib = _lib._lib, run.lib
    try:
        script(run)
    finally:
        _lib._lib = saved
    return run.lib.lines, run


def _public(cls):
    return {k for k, v in vars(cls).items() if not k.startswith("_") and (callable(v) or isinstance(v, staticmethod))}


def test_engine_calls_match_the_parent_transcript():
    lines, run = transcript()
    public = _public(Engine)
    assert public - run.exercised == set(), f"public Engine methods without a scenario: {sorted(public - run.exercised)}"
    assert run.reaching == public - NO_LIBRARY, (sorted(run.reaching ^ (public - NO_LIBRARY)))
    missing = set(_lib.SIGNATURES) - NOT_REACHED - run.lib.called
    assert not missing, f"library functions no scenario reached: {sorted(missing)}"
    with open(GOLDEN) as f:
        head, *golden = f.read().splitlines()
    assert head.startswith("# parent ")
    assert len(lines) == len(golden), f"{len(lines)} lines, the parent's transcript has {len(golden)}"
    for k, (a, b) in enumerate(zip(lines, golden)):
        assert a == b, f"line {k + 2} of the transcript:\n  now:    {a}\n  parent: {b}"


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] != "--write":
        sys.exit("usage: test_engine_calls_host.py --write FILE COMMIT")
    out, _ = transcript()
    with open(sys.argv[2], "w") as f:
        f.write(f"# parent {sys.argv[3]}: Engine's calls into the library, written by tests/test_engine_calls_host.py --write\n")
        f.write("\n".join(out) + "\n")
