"""Transmission eigenchannels of layered devices, held on the CPU: the float64 restatements of rgf_chan_ref.py (both
sweeps; LAPACK and the numpy restatement of the wide kernels) against the extended-precision truth and the bars of
xprec_channels.py, planted defects against the same bars, the second header against its table and the built library, and
the binding of the new front ends in gaunegf_amd/layered.py against a recorded transcript
(tests/golden/layered_channels_calls.txt: ``python tests/test_rgf_chan_host.py --write FILE`` writes it)."""
import ctypes as C
import hashlib
import json
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgf_chan_ref as rc                                      # noqa: E402
import test_engine_calls_host as T                             # noqa: E402
import xprec_channels as xc                                    # noqa: E402
from gaunegf_amd import _lib, layered                          # noqa: E402
from gaunegf_amd.layered import Lead, LayeredSystem           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
GOLDEN_CALLS = os.path.join(GOLDEN_DIR, "layered_channels_calls.txt")
GOLDEN_ABI = os.path.join(GOLDEN_DIR, "layered_channels_parent_abi.json")
TAGS = [t[0] for t in rc.host_table()]


# --------------------------------------------------------------------------- 1. restatements within half the bar
@pytest.mark.parametrize("tag", TAGS)
def test_restatements_stay_within_half_the_bar(tag):
    """both sweeps, with LAPACK and with the restatement of the wide kernels: T, rank and sum-rule ratios <= 0.5"""
    _, c, E, a = next(t for t in rc.host_table() if t[0] == tag)
    cc, truths = rc.truths_of(tag)
    worst = {}
    for m, t in enumerate(truths):
        for sweep in ("lr", "rl"):
            for eig, chol in (("lapack", "ref"), ("wide", "wide")):
                Tn, r = rc.channels_f64(c, E[m], a, sweep=sweep, eig=eig, chol=chol)
                assert np.all(Tn[r:] == 0.0) and np.all(np.diff(Tn[:r]) <= 0)
                got = np.array(t.ratios_T(Tn, r, "chan")) / xc.C_CHAN
                key = f"{sweep}/{eig}"
                worst[key] = np.maximum(worst.get(key, 0.0), got)
    print(f"ACC layered channels {tag}: kappa <= {max(t.kappa for t in truths):.1e} " +
          " ".join(f"{k} T {v[0]:.3g} rank {v[1]:.3g} sum {v[2]:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert np.all(v <= 0.5), (tag, k, v)


def _solver_truths(K):
    """{name: (A, (w, V) truth)} of rgf_chan_ref.solver_spectra(K); the 2^+-64 copies take the scaled truth (exact)"""
    mats = rc.solver_spectra(K)
    out = {}
    for name, A in mats.items():
        base, _, s = name.partition("*2^")
        if s:
            w, V = out[base][1]
            out[name] = (A, (w * np.longdouble(2.0) ** int(s), V))
        else:
            out[name] = (A, xc.herm_eig_ld(A))
    return out


@pytest.mark.parametrize("K", [3, 17, 97, 130, 257])
def test_the_wide_solver_restatement_stays_within_half_the_solver_bar(K):
    worst = 0.0
    for name, (A, truth) in _solver_truths(K).items():
        w = rc.wide_eigvalsh(A)
        assert np.all(np.diff(w) >= 0)
        r = xc.solver_ratios(A, w, truth=truth)[0]
        worst = max(worst, r)
        assert r <= 0.5, (K, name, r)
    print(f"ACC wide solver restatement K = {K}: worst {worst:.3g}")


def test_the_wide_cholesky_restatement_is_the_reference_factorisation():
    """same pivots, rank and factor to rounding as channel_states_ref.pivoted_cholesky, on full and deficient rank"""
    import channel_states_ref as R
    rng = np.random.default_rng(11)
    for K, r in ((1, 1), (5, 5), (40, 7), (128, 33), (130, 130)):
        A = rng.standard_normal((K, r)) + 1j * rng.standard_normal((K, r))
        G = A @ A.conj().T
        L1, L2 = rc.wide_cholesky(G), R.pivoted_cholesky(G)
        assert L1.shape == L2.shape == (K, r)
        assert np.abs(L1 - L2).max() <= 1e-12 * np.abs(G).max() ** 0.5
        assert np.abs(L1 @ L1.conj().T - G).max() <= 1e-13 * np.abs(G).max()
    assert rc.wide_cholesky(np.zeros((4, 4))).shape == (4, 0)


# --------------------------------------------------------------------------- 2. planted defects
def _worst(tag, **defect):
    _, c, E, a = next(t for t in rc.host_table() if t[0] == tag)
    _, truths = rc.truths_of(tag)
    worst = 0.0
    for m, t in enumerate(truths):
        Tn, r = rc.channels_f64(c, E[m], a, **defect)
        worst = max(worst, max(t.ratios_T(Tn, r, "chan")) / xc.C_CHAN)
    return worst


def test_the_bar_rejects_the_transposed_corner_block():
    """G_ab^T in the place of G_ab^H, on the complex-Hermitian wide case in both orders"""
    for tag in ("both a=right", "both a=left"):
        assert _worst(tag) <= 0.5
        bad = _worst(tag, gab="T")
        print(f"planted G_ab^T {tag}: {bad:.3g} bars")
        assert bad > 1.0


def test_the_bar_rejects_a_cholesky_without_pivoting():
    """lowest index instead of largest diagonal on the rank-deficient case"""
    for chol in ("ref", "wide"):
        bad = _worst("rank a=left", chol=chol, pivot="first")
        print(f"planted lowest-index pivot ({chol}): {bad:.3g} bars")
        assert bad > 1.0


def test_the_bar_rejects_a_loose_bisection():
    """bisection stopped at 1e-8 of the tridiagonal's norm"""
    bad = _worst("both a=right", eig="wide", chol="wide", rel_stop=1e-8)
    print(f"planted bisection at 1e-8: {bad:.3g} bars")
    assert bad > 1.0
    A = rc.solver_spectra(97)["cluster"]
    assert xc.solver_ratios(A, rc.wide_eigvalsh(A, rel_stop=1e-8))[0] > 1.0


# --------------------------------------------------------------------------- 3. header, table and library agree
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(negf_[a-z0-9_]+)\s*\(", src)))


def _signatures_source():
    """the text of the SIGNATURES table in _lib.py, from its first line to the closing brace"""
    src = open(os.path.join(ROOT, "gaunegf_amd", "_lib.py")).read()
    start = src.index("SIGNATURES = {")
    return src[start:src.index("\n}\n", start) + 3]


def _declarations(text):
    """a header without its comments, white space collapsed: what a compiler reads of it"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return " ".join(text.split())


def _abi_hashes():
    with open(os.path.join(ROOT, "include", "negf.h")) as f:
        h = hashlib.sha256(_declarations(f.read()).encode()).hexdigest()
    return {"negf.h declarations": h, "SIGNATURES": hashlib.sha256(_signatures_source().encode()).hexdigest()}


def test_the_second_header_its_table_and_the_library_agree():
    from gaunegf_amd import build
    build.build()
    lib = _lib.load()
    names = _declared("negf_layered_channels.h")
    assert len(names) == 5
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/negf_layered_channels.h but not exported"
        assert getattr(lib, n).argtypes == _lib.SIGNATURES_LAYERED_CHANNELS[n][1]
    assert sorted(_lib.SIGNATURES_LAYERED_CHANNELS) == names
    assert not set(_lib.SIGNATURES) & set(_lib.SIGNATURES_LAYERED_CHANNELS)
    assert not set(names) & set(_declared("negf.h"))


def test_the_first_header_and_table_are_the_parents():
    """negf.h's declarations (the header without its comments: the wording of a comment may follow the library, as the
    rules of negf_set_batch did) and the SIGNATURES table byte for byte: their sha256 recorded on the parent commit"""
    with open(GOLDEN_ABI) as f:
        assert _abi_hashes() == json.load(f)


# --------------------------------------------------------------------------- 4. the binding transcript
_SECOND_TRAILING_OUT = {"negf_layered_transmission_channels": 2, "negf_eigvalsh_wide_batched": 2}


def _system():
    F_diag = [T.rm((2, 2), 1) + T.rm((2, 2), 1).T, T.rm((3, 3), 2) + T.rm((3, 3), 2).T, T.rm((2, 2), 3) + T.rm((2, 2), 3).T]
    F_up = [T.rm((2, 3), 4), T.rm((3, 2), 5)]
    S_diag = [np.eye(2), np.eye(3), np.eye(2)]
    S_up = [0.125 * T.rm((2, 3), 6), 0.125 * T.rm((3, 2), 7)]
    return LayeredSystem(F_diag, F_up, S_diag, S_up)


def transcript():
    """The lines of every scenario: the library calls with every argument (checked like ctypes against the table that
    declares them), what the function returned or raised, the warnings, the counters and ``last_info``."""
    run = T.Run()
    lib, eng = run.lib, run.eng
    merged = dict(_lib.SIGNATURES); merged.update(_lib.SIGNATURES_LAYERED_CHANNELS)
    shim = type("LibShim", (), {k: getattr(_lib, k) for k in dir(_lib) if k.startswith("NEGF_")})()
    shim.SIGNATURES = merged
    saved = (T._lib, dict(T._TRAILING_OUT), _lib._lib)
    T._lib = shim
    T._TRAILING_OUT.update(_SECOND_TRAILING_OUT)
    _lib._lib = lib
    second_calls = []

    def one(label, fn, *args, rc=0, rcs=None, info=None, byref=(), nan_row=None, **kw):
        lib.reset()
        lib.rc_all, lib.rc, lib.info, lib.byref, lib.nan_row = rc, dict(rcs or {}), info, list(byref), nan_row
        head, before = f"== {fn.__name__} [{label}] rc={rc}", len(lib.lines)
        eng.last_info = None
        c0, p0 = eng.counters["calls"], eng.counters["points"]
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                end = ["ret " + T.describe(fn(*args, **kw))]
            except Exception as e:
                end = [f"exc {type(e).__name__}: {e}"]
        calls = lib.lines[before:]
        del lib.lines[before:]
        second_calls.extend(line.split("(")[0].split()[1] for line in calls)
        end += [f"warn {wn.category.__name__}: {wn.message}" for wn in caught]
        state = f"calls+{eng.counters['calls'] - c0} points+{eng.counters['points'] - p0}"
        if eng.last_info is not None:
            state += f" info={T.describe(eng.last_info)}"
        lib.lines.append(" | ".join([head] + calls + end + [state]))

    def sweep(label, fn, *args, ok=(), sing_info=(0, 3, 1), **kw):
        """the four kinds of return code of the channel entry point; `ok`: the calls in front of it keep returning 0"""
        rcs = {name: 0 for name in ok}
        one(label, fn, *args, rcs=rcs, **kw)
        one(label, fn, *args, rc=T.EINVAL, rcs=rcs, **kw)
        one(label, fn, *args, rc=T.ESING, rcs=rcs, info=sing_info, **kw)
        one(label, fn, *args, rc=T.EHIP, rcs=rcs, **kw)

    try:
        LH, E3 = 5, T.E3
        setup = ("negf_layered_create", "negf_layered_terminal_const", "negf_layered_terminal_blocks", "negf_layered_free")
        sweep("", layered.set_channel_algo, 1, engine=eng)
        sweep("batch", layered.eigvalsh_wide, T.cm((3, 2, 2), 2), engine=eng)
        sweep("single", layered.eigvalsh_wide, T.cm((2, 2), 2), engine=eng, sing_info=(1,))
        one("m = 0", layered.eigvalsh_wide, T.cm((0, 2, 2), 2), engine=eng)
        one("not square", layered.eigvalsh_wide, T.cm((3, 2, 3), 2), engine=eng)
        one("K too large", layered.eigvalsh_wide, np.zeros((1, 513, 513)), engine=eng)
        sweep("", layered.layered_channel_count, eng, LH, 0, 1, byref=[3])
        sweep("nchan from the count", layered.layered_transmission_channels, eng, LH, 0, 1, E3,
              ok=("negf_layered_channel_count",), byref=[2])
        one("nchan given", layered.layered_transmission_channels, eng, LH, 1, 0, E3, 4)
        one("eigensolver flags", layered.layered_transmission_channels, eng, LH, 0, 1, E3, 2, rc=T.ESING, info=(0, -1, 2), nan_row=1)
        one("nchan = 0", layered.layered_transmission_channels, eng, LH, 0, 1, E3, 0)
        one("m = 0", layered.layered_transmission_channels, eng, LH, 0, 1, T.E0, 2)
        sweep("", layered.layered_transmission_channels_dev, eng, LH, 0, 1, 3, 0x1000, 2, 0x2000)
        one("an address is no number", layered.layered_transmission_channels_dev, eng, LH, 0, 1, 3, 'x', 2, 0x2000)
        system = _system()
        leads = [Lead.const([0, 1], T.cm((2, 2), 4)), Lead.const([5, 6], T.cm((2, 2), 5))]
        sweep("const leads", layered.calculate_eigenchannels_layered, system, leads, E3, engine=eng,
              ok=setup + ("negf_layered_channel_count",), byref=[LH, 0, 1, 2])
        one("pair reversed, nchan", layered.calculate_eigenchannels_layered, system, leads, E3, pair=(1, 0), nchan=1, engine=eng,
            byref=[LH, 0, 1])
        blocks = [Lead.const([0], T.cm((1, 1), 4)), Lead.blocks([5, 6], T.cm((3, 2, 2), 5))]
        one("blocks lead", layered.calculate_eigenchannels_layered, system, blocks, E3, nchan=2, engine=eng, byref=[LH, 0, 1])
        sweep("", layered.channel_count_layered, system, leads, engine=eng, ok=setup, byref=[LH, 0, 1, 2])
        one("spin", layered.calculate_eigenchannels_layered, system, leads, E3, spin='u', engine=eng)
        one("checkpoint", layered.calculate_eigenchannels_layered, system, leads, E3, checkpoint_file='x.npz', engine=eng)
        one("the stub", layered.calculate_transmission_channels_layered)
    finally:
        T._lib, _lib._lib = saved[0], saved[2]
        T._TRAILING_OUT.clear(); T._TRAILING_OUT.update(saved[1])
    lines = list(lib.lines)
    eng._ctx = None                                             # (the stand-in engine has no context to destroy)
    return lines, set(second_calls)


def test_the_front_ends_match_the_recorded_transcript():
    lines, called = transcript()
    missing = set(_lib.SIGNATURES_LAYERED_CHANNELS) - called
    assert not missing, f"entry points of the second header no scenario reached: {sorted(missing)}"
    with open(GOLDEN_CALLS) as f:
        head, *golden = f.read().splitlines()
    assert head.startswith("# ")
    assert len(lines) == len(golden), f"{len(lines)} lines, the recorded transcript has {len(golden)}"
    for k, (a, b) in enumerate(zip(lines, golden)):
        assert a == b, f"line {k + 2} of the transcript:\n  now:      {a}\n  recorded: {b}"


def test_the_stand_in_checks_the_second_table_like_ctypes():
    """a wrong argument count and a wrong argument type are refused against SIGNATURES_LAYERED_CHANNELS"""
    run = T.Run()
    merged = dict(_lib.SIGNATURES); merged.update(_lib.SIGNATURES_LAYERED_CHANNELS)
    shim = type("LibShim", (), {})()
    shim.SIGNATURES = merged
    saved, T._lib = T._lib, shim
    try:
        with pytest.raises(TypeError):
            run.lib.negf_set_channel_algo(run.lib.ctx)
        with pytest.raises((C.ArgumentError, TypeError)):
            run.lib.negf_set_channel_algo(run.lib.ctx, "one")
        assert run.lib.negf_set_channel_algo(run.lib.ctx, 1) == 0
    finally:
        T._lib = saved


# --------------------------------------------------------------------------- 5. refusals of the front end
class _NoEngine:
    """an engine that must not be reached"""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was reached ({name})")


def test_front_end_refusals():
    system = _system()
    leads = [Lead.const([0, 1], T.cm((2, 2), 4)), Lead.const([5, 6], T.cm((2, 2), 5))]
    with pytest.raises(NotImplementedError, match="spin"):
        layered.calculate_eigenchannels_layered(system, leads, T.E3, spin='u', engine=_NoEngine())
    with pytest.raises(NotImplementedError, match="checkpoint"):
        layered.calculate_eigenchannels_layered(system, leads, T.E3, checkpoint_file="x.npz", engine=_NoEngine())
    with pytest.raises(NotImplementedError, match="calculate_eigenchannels_layered"):
        layered.calculate_transmission_channels_layered()
    # a pair on one end: the library's NEGF_EINVAL is the caller's ValueError
    run = T.Run()
    saved, _lib._lib = _lib._lib, run.lib
    merged = dict(_lib.SIGNATURES); merged.update(_lib.SIGNATURES_LAYERED_CHANNELS)
    shim = type("LibShim", (), {})()
    shim.SIGNATURES = merged
    saved_t, T._lib = T._lib, shim
    try:
        run.lib.rc = {"negf_layered_channel_count": T.EINVAL, "negf_layered_transmission_channels": T.EINVAL}
        same_end = [Lead.const([0], T.cm((1, 1), 4)), Lead.const([1], T.cm((1, 1), 5))]
        with pytest.raises(ValueError, match="negf_layered_channel_count"):
            layered.calculate_eigenchannels_layered(system, same_end, T.E3, engine=run.eng)
        with pytest.raises(ValueError, match="negf_layered_transmission_channels"):
            layered.calculate_eigenchannels_layered(system, same_end, T.E3, nchan=1, engine=run.eng)
    finally:
        _lib._lib, T._lib = saved, saved_t


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--write":
        out, _ = transcript()
        with open(sys.argv[2], "w") as f:
            f.write("# the layered channel front ends' calls into the library, written by tests/test_rgf_chan_host.py --write\n")
            f.write("\n".join(out) + "\n")
    elif len(sys.argv) == 3 and sys.argv[1] == "--write-abi":
        with open(sys.argv[2], "w") as f:
            json.dump(_abi_hashes(), f, indent=1, sort_keys=True)
            f.write("\n")
    else:
        sys.exit("usage: test_rgf_chan_host.py --write FILE | --write-abi FILE (the latter on the parent commit's negf.h and _lib.py)")
