"""
The stream contract of the device-resident entry points (include/negf.h, "device-resident variants", and
negf_set_stream): a PRIVATE engine on a non-blocking stream of the caller's, energies, weights and results in the
caller's HBM, work of the caller's in flight in front of the call.

No new truth and no new tolerance: the truth-bar tests hold the host-pointer forms to extended precision on the session
engine; a *_dev call that equals its host-pointer form BITWISE inherits all of that.  The reference of every case is the
host-pointer form on the private engine after set_stream(s), itself compared with the session engine's result on the
default stream (test a).  What is added is the ordering:
  (a) the same bits on the caller's stream into NaN-filled buffers, and again into buffers that hold the last result
      (overwritten, never accumulated into);
  (b) inputs are read in stream order: delay, copies of the true grid and weights over valid but wrong ones, the call
      and a snapshot of the result, all queued before the first wait -- and the call returns while the delay still runs
      wherever the header says it is asynchronous when warm;
  (c) two calls back to back into the same buffer share the context's work areas in stream order;
  (d) negf_set_stream orders the new stream behind the old one, and setting the same stream again is free;
  (e) two contexts interleaved, each with its own stream, system and g(E) cache;
  (f) the per-energy info of an asynchronous call with an exactly singular energy.
The delay is torch.cuda._sleep, calibrated once per module to about 50 ms; the last test asserts that it was at least
three times the host time of the slowest asynchronous call of the run and prints both.

Cases (the smallest shapes that reach each kernel sequence):
  48 x 37    fused small kernel; constant contacts, and chain leads of 6 orbitals at a fixed sweep count (cache off)
  130 x 40   single-workgroup inverse and the kernel sequence, in batches of 16 (the work areas are reused in one call)
  300 x 70   windowed inverse, the sum read through the permutation
  257 x 344  stream groups on side streams with windows in pairs (test_inverse_cells_gpu's cell)
  70 x 40    chain leads of 18 orbitals through the chain provider, g(E) cache on and off
  layered    rgf_ref case b on its contour, terminals bound as rgf_parent_cases binds them, batches of 3
"""
import time
import warnings

import numpy as np
import pytest
import torch    # at collection, before any engine exists: the library then binds to the HIP runtime torch has loaded (as
                # under bench.py); loaded after the library, torch brings a second copy of the runtime and sees no GPU

from helpers import chain_lead, random_system, swept
from test_small_fused_gpu import _const

pytestmark = pytest.mark.gpu

DELAY_MS = 50.0                # aimed at; measured per module (test_zz_... asserts it against the calls' host times)
SLEEP_PROBE = 1_000_000        # cycles of the calibration sleep
REL = 1e-13                    # test_distributed_gpu.py's bound where two contexts group their sums differently


# --------------------------------------------------------------------------------------------------------- cases
class Spec:
    def __init__(self, n, m, batch, kind, cache=None, layered=False):
        self.n, self.m, self.batch, self.kind, self.cache, self.layered = n, m, batch, kind, cache, layered


SPECS = {
    "48x37-const": Spec(48, 37, 37, "const"),
    "48x37-chain": Spec(48, 37, 37, "chain6", cache=False),
    "130x40": Spec(130, 40, 16, "const"),
    "300x70": Spec(300, 70, 70, "const"),
    "257x344": Spec(257, 344, 344, "const"),
    "70x40-cache": Spec(70, 40, 40, "chain18", cache=True),
    "70x40-nocache": Spec(70, 40, 40, "chain18", cache=False),
    "layered-b": Spec(33, 8, 3, "layered", layered=True),
}
CASES = list(SPECS)
_OBJ = {}                      # (id(engine), case) -> (F, S, provider object) or the layered handles


def _chain(N, nc, seed):
    from gaunegf_amd.surfG1D import surfG
    F, S = random_system(N, seed)
    inds = [list(range(nc)), list(range(N - nc, N))]
    aL = chain_lead(nc, seed + 1); aR = chain_lead(nc, seed + 2)
    g = surfG(F, S, inds, taus=[aL[2].copy(), aR[2].copy()], staus=[aL[3].copy(), aR[3].copy()], alphas=[aL[0], aR[0]],
              aOverlaps=[aL[1], aR[1]], betas=[aL[2], aR[2]], bOverlaps=[aL[3], aR[3]], eta=1e-3)
    g.force_iters = 30
    return F, S, g


def _objects(eng, case):
    """The case's system and provider object FOR THIS ENGINE (a provider object releases its handles on other engines
    when it is lowered anew)."""
    key = (id(eng), case)
    if key not in _OBJ:
        sp = SPECS[case]
        if sp.kind == "const":
            F, S, g, _ = _const(sp.n, 40 + sp.n)
        elif sp.kind == "chain6":
            F, S, g = _chain(48, 6, 12)
        else:
            F, S, g = _chain(70, 18, 1100)
        _OBJ[key] = (F, S, g)
    return _OBJ[key]


def _bind(eng, case, private=True):
    """Batch, system, provider (and, on the private engine, the cache setting) of a case; returns what the ops take as
    their handle.  Everything here may wait for the stream: it happens before anything is queued behind a delay."""
    sp = SPECS[case]
    eng.set_batch(sp.batch)
    if sp.layered:
        key = (id(eng), case)
        if key not in _OBJ:
            import rgf_parent_cases as pc
            import rgf_ref as rr
            _OBJ[key] = pc._bind(eng, rr.cases()[1])
        return _OBJ[key]
    F, S, g = _objects(eng, case)
    eng.set_system(F, S)
    if private and sp.cache is not None:
        eng.set_chain_cache(0)                         # drops what earlier tests left
        if sp.cache:
            eng.set_chain_cache(512)
    return g._negf_lower(eng)


def _grid(case, k):
    """Grid k (0, 1) of a case: two different grids and weight vectors of the same length."""
    sp = SPECS[case]
    if sp.layered:
        import rgf_ref as rr
        _, E, w = rr.contour()
        return (E, w) if k == 0 else (E + (0.3 + 0.1j), w * (0.7 - 0.2j))
    j = np.arange(sp.m)
    if k == 0:
        return np.linspace(-1.5, 1.5, sp.m) + 0.02j, (np.cos(j) + 1.5) * (3.0 / sp.m) * (1 + 0.2j)
    return np.linspace(-1.2, 1.7, sp.m) + 0.03j, (np.sin(j) + 1.7) * (2.0 / sp.m) * (1 - 0.1j)


# ----------------------------------------------------------------------------------------------------------- ops
def _f64(a):
    """any result as a flat float64 array (complex values as re, im pairs): what the device buffer holds"""
    a = np.ascontiguousarray(a)
    return (a.view(np.float64) if np.iscomplexobj(a) else a.astype(np.float64, copy=False)).ravel()


def _ends(m):
    return np.array([5, 6, m], dtype=np.int32)         # ragged, the middle segment a single point


def _segs(E, w):
    e = [0, 5, 6, E.size]
    return [(E[a:b], w[a:b]) for a, b in zip(e[:-1], e[1:])]


class Op:
    """host(eng, H, E, w) -> the host-pointer form's result; dev(eng, H, m, E_ptr, w_ptr, out_ptr) queues the *_dev
    form; size(eng, H, n, m) float64 elements of the device buffer; part(flat, m): what of the buffer the call writes;
    blocks: the header says the call waits for the stream even when warm."""

    def __init__(self, name, host, dev, size, part=None, blocks=False):
        self.name, self.host, self.dev, self.size, self.blocks = name, host, dev, size, blocks
        self.part = part or (lambda flat, m: flat)


def _dense_ops(n):
    ops = [Op("gr_int", lambda e, h, E, w: e.gr_int(h, E, w),
              lambda e, h, m, E, w, o: e.gr_int_dev(h, m, E, w, o), lambda e, h, n, m: 2 * n * n)]
    for ind in (None, 0, -1):
        ops.append(Op(f"gless_int[{ind}]", lambda e, h, E, w, ind=ind: e.gless_int(h, ind, E, w),
                      lambda e, h, m, E, w, o, ind=ind: e.gless_int_dev(h, ind, m, E, w, o), lambda e, h, n, m: 2 * n * n))
    ops.append(Op("gr_int_seg", lambda e, h, E, w: np.stack(e.gr_int_seg(h, _segs(E, w))),
                  lambda e, h, m, E, w, o: e.gr_int_seg_dev(h, m, E, w, _ends(m), o), lambda e, h, n, m: 6 * n * n))
    ops.append(Op("gless_int_seg", lambda e, h, E, w: np.stack(e.gless_int_seg(h, 0, _segs(E, w))),
                  lambda e, h, m, E, w, o: e.gless_int_seg_dev(h, 0, m, E, w, _ends(m), o), lambda e, h, n, m: 6 * n * n))
    ops.append(Op("transmission", lambda e, h, E, w: e.transmission(h, 0, 1, E),
                  lambda e, h, m, E, w, o: e.transmission_dev(h, 0, 1, m, E, o), lambda e, h, n, m: m))
    if n % 2 == 0:
        # spin blocks: T_dev is not touched (include/negf.h), the four components follow it in the test's buffer
        ops.append(Op("transmission[spin]", lambda e, h, E, w: e.transmission(h, 0, 1, E, spin_block=True)[1],
                      lambda e, h, m, E, w, o: e.transmission_dev(h, 0, 1, m, E, o, o + 8 * m, spin_block=True),
                      lambda e, h, n, m: 5 * m, part=lambda flat, m: flat[m:]))
    return ops


def _layered_ops():
    from rgf_parent_cases import _flat
    return [
        Op("layered_gr_int", lambda e, H, E, w: _flat(e.layered_gr_int(H[0], E, w)),
           lambda e, H, m, E, w, o: e.layered_gr_int_dev(H[0], m, E, w, o), lambda e, H, n, m: 2 * e.layered_pattern_size(H[0])),
        Op("layered_gless_int", lambda e, H, E, w: _flat(e.layered_gless_int(H[0], None, E, w)),
           lambda e, H, m, E, w, o: e.layered_gless_int_dev(H[0], None, m, E, w, o),
           lambda e, H, n, m: 2 * e.layered_pattern_size(H[0]), blocks=True),      # uploads the terminals' orbital lists
        Op("layered_transmission", lambda e, H, E, w: e.layered_transmission(H[0], H[2], H[1], E),
           lambda e, H, m, E, w, o: e.layered_transmission_dev(H[0], H[2], H[1], m, E, o), lambda e, H, n, m: m),
        Op("layered_dos", lambda e, H, E, w: np.concatenate([a.ravel() for a in e.layered_dos(H[0], E)]),
           lambda e, H, m, E, w, o: e.layered_dos_dev(H[0], m, E, o, o + 8 * m), lambda e, H, n, m: m + m * n),
    ]


def _ops(case):
    return _layered_ops() if SPECS[case].layered else _dense_ops(SPECS[case].n)


def _asynchronous(case, op):
    """The header's table: a warm call returns without waiting unless the chain provider's g(E) cache is on (one download
    of the grid) or the call uploads host tables (layered_gless_int_dev)."""
    return not op.blocks and not SPECS[case].cache


# ------------------------------------------------------------------------------------------- the private context
class Private:
    def __init__(self):
        from gaunegf_amd.engine import Engine
        with open("/proc/self/maps") as f:
            runtimes = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
        assert len(runtimes) == 1, f"torch and libnegf_hip.so must share one HIP runtime (streams, events): {sorted(runtimes)}"
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.eng = Engine(0)
        self.s = torch.cuda.Stream(device=self.dev)                 # non-blocking
        self.eng.set_stream(self.s.cuda_stream)
        self.refs, self.ref_batch = {}, {}
        self.host_ms = {}                                          # (test, case, op) -> host time of an asynchronous call
        # the delay: one timed sleep, scaled to DELAY_MS, timed again
        with torch.cuda.stream(self.s):
            torch.cuda._sleep(1000)                                 # (first launch)
            probe = self._timed_sleep(SLEEP_PROBE)
            self.cycles = int(SLEEP_PROBE * DELAY_MS / probe)
            self.delay_ms = self._timed_sleep(self.cycles)
        print(f"STREAM delay: {SLEEP_PROBE} cycles took {probe:.2f} ms; {self.cycles} cycles took {self.delay_ms:.2f} ms")
        assert self.delay_ms >= 10.0, f"the delay is {self.delay_ms:.2f} ms: too short to show that a call did not wait for it"

    def _timed_sleep(self, cycles):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record(self.s); t.cuda._sleep(int(cycles)); e1.record(self.s)
        self.s.synchronize()
        return e0.elapsed_time(e1)

    def tensor(self, a):
        """a host array on the device, as float64"""
        with self.torch.cuda.stream(self.s):
            return self.torch.from_numpy(_f64(a).copy()).to(self.dev)

    def empty(self, n):
        with self.torch.cuda.stream(self.s):
            return self.torch.empty(int(n), dtype=self.torch.float64, device=self.dev)

    def sleep(self):
        self.torch.cuda._sleep(self.cycles)

    def ref(self, case, op, k, H):
        """the host-pointer form on the private engine, on its stream: once per (case, op, grid)"""
        key = (case, op.name, k)
        if key not in self.refs:
            E, w = _grid(case, k)
            r = _f64(op.host(self.eng, H, E, w)).copy()
            if SPECS[case].n > 96 and not SPECS[case].layered:          # (below, gr_int and gr_int_seg have no workspace)
                swept(self.eng, SPECS[case].batch, E.size, transmission=op.name.startswith("transmission"))
            r.setflags(write=False)
            self.refs[key] = r
            self.ref_batch[key] = self.eng.get_batch()                  # how the workspace grouped its sums
        return self.refs[key]

    def timed(self, key, call, asynchronous):
        """the library call, its host time, and whether the stream was still busy right after it"""
        t0 = time.perf_counter()
        call()
        ms = (time.perf_counter() - t0) * 1e3
        busy = not self.s.query()
        if asynchronous:
            self.host_ms[key] = ms
        return busy, ms


@pytest.fixture(scope="module")
def priv(engine):
    p = Private()
    yield p
    p.eng.sync()
    p.eng.close()                                                   # (before the stream it was running on goes)
    H = _OBJ.pop((id(engine), "layered-b"), None)
    if H:
        engine.layered_free(H[0])
    _OBJ.clear()                                                    # (the provider objects release their handles)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# --------------------------------------------------------------------------------------------------------- tests
def test_the_shapes_reach_their_kernel_sequences():
    from gaunegf_amd.engine import Engine
    assert Engine.inverse_plan(130, 16)["path"] == 1 and Engine.inverse_plan(130, 8)["path"] == 1      # single workgroup
    for defer in (False, True):
        assert Engine.inverse_plan(300, 70, defer=defer)["path"] == 2                                    # windows
        p = Engine.inverse_plan(257, 344, defer=defer)
        assert p["path"] == 2 and len(p["groups"]) > 1 and all(g["pairs"] for g in p["groups"]), p       # side streams, pairs
    assert Engine.inverse_plan(300, 70, defer=True)["deferred"]                                          # the sum reads the permutation


@pytest.mark.parametrize("case", CASES)
def test_a_same_bits_on_a_callers_stream_into_poisoned_buffers(priv, engine, case):
    sp, t = SPECS[case], priv.torch
    H = _bind(priv.eng, case)
    E, w = _grid(case, 0)
    m = E.size
    refs = {op.name: priv.ref(case, op, 0, H) for op in _ops(case)}
    # the private engine's host-pointer forms against the session engine's on the default stream
    try:
        Hs = _bind(engine, case, private=False)
        for op in _ops(case):
            rs = _f64(op.host(engine, Hs, E, w))
            pb = priv.ref_batch[(case, op.name, 0)]
            if sp.layered or engine.get_batch() == pb:
                assert _same(refs[op.name], rs), (case, op.name, "session engine, same batch")
            else:
                d = np.linalg.norm(refs[op.name] - rs)
                print(f"STREAM {case} {op.name}: batches {pb} / {engine.get_batch()}, rel {d / np.linalg.norm(rs):.2e}")
                assert d <= REL * np.linalg.norm(rs), (case, op.name)
    finally:
        engine.set_batch(0)
    Ed, wd = priv.tensor(E), priv.tensor(w)
    for op in _ops(case):
        out = priv.empty(op.size(priv.eng, H, sp.n, m))
        with t.cuda.stream(priv.s):
            out.fill_(float("nan"))
            op.dev(priv.eng, H, m, Ed.data_ptr(), wd.data_ptr(), out.data_ptr())
            priv.eng.sync()
            got = op.part(out.cpu().numpy(), m)
            assert _same(got, refs[op.name]), (case, op.name, "into NaN")
            # once more, the buffer holding the previous result: the same, not twice it
            op.dev(priv.eng, H, m, Ed.data_ptr(), wd.data_ptr(), out.data_ptr())
            priv.eng.sync()
            assert _same(op.part(out.cpu().numpy(), m), refs[op.name]), (case, op.name, "into the previous result")
        assert not np.any(priv.eng.last_info_dev(m)), (case, op.name)


@pytest.mark.parametrize("case", CASES)
def test_b_inputs_are_read_in_stream_order(priv, case):
    sp, t = SPECS[case], priv.torch
    H = _bind(priv.eng, case)
    E, w = _grid(case, 0)
    m = E.size
    ops = _ops(case)
    refs = {op.name: priv.ref(case, op, 0, H) for op in ops}
    E_true, w_true = priv.tensor(E), priv.tensor(w)
    for op in ops:
        Ed, wd = priv.tensor(E + 1.0), priv.tensor(2.0 * w)          # valid, but wrong
        out = priv.empty(op.size(priv.eng, H, sp.n, m))
        if sp.cache:
            # (binding the case emptied the cache: the host-pointer form again, which enters the true grid as this entry
            #  point sweeps it -- and gives the reference's bits)
            assert _same(_f64(op.host(priv.eng, H, E, w)), refs[op.name]), (case, op.name)
        with t.cuda.stream(priv.s):
            out.fill_(float("nan"))
            op.dev(priv.eng, H, m, Ed.data_ptr(), wd.data_ptr(), out.data_ptr())         # warm: every buffer has its size
            priv.s.synchronize()
            assert not _same(op.part(out.cpu().numpy(), m), refs[op.name]), (case, op.name, "the wrong inputs give the right result")
            stats = priv.eng.chain_cache_stats()
            priv.sleep()
            Ed.copy_(E_true); wd.copy_(w_true)
            busy, ms = priv.timed(("b", case, op.name), lambda: op.dev(priv.eng, H, m, Ed.data_ptr(), wd.data_ptr(), out.data_ptr()),
                                  _asynchronous(case, op))
            snap = out.clone()
            priv.s.synchronize()
            got = op.part(snap.cpu().numpy(), m)
        assert _same(got, refs[op.name]), (case, op.name, "stale inputs were read")
        if _asynchronous(case, op):
            assert busy, (case, op.name, f"the call took {ms:.2f} ms on the host and the stream was idle after it: "
                          f"it waited for the {priv.delay_ms:.1f} ms delay, or the delay is too short")
        if sp.cache:
            # the true grid is in the cache, and so is the wrong one (the warm call): the call downloaded the grid in
            # stream order and hit the true one
            now = priv.eng.chain_cache_stats()
            # (one look-up per launch of the chain kernel: the transmission sweeps the grid in two halves)
            assert now["hits"] - stats["hits"] >= 1 and now["misses"] == stats["misses"], (case, op.name, stats, now)


@pytest.mark.parametrize("case", CASES)
def test_c_back_to_back_calls_share_the_workspace(priv, case):
    sp, t = SPECS[case], priv.torch
    H = _bind(priv.eng, case)
    (E1, w1), (E2, w2) = _grid(case, 0), _grid(case, 1)
    m = E1.size
    ops = _ops(case)
    refs = {op.name: (priv.ref(case, op, 0, H), priv.ref(case, op, 1, H)) for op in ops}
    d = [priv.tensor(x) for x in (E1, w1, E2, w2)]
    for op in ops:
        out = priv.empty(op.size(priv.eng, H, sp.n, m))
        with t.cuda.stream(priv.s):
            op.dev(priv.eng, H, m, d[0].data_ptr(), d[1].data_ptr(), out.data_ptr())     # warm
            priv.s.synchronize()
            out.fill_(float("nan"))
            priv.sleep()
            b1, _ = priv.timed(("c1", case, op.name), lambda: op.dev(priv.eng, H, m, d[0].data_ptr(), d[1].data_ptr(), out.data_ptr()),
                               _asynchronous(case, op))
            snap1 = out.clone()
            b2, _ = priv.timed(("c2", case, op.name), lambda: op.dev(priv.eng, H, m, d[2].data_ptr(), d[3].data_ptr(), out.data_ptr()),
                               _asynchronous(case, op))
            priv.s.synchronize()
            got1, got2 = op.part(snap1.cpu().numpy(), m), op.part(out.cpu().numpy(), m)
        assert _same(got1, refs[op.name][0]), (case, op.name, "call 1")
        assert _same(got2, refs[op.name][1]), (case, op.name, "call 2")
        assert not _same(refs[op.name][0], refs[op.name][1])
        if _asynchronous(case, op):
            assert b1 and b2, (case, op.name, "a call waited for the stream")


@pytest.mark.parametrize("case", ["48x37-const", "130x40"])
def test_d_switching_streams_orders_the_new_one_behind_the_old(priv, case):
    """Only the fused kernel and the single-workgroup inverse, the same system in both calls: every index either call
    can read was written as a valid one by the other, so a missing order could only ever show as a wrong number."""
    sp, t = SPECS[case], priv.torch
    H = _bind(priv.eng, case)
    op = _ops(case)[0]
    (E1, w1), (E2, w2) = _grid(case, 0), _grid(case, 1)
    m = E1.size
    r1, r2 = priv.ref(case, op, 0, H), priv.ref(case, op, 1, H)
    d = [priv.tensor(x) for x in (E1, w1, E2, w2)]
    out1, out2 = priv.empty(2 * sp.n * sp.n), priv.empty(2 * sp.n * sp.n)
    s1, s2 = t.cuda.Stream(device=priv.dev), t.cuda.Stream(device=priv.dev)
    try:
        with t.cuda.stream(priv.s):
            op.dev(priv.eng, H, m, d[0].data_ptr(), d[1].data_ptr(), out1.data_ptr())    # warm
            out1.fill_(float("nan")); out2.fill_(float("nan"))
        t.cuda.synchronize(priv.dev)
        priv.eng.set_stream(s1.cuda_stream)
        with t.cuda.stream(s1):
            priv.sleep()
            op.dev(priv.eng, H, m, d[0].data_ptr(), d[1].data_ptr(), out1.data_ptr())
        t0 = time.perf_counter()
        priv.eng.set_stream(s1.cuda_stream); priv.eng.set_stream(s1.cuda_stream)         # the same stream: free
        same_ms = (time.perf_counter() - t0) * 1e3
        assert not s1.query(), f"set_stream(same stream) twice took {same_ms:.2f} ms and the delay is over"
        priv.eng.set_stream(s2.cuda_stream)
        op.dev(priv.eng, H, m, d[2].data_ptr(), d[3].data_ptr(), out2.data_ptr())        # at once, on s2
        switch_busy = not s1.query()
        s2.synchronize()
        # s2 was ordered behind everything queued on s1 before the switch: s2 idle means s1 idle (polled for at most
        # 5 ms, a tenth of what the delay would still have to run without the order)
        t0 = time.perf_counter()
        s1_done_with_s2 = s1.query()
        while not s1_done_with_s2 and time.perf_counter() - t0 < 5e-3:
            s1_done_with_s2 = s1.query()
        s1.synchronize()
        with t.cuda.stream(priv.s):
            got1, got2 = out1.cpu().numpy(), out2.cpu().numpy()
    finally:
        t.cuda.synchronize(priv.dev)
        priv.eng.set_stream(priv.s.cuda_stream)
    assert switch_busy, "the switch or call 2 waited for the delay on the host"
    assert _same(got1, r1), (case, "call 1 on s1")
    assert _same(got2, r2), (case, "call 2 on s2")
    assert s1_done_with_s2, "call 2 on the new stream finished while call 1 on the old one had not: no order between them"


def test_e_two_contexts_interleaved(priv, engine):
    """The private engine on its stream (chain leads of 18 orbitals, cache on) and the session engine on the default
    stream (chain leads of 6, cache on), called alternately for three rounds without a wait of the test's in between."""
    t = priv.torch
    cp, cs = "70x40-cache", "48x37-chain"
    try:
        Hp = _bind(priv.eng, cp)
        Hs = _bind(engine, cs, private=False)
        engine.set_chain_cache(512)
        op = _dense_ops(0)[0]
        (Ep, wp), (Es, ws) = _grid(cp, 0), _grid(cs, 1)
        rp = priv.ref(cp, op, 0, Hp)
        rs = _f64(engine.gr_int(Hs, Es, ws))
        dp = [priv.tensor(Ep), priv.tensor(wp)] + [priv.empty(2 * 70 * 70) for _ in range(3)]
        ds = [t.from_numpy(_f64(x).copy()).to(priv.dev) for x in (Es, ws)] + \
             [t.full((2 * 48 * 48,), float("nan"), dtype=t.float64, device=priv.dev) for _ in range(3)]
        with t.cuda.stream(priv.s):
            for o in dp[2:]:
                o.fill_(float("nan"))
        t.cuda.synchronize(priv.dev)
        priv.eng.chain_cache_clear(); engine.chain_cache_clear()
        st_p, st_s = priv.eng.chain_cache_stats(), engine.chain_cache_stats()
        for k in range(3):
            with t.cuda.stream(priv.s):
                priv.eng.gr_int_dev(Hp, Ep.size, dp[0].data_ptr(), dp[1].data_ptr(), dp[2 + k].data_ptr())
            engine.gr_int_dev(Hs, Es.size, ds[0].data_ptr(), ds[1].data_ptr(), ds[2 + k].data_ptr())
        priv.eng.sync(); engine.sync()
        for k in range(3):
            with t.cuda.stream(priv.s):
                assert _same(dp[2 + k].cpu().numpy(), rp), ("private", k)
            assert _same(ds[2 + k].cpu().numpy(), rs), ("session", k)
        for eng, st, who in ((priv.eng, st_p, "private"), (engine, st_s, "session")):
            now = eng.chain_cache_stats()
            assert (now["hits"] - st["hits"], now["misses"] - st["misses"]) == (2, 1), (who, st, now)
    finally:
        engine.set_batch(0)


@pytest.mark.parametrize("n", [48, 130])
def test_f_info_after_an_asynchronous_call(priv, n):
    """F = S, Sigma = 0: E S - F - Sigma is the zero matrix at E = 1, position 5 of 12 (test_small_fused_gpu's singular
    case: handled, reported through info).  gr_int_dev behind a delay: info is non-zero at 5 only, also in a second call
    with weight 0 there (what test_inverse_cells_gpu asserts of it), whose result equals the host-pointer form's bit
    for bit and, wherever it is finite, the sum of the other eleven energies, G(E) = S^-1 / (E - 1)."""
    t = priv.torch
    eng = priv.eng
    m, at = 12, 5
    _, S = random_system(n, 7)
    eng.set_batch(16)                                   # (above the 12 energies: one sweep, nothing is cut)
    eng.set_system(S, S)
    h = eng.sigma_precomputed(np.zeros((m, n, n), dtype=complex))
    try:
        E = np.linspace(-1.5, 2.5, m) + 0.1j
        E[at] = 1.0 + 0j
        w = (np.cos(np.arange(m)) + 1.5) * (1 + 0.2j)
        w0 = w.copy(); w0[at] = 0.0
        only = np.zeros(m, dtype=bool); only[at] = True
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ref, ref0 = _f64(eng.gr_int(h, E, w)).copy(), _f64(eng.gr_int(h, E, w0)).copy()
        Ed, wd, w0d = priv.tensor(E), priv.tensor(w), priv.tensor(w0)
        out = priv.empty(2 * n * n)
        with t.cuda.stream(priv.s):
            eng.gr_int_dev(h, m, Ed.data_ptr(), wd.data_ptr(), out.data_ptr())           # warm
            priv.s.synchronize()
            for tag, wt, want in (("all weights", wd, ref), ("weight 0 at the singular energy", w0d, ref0)):
                out.fill_(0.0)
                priv.sleep()
                busy, ms = priv.timed(("f", n, tag), lambda: eng.gr_int_dev(h, m, Ed.data_ptr(), wt.data_ptr(), out.data_ptr()), True)
                assert busy, (n, tag, ms)
                info = eng.last_info_dev(m)                                              # waits for the stream itself
                assert priv.s.query()
                assert np.array_equal(info != 0, only), (n, tag, info)
                got = out.cpu().numpy()
                assert _same(got, want), (n, tag)
                nan = int(np.isnan(got).sum())
                print(f"STREAM singular n={n}, {tag}: {nan} of {got.size} values are NaN")
                if tag.startswith("all"):
                    assert nan > 0
        rest = sum(w0[k] / (E[k] - 1.0) for k in range(m) if k != at) * np.linalg.inv(S)
        fin = np.isfinite(got)
        assert np.allclose(got[fin], _f64(rest)[fin], rtol=0, atol=1e-8 * np.abs(rest).max())
    finally:
        eng.sync()
        eng.sigma_free(h)


def test_zz_the_delay_covers_the_slowest_asynchronous_call(priv):
    """The delay must exceed the host time of the slowest asynchronous call of this run by a factor of three: otherwise
    'the stream was still busy after the call' proves nothing about a shorter one."""
    assert priv.delay_ms >= 10.0, priv.delay_ms
    if not priv.host_ms:
        return
    worst = max(priv.host_ms, key=priv.host_ms.get)
    print(f"STREAM delay {priv.delay_ms:.2f} ms; slowest asynchronous call on the host: {priv.host_ms[worst]:.3f} ms {worst}; "
          f"median {np.median(list(priv.host_ms.values())):.3f} ms over {len(priv.host_ms)} calls")
    assert priv.delay_ms >= 3.0 * priv.host_ms[worst], (priv.delay_ms, worst, priv.host_ms[worst])
