"""
The launch rule of the chain fixed-point kernels (k_chain1d_rs.hip, chain1d_rs_launch): a launch with more fixed points
than resident slots runs from the job queue (round robin) whether or not the provider has learned an order, and takes
no order; a launch that fits the chip runs the plain kernel in the predicted order; negf_set_chain_round_robin(0, ..)
forces the plain kernel.  A fixed point is a sequence of sweeps on its own data, so the schedule changes no bit of Sigma,
of the sweep counts or of the convergence flags: every comparison here is array_equal against the forced plain launch.
"""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from helpers import chain_lead, random_system, swept

pytestmark = pytest.mark.gpu

MAX_ITER = 300          # the sweep cap of these providers (above the default quantum of 100 sweeps: the queue has a ring)
SLOTS = 5               # set_chain_round_robin(-1, 5): the 24-job launches below are oversubscribed
M = 12                  # energies (x 2 contacts = 24 jobs)
SHAPES = [(50, 50), (35, 35), (19, 9), (20, 20)]    # strip classes 51, 35; unequal contacts (class 25); a class without strips


def _grid(shift=0.0):
    E = np.linspace(-1.6, 1.5, M) + shift + 0.0j
    E[1] += 0.05j; E[4] += 1.0j; E[M // 2] += 0.2j; E[9] += 3.0j    # (off the axis: fixed points of ~20 to ~150 sweeps)
    return E


class _System:
    """F, S and the lead blocks of one shape; provider() lowers a FRESH chain provider with the 300-sweep cap.
    Mixing factor 0.5: a well-damped energy converges in ~20 sweeps (the default 0.1 needs 110 at the least), the
    energies on the axis inside the band run to the cap."""
    def __init__(self, engine, ncL, ncR, eta=1e-3):
        self.engine = engine
        N = ncL + ncR + 9
        self.F, self.S = random_system(N, 500 + ncL)
        self.inds = [list(range(ncL)), list(range(N - ncR, N))]
        aL = chain_lead(ncL, 501 + ncL); aR = chain_lead(ncR, 502 + ncL)
        self.args = ([aL[0], aR[0]], [aL[1], aR[1]], [aL[2], aR[2]], [aL[3], aR[3]],
                     [aL[2].copy(), aR[2].copy()], [aL[3].copy(), aR[3].copy()], eta, 1e-5, 0.5)
        self.handles = []
        engine.set_system(self.F, self.S)

    def provider(self, max_iter=MAX_ITER):
        h = self.engine.sigma_chain1d(self.inds, *self.args, max_iter=max_iter)
        self.handles.append(h)
        return h

    def sigma(self, h, E):
        eng = self.engine
        sig = eng.sigma_eval(h, None, E, 2)
        return sig, eng.last_iters.copy(), eng.last_converged.copy()

    def free(self):
        for h in self.handles:
            self.engine.sigma_free(h)


@pytest.fixture
def rule(engine):
    engine.set_chain_cache(0)                      # every evaluation runs its fixed points
    systems = []

    def make(ncL, ncR):
        systems.append(_System(engine, ncL, ncR))
        return systems[-1]
    yield make
    for s in systems:
        s.free()
    engine.set_batch(0)
    engine.set_chain_round_robin(-1, 0)
    engine.set_chain_cache(512)


def _same(got, ref, what):
    for a, b, name in zip(got, ref, ("Sigma", "sweep counts", "flags")):
        assert np.array_equal(a, b), (what, name)


@pytest.mark.parametrize("ncL,ncR", SHAPES)
def test_default_rule_equals_forced_plain(rule, engine, ncL, ncR):
    """Three evaluations by one provider under the default quantum on 5 slots -- the queue without an order, then twice
    with an order learned -- equal the forced plain launch; so does GrInt, straight and through the g(E) cache."""
    s = rule(ncL, ncR)
    E = _grid(); w = np.full(M, 3.1 / M) + 0j
    engine.set_chain_round_robin(0, 0)
    h0 = s.provider()
    ref = s.sigma(h0, E)
    it0 = ref[1]
    print(f"n_c = ({ncL}, {ncR}): sweep counts {it0.min()} .. {it0.max()}")
    assert it0.max() == MAX_ITER and it0.min() < MAX_ITER // 3, "job lengths from tens of sweeps to the cap"
    gref = engine.gr_int(s.provider(), E, w)
    engine.set_chain_round_robin(-1, SLOTS)
    h = s.provider()
    for rep in range(3):
        _same(s.sigma(h, E), ref, f"evaluation {rep}")
    assert np.array_equal(engine.gr_int(s.provider(), E, w), gref), "GrInt"
    engine.set_chain_cache(512); engine.chain_cache_clear()
    hc = s.provider()
    hits = engine.chain_cache_stats()["hits"]
    assert np.array_equal(engine.gr_int(hc, E, w), gref), "GrInt filling the cache"
    assert np.array_equal(engine.gr_int(hc, E, w), gref), "GrInt from the cache"
    assert engine.chain_cache_stats()["hits"] > hits


@pytest.mark.parametrize("ncL,ncR", [(50, 50), (19, 9)])
def test_default_rule_chunked(rule, engine, ncL, ncR):
    """The grid in two chunks of 6 energies (12 jobs each on 5 slots; the second chunk reaches the order record at
    m0 = 6), the same grid again, then the grid moved by a small shift: every evaluation equals the forced plain launch
    of the whole grid by a fresh provider."""
    s = rule(ncL, ncR)
    engine.set_chain_round_robin(-1, SLOTS)
    h = s.provider()
    for shift in (0.0, 0.0, 0.013, 0.0):
        E = _grid(shift)
        engine.set_batch(0); engine.set_chain_round_robin(0, 0)
        ref = s.sigma(s.provider(), E)
        engine.set_batch(6); engine.set_chain_round_robin(-1, SLOTS)
        got = s.sigma(h, E)
        swept(engine, 6, M)
        _same(got, ref, f"shift {shift}")


_CHILD = """
    import os, sys
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import numpy as np
    from gaunegf_amd.engine import get_engine
    from test_chain_launch_rule_gpu import _System, _grid
    eng = get_engine(); eng.set_chain_cache(0)
    s = _System(eng, 20, 20)
    E = _grid()
    for tag, slots, max_iter in (("oversubscribed", 5, 300), ("fits", 0, 300), ("no-ring", 5, 50)):
        eng.set_chain_round_robin(-1, slots)
        h = s.provider(max_iter)
        for rep in range(3):
            os.write(2, f"[case] {tag} {rep}\\n".encode())
            s.sigma(h, E)
    s.free()
    print("ok")
"""


def test_launch_rule_log():
    """What the launcher logs (NEGF_CHAIN_LOG, read once per process: a fresh child) for three evaluations by one provider:
    24 jobs on 5 slots run from the queue and take no order, every time; on the whole chip (24 jobs fit) the plain kernel,
    in the predicted order from the second evaluation on; with a sweep cap below the quantum (no ring) the plain kernel."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = textwrap.dedent(_CHILD) % (os.path.dirname(here), here)
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code]
    r = subprocess.run(cmd, env=dict(os.environ, NEGF_CHAIN_LOG="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
    seen = {}
    case = None
    for line in r.stderr.splitlines():
        m = re.match(r"\[case\] (\S+) (\d)", line)
        if m:
            case = (m.group(1), int(m.group(2))); seen[case] = []
            continue
        m = re.match(r"\[chain launch\] jobs (\d+) slots (\d+) quantum (\d+) order (\d) gc_mode (\d)", line)
        if m and case:
            seen[case].append(tuple(int(x) for x in m.groups()))
    assert len(seen) == 9 and all(len(v) == 1 for v in seen.values()), seen
    for rep in range(3):
        jobs, slots, quantum, order, _ = seen[("oversubscribed", rep)][0]
        assert (jobs, slots) == (24, 5) and quantum > 0 and order == 0, (rep, seen)
        jobs, slots, quantum, order, _ = seen[("fits", rep)][0]
        assert jobs == 24 and slots >= 24 and quantum == 0 and order == (1 if rep else 0), (rep, seen)
        jobs, slots, quantum, order, _ = seen[("no-ring", rep)][0]
        assert (jobs, slots) == (24, 5) and quantum == 0, (rep, seen)
