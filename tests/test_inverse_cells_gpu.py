"""
Every cell of the blocked inverse's launch rule under the AUTOMATIC rule, held to the conditioning bar of tests/xprec.py
(||G_hat e_j - G e_j|| / ||G e_j|| <= C_BAR sqrt(n) u kappa_2(A) on every sampled column).  A cell is a shape (n, nb)
and what the rule does with it: single workgroup or windows, the class, the stream groups, the window kernel of each
group, windows in pairs or one by one, fat or lean column updates, gather or the un-gathered form that GrInt reads.
For each cell the test
  1. asserts through Engine.inverse_plan that the shape reaches the cell,
  2. runs one batch of nb energies (engine.set_batch(nb)),
  3. asserts that Engine.inverse_last -- one bit per launch site, set next to the launch -- equals the plan,
  4. checks the results: the six ladder energies of xprec.ladder(n) sit first, last and on either side of every group
     boundary (every group carries one of the three ill-conditioned ones) and must be within the bar; a seeded sample
     of eight well-conditioned fillers must satisfy ||G A - I|| / sqrt(n) < 1e-9; a ladder energy placed a second time
     gives bitwise the same result wherever the plan launches the same kernels for both groups.
Batches above 300 MB are not downloaded: their G(E_p) are read through GrInt with a weight vector that is 1 at p and 0
elsewhere -- the un-gathered launch_accumulate_perm path.
Lines 'ACC cell ...' report plan, launch record and the worst ratio of each cell.
"""
import functools
import warnings

import numpy as np
import pytest

import xprec
from helpers import random_system, rel_fro
from xprec import Truth

pytestmark = pytest.mark.gpu

xprec.require_extended()

S256, S512, S1024, LA12, TEAM, SINGLE = 1, 5, 6, 8, 9, 10
DOWNLOAD_MAX = 300e6                 # bytes of a batch of G above which GrBatch is not used
TOL = 1e-8

# (n, nb, name, path, class, counts, window kernels, pairs, update waves over all other blocks, of a pair's single blocks)
CELLS = [
    (100, 256, "single workgroup", 1, (0, 0), [256], [SINGLE], [0], [0], [0]),
    (100, 257, "small windowed: 4 groups, 32-wide strip, 2 windows, fat", 2, (16, 1), [65, 65, 65, 62], [S256] * 4, [0] * 4, [8] * 4, [0] * 4),
    (208, 257, "small windowed with a ragged fourth window", 2, (16, 1), [65, 65, 65, 62], [S256] * 4, [0] * 4, [8] * 4, [0] * 4),
    (257, 6, "one group, la<16,8,12>, fat", 2, (16, 1), [6], [LA12], [0], [8], [0]),
    (257, 255, "mixed: lean strip x 3, la<16,8,12> x 1", 2, (16, 1), [64, 64, 64, 63], [S512] * 3 + [LA12], [0] * 4, [8] * 4, [0] * 4),
    (257, 344, "pairs on side streams, fat single-block updates, lean odd last window", 2, (16, 1), [86] * 4, [S512] * 4, [1] * 4, [4] * 4, [8] * 4),
    (257, 401, "lean by nb * nblk > 2000", 2, (16, 1), [101, 101, 101, 98], [S512] * 4, [1] * 4, [4] * 4, [4] * 4),
    (513, 37, "three uneven groups, 8-wave strip", 2, (16, 2), [13, 13, 11], [S1024] * 3, [0] * 3, [8] * 3, [0] * 3),
    (513, 148, "pairs at RPT = 2", 2, (16, 2), [37] * 4, [S1024] * 4, [1] * 4, [4] * 4, [8] * 4),
    (513, 641, "gj_window_kernel<16,2> x 3, strip x 1", 2, (16, 2), [161, 161, 161, 158], [TEAM] * 3 + [S1024], [1] * 4, [4] * 4, [4] * 4),
    (900, 6, "strip by n >= 900", 2, (16, 2), [6], [S1024], [0], [8], [0]),
    (1025, 25, "<8,4>, two groups", 2, (8, 4), [13, 12], [TEAM] * 2, [0] * 2, [8] * 2, [0] * 2),
]


@functools.lru_cache(maxsize=None)
def _ladder(n):
    """(case, truth, provider) of the ladder system at dimension n, once per module."""
    from gaunegf_amd.surfGTester import surfGTest
    case = xprec.ladder(n)
    g = surfGTest(case.F, case.S, case.inds, -1j * xprec.GAMMA)
    assert all(np.array_equal(a, b) for a, b in zip(g.sig, case.sigs))
    return case, Truth(case), g


def _kern(group):
    return tuple(group[k] for k in ("wk", "pairs", "upd_full", "upd_single"))


def _place(plan, nb):
    """{position: ladder index}: first, last and either side of every group boundary, filled up to six positions (eight
    with several groups) from inside the groups.  The first position of every group takes one of the ill-conditioned
    energies (4: on the resonance, 3: 1e-8 off, 2: 1e-5 off) -- the first two groups for which the plan launches the
    same kernels both take 4, the pair whose results must agree bitwise --, then every ladder energy not placed yet
    goes in, and what is left takes further copies of the ill-conditioned ones."""
    groups = plan["groups"]
    pos = {0, nb - 1}
    for g in groups[1:]:
        pos |= {g["first"] - 1, g["first"]}
    want = 6 if len(groups) == 1 else 8
    fill = [g["first"] + g["count"] * k // 4 for k in (2, 1, 3) for g in groups] + list(range(nb))
    for p in fill:
        if len(pos) >= min(want, nb):
            break
        pos.add(p)
    pos = sorted(pos)
    gid = lambda p: max(i for i, g in enumerate(groups) if g["first"] <= p)
    twin = next(((a, b) for a in range(len(groups)) for b in range(a + 1, len(groups))
                 if _kern(groups[a]) == _kern(groups[b])), ())
    others = iter((3, 2, 4, 3, 2) if twin else (4, 3, 2, 4))
    assign = {}
    for i in range(len(groups)):
        assign[next(q for q in pos if gid(q) == i)] = 4 if i in twin else next(others)
    rest = [p for p in pos if p not in assign]
    for k in (4, 3, 2, 1, 0, 5):
        if k not in assign.values():
            assign[rest.pop(0)] = k
    for p in rest:
        assign[p] = min((3, 2, 4), key=lambda k: sum(1 for v in assign.values() if v == k))
    return assign, gid


def _one_hot(F, S, g, E, p):
    from gaunegf_amd.integrate import GrInt
    w = np.zeros(E.size, dtype=np.complex128)
    w[p] = 1.0
    return GrInt(F, S, g, E, w)


def _masks(plan):
    return [g["mask"] for g in plan["groups"]]


def _names(engine, plan):
    return "+".join(engine.INVERSE_WINDOW_KERNELS[g["wk"]] for g in plan["groups"])


@pytest.mark.parametrize("n,nb,name,path,cls,cnt,wk,pairs,full,single", CELLS, ids=[f"{c[0]}x{c[1]}" for c in CELLS])
def test_cell_against_the_conditioning_bar(engine, n, nb, name, path, cls, cnt, wk, pairs, full, single):
    from gaunegf_amd.integrate import GrBatch
    plan = engine.inverse_plan(n, nb)
    got = (plan["path"], plan["cls"], [g["count"] for g in plan["groups"]], [g["wk"] for g in plan["groups"]],
           [g["pairs"] for g in plan["groups"]], [g["upd_full"] for g in plan["groups"]],
           [g["upd_single"] for g in plan["groups"]])
    assert got == (path, cls, cnt, wk, pairs, full, single), (name, got)
    case, t, g = _ladder(n)
    assign, gid = _place(plan, nb)
    assert set(assign.values()) == set(range(6)) and {gid(p) for p in assign} == set(range(len(cnt)))
    assert all(any(assign[p] in (2, 3, 4) for p in assign if gid(p) == i) for i in range(len(cnt)))
    E = np.linspace(-2.5, 2.5, nb) + 0.02j
    for p, k in assign.items():
        E[p] = case.energies[k]
    rng = np.random.default_rng(1000 * n + nb)
    free = np.array([p for p in range(nb) if p not in assign])
    fillers = [int(p) for p in rng.choice(free, min(8, free.size), replace=False)] if free.size else []
    sig = case.sig_tot
    kern = lambda p: _kern(plan["groups"][gid(p)])
    forms = []
    if 16.0 * n * n * nb <= DOWNLOAD_MAX:
        forms.append("GrBatch")
    if 16.0 * n * n * nb > DOWNLOAD_MAX or (n, nb) == (257, 255):
        forms.append("GrInt")
    engine.set_batch(nb)
    try:
        for form in forms:
            if form == "GrBatch":
                G = GrBatch(case.F, case.S, g, E)
                last, want = engine.inverse_last(), plan
                get = lambda p: G[p]
            else:
                want = engine.inverse_plan(n, nb, defer=True)
                if want["deferred"]:
                    print(f"ACC cell n={n} nb={nb}: {16.0 * n * n * nb / 1e6:.0f} MB of G are not downloaded: the gather is "
                          f"deferred, G(E_p) read through GrInt with one-hot weights")
                cache = {}
                def get(p, cache=cache):
                    if p not in cache:
                        cache[p] = _one_hot(case.F, case.S, g, E, p)
                    return cache[p]
                get(next(iter(assign)))
                last = engine.inverse_last()
            assert last == {"path": want["path"], "masks": _masks(want)}, (name, form, last, _masks(want))
            ratios = {p: t.ratio(k, get(p)) for p, k in assign.items()}
            res = []
            for p in fillers:
                A = E[p] * case.S - case.F - sig
                res.append(np.linalg.norm(get(p) @ A - np.eye(n)) / np.sqrt(n))
            print(f"ACC cell n={n} nb={nb} [{name}] {form}: plan path {plan['path']} class {plan['cls']} groups {cnt} "
                  f"kernels {_names(engine, plan)} masks {[hex(m) for m in _masks(want)]}; launched "
                  f"{[hex(m) for m in last['masks']]}; worst ratio {max(ratios.values()):.3g} "
                  f"(ladder index {assign[max(ratios, key=ratios.get)]}), worst filler residual {max(res, default=0.0):.3g}")
            bad = {p: r for p, r in ratios.items() if not r <= 1.0}
            assert not bad, (name, form, bad)
            assert all(r < 1e-9 for r in res), (name, form, res)
            # second copies: bitwise where the plan launches the same kernels for both groups
            twins = 0
            for k in range(6):
                ps = [p for p in assign if assign[p] == k]
                for q in ps[1:]:
                    if gid(q) != gid(ps[0]) and kern(q) == kern(ps[0]):
                        assert np.array_equal(get(q), get(ps[0])), (name, form, k, ps[0], q)
                        twins += 1
            assert twins >= 1 or len({kern(p) for p in assign}) == len(cnt), (name, "no second copy in a group of the same kernels")
    finally:
        engine.set_batch(0)


class _Probe:
    """Sigma = 0, or NaN in column 3 at E = 1 (the provider of test_singular_and_nan_matrices_by_window_kernel)."""

    def __init__(self, n, bad):
        self.n, self.bad = n, bad

    def sigmaTot(self, E):
        z = np.zeros((self.n, self.n), dtype=complex)
        if self.bad == "nan" and abs(E - 1.0) < 1e-12:
            z[:, 3] = np.nan
        return z

    def sigma(self, E, i):
        return np.zeros((self.n, self.n), dtype=complex)


@pytest.mark.parametrize("bad", ["singular", "nan"])
def test_singular_and_nan_in_a_later_stream_group(engine, bad):
    """n = 257, nb = 48: four stream groups of 12, the bad matrix at position 30, in the third.  Its info goes through
    the group's offsets (info + first, piv + first * 2 n).  GrBatch: G[30] all NaN, info non-zero at 30 only, the
    neighbours and the ends untouched.  GrInt with all weights 1 (the un-gathered form): every entry NaN, the same info.
    GrInt with weight 0 at the bad energy is not required to be finite and is not: on the MI355X all 66049 entries are
    NaN, for the singular and for the NaN matrix -- the bad matrix counts as NaN in the un-gathered sum whatever its
    weight (0 x NaN), exactly as its NaN-filled gathered form would.  Printed, not asserted; info is as before."""
    from gaunegf_amd.integrate import GrBatch, GrInt
    n, nb, at = 257, 48, 30
    plan = engine.inverse_plan(n, nb)
    assert [(g["first"], g["count"]) for g in plan["groups"]] == [(0, 12), (12, 12), (24, 12), (36, 12)]
    assert plan["groups"][2]["first"] <= at < plan["groups"][3]["first"]
    S = np.eye(n)
    F = np.eye(n) if bad == "singular" else random_system(n, 7)[0]
    E = np.linspace(0.5, 2.0, nb) + 0.1j
    E[at] = 1.0 + 0j
    probe = _Probe(n, bad)
    only = np.zeros(nb, dtype=bool)
    only[at] = True
    engine.set_batch(nb)
    try:
        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            G = GrBatch(F, S, probe, E)
        info = np.array(engine.last_info[:nb])
        assert engine.inverse_last() == {"path": 2, "masks": [g["mask"] for g in plan["groups"]]}
        assert np.all(np.isnan(G[at])), bad
        assert np.array_equal(info != 0, only), info
        for k in (0, at - 1, at + 1, nb - 1):
            ref = np.linalg.inv(E[k] * S - F)
            assert rel_fro(G[k], ref) < TOL, (bad, k, rel_fro(G[k], ref))
        deferred = engine.inverse_plan(n, nb, defer=True)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            P = GrInt(F, S, probe, E, np.ones(nb, dtype=complex))
        assert engine.inverse_last() == {"path": 2, "masks": [g["mask"] for g in deferred["groups"]]}
        assert np.all(np.isnan(P)) and any("singular" in str(r.message) for r in rec), bad
        assert np.array_equal(np.array(engine.last_info[:nb]) != 0, only)
        w0 = np.ones(nb, dtype=complex)
        w0[at] = 0.0
        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            P0 = GrInt(F, S, probe, E, w0)
        print(f"ACC cell n={n} nb={nb} {bad} at {at}, GrInt with weight 0 there: {int(np.isnan(P0).sum())} of {P0.size} "
              f"entries are NaN")
        assert np.array_equal(np.array(engine.last_info[:nb]) != 0, only)
    finally:
        engine.set_batch(0)
