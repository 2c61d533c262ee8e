"""The layered path through the windowed inverse at a FOREIGN stride, on the MI355X.  The layered system strides every
layer's matrices by nmax^2, so in rgf_ref.window_case() (layers of 40, 257 and 300 orbitals) the 257 layer runs the
windowed kernels -- window kernels, column updates, the fused update of a pair, the gather, the side-stream groups --
at a stride that is not n * n.  The case's four truth energies sit first, last and at the group boundaries of a batch of
nb well-conditioned fillers (E + 0.05j), one in every stream group, with engine.set_batch(nb):
  nb = 4     one group, the look-ahead team kernel la<16,8,12>, fat updates
  nb = 255   groups of 64, 64, 64, 63: the lean strip kernel three times, la<16,8,12> once
  nb = 344   the smallest batch whose groups all run the 257 layer's windows in pairs (fused update on side streams)
What Engine.inverse_plan says of every layer is asserted, and that the last inverse launched matches one of them.
Bars: rgf_ref.bar / rgf_less_ref.bar (C_RGF, C_LESS times the larger error of the two float64 sweeps, as calibrated),
PROJECT_BAR against the dense engine."""
import functools
import warnings

import numpy as np
import pytest

import rgf_less_ref as lr
import rgf_ref as rr

pytestmark = pytest.mark.gpu

S512, LA12, SINGLE = 5, 8, 10
NBS = (4, 255, 344)
# nb -> (counts, window kernels, pairs) of the two windowed layers (257 and 300: five windows each)
EXPECT = {4: ([4], [LA12], [0]),
          255: ([64, 64, 64, 63], [S512] * 3 + [LA12], [0] * 4),
          344: ([86] * 4, [S512] * 4, [1] * 4)}


def _positions(plan, nb):
    """where the four truth energies go: one per stream group, at the first and last position of the batch and on
    either side of a group boundary"""
    g = plan["groups"]
    if len(g) == 1:
        return [0, nb // 3, 2 * nb // 3, nb - 1] if nb > 4 else list(range(4))
    assert len(g) == 4
    return [0, g[1]["first"], g[3]["first"] - 1, nb - 1]


@functools.lru_cache(maxsize=None)
def _batch(nb):
    from gaunegf_amd.engine import Engine
    c = rr.window_case()
    plans = [Engine.inverse_plan(n, nb) for n in c.sizes]
    assert plans[0]["path"] == 1 and [g["wk"] for g in plans[0]["groups"]] == [SINGLE]
    counts, wk, pairs = EXPECT[nb]
    for n, p in zip(c.sizes[1:], plans[1:]):
        got = ([g["count"] for g in p["groups"]], [g["wk"] for g in p["groups"]], [g["pairs"] for g in p["groups"]])
        assert p["path"] == 2 and p["cls"] == (16, 1) and p["nblk"] == 5 and got == (counts, wk, pairs), (n, nb, got)
    if nb == 344:                        # ... and no smaller batch has every group of the 257 layer in pairs
        assert not all(g["pairs"] for g in Engine.inverse_plan(257, 343)["groups"])
    pos = _positions(plans[1], nb)
    E = (np.linspace(-1.0, 1.0, nb) + 0.05j).astype(complex)
    E[pos] = c.energies
    return c, plans, pos, E


def _bind(eng, c):
    h = eng.layered_create(c.F_diag, c.F_up, c.S_diag, c.S_up)
    tl = eng.layered_terminal_const(h, 0, c.left, c.sig_left)
    tr = eng.layered_terminal_const(h, len(c.sizes) - 1, c.right, c.sig_right)
    assert (tl, tr) == (0, 1)
    return h


def _flat(split):
    d, u, l = split
    return np.concatenate([b.ravel() for b in d + u + l])


def _last_is_planned(eng, plans):
    last = eng.inverse_last()
    assert last in [{"path": p["path"], "masks": [g["mask"] for g in p["groups"]]} for p in plans], last
    return last


@pytest.mark.parametrize("nb", NBS)
def test_truth_and_dense_parity(engine, nb):
    """T, dos and pdos at the four truth positions within rr.bar; all nb energies within PROJECT_BAR of the dense engine"""
    c, plans, pos, E = _batch(nb)
    ent = rr.window_truth()
    engine.set_batch(nb)
    try:
        h = _bind(engine, c)
        try:
            T = engine.layered_transmission(h, 1, 0, E)
            last = _last_is_planned(engine, plans)
            tot, dos = engine.layered_dos(h, E)
            ptot, pdos = engine.layered_dos(h, E, mulliken=True)
        finally:
            engine.layered_free(h)
        F, S = c.to_dense()
        engine.set_system(F, S)
        sl = np.zeros((c.N, c.N), complex); sl[np.ix_(c.left_global, c.left_global)] = c.sig_left
        sr = np.zeros((c.N, c.N), complex); sr[np.ix_(c.right_global, c.right_global)] = c.sig_right
        hd = engine.sigma_const([sl, sr])
        try:
            Td = engine.transmission(hd, 1, 0, E)
            totd, dosd = engine.dos(hd, E)
            pdd = engine.population(hd, engine.RETARDED, E, rows=True)
        finally:
            engine.sigma_free(hd)
    finally:
        engine.set_batch(0)
    got = dict(T=T[pos], dos=dos[pos], pdos=pdos[pos])
    res = []
    for k in ent["keys"]:
        err, bar = rr.rel_err(got[k], ent["truth"][k]), rr.bar(ent, k)
        print(f"ACC rgf cell nb={nb} {k:5s} err {err:.3g} bar {bar:.3g} ratio {err / bar:.3g} (lr {ent['err_lr'][k]:.3g}, "
              f"rl {ent['err_rl'][k]:.3g}); last inverse launched {[hex(m) for m in last['masks']]}")
        res.append((k, err, bar))
    for k, err, bar in res:
        assert err <= bar, (nb, k, err, bar)
    assert np.allclose(tot, dos.sum(axis=1), rtol=1e-13, atol=0) and np.allclose(ptot, pdos.sum(axis=1), rtol=1e-13, atol=0)
    par = dict(T=rr.rel_err(T, Td), dos=rr.rel_err(dos, dosd), dos_tot=rr.rel_err(tot, totd), pdos=rr.rel_err(pdos, pdd))
    print(f"ACC rgf cell nb={nb} parity with the dense engine over all {nb} energies: " +
          ", ".join(f"{k} {v:.3g}" for k, v in par.items()))
    assert max(par.values()) <= rr.PROJECT_BAR, par


@pytest.mark.parametrize("nb", NBS)
def test_one_hot_weights_return_one_energy(engine, nb):
    """layered_gr_int and layered_gless_int (all terminals) with a weight vector that is 1 at a truth position and 0
    elsewhere: the blocks of that energy alone, within the bar of that energy alone"""
    c, plans, pos, E = _batch(nb)
    ent, less = rr.window_truth(), lr.window_entry("LR")
    res = []
    engine.set_batch(nb)
    try:
        h = _bind(engine, c)
        try:
            for j, p in enumerate(pos):
                w = np.zeros(nb, dtype=complex)
                w[p] = 1.0
                g = _flat(engine.layered_gr_int(h, E, w))
                _last_is_planned(engine, plans)
                res.append(("gr_int", j, rr.rel_err(g, ent["truth"]["single"][j]), rr.bar_single(ent, j)))
                a = _flat(engine.layered_gless_int(h, None, E, w))
                res.append(("gless_int", j, rr.rel_err(a, less["truth"]["single"][j]), lr.bar_single(less, j)))
        finally:
            engine.layered_free(h)
    finally:
        engine.set_batch(0)
    for what, j, err, bar in res:
        print(f"ACC rgf cell nb={nb} {what:9s} one-hot at position {pos[j]} (energy {j}) err {err:.3g} bar {bar:.3g} "
              f"ratio {err / bar:.3g}")
    for what, j, err, bar in res:
        assert err <= bar, (nb, what, j, err, bar)


def test_a_singular_layer_in_the_third_stream_group(engine):
    """A decoupled 257 layer with F = 0, S = 1 behind the 300 layer of the window case (stride 300^2), 48 energies in four
    stream groups of 12 and E = 0 at position 30: info is non-zero there only, and NaN appears there only."""
    nb, at = 48, 30
    c = rr.window_case()
    plan = engine.inverse_plan(257, nb)
    assert [(g["first"], g["count"]) for g in plan["groups"]] == [(0, 12), (12, 12), (24, 12), (36, 12)]
    assert plan["groups"][2]["first"] <= at < plan["groups"][3]["first"]
    Fd = [c.F_diag[2], np.zeros((257, 257))]
    Sd = [c.S_diag[2], np.eye(257)]
    Fu = [np.zeros((300, 257))]
    E = (np.linspace(-1.0, 1.0, nb) + 0.05j).astype(complex)
    E[at] = 0.0
    only = np.zeros(nb, dtype=bool)
    only[at] = True
    engine.set_batch(nb)
    try:
        h = engine.layered_create(Fd, Fu, Sd, Fu)
        try:
            engine.layered_terminal_const(h, 0, c.left, c.sig_left)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                tot, site = engine.layered_dos(h, E)
                info_dos = np.array(engine.last_info[:nb])
                last = engine.inverse_last()
                P = _flat(engine.layered_gr_int(h, E, np.ones(nb)))
                info_int = np.array(engine.last_info[:nb])
        finally:
            engine.layered_free(h)
    finally:
        engine.set_batch(0)
    assert last == {"path": 2, "masks": [g["mask"] for g in plan["groups"]]}, last
    assert np.array_equal(info_dos != 0, only) and np.array_equal(info_int, info_dos), (info_dos, info_int)
    assert np.array_equal(np.isnan(site).any(axis=1), only) and np.array_equal(np.isnan(tot), only)
    assert np.all(np.isfinite(site[~only]))
    # the healthy layer-1 block is 1 / E on the diagonal: -Im / pi of it, exactly decoupled from layer 0
    k = at + 1
    assert np.allclose(site[k, 300:], -np.imag(1.0 / E[k]) / np.pi, rtol=1e-12, atol=0)
    assert np.all(np.isnan(P))
