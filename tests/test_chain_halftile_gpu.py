"""
The half-tile updates of the chain kernels' small inverse (chain_rs_inverse.h, rs_half_strips): with panels of 8 columns
the look-ahead, the other half of the panel's own column tile and the other half of the next tile update 8 columns of
a 16-column tile, as two 16 x 4 column strips on the 4x4x4 matrix instruction.  Which of them a sweep runs, and where
the ragged last panel falls back to the whole tile, depends on n_c alone, so the sizes are swept one by one:
  * every n_c from 9 to 64 (every pitch class, every position of the last panel), two contacts, 0 and 3 sweeps:
    Sigma and g against the oracle at the tolerance of test_chain1d_fixed_trip_count, and the doubling solver
    (k_chain1d_rd.hip shares the inverse) on the same leads against its float64 restatement at that solver's tolerance;
  * contacts of unequal size whose kernels differ in class, and a free-running C3-like lead (sweep counts +- 1);
  * a lead with an exactly zero column and one with a NaN entry -- the factoring wave's "no usable candidate" path --
    as properties: the unit reports converged = 0 and a non-finite block, the other units of the launch are what they
    are in a launch without the bad unit, bit for bit.
"""
import numpy as np
import pytest

import oracle
import xprec_chain as xc
import xprec_rd as xr
from helpers import chain_lead, random_system, rel_fro

pytestmark = pytest.mark.gpu

TOL_FIXED = 1e-10                     # test_gpu_parity.test_chain1d_fixed_trip_count
TOL_RD = 1e-8                         # test_chain_rd_gpu.TOL
ETA = 1e-4


def _system(ncL, ncR, seed, eta=ETA, leads=None, solver=None):
    """(device provider, oracle provider, index lists, the two leads) of a device with two chain contacts."""
    from gaunegf_amd.surfG1D import surfG
    N = ncL + ncR + 7
    F, S = random_system(N, seed)
    inds = [list(range(ncL)), list(range(N - ncR, N))]
    aL, aR = leads or (chain_lead(ncL, seed + 1), chain_lead(ncR, seed + 2))
    taus = [aL[2].copy(), aR[2].copy()]; staus = [aL[3].copy(), aR[3].copy()]
    kw = dict(taus=taus, staus=staus, alphas=[aL[0], aR[0]], aOverlaps=[aL[1], aR[1]],
              betas=[aL[2], aR[2]], bOverlaps=[aL[3], aR[3]], eta=eta)
    g_dev = surfG(F, S, inds, **kw) if solver is None else surfG(F, S, inds, solver=solver, **kw)
    g_ref = oracle.Chain1DSigma(F, S, inds, taus, staus, [aL[0], aR[0]], [aL[1], aR[1]], [aL[2], aR[2]],
                                [aL[3], aR[3]], eta=eta)
    return g_dev, g_ref, inds, (aL, aR)


def _check_fixed_trips(ncL, ncR, seed, sweeps):
    g_dev, g_ref, inds, _ = _system(ncL, ncR, seed)
    g_dev.force_iters = sweeps; g_ref.force_iters = sweeps
    Es = np.array([0.3, 0.1 + 0.2j])
    tot, its, _ = g_dev.sigma_batch(Es)
    assert np.all(its == sweeps)
    for c in (0, 1):
        sig = g_dev.sigma_batch(Es, c)[0]
        for m, E in enumerate(Es):
            E = complex(E)
            assert rel_fro(sig[m], g_ref.sigma(E, c)) < TOL_FIXED, (ncL, ncR, sweeps, c, E)
            gi = oracle.chain1d_g(E, g_ref.aList[c], g_ref.aSList[c], g_ref.bList[c], g_ref.bSList[c], ETA,
                                  force_iters=sweeps)[0]
            assert rel_fro(g_dev.g(E, c), gi) < TOL_FIXED, (ncL, ncR, sweeps, c, E)
    for m, E in enumerate(Es):
        assert rel_fro(tot[m], g_ref.sigmaTot(complex(E))) < TOL_FIXED, (ncL, ncR, sweeps, E)


@pytest.mark.parametrize("sweeps", [0, 3])
@pytest.mark.parametrize("nc", list(range(9, 65)))
def test_every_size_fixed_trip_count(engine, nc, sweeps):
    _check_fixed_trips(nc, nc, 300 + nc, sweeps)


@pytest.mark.parametrize("nc", list(range(9, 65)))
def test_every_size_doubling_solver(engine, nc):
    """The renormalisation-decimation kernel on the same leads: Sigma of both contacts against the float64
    restatement, step counts +- 1."""
    g_dev, _, inds, leads = _system(nc, nc, 300 + nc, solver="doubling")
    Es = np.array([0.3, 0.1 + 0.2j])
    for c in (0, 1):
        a = leads[c]
        lead = xc.Lead("L", a[0], a[1], a[2], a[3], a[2], a[3], [], eta=ETA)
        sig, its, cv = g_dev.sigma_batch(Es, c)
        assert np.all(cv == 1)
        for m, E in enumerate(Es):
            ref, steps = xr.rd64(lead, complex(E))[1:3]
            blk = sig[m][np.ix_(inds[c], inds[c])]
            assert rel_fro(blk, ref) < TOL_RD, (nc, c, E, rel_fro(blk, ref))
            assert abs(int(its[m, c]) - steps) <= 1, (nc, c, E)


@pytest.mark.parametrize("sweeps", [0, 3])
@pytest.mark.parametrize("ncL,ncR", [(50, 40), (35, 20), (19, 9)])
def test_unequal_contacts_switch_class(engine, ncL, ncR, sweeps):
    _check_fixed_trips(ncL, ncR, 500 + ncL, sweeps)


def test_free_running_c3_like_lead(engine):
    """n_c = 50, eta = 1e-4, the reference's stopping rule: sweep counts as the oracle's (+- 1 at a threshold
    crossing, also at the 2000 cap), Sigma within 10 * conv."""
    nc = 50
    g_dev, g_ref, _, _ = _system(nc, nc, 55, eta=1e-4)
    E = np.linspace(-1.9, 1.9, 16)
    sig, iters, conv = g_dev.sigma_batch(E)
    for k, e in enumerate(E):
        ref = g_ref.sigmaTot(e)
        for c in (0, 1):
            cnt = g_ref.last_iters[(complex(e), c)][0]
            assert abs(int(iters[k, c]) - cnt) <= 1, (e, c, int(iters[k, c]), cnt)
        assert rel_fro(sig[k], ref) < 10 * 1e-5, e


def _nonfinite(x):
    return ~(np.isfinite(x.real) & np.isfinite(x.imag))


@pytest.mark.parametrize("defect", ["zero_column", "nan_entry"])
@pytest.mark.parametrize("ncL,ncR", [(50, 50), (40, 24), (19, 33)])
def test_bad_unit_is_reported_and_contained(engine, ncL, ncR, defect):
    """Contact 1's lead cannot be factored (a zero column of A at every energy / a NaN in alpha): each of its units
    reports converged = 0 and a block without a finite entry; contact 0's units of the same launch equal those of a
    launch whose contact 1 is sound -- Sigma block, sweep counts and flags, bit for bit."""
    good = (chain_lead(ncL, 801), chain_lead(ncR, 802))
    alpha, Salpha = good[1][0].copy(), good[1][1].copy()
    if defect == "zero_column":
        alpha[:, ncR // 2] = 0.0; Salpha[:, ncR // 2] = 0.0
    else:
        alpha[1, 2] = np.nan
    bad = (good[0], (alpha, Salpha, good[1][2], good[1][3]))
    E = np.array([-0.8, 0.3, 0.1 + 0.2j, 1.1])
    engine.set_chain_cache(0)                                   # every evaluation runs the fixed point
    try:
        d_bad, _, inds, _ = _system(ncL, ncR, 800, leads=bad)
        s_bad, it_bad, cv_bad = d_bad.sigma_batch(E)
        d_good, _, _, _ = _system(ncL, ncR, 800, leads=good)
        s_good, it_good, cv_good = d_good.sigma_batch(E)
    finally:
        engine.set_chain_cache(512)
    i0, i1 = np.ix_(inds[0], inds[0]), np.ix_(inds[1], inds[1])
    for m in range(E.size):
        assert int(cv_bad[m, 1]) == 0 and np.all(_nonfinite(s_bad[m][i1])), (defect, m)
        assert np.array_equal(s_bad[m][i0], s_good[m][i0]), (defect, m)
        assert np.all(np.isfinite(s_good[m]))
    assert np.array_equal(it_bad[:, 0], it_good[:, 0]) and np.array_equal(cv_bad[:, 0], cv_good[:, 0])
