"""
CPU side of the complex-Hermitian truth cases of tests/xprec_hermitian.py: the cases are admitted (rows and columns
really differ, and LAPACK's inverse and a textbook Gauss-Jordan sit within HALF the unchanged bar of tests/xprec.py),
every planted defect that a complex-symmetric input hides is detected by a factor of at least 1e3, and the blindness
of the older ladder is recorded.  Lines 'HERM ...' print every ratio; the worst ones stand in xprec_hermitian's docstring.
"""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import rgf_ref as rr
import xprec
import xprec_chain as xc
import xprec_hermitian as xh
from xprec import Truth

xprec.require_extended()

ADMIT = 0.5                          # a condition on the cases, not a calibration: C_BAR stays as it is
DETECT = 1e3
SIZES = (2, 17, 64, 100, 257)
LEAD_SIZES = (9, 17, 50, 64)
KMAX = 10


@functools.lru_cache(maxsize=None)
def _case(name, n):
    c = xh.hermitian_ladder(n) if name == "G6" else xh.hermitian_confined(n)
    return c, Truth(c)


@functools.lru_cache(maxsize=None)
def _chain_truths(n):
    lead = xh.hermitian_lead(n)
    return lead, [xc.ChainTruth(lead, E, KMAX) for E in lead.energies]


# --------------------------------------------------------------------------- #
# admission
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["G6", "G6c"])
def test_admission(name, n):
    """||A - A^T||_F / ||A||_F >= 0.5 at every energy; numpy.linalg.inv, and up to n = 100 xprec.gauss_jordan, within
    0.5 of the bar C_BAR sqrt(n) u kappa_2 on every sampled column."""
    c, t = _case(name, n)
    assert c.name == name and np.array_equal(c.F, c.F.conj().T) and np.array_equal(c.S, c.S.conj().T)
    for s in (c.sigs if len(c.inds[0]) >= 2 else []):          # (a contact of one orbital has a 1 x 1 block)
        assert np.linalg.norm(s - s.T) > 0.1 * np.linalg.norm(s) and np.linalg.norm(s + s.conj().T) > 0.1 * np.linalg.norm(s)
    rows = []
    for m, E in enumerate(c.energies):
        A = c.A64(E)
        r_gj = t.ratio(m, xprec.gauss_jordan(A)) if n <= 100 else float("nan")
        rows.append((xh.asymmetry(A), t.ratio(m, np.linalg.inv(A)), r_gj))
        print(f"HERM admission {name} n={n} E={complex(E):.9g}: kappa {t.kappa[m]:.3g}  asym {rows[-1][0]:.3f}  "
              f"inv {rows[-1][1]:.3g}  gj {r_gj:.3g}")
    assert min(r[0] for r in rows) >= 0.5, rows
    assert max(r[1] for r in rows) <= ADMIT, rows
    assert all(r[2] <= ADMIT for r in rows if n <= 100), rows
    if name == "G6" and n >= xh.SPECTATOR_FROM:                # the ladder spans the conditioning of xprec.ladder
        assert t.kappa.max() > 1e8 and t.kappa.min() < 1e3, t.kappa
        # ... and hangs on the eigenvalue nearest the spectator's level, as xprec.ladder's does
        lam = sla.eig(c.F + c.sig_tot, c.S, right=False)
        lam0 = lam[np.argmin(np.abs(lam - c.F[c.resonant, c.resonant].real))]
        assert abs(c.energies[4] - lam0.real) <= 1e-12 and -1e-8 < lam0.imag < 0, (c.energies[4], lam0)
    if name == "G6c" and n >= 17:                              # confined: well conditioned, the product bounds are tight
        assert t.kappa.max() <= 2e2, t.kappa


@pytest.mark.parametrize("n", LEAD_SIZES)
def test_lead_admission(n):
    """L4: the float64 fixed point (xprec_chain.chain64) at or below 0.5 of the propagated bar on g and on Sigma for
    every checked K, and B really is neither symmetric nor Hermitian."""
    lead, truths = _chain_truths(n)
    assert np.array_equal(lead.alpha, lead.alpha.conj().T) and np.array_equal(lead.Salpha, lead.Salpha.conj().T)
    worst = 0.0
    for E, t in zip(lead.energies, truths):
        B = lead.B64(E)
        assert xh.asymmetry(B) >= 0.5 and xh.asymmetry(lead.A64(E)) >= 0.5
        assert np.linalg.norm(B - B.conj().T) >= 0.5 * np.linalg.norm(B)
        for K in xc.checked_k(t, KMAX):
            g, s = xc.chain64(lead, E, K)
            rg, rs = t.g_ratio(K, g), t.sigma_ratio(K, s)
            print(f"HERM admission L4 n={n} E={complex(E):.6g} K={K}: g {rg:.3g}  Sigma {rs:.3g}")
            worst = max(worst, rg, rs)
    assert worst <= ADMIT, worst


def test_layered_case_is_within_the_calibration():
    """Case h is no input of rgf_ref's calibration, so it may not stretch it (the rule of rgf_ref.window_case): on every
    quantity -- T in both directions, dos, pdos, the blocks of each energy alone -- the two float64 sweeps' errors
    differ by at most C_RGF / 2 = 16, and all forms agree at the project bar.  Rows and columns differ, and at the
    complex energy so do the two directions of T."""
    c = xh.rgf_case()
    assert c.name not in {k.name for k in rr.cases()} and c.sizes == (40, 100, 33) and not c.real
    assert all(32 <= n <= 208 for n in c.sizes)                # the single-workgroup blocked inverse for every layer
    fwd, back = xh.rgf_truth()
    worst = 1.0
    for tag, ent in (("h", fwd), ("h mirrored", back)):
        pairs = [(k, ent["err_lr"][k], ent["err_rl"][k], ent["err_dense"][k]) for k in ent["keys"]]
        pairs += [(f"single[{j}]", ent["err_lr"]["single"][j], ent["err_rl"]["single"][j], ent["err_dense"]["single"][j])
                  for j in range(len(ent["E"]))]
        for k, a, b, d in pairs:
            print(f"HERM layered {tag:10s} {k:10s} lr {a:.3g} rl {b:.3g} dense {d:.3g} ratio {max(a / b, b / a):.2f}")
            worst = max(worst, a / b, b / a)
            assert max(a, b, d) <= rr.PROJECT_BAR, (tag, k)
    print(f"HERM layered case h: worst ratio between the sweeps {worst:.2f} (bar {rr.C_RGF / 2:g})")
    assert worst <= rr.C_RGF / 2, worst
    Tf, Tb = np.asarray(fwd["truth"]["T"], dtype=float), np.asarray(back["truth"]["T"], dtype=float)
    print("HERM layered case h: T into the right terminal", Tf, "into the left one", Tb)
    # reciprocal at the real energies whatever the matrices; the complex energy tells the directions apart
    assert fwd["E"][-1] == xh.RGF_COMPLEX_E and np.all(fwd["E"][:-1].imag == 0)
    assert Tf.min() > 1e-3 and np.all(np.abs(Tf - Tb)[:-1] <= 1e-12 * Tf[:-1])
    assert abs(Tf[-1] - Tb[-1]) > 1e-4 * abs(Tf[-1])
    # the mirror's dos is case h's with the layers in reverse order: the same device
    o = c.offsets
    flip = np.concatenate([np.arange(o[i], o[i + 1]) for i in range(len(c.sizes) - 1, -1, -1)])
    assert rr.rel_err(back["truth"]["dos"], fwd["truth"]["dos"][:, flip]) <= 2.0 ** -50


# --------------------------------------------------------------------------- #
# detection
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n", [17, 64, 100, 257])
def test_transposed_inverse_is_detected(n):
    c, t = _case("G6", n)
    r = [t.ratio(m, xh.inv_transposed(c.A64(E))) for m, E in enumerate(c.energies)]
    print(f"HERM detection transposed inverse G6 n={n}: ratios {min(r):.3g} ... {max(r):.3g}")
    assert min(r) >= DETECT, r


def _weights(M, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(M) + 1j * rng.standard_normal(M)


@pytest.mark.parametrize("n", [17, 64])
@pytest.mark.parametrize("ind", [None, 0, -1])
def test_gless_defects_are_detected(n, ind):
    """sum_m w_m G_m Gamma G_m^H on G6c against xprec.grless_truth_and_bound: the float64 reference within half the
    bound, conj-only G^H, the transposed G and contact rows for contact columns at least 1e3 bounds off."""
    c, t = _case("G6c", n)
    w = _weights(c.energies.size)
    ref, bound = xprec.grless_truth_and_bound(t, w, ind)
    ratio = lambda P: float(np.linalg.norm((P.astype(xprec.LD) - ref).astype(np.complex128)) / bound)
    ok = ratio(xh.gless_int(c, w, ind))
    bad = {d: ratio(xh.gless_int(c, w, ind, d)) for d in ("conj", "trans", "rows")}
    print(f"HERM detection GrLessInt G6c n={n} ind={ind}: reference {ok:.3g}  " +
          "  ".join(f"{d} {v:.3g}" for d, v in bad.items()))
    assert ok <= ADMIT, ok
    assert min(bad.values()) >= DETECT, bad


@pytest.mark.parametrize("n", [17, 64])
def test_exchanged_contacts_are_detected_at_the_complex_energy(n):
    """A two-terminal T is reciprocal at real energies whatever the matrices (printed); at 0.3 + 2i it is not."""
    c, t = _case("G6c", n)
    ref, bound = xprec.transmission_truth_and_bound(t)
    refx, boundx = xprec.transmission_truth_and_bound(xh.truth_of_exchanged(t))
    m = int(np.argmax(np.abs(c.energies.imag)))
    assert c.energies[m] == 0.3 + 2j
    for k, E in enumerate(c.energies):
        ok = abs(xh.transmission(c, E) - ref[k]) / bound[k]
        sw = abs(xh.transmission(c, E, exchange=True) - ref[k]) / bound[k]
        okx = abs(xh.transmission(c, E, exchange=True) - refx[k]) / boundx[k]
        print(f"HERM detection T G6c n={n} E={complex(E):.6g}: reference {ok:.3g}  exchanged {sw:.3g}  "
              f"(exchanged against its own truth {okx:.3g})")
        assert ok <= ADMIT and okx <= ADMIT
        if k == m:
            assert sw >= DETECT, sw
            assert abs(ref[k] - refx[k]) > 1e-4 * abs(ref[k])


@pytest.mark.parametrize("n", LEAD_SIZES)
def test_chain_with_a_transposed_inverse_is_detected(n):
    lead, truths = _chain_truths(n)
    worst = np.inf
    for E, t in zip(lead.energies, truths):
        ks = xc.checked_k(t, KMAX)
        assert 0 in ks
        for K in ks:
            g, s = xc.chain64(lead, E, K, inv=xh.inv_transposed)
            rg, rs = t.g_ratio(K, g), t.sigma_ratio(K, s)
            print(f"HERM detection chain64(inv = transposed) L4 n={n} E={complex(E):.6g} K={K}: g {rg:.3g}  Sigma {rs:.3g}")
            worst = min(worst, rg, rs)
    assert worst >= DETECT, worst


# --------------------------------------------------------------------------- #
# blindness, recorded
# --------------------------------------------------------------------------- #
def test_the_symmetric_ladder_is_blind_to_a_transposed_inverse():
    """The reason for this family: on xprec.ladder(64), complex symmetric, numpy.linalg.inv(A).T passes the column bar at
    every energy."""
    c = xprec.ladder(64)
    t = Truth(c)
    r = [t.ratio(m, xh.inv_transposed(c.A64(E))) for m, E in enumerate(c.energies)]
    print(f"HERM blindness xprec.ladder(64), transposed inverse: ratios {min(r):.3g} ... {max(r):.3g}")
    assert max(r) <= 1.0, r
    assert max(xh.asymmetry(c.A64(E)) for E in c.energies) < 1e-12
