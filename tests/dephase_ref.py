"""numpy restatement, extended-precision truth and seeded inputs for the floating dephasing probes: the probes' response R
and the lesser Green's function's weighted sum with the dephased coupling (test_dephase_host.py on the CPU,
test_dephase_gpu.py on the MI355X).  Junctions and terminals as in tmatrix_ref.py: the contacts first, then the probes.

    To = T with zero diagonal,  W_pp = sum_{c != p} To[p][c] (c over ALL terminals),  W_pq = -To[p][q],
    P' = probes with W_pp > 0,  R[P', :] = W^-1 To[P', 0:n_c]  (other rows exact zeros)
    D_s = scatter(Gamma_s) + sum_p R[p][s] scatter(Gamma_p)       (s = None: the sum of all terminals' Gamma)
    out = sum_k w_k G(E_k) D_s(E_k) G(E_k)^H

Float64 forms: ``response`` (numpy.linalg.solve on the active block alone) and ``gless_probes`` (explicit inverse, literal
D_s).  The truths run in clongdouble on xprec.refine's inverse (tmatrix_ref's machinery) with the small solve a Gaussian
elimination written out in long double.

C_DEPH is the accuracy constant of the calibrated bar (test_dephase_host.test_calibration, the procedure that produced
tmatrix_ref.C_TM): a result passes when its relative Frobenius error against the truth is at most C_DEPH times the
larger error of the two float64 forms on that input.  The two forms of R: ``response`` on tmatrix_ref.tmatrix's T, and
transport.probe_response (one batched solve with the inactive probes masked) on tmatrix_ref.tmatrix_alt's T.  Measured on
the CPU over cases() x their four energies: R = 1.84 (worst ratio between the two forms' errors, at n200, E = -1) ->
C_DEPH = 4; the float64 errors themselves are 6.3e-17 ... 5.7e-16.  For the weighted sum of G D_s G^H, which has one
float64 form (``gless_probes``), the bar is C_DEPH times that form's error.
"""
import functools

import numpy as np

import bond_ref as br
import tmatrix_ref as tr
import xprec

LD = np.clongdouble
LR = np.longdouble
R_MEASURED = 1.84     # test_dephase_host.test_calibration
C_DEPH = 4.0          # smallest power of two >= 2 R
PROJECT_BAR = br.PROJECT_BAR


# --------------------------------------------------------------------------- float64
def _active(To, n_real):
    return [p for p in range(n_real, To.shape[0]) if To[p].sum() > 0]


def response(T, n_real):
    """R [P, n_real] of ONE transmission matrix T [C, C]; a NaN matrix gives NaN."""
    T = np.asarray(T, dtype=float)
    C = T.shape[0]
    R = np.zeros((C - n_real, n_real))
    if not np.isfinite(T).all():
        return R + np.nan
    To = T - np.diag(np.diag(T))
    P = _active(To, n_real)
    if P:
        W = -To[np.ix_(P, P)]
        W[np.arange(len(P)), np.arange(len(P))] = [To[p].sum() for p in P]
        R[np.asarray(P) - n_real] = np.linalg.solve(W, To[np.ix_(P, np.arange(n_real))])
    return R


def coupling(n, terms, n_real, s, R):
    """dense D_s [n, n] (s = None: all terminals with weight 1)"""
    D = np.zeros((n, n), dtype=np.result_type(R.dtype, complex))
    for t, (idx, blk) in enumerate(terms):
        if t < n_real and s is not None and t != s:
            continue
        wgt = 1.0 if (s is None or t < n_real) else R[t - n_real, s]
        b = np.asarray(blk).astype(D.dtype)
        D[np.ix_(idx, idx)] += wgt * (D.dtype.type(1j) * (b - b.conj().T))
    return D


def gless_probes(F, S, terms, n_real, s, E, w):
    """sum_k w_k G D_s G^H in float64: explicit inverse, tmatrix_ref.tmatrix's T, ``response``, literal D_s"""
    n = F.shape[0]
    out = np.zeros((n, n), complex)
    for e, wk in zip(np.atleast_1d(E), np.atleast_1d(w)):
        G = np.linalg.inv(tr.assembled(F, S, terms, e))
        R = response(tr.tmatrix(F, S, terms, e), n_real) if s is not None else np.zeros((len(terms) - n_real, n_real))
        out += wk * (G @ coupling(n, terms, n_real, s, R) @ G.conj().T)
    return out


def occupations(R, f):
    """f_p = sum_c R[p][c] f_c"""
    return np.asarray(R) @ np.asarray(f, dtype=float)


# --------------------------------------------------------------------------- clongdouble truth
def _solve_ld(W, B):
    """W X = B by Gaussian elimination with partial pivoting, written out in long double."""
    W = np.array(W, dtype=LR); B = np.array(B, dtype=LR)
    k = W.shape[0]
    for j in range(k):
        piv = j + int(np.argmax(np.abs(W[j:, j])))
        if piv != j:
            W[[j, piv]] = W[[piv, j]]; B[[j, piv]] = B[[piv, j]]
        l = W[j + 1:, j] / W[j, j]
        W[j + 1:, j:] -= l[:, None] * W[j, j:][None, :]
        B[j + 1:] -= l[:, None] * B[j][None, :]
    X = np.zeros_like(B)
    for j in range(k - 1, -1, -1):
        X[j] = (B[j] - W[j, j + 1:] @ X[j + 1:]) / W[j, j]
    return X


def response_truth(T, n_real):
    """R [P, n_real] in long double from a long-double T"""
    T = np.asarray(T, dtype=LR)
    C = T.shape[0]
    R = np.zeros((C - n_real, n_real), dtype=LR)
    To = T - np.diag(np.diag(T))
    P = _active(To, n_real)
    if P:
        W = -To[np.ix_(P, P)]
        W[np.arange(len(P)), np.arange(len(P))] = [To[p].sum() for p in P]
        R[np.asarray(P) - n_real] = _solve_ld(W, To[np.ix_(P, np.arange(n_real))])
    return R


def truth_parts(F, S, terms, E):
    """(G, T) in extended precision: tmatrix_ref.tmatrix_truth's inverse and its block form of T, the products of the
    one-orbital terminals (the probe-count edge shapes have dozens) taken in one vectorised step"""
    xprec.require_extended()
    n = F.shape[0]
    A = tr.assembled(F, S, terms, E, LD)
    (G, _), = xprec.refine([(A, np.arange(n))], [2.0 ** -55])
    gams = []
    for _, blk in terms:
        b = np.asarray(blk).astype(LD)
        gams.append(LD(1j) * (b - b.conj().T))
    C = len(terms)
    T = np.zeros((C, C), dtype=LR)
    one = np.array([t for t, (ix, _) in enumerate(terms) if len(ix) == 1], dtype=int)
    if one.size:
        at = np.array([terms[t][0][0] for t in one])
        g1 = np.array([gams[t][0, 0].real for t in one], dtype=LR)
        G11 = G[np.ix_(at, at)]
        T[np.ix_(one, one)] = g1[:, None] * g1[None, :] * (G11.real ** 2 + G11.imag ** 2)
    single = set(one.tolist())
    for a, (ia, _) in enumerate(terms):
        for b, (ib, _) in enumerate(terms):
            if a in single and b in single:
                continue
            Gab = np.ascontiguousarray(G[np.ix_(ia, ib)])
            Y = br._matmul_ld(br._matmul_ld(gams[a], Gab), gams[b])
            T[a, b] = (Y * np.conj(Gab)).real.sum()
    return G, T


def gless_truth_parts(F, S, terms, n_real, E):
    """(R, [M_s for s in 0 .. n_real - 1] + [M_total]) of ONE energy: M_s = G D_s G^H in clongdouble"""
    n = F.shape[0]
    G, T = truth_parts(F, S, terms, E)
    R = response_truth(T, n_real)
    Gh = np.ascontiguousarray(G.conj().T)
    Ms = [br._matmul_ld(br._matmul_ld(G, coupling(n, terms, n_real, s, R.astype(LD))), Gh)
          for s in list(range(n_real)) + [None]]
    return R, Ms, T


def gless_probes_truth(F, S, terms, n_real, s, E, w):
    n = F.shape[0]
    out = np.zeros((n, n), dtype=LD)
    for e, wk in zip(np.atleast_1d(E), np.atleast_1d(w)):
        _, Ms, _ = gless_truth_parts(F, S, terms, n_real, e)
        out += LD(wk) * Ms[-1 if s is None else s]
    return out


def rel_err(x, truth):
    """relative Frobenius error of a float64 (real or complex) table against its extended-precision truth"""
    d = np.asarray(x).astype(LD) - np.asarray(truth).astype(LD)
    return float(np.sqrt((d.real ** 2 + d.imag ** 2).sum()) / np.sqrt((truth.real ** 2 + truth.imag ** 2).sum()))


# --------------------------------------------------------------------------- seeded inputs
def edge_case(P, seed=70):
    """P one-orbital probes on n = P + 8 orbitals between two contacts of 4"""
    n = P + 8
    r = np.arange
    return tr.TCase(f"P{P}", n, seed + P, [r(0, 4), r(n - 4, n)] + [[4 + q] for q in range(P)], 2)


@functools.lru_cache(maxsize=None)
def shape_a():
    """n = 24, two contacts of 4, six probes of 1 - 3 orbitals: [2] on a lead, [6, 7] and [7, 8, 9] overlapping, [18]
    with Sigma = 0 (decoupled)"""
    r = np.arange
    return tr.TCase("a24", 24, 21, [r(0, 4), r(20, 24), [2], [6, 7], [7, 8, 9], [12], [14, 15, 16], [18]], 2, zero=(7,))


@functools.lru_cache(maxsize=None)
def shape_b():
    """n = 40, complex-Hermitian F (T != T^T), three contacts and five probes, two of them overlapping"""
    r = np.arange
    return tr.TCase("b40", 40, 22, [r(0, 5), r(17, 22), r(31, 40), [7], [9, 10, 11], [12, 13], [25, 26, 27], [24, 25]], 3,
                    hermitian_complex=True)


@functools.lru_cache(maxsize=None)
def many_contacts_case():
    """n = 40 with 17 one-orbital contacts and three probes: more right-hand sides than the response kernel keeps in LDS"""
    return tr.TCase("c17", 40, 23, [[q] for q in range(17)] + [[20], [22, 23], [25, 26, 27]], 17)


@functools.lru_cache(maxsize=None)
def cases():
    """what the calibration and the host tests run over: tmatrix_ref's cases with probes, the shapes (a) and (b) and three
    probe-count edges"""
    base = tuple(c for c in tr.cases() if len(c.probes))
    return base + (shape_a(), shape_b(), edge_case(1), edge_case(2), edge_case(33))


def truth_and_errors(F, S, terms, n_real, E):
    """(R_truth, [M_s ...] + [M_total], T_truth, err_a, err_b) of a junction at energy E: the errors of the two float64
    forms of R against the truth"""
    from gaunegf_amd import transport
    R, Ms, T = gless_truth_parts(F, S, terms, n_real, E)
    ea = rel_err(response(tr.tmatrix(F, S, terms, E), n_real), R)
    eb = rel_err(transport.probe_response(tr.tmatrix_alt(F, S, terms, E)[None], n_real)[0], R)
    return R, Ms, T, ea, eb


@functools.lru_cache(maxsize=None)
def truth_row(c, E):
    """truth_and_errors of case c at energy E, computed once per process."""
    return truth_and_errors(c.F, c.S, c.terms, c.n_c, E)


def truth_table():
    """[(tag, case, E) + truth_row] over every (case, energy) of cases()"""
    items = [(c, float(E)) for c in cases() for E in c.energies]
    rows = xprec.pmap(lambda it: truth_row(*it), items)
    return [(f"{c.name} E={E:.6g}", c, E) + tuple(row) for (c, E), row in zip(items, rows)]


# --------------------------------------------------------------------------- shape (d): two 1-D chain leads
D_ENERGIES = np.array([-1.0, 0.2, 1.1])


@functools.lru_cache(maxsize=None)
def shape_d():
    """n = 130 with two chain leads of 6 and 20 orbitals and ten probes of 9, neighbours overlapping by 3:
    (F, S, contact lists, surfG keyword arguments, probes)"""
    from helpers import chain_lead, random_system
    n, ncs = 130, (6, 20)
    F, S = random_system(n, 77)
    lead = [chain_lead(k, 50 + q) for q, k in enumerate(ncs)]
    ci = [list(range(ncs[0])), list(range(n - ncs[1], n))]
    rng = np.random.default_rng(77)
    kw = dict(taus=[0.2 * rng.standard_normal((k, k)) for k in ncs], staus=[0.02 * rng.standard_normal((k, k)) for k in ncs],
              alphas=[l[0] for l in lead], aOverlaps=[l[1] for l in lead], betas=[l[2] for l in lead],
              bOverlaps=[l[3] for l in lead], eta=1e-3)
    probes = [(np.arange(30 + 6 * q, 39 + 6 * q), tr.sigma_block(9, rng)) for q in range(10)]
    return F, S, ci, kw, probes


def lower_d(engine, solver):
    """the chain provider of shape (d) on ``engine`` (set_system included): (handle, surfG object)"""
    from gaunegf_amd.surfG1D import surfG
    F, S, ci, kw, _ = shape_d()
    g = surfG(F, S, ci, solver=solver, **kw)
    engine.set_system(F, S)
    return g._negf_lower(engine), g


def terms_d(engine, h, E):
    """[terms at E_k]: the contacts' blocks as the provider itself evaluates them (sigma_eval), then the probes"""
    F, S, ci, _, probes = shape_d()
    sig = [engine.sigma_eval(h, k, E, len(ci)) for k in range(len(ci))]
    return [[(np.asarray(ix), sig[q][k][np.ix_(ix, ix)]) for q, ix in enumerate(ci)] + list(probes) for k in range(len(E))]
