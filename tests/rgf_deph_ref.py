"""numpy restatement, extended-precision truth and bars for the floating dephasing probes of a layered device
(negf_layered_probe_response, negf_layered_gless_int_probes, negf_layered_gr_int_probes; test_rgf_deph_host.py on the CPU,
test_rgf_deph_gpu.py on the MI355X).  The inputs are rgf_tmat_ref.cases() (a - d) at their own energies: terminals = the
end terminals, then the probes, every one (layer, orbitals inside the layer, K x K block);

    To = T with zero diagonal,  W_pp = sum_{c != p} To[p][c],  W_pq = -To[p][q],  R[P', :] = W^-1 To[P', 0:n_t]
    D_s = scatter(Gamma_s) + sum_p R[p][s] scatter(Gamma_p)       (s = None: all terminals with weight 1)
    A   = G D_s G^H on the pattern of S: diagonal blocks A_ii, upper blocks A_{i,i+1}, lower blocks conj(A_{i,i+1})^T

Float64 forms:
  strips   the recursion the engine runs.  Pass over the layers as they are: g_i, G_ii, U_i = g_i C_{i,i+1}; the kept strip
           Cfull_i = [G_{i,q}[:, J_q]]_q gets its blocks q >= i, the head G_ii[:, J_i] and U_i Cfull_{i+1}[:, q > i].  Pass over
           the layers in reverse order: the blocks q < i as U'_i Cfull_{i-1}[:, q < i], U'_i = g'_i C_{i,i-1} (the same-layer
           block stays the first pass's).  T from the blocks G_ab read out of Cfull, R by dephase_ref.response, D_q per layer
           on J_q, Y_i = Cfull_i blockdiag(D_q), A_ii = Y_i Cfull_i^H, A_{i,i+1} = Y_i Cfull_{i+1}^H.  G itself on the pattern
           (negf_layered_gr_int_probes) is the first pass's G_ii, U_i G_{i+1,i+1}, G_{i+1,i+1} V_i.
  dense    on to_dense() with global_terms(): dephase_ref.response on rgf_tmat_ref.dense's T, and dephase_ref.gless_probes'
           form -- the explicit inverse and the literal D_s of dephase_ref.coupling -- cut to the pattern, with the inverse and
           R formed once per energy for all selections (gless_probes itself forms tmatrix_ref.tmatrix's T anew for every
           selection, C^2 products of size N: seconds per energy on the 501-orbital case); G: that inverse, cut.
Truth: dephase_ref.truth_parts / response_truth in clongdouble on to_dense(); G D_s G^H is formed on the pattern only, from
the columns of G on the terminals' orbitals (D_s vanishes elsewhere), which is gless_probes_truth cut to the pattern.

C_RDEPH is the accuracy constant of the calibrated bar (test_rgf_deph_host.test_calibration, the procedure that produced
C_DEPH and C_RTM): a device result passes when its relative Frobenius error against the truth is at most C_RDEPH times the
larger error of the two float64 forms on that input (errors floored at 2^-52); for the weighted sums, which the engine
forms by the strips recursion, C_RDEPH times the strips form's error.  Measured on the CPU over cases() x their energies x
(R, every end terminal, the total): R = 3.05 (worst ratio between the two forms' errors: the response of case d at
E = 0.45, 3.7e-16 by the strips against 1.1e-15 by the dense form) -> C_RDEPH = 8; the ratios of G D_s G^H are at most
2.0, the float64 errors themselves 2.2e-16 ... 1.4e-14.  The responses' errors sit within a few units of the floor, and the
float64 forms run through the host's BLAS, whose summation order differs between builds and thread counts: on a second
host the same inputs give R = 2.68 (the response of case c at E = -0.0097).  Both lie well inside (2, 4], so C_RDEPH is
the same; the host test asserts C_RDEPH exactly and R_MEASURED to 20 %.
negf_layered_gr_int_probes is negf_layered_gr_int's recursion with the probes in the diagonal: its bar is rgf_ref.C_RGF --
the constant calibrated for exactly that recursion's blocks -- times the strips form's error of G on the pattern.
"""
import functools

import numpy as np

import bond_ref as br
import dephase_ref as dr
import rgf_ref as rr
import rgf_tmat_ref as rt
import tmatrix_ref as tr
import xprec

LD = np.clongdouble
R_MEASURED = 3.05      # test_rgf_deph_host.test_calibration measures it again and asserts both
C_RDEPH = 8.0          # smallest power of two >= 2 R_MEASURED
C_RGF = rr.C_RGF
PROJECT_BAR = rr.PROJECT_BAR
FLOOR = rr.FLOOR
DEFECTS = ("no_reverse", "wrong_s", "no_gamma_s", "same_side")


def cases():
    return rt.cases()


def weights(c):
    """the complex weights of a case's energies in the weighted sums (seeded by nothing: a fixed ramp)"""
    k = np.arange(len(c.energies))
    return (0.5 + 0.25 * k) + 0.125j * (k - 1)


def selections(c):
    """every end terminal, then the total"""
    return list(range(c.n_t)) + [None]


def flat_of(Ad, Au, Al):
    return np.concatenate([np.asarray(b).ravel() for b in list(Ad) + list(Au) + list(Al)])


def lower_of(Au):
    return [np.conj(b).T for b in Au]


def rel_err(x, t):
    return rr.rel_err(x, t)


# --------------------------------------------------------------------------- the recursion
def _unions(c):
    L = len(c.sizes)
    layer = [t[0] for t in c.terms]
    idx = [np.asarray(t[1]) for t in c.terms]
    on = [[t for t in range(len(layer)) if layer[t] == q] for q in range(L)]
    J = [np.unique(np.concatenate([idx[t] for t in on[q]])) if on[q] else np.zeros(0, int) for q in range(L)]
    Joff = np.concatenate([[0], np.cumsum([len(j) for j in J])]).astype(int)
    pos = [{int(o): k for k, o in enumerate(J[q])} for q in range(L)]
    cpos = [np.array([pos[layer[t]][int(o)] for o in idx[t]], dtype=int) for t in range(len(layer))]
    return layer, idx, on, J, Joff, cpos


def kept_strips(c, E, defect=None):
    """(Cfull [L] of n_i x K_tot, (Gd, Gu, Gl): G on the pattern from the first pass) at one energy"""
    L = len(c.sizes)
    Ad, Au, Al = rt._layer_blocks(c, E, c.terms)
    layer, idx, on, J, Joff, cpos = _unions(c)
    Kt = int(Joff[-1])
    Cf = [np.zeros((c.sizes[i], Kt), complex) for i in range(L)]
    g = [np.linalg.inv(Ad[0])]
    for i in range(1, L):
        g.append(np.linalg.inv(Ad[i] - Al[i - 1] @ g[i - 1] @ Au[i - 1]))
    Gd, Gu, Gl = [None] * L, [None] * (L - 1), [None] * (L - 1)
    for i in range(L - 1, -1, -1):
        if i == L - 1:
            G = g[i]
        else:
            U = -g[i] @ Au[i]                                           # g_i C_{i,i+1}
            V = -Al[i] @ g[i]
            Gu[i] = U @ Gd[i + 1]
            Gl[i] = Gd[i + 1] @ V
            G = g[i] + Gu[i] @ V
            Cf[i][:, Joff[i + 1]:] = U @ Cf[i + 1][:, Joff[i + 1]:]
        Gd[i] = G
        Cf[i][:, Joff[i]:Joff[i + 1]] = G[:, J[i]]
    gm = [None] * L
    gm[L - 1] = np.linalg.inv(Ad[L - 1])
    for i in range(L - 2, -1, -1):
        gm[i] = np.linalg.inv(Ad[i] - Au[i] @ gm[i + 1] @ Al[i])
    if defect != "no_reverse":
        for p in range(1, L):
            Cf[p][:, :Joff[p]] = (-gm[p] @ Al[p - 1]) @ Cf[p - 1][:, :Joff[p]]       # g'_p C_{p,p-1}
    return Cf, (Gd, Gu, Gl)


def tmatrix_of(c, Cf):
    """T [C, C] from the blocks G_ab the kept strips hold"""
    layer, idx, on, J, Joff, cpos = _unions(c)
    gam = [tr.gamma(t[2]) for t in c.terms]
    C = len(c.terms)
    T = np.zeros((C, C))
    for a in range(C):
        for b in range(C):
            Gab = Cf[layer[a]][np.ix_(idx[a], Joff[layer[b]] + cpos[b])]
            T[a, b] = np.real(np.sum((gam[a] @ Gab @ gam[b]) * np.conj(Gab)))
    return T


def coupling_blocks(c, s, R, defect=None, dtype=complex):
    """[D_q on J_q]: the selected end terminal(s) in the order they were made, then the layer's probes"""
    layer, idx, on, J, Joff, cpos = _unions(c)
    n_t = c.n_t
    col = s
    if defect == "wrong_s" and s is not None:
        col = (s + 1) % n_t
    D = [np.zeros((len(J[q]), len(J[q])), dtype=dtype) for q in range(len(c.sizes))]
    for t, (lay, _, blk) in enumerate(c.terms):
        if t < n_t and s is not None and t != s:
            continue
        if t < n_t and defect == "no_gamma_s" and s is not None:
            continue
        wgt = 1.0 if (s is None or t < n_t) else R[t - n_t, col]
        b = np.asarray(blk).astype(dtype)
        D[lay][np.ix_(cpos[t], cpos[t])] += wgt * (dtype(1j) * (b - b.conj().T))
    return D


def pattern_of(c, Cf, D, defect=None):
    """(A_ii [L], A_{i,i+1} [L - 1]) from the kept strips and the blocks of D"""
    layer, idx, on, J, Joff, cpos = _unions(c)
    L = len(c.sizes)
    Y = []
    for i in range(L):
        y = np.zeros_like(Cf[i])
        for q in range(L):
            y[:, Joff[q]:Joff[q + 1]] = Cf[i][:, Joff[q]:Joff[q + 1]] @ D[q]
        Y.append(y)
    Ad = [Y[i] @ Cf[i].conj().T for i in range(L)]
    if defect == "same_side":       # Cfull_i on both sides; where n_{i+1} != n_i its rows are repeated / cut to the block's shape
        Au = [Y[i] @ Cf[i][np.arange(c.sizes[i + 1]) % c.sizes[i]].conj().T for i in range(L - 1)]
    else:
        Au = [Y[i] @ Cf[i + 1].conj().T for i in range(L - 1)]
    return Ad, Au


def strips(c, E, defect=None):
    """dict(R [P, n_t], A {s: flat pattern of G D_s G^H}, G: flat pattern of G) at one energy by the recursion"""
    Cf, (Gd, Gu, Gl) = kept_strips(c, E, defect)
    R = dr.response(tmatrix_of(c, Cf), c.n_t)
    out = dict(R=R, A={}, G=flat_of(Gd, Gu, Gl))
    for s in selections(c):
        Ad, Au = pattern_of(c, Cf, coupling_blocks(c, s, R, defect), defect)
        out["A"][s] = flat_of(Ad, Au, lower_of(Au))
    return out


def _cut(c, M):
    o = c.offsets
    L = len(c.sizes)
    return ([M[o[i]:o[i + 1], o[i]:o[i + 1]] for i in range(L)], [M[o[i]:o[i + 1], o[i + 1]:o[i + 2]] for i in range(L - 1)],
            [M[o[i + 1]:o[i + 2], o[i]:o[i + 1]] for i in range(L - 1)])


def dense(c, E):
    F, S = c.to_dense()
    terms = c.global_terms()
    G = np.linalg.inv(tr.assembled(F, S, terms, E))
    Gh = G.conj().T
    out = dict(R=dr.response(rt.dense(c, E), c.n_t), A={}, G=flat_of(*_cut(c, G)))
    for s in selections(c):
        Ad, Au, _ = _cut(c, G @ dr.coupling(c.N, terms, c.n_t, s, out["R"]) @ Gh)
        out["A"][s] = flat_of(Ad, Au, lower_of(Au))
    return out


def truth(c, E):
    """the same dict in clongdouble; G D_s G^H on the pattern from the columns of G on the terminals' orbitals"""
    F, S = c.to_dense()
    terms = c.global_terms()
    n = F.shape[0]
    G, T = dr.truth_parts(F, S, terms, E)
    R = dr.response_truth(T, c.n_t)
    U = np.unique(np.concatenate([np.asarray(ix) for ix, _ in terms]))
    GU = np.ascontiguousarray(G[:, U])
    GUh = np.ascontiguousarray(GU.conj().T)
    o = c.offsets
    L = len(c.sizes)
    out = dict(R=R, A={}, G=flat_of(*_cut(c, G)))
    for s in selections(c):
        D = np.ascontiguousarray(dr.coupling(n, terms, c.n_t, s, R.astype(LD))[np.ix_(U, U)])
        Y = br._matmul_ld(GU, D)
        Ad = [br._matmul_ld(np.ascontiguousarray(Y[o[i]:o[i + 1]]), np.ascontiguousarray(GUh[:, o[i]:o[i + 1]])) for i in range(L)]
        Au = [br._matmul_ld(np.ascontiguousarray(Y[o[i]:o[i + 1]]), np.ascontiguousarray(GUh[:, o[i + 1]:o[i + 2]]))
              for i in range(L - 1)]
        out["A"][s] = flat_of(Ad, Au, lower_of(Au))
    return out


# --------------------------------------------------------------------------- the tables
def _errors(form, t, c):
    e = dict(R=rel_err(form["R"], t["R"]), G=rel_err(form["G"], t["G"]))
    for s in selections(c):
        e[s] = rel_err(form["A"][s], t["A"][s])
    return e


@functools.lru_cache(maxsize=None)
def truth_table():
    """[dict(tag, case, E, truth, strips, dense, err_strips, err_dense)] over every (case, energy): computed once per process
    and shared by the tests that need it; err_* = {'R', 'G', 0 .. n_t - 1, None: relative error against the truth}."""
    items = [(c, E) for c in cases() for E in c.energies]

    def make(item):
        c, E = item
        ent = dict(tag=f"{c.name} E={E:.6g}", case=c, E=E, truth=truth(c, E), strips=strips(c, E), dense=dense(c, E))
        for k in ("strips", "dense"):
            ent["err_" + k] = _errors(ent[k], ent["truth"], c)
        return ent
    return xprec.pmap(make, items)


def entries(c):
    return [ent for ent in truth_table() if ent["case"] is c]


def bar_R(ent):
    """what a response on this input may err by"""
    return C_RDEPH * max(ent["err_strips"]["R"], ent["err_dense"]["R"])


@functools.lru_cache(maxsize=None)
def sums(name):
    """dict(case, E, w, truth, strips, err: {sel or 'G': the strips form's error}) of the weighted sums of a case over its
    energies with weights(c): sum_k w_k A_s(E_k) (lower blocks: sum_k w_k conj(A_{i,i+1}(E_k))^T) and sum_k w_k G(E_k)"""
    c = next(x for x in cases() if x.name == name)
    ents = entries(c)
    w = weights(c)
    out = dict(case=c, E=np.array([e["E"] for e in ents]), w=w, truth={}, strips={}, err={})
    for key in selections(c) + ["G"]:
        for form, dtype in (("truth", LD), ("strips", complex)):
            acc = 0
            for wk, e in zip(w, ents):
                x = e[form]["G"] if key == "G" else e[form]["A"][key]
                acc = acc + dtype(wk) * np.asarray(x).astype(dtype)      # (the lower part conj(A_up)^T takes w_k itself)
            out[form][key] = acc
        out["err"][key] = rel_err(out["strips"][key], out["truth"][key])
    return out


def bar_sum(s, key):
    """what a weighted sum on this input may err by: G D_s G^H at C_RDEPH, G at rgf_ref's C_RGF, times the strips form's error"""
    return (C_RGF if key == "G" else C_RDEPH) * s["err"][key]
