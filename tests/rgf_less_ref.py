"""numpy restatements and extended-precision truth of A = G Gamma G^H on the pattern of S for layered devices
(negf_layered_gless_int, negf_layered_contact_dos; test_rgf_less_host.py on the CPU, test_rgf_less_gpu.py on the MI355X).
Cases, inputs and the assembled blocks are rgf_ref.py's.

A terminal touches the orbitals I of its end layer, Gamma = i (Sigma - Sigma^H) on I x I, so only the columns
W_i = G_{i,end}[:, I] enter.  With C_ij = F_ij - E S_ij = -A_ij, g_i the left-connected inverses and U_i = g_i C_{i,i+1}:
  terminal on the last layer:  W_{L-1} = G_{L-1,L-1}[:, I],  W_i = U_i W_{i+1}
  terminal on layer 0:         x_0 = g_0[:, I],  z_i = C_{i,i-1} x_{i-1},  x_i = g_i z_i;   W_0 = G_00[:, I],  W_i = G_ii z_i
  A_ii = (W_i Gamma) W_i^H,  A_{i,i+1} = (W_i Gamma) W_{i+1}^H,  A_{i+1,i} = A_{i,i+1}^H

Three float64 forms:
  lr      that recursion, sweeping left to right with explicit inverses
  rl      the same code run on RCase.mirrored() with the layers reversed again: every block is reached from the other end
  dense   numpy.linalg.inv of the assembled N x N matrix, A = G[:, I] Gamma G[:, I]^H cut to the pattern
The truth is the dense form in clongdouble on xprec.refine's columns of the inverse.

Quantities of an input and a terminal selection `sel` ('L': the left terminal, 'R': the right one, 'LR': both, the left
one's contribution added first):
  blocks  sum_k w_k [A_ii | A_{i,i+1} | conj(A_{i,i+1})^T](E_k), flattened in negf_layered_gr_int's layout
  rows    [m, N] the contact Mulliken rows (1/2pi) Re sum_j A_ij conj(S_ij) over the pattern

C_LESS is the accuracy constant of the calibrated bar (test_rgf_less_host.test_calibration): a result passes when its
relative Frobenius error against the truth is at most C_LESS times the larger error of the two float64 sweep forms on
that input (errors floored at 2^-52).
Measured on the CPU over inputs() x ('L', 'R', 'LR') x ('blocks', 'rows'), each input taken whole and energy by energy (a
sum over four energies hides the one energy at which the sweeps differ most): R = 23.82 (worst ratio between the two
sweeps' errors: case d, terminal L, blocks at E = 0 alone, 1.3e-13 left-to-right against 5.5e-15 right-to-left) ->
C_LESS = 64; on the whole inputs the ratio is at most 2.8, the sweeps' errors are 2.2e-16 ... 3.2e-13 and the dense
form's 2.2e-16 ... 3.1e-14.
"""
import functools

import numpy as np

import rgf_ref as rr
import xprec

LD = np.clongdouble
R_MEASURED = 23.82     # test_rgf_less_host.test_calibration measures it again and asserts both
C_LESS = 64.0          # smallest power of two >= 2 R_MEASURED
PROJECT_BAR = rr.PROJECT_BAR
SELECTIONS = ("L", "R", "LR")
KEYS = ("blocks", "rows")


def gamma_of(sig, dtype=complex):
    s = np.asarray(sig).astype(dtype)
    return dtype(1j) * (s - s.conj().T)


# --------------------------------------------------------------------------- per-energy pattern blocks of A
# every form returns (Ad, Au): the diagonal blocks A_ii and the upper blocks A_{i,i+1}
def _products(W, gam):
    L = len(W)
    Y = [W[i] @ gam for i in range(L)]
    return [Y[i] @ W[i].conj().T for i in range(L)], [Y[i] @ W[i + 1].conj().T for i in range(L - 1)]


def _add(a, b):
    if a is None:
        return b
    return [x + y for x, y in zip(a[0], b[0])], [x + y for x, y in zip(a[1], b[1])]


def sweep(c, E, sel):
    """the recursion of the module docstring on case c"""
    Ad, Au, Al = rr._blocks(c, E)
    L = len(Ad)
    CU = [-b for b in Au]
    CL = [-b for b in Al]
    g = [np.linalg.inv(Ad[0])]
    for i in range(1, L):
        g.append(np.linalg.inv(Ad[i] - CL[i - 1] @ g[i - 1] @ CU[i - 1]))
    U = [g[i] @ CU[i] for i in range(L - 1)]
    G = [None] * L
    G[L - 1] = g[L - 1]
    for i in range(L - 2, -1, -1):
        G[i] = g[i] + U[i] @ G[i + 1] @ (CL[i] @ g[i])
    out = None
    if "L" in sel:
        x = g[0][:, c.left]
        z = [None] * L
        for i in range(1, L):
            z[i] = CL[i - 1] @ x
            x = g[i] @ z[i]
        W = [G[0][:, c.left]] + [G[i] @ z[i] for i in range(1, L)]
        out = _add(out, _products(W, gamma_of(c.sig_left)))
    if "R" in sel:
        W = [None] * L
        W[L - 1] = G[L - 1][:, c.right]
        for i in range(L - 2, -1, -1):
            W[i] = U[i] @ W[i + 1]
        out = _add(out, _products(W, gamma_of(c.sig_right)))
    return out


def sweep_lr(c, E, sel):
    return sweep(c, E, sel)


def sweep_rl(c, E, sel):
    """the same code on the mirrored device: its left terminal is this one's right; block (j, j+1) of this device is the
    conjugate transpose of the mirror's block (L-2-j, L-1-j)"""
    m = c.mirrored()
    Ad, Au = sweep(m, E, sel.translate(str.maketrans("LR", "RL")))
    return Ad[::-1], [b.conj().T for b in Au[::-1]]


def _cut(c, A):
    o = c.offsets
    L = len(c.sizes)
    return ([A[o[i]:o[i + 1], o[i]:o[i + 1]] for i in range(L)],
            [A[o[i]:o[i + 1], o[i + 1]:o[i + 2]] for i in range(L - 1)])


def _from_columns(c, cols, sel, dtype):
    """cols = (G[:, I_left], G[:, I_right]) of the whole system"""
    A = None
    for s, W, sig in (("L", cols[0], c.sig_left), ("R", cols[1], c.sig_right)):
        if s in sel:
            t = (W @ gamma_of(sig, dtype)) @ W.conj().T
            A = t if A is None else A + t
    return _cut(c, A)


def dense(c, E, sel):
    G = np.linalg.inv(rr.assembled(c, E))
    return _from_columns(c, (G[:, c.left_global], G[:, c.right_global]), sel, complex)


@functools.lru_cache(maxsize=None)
def _truth_columns(name, E):
    c = rr.window_case() if name == "w" else {k.name: k for k in rr.cases()}[name]
    xprec.require_extended()
    cols = np.concatenate([c.left_global, c.right_global])
    (X, _), = xprec.refine([(rr.assembled(c, E, LD), cols)], [2.0 ** -55])
    return X[:, :c.left.size], X[:, c.left.size:]


def truth_blocks(c, E, sel):
    return _from_columns(c, _truth_columns(c.name, complex(E)), sel, LD)


# --------------------------------------------------------------------------- the quantities
def flat_of(Ad, Au):
    """the layout of negf_layered_gr_int: diagonal | upper | lower blocks, the lower ones conj(A_{i,i+1})^T"""
    return np.concatenate([np.asarray(b).ravel() for b in list(Ad) + list(Au) + [b.conj().T for b in Au]])


def rows_of(c, Ad, Au, dtype):
    L = len(c.sizes)
    Sd = [np.asarray(b).astype(dtype) for b in c.S_diag]
    Su = [np.asarray(b).astype(dtype) for b in c.S_up]
    rows = []
    for i in range(L):
        r = (Ad[i] * Sd[i].conj()).real.sum(axis=1)
        if i + 1 < L:
            r = r + (Au[i] * Su[i].conj()).real.sum(axis=1)
        if i > 0:
            r = r + (Au[i - 1] * Su[i - 1].conj()).real.sum(axis=0)     # A_{i,i-1}[r,k] conj(S_{i,i-1}[r,k]), real part
        rows.append(r)
    two_pi = 2 * (np.longdouble(np.pi) if dtype is LD else np.pi)
    return np.concatenate(rows) / two_pi


def evaluate(form, c, energies, weights, sel):
    """dict(blocks [pattern], rows [m, N], single [m, pattern]: the blocks of each energy alone) of one form ('lr', 'rl',
    'dense', 'truth')"""
    fn = {"lr": sweep_lr, "rl": sweep_rl, "dense": dense, "truth": truth_blocks}[form]
    dtype = LD if form == "truth" else complex

    def one(E):
        Ad, Au = fn(c, E, sel)
        return flat_of(Ad, Au), rows_of(c, Ad, Au, dtype)
    per = xprec.pmap(one, list(energies))
    acc = np.zeros(per[0][0].shape, dtype=dtype)
    for w, p in zip(weights, per):
        acc = acc + dtype(w) * p[0]
    return dict(blocks=acc, rows=np.array([p[1] for p in per]), single=np.array([p[0] for p in per]))


def inputs():
    """[(tag, case, energies, weights)]: cases a-d at their four real energies with distinct real weights, and
    rgf_ref.contour()'s complex energies and weights (the lower blocks are then no transposes of the upper sums)"""
    items = [(c.name, c, c.energies, np.array([0.4, 0.7, 1.1, 1.6])) for c in rr.cases()]
    c, E, w = rr.contour()
    items.append(("contour", c, E, w))
    return items


@functools.lru_cache(maxsize=None)
def truth_table():
    """{(tag, sel): dict(case, E, w, truth, lr, rl, dense, err_lr, err_rl, err_dense, err1_*)} -- computed once per process
    and shared by the tests that need it; err_* are {quantity: relative error against the truth}, err1_* the same energy
    by energy."""
    table = {}
    for tag, c, E, w in inputs():
        for sel in SELECTIONS:
            table[(tag, sel)] = _entry(c, E, w, sel)
    return table


def _entry(c, E, w, sel):
    ent = dict(case=c, E=E, w=w, sel=sel)
    for form in ("truth", "lr", "rl", "dense"):
        ent[form] = evaluate(form, c, E, w, sel)
    for form in ("lr", "rl", "dense"):
        ent["err_" + form] = {k: rr.rel_err(ent[form][k], ent["truth"][k]) for k in KEYS}
        # energy by energy, for the calibration: (blocks, rows) of each energy alone
        ent["err1_" + form] = [(rr.rel_err(ent[form]["single"][j], ent["truth"]["single"][j]),
                                rr.rel_err(ent[form]["rows"][j], ent["truth"]["rows"][j])) for j in range(len(E))]
    return ent


@functools.lru_cache(maxsize=None)
def window_entry(sel="LR"):
    """the truth_table()-style entry of rgf_ref.window_case() (not an input of the calibration) for one selection; the
    blocks of energy j alone -- layered_gless_int with one-hot weights -- are ent[form]["single"][j], bar_single"""
    c = rr.window_case()
    return _entry(c, c.energies, np.array([0.4, 0.7, 1.1, 1.6]), sel)


def bar(ent, key):
    """what a result of quantity `key` on this input may err by"""
    return C_LESS * max(ent["err_lr"][key], ent["err_rl"][key])


def bar_single(ent, j):
    """... and the blocks of energy j alone"""
    return C_LESS * max(ent["err1_lr"][j][0], ent["err1_rl"][j][0])


def ind_of(sel):
    """the engine's `ind` for a selection when the left terminal was made first: 0, 1 or None (all)"""
    return {"L": 0, "R": 1, "LR": None}[sel]
