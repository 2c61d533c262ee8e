"""numpy restatements, extended-precision truth and seeded inputs for the recursive Green's function path of layered
devices (test_rgf_host.py on the CPU, test_rgf_gpu.py on the MI355X).

A layered system is L diagonal blocks F_ii, S_ii and L - 1 upper blocks F_{i,i+1}, S_{i,i+1} (the lower ones are their
conjugate transposes), with a left terminal on layer 0 and a right terminal on layer L - 1.  A_ij = E S_ij - F_ij.

Three float64 forms:
  sweep_lr   the left-to-right sweep with explicit inverses: g_i = inv(A_ii - A_{i,i-1} g_{i-1} A_{i-1,i} - Sigma), the
             corner block carried along, then the backward recursion for G_ii, G_{i,i+1}, G_{i+1,i}
  sweep_rl   the mirror image, right to left, with LU factorisations and solves instead of inverses: the recursion
             starts at the other end, so every block is reached through different intermediate quantities
  dense      numpy.linalg.inv of the assembled N x N matrix
The truth is the dense form in clongdouble on xprec.refine's inverse.

Quantities of a case (`evaluate`): T [m] = Re Tr[Gamma_R G_RL Gamma_L G_RL^H] (the transmission from the left terminal
into the right one), dos [m, N] = -Im diag G / pi, pdos [m, N] = -Im diag(G S) / pi (what the engine returns of diag G
and diag(G S)), and with weights `blocks` = sum_m w_m G(E_m) on the pattern of S (diagonal | upper | lower blocks,
flattened).

C_RGF is the accuracy constant of the calibrated bar (test_rgf_host.test_calibration): a result passes when its
relative Frobenius error against the truth is at most C_RGF times the larger error of the two float64 SWEEP forms on
that input (errors floored at 2^-52).  The sweeps' errors are up to ~30 times the dense form's, so the bar hangs on them.
Measured on the CPU over cases() x their four energies and the contour case: R = 13.50 (worst ratio between the two
sweeps' errors: case c, T, 5.6e-13 left-to-right against 4.2e-14 right-to-left) -> C_RGF = 32; the sweeps' errors are
2.4e-16 ... 5.6e-13 on T and 2.2e-16 ... 5.7e-13 on the two DOS forms, the dense form's 2.2e-16 ... 1.4e-14.
"""
import functools

import numpy as np
import scipy.linalg as sla

import tmatrix_ref as tr
import xprec

LD = np.clongdouble
R_MEASURED = 13.50     # test_rgf_host.test_calibration measures it again and asserts both
C_RGF = 32.0           # smallest power of two >= 2 R_MEASURED
PROJECT_BAR = 1e-8
FLOOR = 2.0 ** -52


class RCase:
    def __init__(self, name, sizes, seed, hermitian_complex=False, left=None, right=None):
        self.name, self.sizes, self.real = name, tuple(sizes), not hermitian_complex
        rng = np.random.default_rng(7100 + seed)
        L = len(sizes)

        def rnd(a, b):
            x = rng.standard_normal((a, b))
            return x if self.real else x + 1j * rng.standard_normal((a, b))
        self.F_diag, self.S_diag, self.F_up, self.S_up = [], [], [], []
        for n in sizes:
            a = rnd(n, n)
            self.F_diag.append((a + a.conj().T) / np.sqrt(2 * n))
            s = rnd(n, n)
            self.S_diag.append(np.eye(n) + 0.1 * (s + s.conj().T) / np.sqrt(2 * n))
        for i in range(L - 1):
            mx = max(sizes[i], sizes[i + 1])
            self.F_up.append(0.6 * rnd(sizes[i], sizes[i + 1]) / np.sqrt(mx))
            self.S_up.append(0.05 * rnd(sizes[i], sizes[i + 1]) / np.sqrt(mx))
        n0, nl = sizes[0], sizes[-1]
        self.left = np.asarray(left if left is not None else np.arange(min(3, n0)), dtype=int)           # inside layer 0
        self.right = np.asarray(right if right is not None else np.arange(nl - min(4, nl), nl), dtype=int)   # inside layer L - 1
        self.sig_left = tr.sigma_block(self.left.size, rng, real=self.real)
        self.sig_right = tr.sigma_block(self.right.size, rng, real=self.real)
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        self.N = int(self.offsets[-1])
        F, S = self.to_dense()
        ev = sla.eigh(F, S, eigvals_only=True)
        self.energies = np.array([-0.7, 0.0, 0.45, ev[len(ev) // 2] + 5e-4])

    def to_dense(self, dtype=None):
        o = self.offsets
        out = []
        for diag, up in ((self.F_diag, self.F_up), (self.S_diag, self.S_up)):
            M = np.zeros((self.N, self.N), dtype=dtype or (float if self.real else complex))
            for i, b in enumerate(diag):
                M[o[i]:o[i + 1], o[i]:o[i + 1]] = b
            for i, b in enumerate(up):
                M[o[i]:o[i + 1], o[i + 1]:o[i + 2]] = b
                M[o[i + 1]:o[i + 2], o[i]:o[i + 1]] = b.conj().T
            out.append(M)
        return out

    @property
    def left_global(self):
        return self.left

    @property
    def right_global(self):
        return self.offsets[-2] + self.right

    def mirrored(self):
        """The same device with its layers in reverse order (left and right terminals swapped)."""
        m = object.__new__(RCase)
        m.__dict__.update(self.__dict__)
        m.name, m.sizes = self.name + "-mirror", self.sizes[::-1]
        m.F_diag, m.S_diag = self.F_diag[::-1], self.S_diag[::-1]
        m.F_up = [b.conj().T for b in self.F_up[::-1]]
        m.S_up = [b.conj().T for b in self.S_up[::-1]]
        m.left, m.right, m.sig_left, m.sig_right = self.right, self.left, self.sig_right, self.sig_left
        m.offsets = np.concatenate([[0], np.cumsum(m.sizes)]).astype(int)
        return m


@functools.lru_cache(maxsize=None)
def cases():
    return (
        RCase("a", (3, 5), 1),
        # terminal lists not contiguous
        RCase("b", (7, 12, 5, 9), 2, hermitian_complex=True, left=[0, 2, 5], right=[1, 3, 6, 8]),
        # every route of the block inverse at four energies per batch: the unblocked kernel (18 < 32), the single-workgroup
        # blocked kernel (33, 40, 97, 100: sizes that are no multiple of 4, and above 96 no multiple of 16) and the windowed
        # one (213 >= 209, no multiple of 4)
        RCase("c", (40, 100, 97, 33, 213, 18), 3),
        RCase("d", (20,) * 8, 5, hermitian_complex=True),
    )


@functools.lru_cache(maxsize=None)
def window_case():
    """Three real layers for the windowed inverse at a FOREIGN stride: 40 (single-workgroup kernel), 257 and 300 (both
    windowed, 257 with a last window of one column); the layered path strides every layer's matrices by nmax^2 = 300^2,
    so the 257 layer runs every windowed kernel at a stride that is not n * n.  N = 597: the extended-precision truth
    costs what case c's does.  Not an entry of cases(): test_rgf_host.test_calibration measures over those, and C_RGF
    is not recalibrated for this case -- instead the case is admitted only if the two float64 sweeps' errors differ by
    at most C_RGF / 2 = 16 on every quantity (test_rgf_host.test_window_case_is_within_the_calibration prints them).
    Measured on the CPU with seed 41, larger over smaller error of the two sweeps: T 1.98 (3.8e-14 left-to-right, 7.5e-14
    right-to-left), dos 6.89 (1.4e-13, 9.8e-13), pdos 6.91, the blocks of one energy alone 5.12, 3.75, 1.23, 6.53; for
    G Gamma G^H (rgf_less_ref.window_entry, against C_LESS / 2 = 32): blocks 4.55, rows 3.79, one energy alone 4.71,
    2.85, 1.01, 11.48.  The seed is the one of 11 ... 59 with the smallest kappa_2(A) over the four energies (881): the
    last correction of the truth's refinement is then 1.7e-17 at worst, against its bar of 2^-55 = 2.8e-17 (seeds 11 to
    14 end above it).  Its entry: window_truth()."""
    return RCase("w", (40, 257, 300), 41)


def contour():
    """(case b, eight complex energies on a semicircle, complex weights)"""
    c = cases()[1]
    th = np.pi * (np.arange(8) + 0.5) / 8
    E = -0.4 + 1.9 * np.exp(1j * th)
    w = 1.9j * np.exp(1j * th) * (np.pi / 8) * (1.0 + 0.1 * np.arange(8))
    return c, E, w


# --------------------------------------------------------------------------- the blocks of A
def _blocks(c, E, dtype=complex):
    E = dtype(E)
    L = len(c.sizes)
    Ad = [E * np.asarray(c.S_diag[i]).astype(dtype) - np.asarray(c.F_diag[i]).astype(dtype) for i in range(L)]
    Au = [E * np.asarray(c.S_up[i]).astype(dtype) - np.asarray(c.F_up[i]).astype(dtype) for i in range(L - 1)]
    Al = [E * np.asarray(c.S_up[i]).astype(dtype).conj().T - np.asarray(c.F_up[i]).astype(dtype).conj().T for i in range(L - 1)]
    Ad[0] = Ad[0].copy(); Ad[-1] = Ad[-1].copy()
    Ad[0][np.ix_(c.left, c.left)] -= np.asarray(c.sig_left).astype(dtype)
    Ad[-1][np.ix_(c.right, c.right)] -= np.asarray(c.sig_right).astype(dtype)
    return Ad, Au, Al


def assembled(c, E, dtype=complex):
    Ad, Au, Al = _blocks(c, E, dtype)
    o = c.offsets
    A = np.zeros((c.N, c.N), dtype=dtype)
    for i, b in enumerate(Ad):
        A[o[i]:o[i + 1], o[i]:o[i + 1]] = b
    for i in range(len(Au)):
        A[o[i]:o[i + 1], o[i + 1]:o[i + 2]] = Au[i]
        A[o[i + 1]:o[i + 2], o[i]:o[i + 1]] = Al[i]
    return A


# --------------------------------------------------------------------------- per-energy pieces of G
# every form returns (Gd, Gu, Gl, G_RL): diagonal blocks, upper blocks G_{i,i+1}, lower blocks G_{i+1,i}, and the corner
# block G_{L-1,0} cut to [I_right, I_left]
def sweep_lr(c, E):
    Ad, Au, Al = _blocks(c, E)
    L = len(Ad)
    g = [np.linalg.inv(Ad[0])]
    X = g[0]
    for i in range(1, L):
        g.append(np.linalg.inv(Ad[i] - Al[i - 1] @ g[i - 1] @ Au[i - 1]))
        X = -g[i] @ (Al[i - 1] @ X)
    Gd = [None] * L; Gu = [None] * (L - 1); Gl = [None] * (L - 1)
    Gd[L - 1] = g[L - 1]
    for i in range(L - 2, -1, -1):
        Gu[i] = -g[i] @ Au[i] @ Gd[i + 1]
        Gl[i] = -Gd[i + 1] @ Al[i] @ g[i]
        Gd[i] = g[i] + g[i] @ Au[i] @ Gd[i + 1] @ Al[i] @ g[i]
    return Gd, Gu, Gl, X[np.ix_(c.right, c.left)]


def sweep_rl(c, E):
    Ad, Au, Al = _blocks(c, E)
    L = len(Ad)
    lu = [None] * L                                     # LU of the right-connected blocks D_i
    lu[L - 1] = sla.lu_factor(Ad[L - 1])
    for i in range(L - 2, -1, -1):
        lu[i] = sla.lu_factor(Ad[i] - Au[i] @ sla.lu_solve(lu[i + 1], Al[i]))

    def right_apply(M, k):                              # M D_k^-1
        return sla.lu_solve(lu[k], M.T, trans=1).T
    Gd = [None] * L; Gu = [None] * (L - 1); Gl = [None] * (L - 1)
    Gd[0] = sla.lu_solve(lu[0], np.eye(c.sizes[0], dtype=complex))
    Z = Gd[0]                                           # G_{i,0}
    for i in range(L - 1):
        Gl[i] = -sla.lu_solve(lu[i + 1], Al[i] @ Gd[i])                  # G_{i+1,i} = -gR_{i+1} A_{i+1,i} G_ii
        Gu[i] = -right_apply(Gd[i] @ Au[i], i + 1)                       # G_{i,i+1} = -G_ii A_{i,i+1} gR_{i+1}
        gR = sla.lu_solve(lu[i + 1], np.eye(c.sizes[i + 1], dtype=complex))
        Gd[i + 1] = gR - Gl[i] @ right_apply(Au[i], i + 1)               # gR + gR A G_ii A gR
        Z = -sla.lu_solve(lu[i + 1], Al[i] @ Z)
    return Gd, Gu, Gl, Z[np.ix_(c.right, c.left)]


def _cut(c, G):
    o = c.offsets
    L = len(c.sizes)
    Gd = [G[o[i]:o[i + 1], o[i]:o[i + 1]] for i in range(L)]
    Gu = [G[o[i]:o[i + 1], o[i + 1]:o[i + 2]] for i in range(L - 1)]
    Gl = [G[o[i + 1]:o[i + 2], o[i]:o[i + 1]] for i in range(L - 1)]
    return Gd, Gu, Gl, G[np.ix_(c.right_global, c.left_global)]


def dense(c, E):
    return _cut(c, np.linalg.inv(assembled(c, E)))


def truth_pieces(c, E):
    xprec.require_extended()
    A = assembled(c, E, LD)
    (G, _), = xprec.refine([(A, np.arange(c.N))], [2.0 ** -55])
    return _cut(c, G)


# --------------------------------------------------------------------------- the quantities
def _quantities(c, pieces, dtype):
    Gd, Gu, Gl, Grl = pieces
    L = len(c.sizes)
    gR = np.asarray(c.sig_right).astype(dtype); gR = dtype(1j) * (gR - gR.conj().T)
    gL = np.asarray(c.sig_left).astype(dtype); gL = dtype(1j) * (gL - gL.conj().T)
    Grl = np.ascontiguousarray(Grl)
    T = ((gR @ Grl @ gL) * np.conj(Grl)).real.sum()
    dg = np.concatenate([np.diagonal(b) for b in Gd])
    Sd = [np.asarray(b).astype(dtype) for b in c.S_diag]
    Su = [np.asarray(b).astype(dtype) for b in c.S_up]
    rows = []
    for i in range(L):
        r = (Gd[i] * Sd[i].T).sum(axis=1)                               # sum_k G_ii[r,k] S_ii[k,r]
        if i + 1 < L:
            r = r + (Gu[i] * Su[i].conj()).sum(axis=1)                  # S_{i+1,i}[k,r] = conj(S_{i,i+1}[r,k])
        if i > 0:
            r = r + (Gl[i - 1] * Su[i - 1].T).sum(axis=1)               # S_{i-1,i}[k,r]
        rows.append(r)
    flat = np.concatenate([np.asarray(b).ravel() for b in list(Gd) + list(Gu) + list(Gl)])
    pi = np.longdouble(np.pi) if dtype is LD else np.pi
    return T, -dg.imag / pi, -np.concatenate(rows).imag / pi, flat


def evaluate(form, c, energies, weights=None):
    """dict(T [m], dos [m, N], pdos [m, N], blocks [pattern] when weights are given) of one form ('lr', 'rl', 'dense', 'truth')."""
    fn = {"lr": sweep_lr, "rl": sweep_rl, "dense": dense, "truth": truth_pieces}[form]
    dtype = LD if form == "truth" else complex
    per = xprec.pmap(lambda E: _quantities(c, fn(c, E), dtype), list(energies))
    out = dict(T=np.array([p[0] for p in per]), dos=np.array([p[1] for p in per]), pdos=np.array([p[2] for p in per]))
    if weights is not None:
        acc = np.zeros(per[0][3].shape, dtype=dtype)
        for w, p in zip(weights, per):
            acc = acc + dtype(w) * p[3]
        out["blocks"] = acc
    return out


def rel_err(x, truth):
    """relative Frobenius error over all entries, floored at 2^-52"""
    truth = np.asarray(truth)
    d = np.asarray(x).astype(truth.dtype) - truth
    nd = float(np.sqrt((np.abs(d).astype(np.longdouble) ** 2).sum()))
    nt = float(np.sqrt((np.abs(truth).astype(np.longdouble) ** 2).sum()))
    return max(nd / nt if nt > 0 else nd, FLOOR)


def inputs():
    """[(tag, case, energies, weights or None, quantities checked)]: the four cases at their real energies and the contour"""
    items = [(c.name, c, c.energies, None, ("T", "dos", "pdos")) for c in cases()]
    c, E, w = contour()
    items.append(("contour", c, E, w, ("blocks",)))
    return items


@functools.lru_cache(maxsize=None)
def truth_table():
    """{tag: dict(case, E, w, keys, truth, lr, rl, dense, err_lr, err_rl, err_dense)} -- computed once per process and
    shared by the tests that need it; err_* are {quantity: relative error against the truth}."""
    table = {}
    for tag, c, E, w, keys in inputs():
        ent = dict(case=c, E=E, w=w, keys=keys)
        for form in ("truth", "lr", "rl", "dense"):
            ent[form] = evaluate(form, c, E, w)
        for form in ("lr", "rl", "dense"):
            ent["err_" + form] = {k: rel_err(ent[form][k], ent["truth"][k]) for k in keys}
        table[tag] = ent
    return table


@functools.lru_cache(maxsize=None)
def window_truth():
    """The truth_table()-style entry of window_case(): dict(case, E, keys, truth, lr, rl, dense, err_lr, err_rl,
    err_dense) over its four energies for T, dos and pdos, and for 'single': [m, pattern], the blocks of G(E_j) on the
    pattern of S for each energy alone (what layered_gr_int returns with one-hot weights), whose err_* are lists
    energy by energy.  Computed once per process."""
    c = window_case()
    ent = dict(case=c, E=c.energies, w=None, keys=("T", "dos", "pdos"))
    for form, fn in (("truth", truth_pieces), ("lr", sweep_lr), ("rl", sweep_rl), ("dense", dense)):
        dtype = LD if form == "truth" else complex
        per = xprec.pmap(lambda E: _quantities(c, fn(c, E), dtype), list(c.energies))
        ent[form] = dict(T=np.array([p[0] for p in per]), dos=np.array([p[1] for p in per]),
                         pdos=np.array([p[2] for p in per]), single=np.array([p[3] for p in per]))
    for form in ("lr", "rl", "dense"):
        ent["err_" + form] = {k: rel_err(ent[form][k], ent["truth"][k]) for k in ent["keys"]}
        ent["err_" + form]["single"] = [rel_err(ent[form]["single"][j], ent["truth"]["single"][j])
                                        for j in range(len(c.energies))]
    return ent


def bar(ent, key):
    """what a result of quantity `key` on this input may err by"""
    return C_RGF * max(ent["err_lr"][key], ent["err_rl"][key])


def bar_single(ent, j):
    """... and the blocks of energy j alone (window_truth)"""
    return C_RGF * max(ent["err_lr"]["single"][j], ent["err_rl"]["single"][j])
