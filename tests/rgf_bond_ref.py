"""numpy restatements and extended-precision truth of the local (bond) transmission on the pattern of S for layered devices
(negf_layered_local_transmission, negf_layered_bond_int; test_rgf_bond_host.py on the CPU, test_rgf_bond_gpu.py on the
MI355X).  Cases and inputs are rgf_ref.py's, the blocks of A = G Gamma G^H rgf_less_ref.py's, and one tiny case of its own
with a layer of one orbital and one of 17 beside one of 16 (the edges of the 16-wide transpose tile).

With K = E S - F (no self-energies) and A_ii, A_{i,i+1} the blocks of A:
  diagonal block i:     flow[r][c] = 2 Im[K_ii[r][c] conj(A_ii[r][c])]
  upper block (i, i+1): flow[r][c] = 2 Im[K_u[r][c] conj(A_u[r][c])]
  lower block (i+1, i): flow[r][c] = 2 Im[K_l[r][c] A_u[c][r]],  K_l = E S_u^H - F_u^H
elementwise, so every form of rgf_less_ref.py ('lr', 'rl', 'dense', and the clongdouble truth) has its flow.  A flow table
is flattened in negf_layered_gr_int's order: diagonal | upper | lower blocks.  Group tables, cuts (the sum of an upper
block: the flow from layer i into layer i + 1) and the weighted integral with real weights follow from it.

C_BOND is the accuracy constant of the calibrated bar (test_rgf_bond_host.test_calibration): a result passes when its
relative Frobenius error against the truth is at most C_BOND times the larger error of the two float64 sweep forms on that
input (errors floored at 2^-52).
Measured on the CPU over inputs() x ('L', 'R', 'LR') energy by energy and summed with the weights, without the selection
'LR' on the real cases a and c (see ZERO_FLOW): R = 24.04 (worst ratio between the two sweeps' errors: case d, terminal
L, E = 0 alone, 1.3e-13 left-to-right against 5.5e-15 right-to-left) -> C_BOND = 64; the sweeps' errors are 2.2e-16 ...
1.1e-12 and the dense form's 2.2e-16 ... 1.3e-13.

Two conditions shape every check:
  ZERO_FLOW  For real symmetric F, S and real E the total A (selection 'LR') is real, so the flow is exactly zero and a
             relative error means nothing; the float64 forms give 1e-19 ... 1e-15 there.  The flow is linear in A,
             |d flow| <= 2 |K| |dA|, so such a table is checked as max|flow| <= bar_A max|K| max|A| with bar_A the calibrated
             bar of the A blocks themselves (rgf_less_ref.bar_single) -- zero_bar().
  cuts       A cut cancels heavily (on case c sum|flow_u| reaches 134 against T = 0.79): its error is judged against
             bar x sum|flow_u| of its block, not against |T| -- cut_bar().
"""
import functools

import numpy as np

import rgf_less_ref as lr
import rgf_ref as rr
import xprec

LD = np.clongdouble
R_MEASURED = 24.04     # test_rgf_bond_host.test_calibration measures it again and asserts both
C_BOND = 64.0          # smallest power of two >= 2 R_MEASURED
SELECTIONS = lr.SELECTIONS
EPS = 2.0 ** -52


def zero_flow(c, sel):
    """the flow of this selection is exactly zero at real energies (real case, all terminals together)"""
    return c.real and sel == "LR"


# --------------------------------------------------------------------------- K and the flow of given A blocks
def k_blocks(c, E, dtype=complex):
    """(K_ii, K_{i,i+1}, K_{i+1,i}) of K = E S - F, no self-energies; the lower blocks are the stored conjugate transposes"""
    E = dtype(E)
    L = len(c.sizes)
    Sd = [np.asarray(b).astype(dtype) for b in c.S_diag]; Fd = [np.asarray(b).astype(dtype) for b in c.F_diag]
    Su = [np.asarray(b).astype(dtype) for b in c.S_up]; Fu = [np.asarray(b).astype(dtype) for b in c.F_up]
    return ([E * Sd[i] - Fd[i] for i in range(L)], [E * Su[i] - Fu[i] for i in range(L - 1)],
            [E * Su[i].conj().T - Fu[i].conj().T for i in range(L - 1)])


def flow_blocks(c, E, Ad, Au, dtype=complex):
    """(diagonal, upper, lower) flow blocks from the diagonal and upper blocks of A"""
    Kd, Ku, Kl = k_blocks(c, E, dtype)
    fd = [2 * (Kd[i] * np.conj(Ad[i])).imag for i in range(len(Kd))]
    fu = [2 * (Ku[i] * np.conj(Au[i])).imag for i in range(len(Ku))]
    fl = [2 * (Kl[i] * np.asarray(Au[i]).T).imag for i in range(len(Ku))]
    return fd, fu, fl


def split(sizes, flat):
    """a table flattened in negf_layered_gr_int's order -> (diagonal, upper, lower) blocks"""
    d, u, l, o = [], [], [], 0
    for n in sizes:
        d.append(flat[o:o + n * n].reshape(n, n)); o += n * n
    for a, b in zip(sizes[:-1], sizes[1:]):
        u.append(flat[o:o + a * b].reshape(a, b)); o += a * b
    for a, b in zip(sizes[:-1], sizes[1:]):
        l.append(flat[o:o + a * b].reshape(b, a)); o += a * b
    assert o == flat.size
    return d, u, l


def flat_of(blocks):
    d, u, l = blocks
    return np.concatenate([np.asarray(b).ravel() for b in list(d) + list(u) + list(l)])


def flow_of_single(c, E, single, dtype=complex):
    """the flattened flow table of one energy from rgf_less_ref's flattened A blocks of that energy"""
    Ad, Au, _ = split(c.sizes, np.asarray(single))
    return flat_of(flow_blocks(c, E, Ad, Au, dtype))


def scale_of(c, E, single):
    """max|K| max|A| of an energy: what an absolute error of a flow entry is measured in"""
    Kd, Ku, _ = k_blocks(c, E)
    return float(max(np.abs(b).max() for b in Kd + Ku)) * float(np.abs(np.asarray(single).astype(complex)).max())


def group_tables(blocks, loc, g):
    """host sum of flow blocks into group tables: loc[i] = the group of each orbital of layer i inside its layer, g[i] the
    number of groups; the orbitals of a group in ascending order"""
    d, u, l = blocks
    L = len(d)

    def summed(blk, i, j):
        out = np.zeros((g[i], g[j]), dtype=np.asarray(blk).dtype)
        for a in range(g[i]):
            rows = np.asarray(blk)[loc[i] == a]
            for b in range(g[j]):
                out[a, b] = rows[:, loc[j] == b].sum()
        return out
    return ([summed(d[i], i, i) for i in range(L)], [summed(u[i], i, i + 1) for i in range(L - 1)],
            [summed(l[i], i + 1, i) for i in range(L - 1)])


def cuts(c, flat):
    """[L - 1]: the sum of each upper block, and sum|.| of it"""
    _, u, _ = split(c.sizes, np.asarray(flat))
    return np.array([b.sum() for b in u]), np.array([np.abs(b).sum() for b in u])


def weights_of(tag, m):
    """real weights of the integral: rgf_less_ref's for the cases, a ramp for the contour (its own are complex)"""
    return np.array([0.4, 0.7, 1.1, 1.6]) if m == 4 else 0.3 + 0.1 * np.arange(m)


# --------------------------------------------------------------------------- entries
def _entry_from(c, E, sel, singles, errA):
    """singles: {form: [m, pattern] A blocks}; errA: {form: per-energy errors of the A blocks}"""
    w = weights_of(c.name, len(E))
    ent = dict(case=c, E=np.asarray(E), w=w, sel=sel, zero=zero_flow(c, sel) and not np.iscomplexobj(E))
    for form in ("truth", "lr", "rl", "dense"):
        dtype = LD if form == "truth" else complex
        flow = np.array([flow_of_single(c, E[j], singles[form][j], dtype) for j in range(len(E))])
        acc = np.zeros(flow.shape[1], dtype=flow.dtype)
        for k in range(len(E)):
            acc = acc + flow.dtype.type(w[k]) * flow[k]
        ent[form] = dict(flow=flow, int=acc)
    ent["scale"] = [scale_of(c, E[j], singles["truth"][j]) for j in range(len(E))]
    ent["errA_lr"], ent["errA_rl"] = errA["lr"], errA["rl"]
    for form in ("lr", "rl", "dense"):
        ent["err1_" + form] = [rr.rel_err(ent[form]["flow"][j], ent["truth"]["flow"][j]) for j in range(len(E))]
        ent["err_" + form] = rr.rel_err(ent[form]["int"], ent["truth"]["int"])
    return ent


@functools.lru_cache(maxsize=None)
def truth_table():
    """{(tag, sel): dict(case, E, w, sel, zero, truth / lr / rl / dense: dict(flow [m, pattern], int [pattern]), scale [m],
    err1_* [m] energy by energy, err_* of the integral)} over rgf_less_ref.inputs() -- computed once per process from
    rgf_less_ref.truth_table()'s A blocks and shared by the tests that need it"""
    table = {}
    for key, le in lr.truth_table().items():
        tag, sel = key
        singles = {form: le[form]["single"] for form in ("truth", "lr", "rl", "dense")}
        errA = {form: [e[0] for e in le["err1_" + form]] for form in ("lr", "rl")}
        table[key] = _entry_from(le["case"], le["E"], sel, singles, errA)
    return table


@functools.lru_cache(maxsize=None)
def tiny_case():
    """layers of 1, 17 and 16 orbitals, complex Hermitian: a layer of one orbital, and blocks one past and exactly at the
    16-wide tile of the transposed kernels.  Not an input of the calibration; its bar uses the same C_BOND."""
    return rr.RCase("t", (1, 17, 16), 61, hermitian_complex=True)


@functools.lru_cache(maxsize=None)
def tiny_entry(sel):
    c = tiny_case()
    E = c.energies
    xprec.require_extended()
    cols = np.concatenate([c.left_global, c.right_global])
    singles = {form: [] for form in ("truth", "lr", "rl", "dense")}
    for e in E:
        (X, _), = xprec.refine([(rr.assembled(c, e, LD), cols)], [2.0 ** -55])
        Ad, Au = lr._from_columns(c, (X[:, :c.left.size], X[:, c.left.size:]), sel, LD)
        singles["truth"].append(lr.flat_of(Ad, Au))
        for form, fn in (("lr", lr.sweep_lr), ("rl", lr.sweep_rl), ("dense", lr.dense)):
            singles[form].append(lr.flat_of(*fn(c, e, sel)))
    errA = {form: [rr.rel_err(singles[form][j], singles["truth"][j]) for j in range(len(E))] for form in ("lr", "rl")}
    return _entry_from(c, E, sel, singles, errA)


# --------------------------------------------------------------------------- bars
def bar_single(ent, j):
    """what the flow table of energy j may err by, relative Frobenius"""
    return C_BOND * max(ent["err1_lr"][j], ent["err1_rl"][j])


def bar_int(ent):
    """... and the weighted integral"""
    return C_BOND * max(ent["err_lr"], ent["err_rl"])


def zero_bar(ent, j):
    """an exactly vanishing table (ent['zero']): max|flow| may reach this -- the flow is linear in A, |d flow| <= 2 |K| |dA|,
    and dA is what the calibrated bar of the A blocks allows (relative Frobenius, against max|A| <= |A|_F)"""
    return lr.C_LESS * max(ent["errA_lr"][j], ent["errA_rl"][j]) * ent["scale"][j]


def check_table(ent, j, got):
    """(measure, bar) of a flow table of energy j: the relative error and its bar, or for a vanishing table max|flow| and
    the zero bar"""
    if ent["zero"]:
        return float(np.abs(got).max()), zero_bar(ent, j)
    return rr.rel_err(got, ent["truth"]["flow"][j]), bar_single(ent, j)


def cut_bar(ent, j):
    """[L - 1] what the cuts of energy j may err by: the table's bar times sum|flow_u| of the block"""
    _, mag = cuts(ent["case"], np.asarray(ent["truth"]["flow"][j]).astype(float))
    rel = zero_bar(ent, j) / ent["scale"][j] if ent["zero"] else bar_single(ent, j)
    return rel * mag
