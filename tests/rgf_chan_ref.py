"""Case table, float64 restatement and numpy restatements of the wide kernels for the transmission eigenchannels of
layered devices (negf_layered_transmission_channels, k_eig_wide.hip), shared by test_rgf_chan_host.py (CPU) and
test_rgf_chan_gpu.py (MI355X).

Truth and bars are xprec_channels': a layered case (rgf_ref.RCase) becomes a ChanCase by to_dense() with the two terminal
blocks scattered into N x N self-energies.  The pair (a, b) of the layered call is (destination, source) of the ChanCase
-- transmission_channels(L, R) are the channels injected by R and collected by L -- and ChannelTruth.chan factors the
side the device factors (a unless K_b < K_a).  Every check is error <= C_CHAN beta_T (ratios_T(T, rank, "chan")).

Restatements:
  channels_f64      the call in float64: the corner block from rgf_ref.sweep_lr / sweep_rl (G[I_a, I_b] with a on the last
                    layer; a on layer 0 is the same sweep on the mirrored device), channel_states_ref.pivoted_cholesky or
                    wide_cholesky, LAPACK's eigvalsh or wide_eigvalsh.
  wide_cholesky     pchol_wide_kernel: left-looking, column k = (Gamma[:, p] - sum_{t<k} l_t conj(l_t[p])) / sqrt(d_p) from
                    the separately tracked diagonal d, pivot = largest remaining d (lowest index on ties), cut at
                    1e-14 max diag, stop at a non-positive d.
  wide_eigvalsh     eig_wide_kernel: power-of-two prescale, Householder reflections u = x + e^{i arg x_0} ||x|| e_0 on the
                    full-stored matrix (p = g B u, w = p - (g u^H p / 2) u, B -= u w^H + w u^H), keeping (d, e^2) only,
                    then bisection with Sturm counts: dstebz's widened Gershgorin interval, dlaebz's pivmin safeguard,
                    stop at 2^-56 of the tridiagonal's norm or when the interval stops shrinking.
"""
import functools

import numpy as np

import channel_states_ref as R
import rgf_ref as rr
import xprec_channels as xc

CUT = xc.CUT
EPS = np.finfo(float).eps
TINY = np.finfo(float).tiny


# --------------------------------------------------------------------------- the wide kernels in numpy
def wide_cholesky(G, cut=CUT, pivot="max"):
    """L [K, r] with G ~ L L^H as pchol_wide_kernel forms it; pivot="first" takes the lowest remaining index (a planted
    defect)."""
    G = np.array(G, dtype=complex)
    K = G.shape[0]
    d = G.diagonal().real.copy()
    done = np.zeros(K, bool)
    L = np.zeros((K, K), complex)
    thr = None
    k = 0
    for k in range(K + 1):
        if k == K:
            break
        rem = np.where(done, -np.inf, d)
        p = int(np.argmax(rem)) if pivot == "max" else int(np.argmin(done))
        if thr is None:
            thr = cut * (rem[p] if pivot == "max" else np.max(d))
        if not (rem[p] > thr and rem[p] > 0.0):
            break
        done[p] = True
        sp = np.sqrt(d[p])
        col = (G[:, p] - L[:, :k] @ L[p, :k].conj()) / sp
        col[done] = 0.0
        col[p] = sp
        L[:, k] = col
        d = d - np.abs(col) ** 2
    return L[:, :k].copy()


def tridiagonal(A):
    """(d [n], e2 [n - 1], ex): the real tridiagonal (diagonal, squared off-diagonal) of the prescaled lower triangle of
    A, and the exponent of the scale."""
    n = A.shape[0]
    Ah = np.tril(A) + np.tril(A, -1).conj().T
    Ah[np.diag_indices(n)] = Ah.diagonal().real
    amax = max(np.max(np.abs(Ah.real)), np.max(np.abs(Ah.imag))) if n else 0.0
    ex = int(np.frexp(amax)[1]) if amax > 0 else 0
    B = np.ldexp(Ah.real, -ex) + 1j * np.ldexp(Ah.imag, -ex)
    d = np.zeros(n); e2 = np.zeros(max(n - 1, 0))
    for k in range(n - 1):
        d[k] = B[k, k].real
        x = B[k, k + 1:].conj()
        xn2 = float(np.sum(x.real ** 2 + x.imag ** 2))
        e2[k] = xn2
        if not xn2 > 0.0:
            continue
        xn = np.sqrt(xn2)
        aa = abs(x[0])
        ph = x[0] / aa if aa > 0 else 1.0
        g = 1.0 / (xn * (xn + aa))
        u = x.copy(); u[0] = x[0] + ph * xn
        T = B[k + 1:, k + 1:]
        p = g * (T.conj().T @ u)                       # through the columns of B, as the kernel reads it
        kap = 0.5 * g * float(np.sum(u.real * p.real + u.imag * p.imag))
        w = p - kap * u
        B[k + 1:, k + 1:] = T - np.outer(u, w.conj()) - np.outer(w, u.conj())
    if n:
        d[n - 1] = B[n - 1, n - 1].real
    return d, e2, ex


def sturm(d, e2, x, pivmin):
    """number of eigenvalues below each x [j]"""
    q = d[0] - x
    q = np.where(np.abs(q) < pivmin, -pivmin, q)
    cnt = (q < 0).astype(int)
    for i in range(1, d.size):
        q = d[i] - x - e2[i - 1] / q
        q = np.where(np.abs(q) < pivmin, -pivmin, q)
        cnt += q < 0
    return cnt


def bisect(d, e2, rel_stop=None):
    """ascending eigenvalues of the tridiagonal; rel_stop: stop at rel_stop * norm instead of 2^-56 (a planted defect)"""
    n = d.size
    if n == 0:
        return np.zeros(0)
    e = np.sqrt(e2)
    el = np.concatenate([[0.0], e]); er = np.concatenate([e, [0.0]])
    gl, gu = float(np.min(d - el - er)), float(np.max(d + el + er))
    pivmin = TINY * max(1.0, float(np.max(e2, initial=0.0)))
    tnorm = max(abs(gl), abs(gu))
    gl -= 2.1 * tnorm * (0.5 * EPS) * n + 4.2 * pivmin
    gu += 2.1 * tnorm * (0.5 * EPS) * n + 4.2 * pivmin
    atol = tnorm * (2.0 ** -56 if rel_stop is None else rel_stop)
    lo = np.full(n, gl); hi = np.full(n, gu)
    j = np.arange(n)
    active = np.ones(n, bool)
    for _ in range(2200):
        mid = 0.5 * (lo + hi)
        active &= (mid > lo) & (mid < hi)
        if not active.any():
            break
        below = sturm(d, e2, mid, pivmin) <= j
        lo = np.where(active & below, mid, lo)
        hi = np.where(active & ~below, mid, hi)
        active &= ~(hi - lo <= atol)
    return 0.5 * (lo + hi)


def wide_eigvalsh(A, rel_stop=None):
    """ascending eigenvalues of the Hermitian A (lower triangle), as eig_wide_kernel computes them"""
    A = np.asarray(A, dtype=complex)
    if A.shape[0] == 0 or not np.any(np.tril(A)):
        return np.zeros(A.shape[0])
    d, e2, ex = tridiagonal(A)
    return np.ldexp(bisect(d, e2, rel_stop), ex)


def solver_spectra(K):
    """xprec_channels.solver_spectra(K); below K = 6, where its cluster of five eigenvalues beside K - 5 others does not
    exist, the same three families with the cluster as large as fits: min(K, 5) eigenvalues at gaps 1e-10 sqrt(K) beside
    max(K - 5, 0) separated ones."""
    if K >= 6:
        return xc.solver_spectra(K)
    rng = np.random.default_rng(500 + K)
    X = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
    X = X + X.conj().T
    D = np.logspace(0, -6, K)
    graded = D[:, None] * X * D[None, :]
    vals = 1.0 + 1e-10 * np.sqrt(K) * np.arange(K)
    Q, _ = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))
    cluster = (Q * vals) @ Q.conj().T
    cluster = 0.5 * (cluster + cluster.conj().T)
    mw = (K - 1) // 2
    W = np.zeros((K, K), complex)
    k = 2 * mw + 1
    W[np.arange(k), np.arange(k)] = np.abs(np.arange(k) - mw)
    W[np.arange(k - 1), np.arange(1, k)] = 1.0; W[np.arange(1, k), np.arange(k - 1)] = 1.0
    out = {"graded": graded, "cluster": cluster, "wilkinson": W}
    for name in list(out):
        for s in (64, -64):
            out[f"{name}*2^{s}"] = out[name] * 2.0 ** s
    return out


# --------------------------------------------------------------------------- the case table
def _with_rank(c, side, rank, seed):
    """the case with the coupling of one terminal replaced by one of exact rank `rank`: channel_states_ref.block_sigma's
    0.15 A A^H / rank, with the first three orbitals coupled 1e-8 times as strongly -- their diagonal lies below the cut
    of the factorisation, so that the pivot order decides what it keeps (lowest index first: rank 0)"""
    K = (c.left if side == "left" else c.right).size
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, rank)) + 1j * rng.standard_normal((K, rank))
    D = np.ones(K); D[:3] = 1e-8
    gam = D[:, None] * (0.15 * (A @ A.conj().T) / rank) * D[None, :]
    B = rng.standard_normal((K, K))
    setattr(c, "sig_" + side, 0.05 * (B + B.T) - 0.5j * gam)
    return c


@functools.lru_cache(maxsize=None)
def wide_cases():
    """{tag: (RCase, energies)}: the wide shapes of the issue, two energies each"""
    left = np.concatenate([np.arange(60), np.arange(70, 120)])
    both = rr.RCase("wide-both", (130, 40, 120), 61, hermitian_complex=True, left=left, right=np.arange(20, 120))
    edge = rr.RCase("wide-97", (100, 20, 150), 62, left=np.arange(3, 100), right=np.arange(150))
    rank = _with_rank(rr.RCase("wide-rank33", (128, 20, 140), 63, hermitian_complex=True, left=np.arange(128),
                               right=np.arange(5, 135)), "left", 33, 64)
    E = np.array([-0.7, 0.45])
    return {"both": (both, E), "edge": (edge, E), "rank": (rank, E)}


@functools.lru_cache(maxsize=None)
def tiny_case():
    """one- and two-orbital terminals"""
    return rr.RCase("tiny", (4, 6, 5), 65, hermitian_complex=True, left=[2], right=[0, 3])


def small_cases():
    """rgf_ref.cases() a, b, d and the tiny device: K = 1 .. 4"""
    cs = rr.cases()
    return {"a": cs[0], "b": cs[1], "d": cs[3], "tiny": tiny_case()}


def chan_case(c, E, a="right", name=None):
    """The ChanCase of the layered call with a = the right (last layer) or the left (layer 0) terminal: a is the
    destination, the other terminal the source."""
    F, S = c.to_dense(complex)
    N = c.N
    sl = np.zeros((N, N), complex); sl[np.ix_(c.left_global, c.left_global)] = c.sig_left
    sr = np.zeros((N, N), complex); sr[np.ix_(c.right_global, c.right_global)] = c.sig_right
    if a == "right":
        return xc.ChanCase(name or f"{c.name} a=right", F, S, c.left_global, c.right_global, E, ss=sl, sd=sr)
    return xc.ChanCase(name or f"{c.name} a=left", F, S, c.right_global, c.left_global, E, ss=sr, sd=sl)


def host_table():
    """[(tag, RCase, energies, a)]: what the host tests run the restatements on"""
    w = wide_cases()
    out = [("both a=right", *w["both"], "right"), ("both a=left", *w["both"], "left"),
           ("edge a=left", *w["edge"], "left"), ("edge a=right", *w["edge"], "right"),
           ("rank a=left", *w["rank"], "left")]
    cs = rr.cases()
    out.append(("c near-eigenvalue", cs[2], cs[2].energies[[0, 3]], "right"))
    out.append(("b", cs[1], cs[1].energies[:2], "right"))
    return out


@functools.lru_cache(maxsize=None)
def truths_of(tag):
    """(ChanCase, [ChannelTruth]) of an entry of host_table(), computed once per process"""
    for t, c, E, a in host_table():
        if t == tag:
            cc = chan_case(c, E, a)
            return cc, xc.truths(cc)
    raise KeyError(tag)


@functools.lru_cache(maxsize=None)
def small_truths(name, a):
    """(RCase, energies, ChanCase, [ChannelTruth]) of an entry of small_cases() with a = "right" or "left": its first
    two energies, computed once per process"""
    c = small_cases()[name]
    E = c.energies[:2]
    cc = chan_case(c, E, a)
    return c, E, cc, xc.truths(cc)


def check_T(label, truths, T, which="chan", bars=1.0):
    """Every energy of T [m, nchan] against its truth: exact zeros beyond the rank, descending order, and the three
    ratios_T (values, beyond the rank, sum rule) <= bars * C_CHAN beta_T.  Prints one ACC line, returns the worst ratios."""
    worst = np.zeros(3)
    for m, t in enumerate(truths):
        r = xc.device_rank(T[m])
        assert np.all(T[m, r:] == 0.0) and np.all(np.diff(T[m, :r]) <= 0), (label, m, r)
        worst = np.maximum(worst, np.array(t.ratios_T(T[m], r, which)) / xc.C_CHAN)
    print(f"ACC layered channels {label}: kappa <= {max(t.kappa for t in truths):.1e} "
          f"T {worst[0]:.3g} rank {worst[1]:.3g} sum {worst[2]:.3g}")
    assert np.all(worst <= bars), (label, worst)
    return worst


# --------------------------------------------------------------------------- the call in float64
def corner(c, E, a, sweep="lr"):
    """G[I_a, I_b] from a float64 sweep: a on the last layer reads the sweep's G[I_right, I_left], a on layer 0 the same
    block of the mirrored device"""
    fn = rr.sweep_lr if sweep == "lr" else rr.sweep_rl
    return fn(c if a == "right" else c.mirrored(), E)[3]


def channels_f64(c, E, a="right", sweep="lr", eig="lapack", chol="ref", gab="H", pivot="max", rel_stop=None):
    """(T [min(K_a, K_b)] descending with zeros beyond the rank, rank) of one energy.  eig: "lapack" or "wide"; chol: "ref"
    (channel_states_ref.pivoted_cholesky) or "wide".  Planted defects: gab="T" uses G_ab^T for G_ab^H, pivot="first" the
    lowest index, rel_stop a loose bisection."""
    Gab = corner(c, E, a, sweep)
    sa, sb = (c.sig_right, c.sig_left) if a == "right" else (c.sig_left, c.sig_right)
    ga, gb = R.gamma(np.asarray(sa, dtype=complex)), R.gamma(np.asarray(sb, dtype=complex))
    Ka, Kb = ga.shape[0], gb.shape[0]
    mirror = Kb < Ka
    gs, go = (gb, ga) if mirror else (ga, gb)
    if pivot == "first":
        L = wide_cholesky(gs, pivot="first") if chol == "wide" else xc.pivoted_cholesky(gs, CUT, "first")
    else:
        L = wide_cholesky(gs) if chol == "wide" else R.pivoted_cholesky(gs)
    r = L.shape[1]
    GabH = Gab.conj().T if gab == "H" else Gab.T
    if mirror:                                                      # s = b: H = L^H G_ab^H Gamma_a G_ab L
        Z = L.conj().T @ GabH
        H = (Z @ go) @ Z.conj().T
    else:                                                           # s = a: H = L^H G_ab Gamma_b G_ab^H L
        H = (L.conj().T @ Gab @ go) @ (GabH @ L)
    H = 0.5 * (H + H.conj().T)
    if r == 0:
        w = np.zeros(0)
    elif eig == "lapack":
        w = np.linalg.eigvalsh(H)
    else:
        w = wide_eigvalsh(H, rel_stop)
    T = np.zeros(min(Ka, Kb)); T[:r] = w[::-1]
    return T, r
