"""Numpy restatement of the eigenchannel scattering states (negf_channel_states) and of the eigenvector solver behind
them (negf_eigh_batched), the inputs the host and the GPU tests share, and the calibrated constant of the eigh bounds.

Definition (source contact s, destination d, orbital lists I_s, I_d):
    Gamma_c = i (Sigma_c - Sigma_c^H);  Gamma_s[I_s, I_s] = L L^H (pivoted Cholesky, 1e-14 relative cut, rank r);
    H = L^H G[I_d, I_s]^H Gamma_d[I_d, I_d] G[I_d, I_s] L;  H u_n = T_n u_n, T_n descending;
    psi_n = G[:, I_s] L u_n,  multiplied by the unit phase that makes its largest component real positive.
"""
import numpy as np

U_ROUND = 2.0 ** -53

# C of the eigh bounds  max_j ||A v_j - w_j v_j||_2 <= C K u ||A||_F  and  ||V^H V - I||_F <= C K u:  the smallest power
# of two that is at least twice the worst ratio numpy.linalg.eigh and jacobi_eigh (below) reach on eigh_random(K), K in
# EIGH_KS, and eigh_special().  Calibrated on the CPU (test_channel_states_host.py recomputes the ratios):
#   numpy.linalg.eigh   residual 2.20 (K = 2)   orthonormality 3.12 (K = 17)
#   jacobi_eigh         residual 1.68 (K = 3)   orthonormality 19.53 (K = 50, five ten-fold eigenvalues; 13.97 at K = 96)
# worst 19.53, twice that 39.1 -> C = 64.
EIGH_C = 64.0


def gamma(sig):
    return 1j * (sig - sig.conj().T)


def support(sig):
    return np.nonzero(np.any(sig != 0, axis=0) | np.any(sig != 0, axis=1))[0]


def block_sigma(n, idx, rng, scale=0.15, rank=None):
    """A contact self-energy confined to the orbitals idx: -i (PSD coupling of the given rank) / 2 + a Hermitian shift."""
    K = len(idx)
    r = K if rank is None else rank
    A = rng.standard_normal((K, r)) + 1j * rng.standard_normal((K, r))
    gam = scale * (A @ A.conj().T) / r
    B = rng.standard_normal((K, K)); h = 0.05 * (B + B.T)
    s = np.zeros((n, n), complex)
    s[np.ix_(idx, idx)] = h - 0.5j * gam
    return s


def pivoted_cholesky(G, cut=1e-14):
    """G ~ L L^H, L [K, r]: pivots by the largest remaining diagonal (lowest index on ties), truncated where it is
    <= cut * max diag G."""
    G = np.array(G, dtype=complex)
    K = G.shape[0]
    d = G.diagonal().real.copy()
    done = np.zeros(K, bool)
    cols = []
    thr = None
    for _ in range(K):
        rem = np.where(done, -np.inf, d)
        p = int(np.argmax(rem))
        if thr is None:
            thr = cut * rem[p]
        if not (rem[p] > thr and rem[p] > 0.0):
            break
        done[p] = True
        l = np.where(done, 0.0, G[:, p] / np.sqrt(d[p]))
        l[p] = np.sqrt(d[p])
        cols.append(l)
        G = G - np.outer(l, l.conj())
        d = d - np.abs(l) ** 2
    return np.array(cols).T.reshape(K, len(cols))


def fix_gauge(psi):
    """Each row times the unit phase that makes its component of largest |psi_i|^2 real positive (lowest index on ties)."""
    out = np.array(psi, dtype=complex)
    for k in range(out.shape[0]):
        i = int(np.argmax(np.abs(out[k]) ** 2))
        a = abs(out[k, i])
        if a > 0:
            out[k] = out[k] * (out[k, i].conj() / a)
    return out


def channel_states_ref(G, gam_s, gam_d, Is, Id):
    """(T [r], psi [r, n]) of the source-side form; gam_s / gam_d the n x n couplings, Is / Id the orbital lists."""
    L = pivoted_cholesky(gam_s[np.ix_(Is, Is)])
    Gds = G[np.ix_(Id, Is)]
    H = L.conj().T @ Gds.conj().T @ gam_d[np.ix_(Id, Id)] @ Gds @ L
    w, U = np.linalg.eigh(0.5 * (H + H.conj().T))
    w, U = w[::-1], U[:, ::-1]
    psi = (G[:, Is] @ L @ U).T
    return w, fix_gauge(psi)


def identity_errors(T, psi, G, gam_s, gam_d):
    """The four identities' errors for all r channels: (orthogonality |Psi^H Gamma_d Psi - diag T|_max / max T,
    sum rule |sum T - Re Tr[Gamma_d G Gamma_s G^H]| relative, spectral ||Psi Psi^H - G Gamma_s G^H||_F relative)."""
    P = psi.T                                                   # n x r
    tmax = max(np.max(np.abs(T)), 1e-300)
    orth = np.max(np.abs(P.conj().T @ gam_d @ P - np.diag(T))) / tmax
    A = G @ gam_s @ G.conj().T
    tr = np.real(np.trace(gam_d @ A))
    srule = abs(T.sum() - tr) / max(abs(tr), 1e-300)
    spec = np.linalg.norm(P @ P.conj().T - A) / np.linalg.norm(A)
    return orth, srule, spec


def clusters(T, sep):
    """Index groups of the descending T whose members are closer than sep to a neighbour of the group; every group is
    separated from all other values by >= sep."""
    out, cur = [], [0]
    for k in range(1, len(T)):
        if abs(T[k - 1] - T[k]) < sep:
            cur.append(k)
        else:
            out.append(cur); cur = [k]
    out.append(cur)
    return out


def projector(rows):
    """Orthogonal projector on the span of the given states (rows), by QR."""
    Q, _ = np.linalg.qr(np.asarray(rows).T)
    return Q @ Q.conj().T


# ------------------------------------------------------------------------------- shared inputs
CONST_CASES = [(5, 9, 40), (9, 5, 40), (40, 30, 130)]          # (K_s, K_d, n)


def const_case(Ks, Kd, n, rank=None):
    """F, S, (Sigma_src, Sigma_dst) on the first K_s / last K_d orbitals, and three real energies, the last one 5e-4
    above an eigenvalue of (F, S)."""
    from helpers import random_system
    F, S = random_system(n, Ks * 100 + Kd)
    rng = np.random.default_rng(n + Ks)
    Is = np.arange(Ks); Id = np.arange(n - Kd, n)
    ss = block_sigma(n, Is, rng, rank=rank); sd = block_sigma(n, Id, rng)
    lam = np.sort(np.linalg.eigvals(np.linalg.solve(S, F)).real)
    E = np.array([-0.7, 0.45, lam[n // 2] + 5e-4])
    return dict(F=F, S=S, ss=ss, sd=sd, Is=Is, Id=Id, E=E)


def rank_deficient_case():
    """K_s = 9 with a rank-3 Gamma_s."""
    return const_case(9, 5, 40, rank=3)


def case_green(case, e):
    return np.linalg.inv(e * case["S"] - case["F"] - case["ss"] - case["sd"])


EIGH_BOUNDARY = (69, 70)                # the last K whose accumulator lives in LDS, the first whose lives in global memory
EIGH_KS = (1, 2, 3, 17, 50, 64, 96) + EIGH_BOUNDARY


def eigh_random(K, m=5):
    rng = np.random.default_rng(1000 + K)
    A = rng.standard_normal((m, K, K)) + 1j * rng.standard_normal((m, K, K))
    return A + A.conj().transpose(0, 2, 1)


def eigh_special():
    """The spectra of test_eigvalsh_special_spectra (exactly repeated eigenvalues, diagonal, zero, tiny) and a rank-one
    matrix and 2^+-64 scalings."""
    rng = np.random.default_rng(3)
    mats = []
    for K, vals in ((50, np.repeat([1.0, -2.0, 3.0, 0.5, 0.0], 10)), (64, np.repeat([2.0, -1.0], 32)),
                    (17, np.full(17, 0.7))):
        U, _ = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))
        mats.append((U * vals) @ U.conj().T)
    mats.append(np.diag(rng.standard_normal(40)).astype(complex))
    mats.append(np.zeros((30, 30), complex))
    X = rng.standard_normal((33, 33)) + 1j * rng.standard_normal((33, 33))
    mats.append(1e-8 * (X + X.conj().T))
    v = rng.standard_normal(24) + 1j * rng.standard_normal(24)
    mats.append(np.outer(v, v.conj()))
    mats.append((X + X.conj().T) * 2.0 ** 64)
    mats.append((X + X.conj().T) * 2.0 ** -64)
    return mats


def eigh_ratios(A, w, V):
    """(max_j ||A v_j - w_j v_j||_2 / (K u ||A||_F), ||V^H V - I||_F / (K u)) of one matrix; A read as numpy.linalg.eigh
    reads it (lower triangle).  A zero matrix has the residual ratio 0 when its residual is exactly zero."""
    K = A.shape[0]
    Ah = np.tril(A) + np.tril(A, -1).conj().T
    Ah[np.diag_indices(K)] = Ah.diagonal().real
    res = np.max(np.linalg.norm(Ah @ V - V * w, axis=0))
    fro = np.linalg.norm(Ah)
    rr = 0.0 if res == 0.0 else res / (K * U_ROUND * fro) if fro > 0 else np.inf
    return rr, np.linalg.norm(V.conj().T @ V - np.eye(K)) / (K * U_ROUND)


def jacobi_eigh(A, max_sweeps=30, stop_eps=None):
    """Plain numpy restatement of the device solver: cyclic two-sided complex Jacobi in round-robin order, K/2 disjoint
    rotations per step (phase of a_pq removed, real rotation zeroes it), the same skip threshold, power-of-two scaling
    and stop rule, with the rotations accumulated into V.  (w ascending, V).  stop_eps replaces the machine epsilon of the stop
    rule alone (tests/xprec_channels.py plants an early stop with it); the skip threshold stays."""
    K = A.shape[0]
    Ah = np.tril(A) + np.tril(A, -1).conj().T
    Ah[np.diag_indices(K)] = Ah.diagonal().real
    N = K + (K & 1)
    amax = max(np.max(np.abs(Ah.real)), np.max(np.abs(Ah.imag)))
    ex = int(np.frexp(amax)[1]) if amax > 0 else 0
    M = np.zeros((N, N), complex)
    M[:K, :K] = np.ldexp(Ah.real, -ex) + 1j * np.ldexp(Ah.imag, -ex)
    X = np.eye(N, dtype=complex)
    fro2 = np.sum(np.abs(M) ** 2)
    eps = np.finfo(float).eps
    tol2 = (eps if stop_eps is None else stop_eps) ** 2 * fro2
    skip = eps * np.sqrt(fro2) / (4.0 * max(N, 1))
    Mr = N - 1
    for sweep in range(max_sweeps + 1):
        off = M - np.diag(M.diagonal())
        if np.sum(np.abs(off) ** 2) <= tol2 or sweep == max_sweeps:
            break
        for st in range(N - 1):
            J = np.eye(N, dtype=complex)
            rotated = []
            for P in range(N // 2):
                p, q = (Mr, st) if P == 0 else ((st + P) % Mr, (st - P + Mr) % Mr)
                b = M[p, q]
                ab = abs(b)
                if not ab > skip:
                    continue
                z = (M[q, q].real - M[p, p].real) / (2.0 * ab)
                t = (1.0 if z >= 0 else -1.0) / (abs(z) + np.sqrt(z * z + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0); s = t * c
                wph = b / ab
                J[p, p] = c; J[p, q] = s * wph; J[q, p] = -s * np.conj(wph); J[q, q] = c
                rotated.append((p, q))
            M = J.conj().T @ M @ J
            M = 0.5 * (M + M.conj().T)
            for p, q in rotated:
                M[p, q] = M[q, p] = 0.0
            X = X @ J
    w = np.ldexp(M.diagonal().real[:K], ex)
    order = np.argsort(w, kind="stable")
    return w[order], X[:K, :K][:, order]
