"""Extended-precision truth, case table and bars for the Bethe-lattice self-energy kernel (k_bethe.hip; the formulas of
oracle.bethe_sigmaK / bethe_sigma_surface / bethe_atom_sigma / bethe_cluster_sigma_total).  Shared by
test_bethe_accuracy_host.py (CPU) and test_bethe_accuracy_gpu.py (MI355X).

Truth.  np.clongdouble from the float64 inputs; z = E - i eta is formed in float64, as the kernel does:
    A = z I - H,  B_k = z S_k - V_k,  sigma_k = -i I,
    bulk sweep   : Sigma_tot = sum_k sigma_k frozen; k = 0..11 in order: g_k = inv(A - Sigma_tot + sigma[(k+6)%12])
                   (Gauss-Seidel: for k >= 6 that is this sweep's value), sigma_k <- mix B_k g_k B_k^H + (1-mix) sigma_k
    surface sweep: g = inv(A - sum_{k<9} s_k); k in {0,1,2,6,7,8}: s_k <- mix B_k g B_k^H + (1-mix) s_k
    stop         : diff = max|s - s_old| / max|s_old| <= conv or count == max_iter (or a fixed sweep count K).
Every 9x9 inverse goes through xprec.refine (with its convergence assertion) and its kappa_2 is recorded.  The same
loops run in complex128 with any inverse handed in (bulk / surface with ld=False): the calibration references and the
planted defects of test_bethe_accuracy_host.py.

Cases.  B1: the shipped Au / Au2 tables at eta 1e-6 and 1e-4, seven energies each (below the band, sp band, d band, two
band-edge points of a host scan for the largest kappa_2, two contour points).  B2: Au with core levels 1e3 / 1e5 on two
diagonal entries of H.  B3: Au with V times 32, where Gauss-Jordan exchanges rows in sweep 1.  B4: the inverse alone
(see b4_* below): S_k = 0, V_k = -I, mix = 1, one sweep, dyadic eta / Im E, so that sigma_k = g_k = ((x + i d) I - H)^-1
exactly for k < 6 on 9x9 real-symmetric versions of the xprec families.

Bars.
  * B4, k < 6: per column xprec.bar(9, kappa_2) with xprec.C_BAR, unchanged.  k >= 6 inverts M2 = A - Sigma_tot + g_hat
    with the device's own g_hat = g + dg, ||dg||_F <= bar(9, kappa_1) ||g||_F, formed with one rounding per entry (the
    last add; everything before it is exact for these inputs): to first order inv(M2 + dM) e_j - G2 e_j = -G2 dM G2 e_j,
    so per column  bar(9, kappa_2(M2)) + ||G2||_2 (bar(9, kappa_1) ||g||_F + u ||M2||_F).  (A norm bound: at the
    ladder's kappa_2 ~ 1e9 point it exceeds 1, since the error of g lies along the near-null vector, where G2 is small;
    the k >= 6 check has teeth at the well-conditioned points.)
  * sweeps and converged results, per direction:  ||sigma_hat_k - sigma_k||_F <= C_BETHE u kappa_max ||sigma_k||_F,
    kappa_max the largest kappa_2 among the matrices the truth inverted in that loop (the surface loop: its own).
    C_BETHE = 4 is calibrated, not chosen: the smallest power of two at least twice the worst ratio
    error / (u kappa_max ||sigma_k||) of two float64 references over B1-B3 x K in {1, 3, 10, 25} x (bulk, surface,
    cluster, atom assembly): oracle.bethe_* (LAPACK inverse) and the same loops with xprec.gauss_jordan(pivot="abs1").
    Measured worst ratios (test_bethe_accuracy_host.py::test_calibration): LAPACK 1.63, Gauss-Jordan 1.70 (both on
    B1 Au eta = 1e-4), so 2 x 1.70 = 3.4 -> 4.
  * sums of blocks (atom assembly: 9 surface blocks minus the attached ones; cluster: 12 bulk blocks minus one): the
    bars of the summed blocks plus gamma_21 sum ||sigma_k|| for the at most 21 additions.
No norm-propagated first-order bound is used: its per-sweep factor exceeds 1 in band while the iteration contracts.
"""
import functools
import os

import numpy as np

import xprec
from xprec import C_BAR, LD, U, gamma_n, kappa2
from xprec_chain import mm

D = 9
PLANE = (0, 1, 2, 6, 7, 8)
C_BETHE = 4.0
K_CHECKED = (1, 3, 10, 25)
AMBIGUOUS_REL = 1e-6                 # |diff - conv| <= AMBIGUOUS_REL * conv at the stopping sweep or the one before
AMBIGUOUS_CAP = 0.10                 # at most this fraction of a free-running grid may be ambiguous
MAX_ITER = 1000                      # config.BETHE_MAX_ITER


def _nf(X):
    return float(np.linalg.norm(np.asarray(X, dtype=np.complex128)))


def _n2(X):
    return float(np.linalg.norm(np.asarray(X, dtype=np.complex128), 2))


# --------------------------------------------------------------------------- #
# lattices
# --------------------------------------------------------------------------- #
class Lattice:
    """One Bethe atom: H [9,9], S / V [12,9,9] (float64), eta, and the energies its tests run."""

    def __init__(self, name, H, S, V, eta, energies=()):
        self.name, self.eta = name, float(eta)
        self.H = np.ascontiguousarray(H, dtype=np.float64)
        self.S = np.ascontiguousarray(S, dtype=np.float64)
        self.V = np.ascontiguousarray(V, dtype=np.float64)
        self.energies = np.asarray(energies, dtype=np.complex128)

    def z(self, E, eta_sign=-1.0):
        E = complex(E)
        return complex(E.real, E.imag + eta_sign * self.eta)       # the kernel: (e.x, e.y - eta)

    def with_energies(self, energies, name=None):
        return Lattice(name or self.name, self.H, self.S, self.V, self.eta, energies)


@functools.lru_cache(maxsize=None)
def shipped(name, eta):
    """The shipped parameter table `name` on the geometry of test_gpu_parity._bethe_atom."""
    from gaunegf_amd.surfGBethe import construct_sk_matrix, gen_neighbors, lattice_file, read_bethe_params
    _, _, Vd, Sd, H0 = read_bethe_params(lattice_file(name))
    dirs = gen_neighbors(np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.2, 0.0]))
    S = np.stack([construct_sk_matrix(Sd, d) for d in dirs])
    V = np.stack([construct_sk_matrix(Vd, d) for d in dirs])
    return Lattice(f"{name} eta={eta:g}", H0, S, V, eta)


EDGE_GRID = np.linspace(-10.0, 8.0, 91)


def edge_energies(lat, count=2):
    """The `count` points of EDGE_GRID (no two adjacent) with the largest kappa_2 among the matrices of the last bulk
    sweep of the float64 fixed point run to conv = 1e-5 (at most 100 sweeps): the band-edge cases."""
    kap = np.empty(EDGE_GRID.size)
    for m, E in enumerate(EDGE_GRID):
        rec = KappaInv(np.linalg.inv)
        tr = bulk(lat, E, conv=1e-5, max_iter=100, inv=rec, ld=False, extra=0)
        kap[m] = rec.last_sweep(12)
    picked = []
    for m in np.argsort(-kap):
        if all(abs(int(m) - p) > 1 for p in picked):
            picked.append(int(m))
        if len(picked) == count:
            break
    return [float(EDGE_GRID[m]) for m in sorted(picked)]


B1_FIXED = {"Au": (-9.0, 6.0, -1.0), "Au2": (-9.0, 7.5, 2.5)}
"""Below the band, in the sp band, in the d band (the orbital-resolved density of states of the converged lattice:
test_bethe_accuracy_host.py::test_b1_energies)."""
B1_CONTOUR = (-2.0 + 0.3j, 0.3 + 2.0j)


@functools.lru_cache(maxsize=None)
def b1_cases():
    out = []
    for name in ("Au", "Au2"):
        for eta in (1e-6, 1e-4):
            lat = shipped(name, eta)
            out.append(lat.with_energies(list(B1_FIXED[name]) + edge_energies(lat) + list(B1_CONTOUR), "B1 " + lat.name))
    return out


CORE = ((1, 1e3), (5, 1e5))
B23_ENERGIES = (-5.0, 0.7, -2.0 + 0.3j)
B3_SCALE = 32.0


@functools.lru_cache(maxsize=None)
def b2_case():
    au = shipped("Au", 1e-6)
    H = au.H.copy()
    for i, v in CORE:
        H[i, i] += v
    return Lattice("B2 Au core", H, au.S, au.V, au.eta, B23_ENERGIES)


@functools.lru_cache(maxsize=None)
def b3_case():
    """Au with V times 32 (H is diagonal): sigma_k of sweep 1 carries off-diagonal entries of ~|32 V|^2 / 11 > 12, the
    size of the diagonal of the matrices that phase 1 (k >= 6) of sweep 1 inverts."""
    au = shipped("Au", 1e-6)
    return Lattice("B3 Au 32V", au.H, au.S, B3_SCALE * au.V, au.eta, B23_ENERGIES)


def sweep_cases():
    return b1_cases() + [b2_case(), b3_case()]


# --------------------------------------------------------------------------- #
# the loops (clongdouble truth; complex128 references and planted defects)
# --------------------------------------------------------------------------- #
class KappaInv:
    """An inverse that records kappa_2 of every matrix handed to it.  Without `inv`: the truth's inverse, all nine
    columns by xprec.refine in clongdouble."""

    def __init__(self, inv=None):
        self.inv, self.kappas = inv, []

    def __call__(self, A):
        k = kappa2(A)
        self.kappas.append(k)
        if self.inv is not None:
            return self.inv(A)
        X, _ = xprec.refine([(A, np.arange(D))], [max(1e-3 * xprec.bar(D, k, 1.0), 2.0 ** -58)])[0]
        return X

    def last_sweep(self, per_sweep):
        return max(self.kappas[-per_sweep:])


def _setup(lat, E, ld, eta_sign=-1.0):
    z = lat.z(E, eta_sign)
    if ld:
        A = LD(z) * np.eye(D, dtype=LD) - lat.H.astype(LD)
        B = LD(z) * lat.S.astype(LD) - lat.V.astype(LD)
    else:
        A = z * np.eye(D) - lat.H
        B = z * lat.S - lat.V
    return A, B


def _bgb(Bk, g, ld):
    return mm(mm(Bk, g), Bk.conj().T) if ld else Bk @ g @ Bk.conj().T


def _diff(new, old):
    return float(np.max(np.abs(new - old)) / np.max(np.abs(old)))


class Trace:
    """What a loop leaves: `at[c]` = the iterate after c sweeps (the checkpoints asked for, or around the stopping
    count), diffs[c-1] / kappa[c-1] = diff and the running largest kappa_2 after sweep c, count = where it stopped."""

    def __init__(self):
        self.at, self.diffs, self.kappa, self.count = {}, [], [], 0

    def ambiguous(self, conv):
        near = [abs(d - conv) <= AMBIGUOUS_REL * conv for d in self.diffs[max(self.count - 2, 0):self.count]]
        return any(near)

    def converged(self, conv):
        return self.count > 0 and self.diffs[self.count - 1] <= conv


def _drive(step, start, K, conv, max_iter, rec, keep, extra):
    """Run `step` from `start`: K sweeps, or free with the kernel's stop rule plus `extra` sweeps beyond the stop (so
    that the iterate at count + 1 exists).  Fixed K keeps the iterates in `keep`; free running those from count - 1."""
    tr = Trace()
    sig, count, diff = start, 0, np.inf
    tr.at[0] = sig.copy()
    stop = None
    while True:
        if stop is None:
            if K is not None:
                if count >= K:
                    stop = count
            elif not (diff > conv and count < max_iter):
                stop = count
        if stop is not None and (K is not None or count >= stop + extra):
            break
        sig, diff = step(sig)
        count += 1
        tr.diffs.append(diff)
        tr.kappa.append(max(rec.kappas))
        tr.at[count] = sig.copy()
        if K is None:
            tr.at.pop(count - 3, None)
        elif keep is not None and count - 1 not in keep:
            tr.at.pop(count - 1, None)
    tr.count = stop
    return tr


def bulk(lat, E, mix=0.5, K=None, conv=None, max_iter=MAX_ITER, inv=None, ld=True, keep=None, extra=1,
         jacobi=False, unfrozen=False, eta_sign=-1.0):
    """The bulk loop.  inv: a KappaInv (the truth's by default) or any callable.  Planted defects: jacobi (phase 1 reads
    the previous sweep's sigma), unfrozen (Sigma_tot recomputed for every direction), eta_sign = +1."""
    rec = inv if isinstance(inv, KappaInv) else KappaInv(inv)
    assert ld == (rec.inv is None)
    A, B = _setup(lat, E, ld, eta_sign)
    start = np.stack([-1j * np.eye(D)] * 12).astype(LD if ld else np.complex128)

    def step(sig):
        old = sig.copy()
        sig = sig.copy()
        tot = np.sum(sig, axis=0)
        for k in range(12):
            if unfrozen:
                tot = np.sum(sig, axis=0)
            src = old if jacobi else sig
            g = rec(A - tot + src[(k + 6) % 12])
            sig[k] = mix * _bgb(B[k], g, ld) + (1 - mix) * old[k]
        return sig, _diff(sig, old)
    return _drive(step, start, K, conv, max_iter, rec, keep, extra)


def surface(lat, E, sigK, mix=0.5, K=None, conv=None, max_iter=MAX_ITER, inv=None, ld=True, keep=None, extra=1,
            plane=PLANE, eta_sign=-1.0):
    """The surface loop from the bulk self-energies sigK (its first nine).  Planted defect: another `plane`."""
    rec = inv if isinstance(inv, KappaInv) else KappaInv(inv)
    assert ld == (rec.inv is None)
    A, B = _setup(lat, E, ld, eta_sign)
    start = np.array(sigK[:9]).astype(LD if ld else np.complex128)

    def step(s):
        old = s.copy()
        s = s.copy()
        g = rec(A - np.sum(old, axis=0))
        for k in plane:
            s[k] = mix * _bgb(B[k], g, ld) + (1 - mix) * old[k]
        return s, _diff(s, old)
    return _drive(step, start, K, conv, max_iter, rec, keep, extra)


def atom_sigma(s9, nInds):
    """oracle.bethe_atom_sigma in the dtype of s9, summed in the kernel's order; and the blocks it used."""
    used = list(range(9))
    out = s9[0].copy()
    for k in range(1, 9):
        out = out + s9[k]
    for nb in nInds:
        nb = int(nb)
        if nb < 0:
            nb += 9
        nb = min(max(nb, 0), 8)
        out = out - s9[nb]
        used.append(nb)
    return out, used


def cluster_blocks(sigK):
    """The twelve diagonal blocks Sigma_tot - sigma_{(k+6)%12} of oracle.bethe_cluster_sigma_total."""
    tot = np.sum(sigK, axis=0)
    return np.stack([tot - sigK[(k + 6) % 12] for k in range(12)])


# --------------------------------------------------------------------------- #
# bars
# --------------------------------------------------------------------------- #
def block_bars(sig, kappa_max, c=C_BETHE):
    """delta_k = c u kappa_max ||sigma_k||_F of every direction."""
    return np.array([c * U * kappa_max * _nf(s) for s in sig])


def sweep_ratio(got, sig, kappa_max, c=C_BETHE):
    """worst over the directions of ||got_k - sigma_k||_F / delta_k."""
    err = np.array([_nf(np.asarray(g).astype(LD) - s) for g, s in zip(got, sig)])
    return float(np.max(err / block_bars(sig, kappa_max, c)))


def sum_bar(sig, used, kappa_max, c=C_BETHE):
    """The bar of a signed sum of the blocks sig[used]: their bars plus gamma_21 sum ||sigma_k||."""
    n = np.array([_nf(sig[k]) for k in used])
    return float(np.sum(c * U * kappa_max * n + gamma_n(21) * n))


def sum_ratio(got, true, sig, used, kappa_max, c=C_BETHE):
    return _nf(np.asarray(got).astype(LD) - true) / sum_bar(sig, used, kappa_max, c)


def cluster_ratio(got_blocks, sigK, kappa_max, c=C_BETHE):
    true = cluster_blocks(sigK)
    return max(sum_ratio(got_blocks[k], true[k], sigK, list(range(12)) + [(k + 6) % 12], kappa_max, c)
               for k in range(12))


class SweepTruth:
    """Bulk and surface truths of one (lattice, energy) at the sweep counts K_CHECKED: bulk[K] = sigma after K bulk
    sweeps, surf[K] = s after K bulk and then K surface sweeps, with the kappa_max of each loop."""

    def __init__(self, lat, E, mix=0.5, ks=K_CHECKED):
        self.lat, self.E = lat, complex(E)
        tr = bulk(lat, E, mix, K=max(ks), keep=set(ks))
        self.bulk = {K: tr.at[K] for K in ks}
        self.kappa_bulk = {K: tr.kappa[K - 1] for K in ks}
        self.surf, self.kappa_surf = {}, {}
        for K in ks:
            ts = surface(lat, E, self.bulk[K], mix, K=K, keep={K})
            self.surf[K], self.kappa_surf[K] = ts.at[K], ts.kappa[K - 1]


@functools.lru_cache(maxsize=None)
def sweep_truth(case_index, m):
    lat = sweep_cases()[case_index]
    return SweepTruth(lat, lat.energies[m])


# --------------------------------------------------------------------------- #
# B4: the inverse alone
# --------------------------------------------------------------------------- #
B4_ETA = 2.0 ** -20


class B4Family:
    """A real-symmetric dyadic H and points (x, d): with S_k = 0, V_k = -I, mix = 1, one sweep, eta = 2^-20 and
    E = x + i (eta - 11 + d) the kernel's matrix for k < 6 is (x + i d) I - H exactly (test_b4_is_exact)."""

    def __init__(self, name, H, points):
        self.name, self.H, self.points = name, H, [(float(x), float(d)) for x, d in points]
        self.S = np.zeros((12, D, D))
        self.V = np.stack([-np.eye(D)] * 12)
        self.lat = Lattice("B4 " + name, H, self.S, self.V, B4_ETA)

    @property
    def energies(self):
        return np.array([complex(x, B4_ETA - 11.0 + d) for x, d in self.points])

    def matrix_ld(self, m):
        x, d = self.points[m]
        M = -self.H.astype(LD)
        M[np.arange(D), np.arange(D)] += LD(complex(x, d))
        return M


def _dyadic(X, bits):
    return np.round(np.asarray(X) * 2.0 ** bits) / 2.0 ** bits


def _sym(seed):
    T = np.random.default_rng(seed).standard_normal((D, D))
    return (T + T.T) / np.sqrt(2 * D) * 2


@functools.lru_cache(maxsize=None)
def b4_families():
    """ladder: x moves onto an eigenvalue of H at d = 2^-28 (kappa_2 ~ 10 ... 1e9), a contour point, and x = H_00 + 2^-30:
    a first pivot candidate of 4e-9 in a matrix of moderate kappa_2, which loses seven digits without a row exchange.
    bipartite: zero diagonal, even-odd hoppings only, so the first pivot candidates on the diagonal are x + i d,
    far below the hoppings, and rows must be exchanged; a 9x9 bipartite H has a zero eigenvalue, so x or d sets kappa_2.
    weak: the bipartite H times 2^-24 at x = 0, d = 1: a diagonal of i against real couplings of 1e-7, where a pivot
    key that looks at real parts only picks the couplings.
    graded: core levels 2^10 and 2^17 on two diagonal entries."""
    Hl = _dyadic(_sym(9101), 20)
    lam = np.linalg.eigvalsh(Hl)
    lam0 = float(lam[np.argmin(np.abs(lam - 0.1))])
    d = 2.0 ** -28
    ladder = B4Family("ladder", Hl, [(_dyadic(lam0 + s, 40), d) for s in (1.0, 1e-2, 1e-4, 1e-6, 0.0)] + [(0.25, 2.0)]
                      + [(Hl[0, 0] + 2.0 ** -30, d)])
    idx = np.arange(D)
    Hb = np.where((idx[:, None] + idx[None, :]) % 2 == 1, _dyadic(_sym(9102), 20), 0.0)
    bip = B4Family("bipartite", Hb, [(2.0 ** -4, 2.0 ** -30), (2.0 ** -10, 2.0 ** -30), (2.0 ** -20, 2.0 ** -30),
                                     (0.0, 2.0 ** -20), (0.0, 2.0 ** -28), (0.25, 2.0)])
    weak = B4Family("weak", Hb * 2.0 ** -24, [(0.0, 1.0), (0.0, 2.0 ** -4)])
    Hg = _dyadic(_sym(9103), 20)
    Hg[1, 1] += 2.0 ** 10
    Hg[5, 5] += 2.0 ** 17
    graded = B4Family("graded", Hg, [(0.25, 2.0 ** -10), (-0.75, 2.0 ** -20), (0.25, 2.0)])
    return [ladder, bip, weak, graded]


class B4Truth:
    """g = M^-1 (k < 6) and G2 = (M + i I + g)^-1 (k >= 6: A - Sigma_tot + sigma_{k-6} with Sigma_tot = -12 i I) of one
    point, clongdouble, with kappa_2 of both and the norms of the k >= 6 bar."""

    def __init__(self, fam, m):
        M = fam.matrix_ld(m)
        self.M64 = M.astype(np.complex128)
        rec = KappaInv()
        self.g = rec(M)
        self.M2 = M + LD(1j) * np.eye(D, dtype=LD) + self.g
        self.G2 = rec(self.M2)
        self.kappa1, self.kappa2 = rec.kappas
        self.first_order = _n2(self.G2) * (xprec.bar(D, self.kappa1) * _nf(self.g) + U * _nf(self.M2))

    @staticmethod
    def _col_err(got, true):
        Dm = np.asarray(got).astype(LD) - true
        return (np.linalg.norm(Dm.astype(np.complex128), axis=0) / np.linalg.norm(true.astype(np.complex128), axis=0))

    def ratio_first(self, got):
        """worst column error of a k < 6 block over xprec.bar(9, kappa_1)."""
        return float(np.max(self._col_err(got, self.g)) / xprec.bar(D, self.kappa1))

    def ratio_second(self, got):
        """worst column error of a k >= 6 block over bar(9, kappa_2(M2)) + the first-order term of the error in g."""
        return float(np.max(self._col_err(got, self.G2)) / (xprec.bar(D, self.kappa2) + self.first_order))


@functools.lru_cache(maxsize=None)
def b4_truth(f, m):
    return B4Truth(b4_families()[f], m)


def b4_reference(fam, m, inv):
    """The kernel's one sweep on a B4 point in complex128 with the inverse `inv`: (g, G2)."""
    M = fam.matrix_ld(m).astype(np.complex128)
    g = inv(M)
    return g, inv(M + 1j * np.eye(D) + g)


# --------------------------------------------------------------------------- #
# free running
# --------------------------------------------------------------------------- #
FREE_CONVS = (1e-5, 1e-8)
FREE_MIX = 0.5


def free_grid(conv):
    """The energies of the free-running tests on Au, eta = 1e-4: a real grid across the band and two contour points
    (fewer at 1e-8, where a point takes several hundred sweeps)."""
    real = np.linspace(-9.0, 5.0, 15 if conv >= 1e-6 else 8)
    return np.concatenate([real.astype(np.complex128), np.array(B1_CONTOUR)])


class FreeTruth:
    """Free-running bulk loop of one energy and, from the bulk iterate at any of its kept counts, the surface loop."""

    def __init__(self, lat, E, conv, mix=FREE_MIX):
        self.lat, self.E, self.conv, self.mix = lat, complex(E), conv, mix
        self.bulk = bulk(lat, E, mix, conv=conv)
        self._surf = {}

    def surf(self, bulk_count):
        if bulk_count not in self._surf:
            self._surf[bulk_count] = surface(self.lat, self.E, self.bulk.at[bulk_count], self.mix, conv=self.conv)
        return self._surf[bulk_count]

    def ambiguous(self):
        return self.bulk.ambiguous(self.conv) or self.surf(self.bulk.count).ambiguous(self.conv)


@functools.lru_cache(maxsize=None)
def free_truths(conv):
    lat = shipped("Au", 1e-4)
    return [FreeTruth(lat, E, conv) for E in free_grid(conv)]


def data_file(name):
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaunegf_amd", "data", name)
