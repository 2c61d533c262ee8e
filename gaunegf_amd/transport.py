"""
Transmission, DOS and current -- drop-in for gauNEGF/transport.py.

The reference walks the energy list in a Python loop, one jitted call and one
device->host sync per energy (transport.py:452-469, 567-591).  Here the host keeps
exactly the same bookkeeping (``-1`` sentinels, ``.npz`` checkpoint keys, resume
check, ``np.arange`` current grid, trapezoid rule, e/h and spin factors) and hands
every chunk of uncalculated energies to the GPU in one call: per energy one blocked
Gauss-Jordan inverse, two complex GEMMs on the FP64 matrix cores and a wavefront
trace reduction.
"""
import os

import numpy as np
from scipy.integrate import trapezoid

from . import distributed as _dist
from .config import ENERGY_STEP, N_KT, TEMPERATURE
from .engine import get_engine

# CONSTANTS (transport.py:33-37)
har_to_eV = 27.211386   # eV/Hartree
eoverh = 3.874e-5       # A/eV
kB = 8.617e-5           # eV/Kelvin
V_to_au = 0.03675       # Volts to Hartree/elementary Charge

GPU_CHUNK = 512         # energies per engine call when checkpointing is on


class SigmaCalculator:
    """Uniform access to static (sig1, sig2) arrays or an energy-dependent surfG-like
    object (transport.py:40-146): ``get_sigma_total / get_sigma / get_gamma`` with the
    reference's spin expansion (kron(I2, s) for 'u'/'ro', kron(s, I2) for 'g' when
    the Fock matrix is twice the size of sigma)."""

    def __init__(self, sig1, sig2=None, energy_dependent=None):
        self.sig1 = sig1
        self.sig2 = sig2
        if energy_dependent is None:
            self.energy_dependent = hasattr(sig1, 'sigma') and hasattr(sig1, 'sigmaTot')
        else:
            self.energy_dependent = energy_dependent
        if self.energy_dependent and sig2 is not None:
            raise ValueError("For energy-dependent calculations, provide only surfG object as sig1")
        if not self.energy_dependent and sig2 is None:
            raise ValueError("For energy-independent calculations, provide both sig1 and sig2")

    @staticmethod
    def _expand(sigma, spin, matrix_size):
        if spin in ['u', 'ro', 'g'] and matrix_size is not None and matrix_size == 2 * sigma.shape[0]:
            if spin in ['u', 'ro']:
                return np.kron(np.eye(2), sigma)
            return np.kron(sigma, np.eye(2))
        return sigma

    @staticmethod
    def _static(sig):
        a = np.asarray(sig)
        return np.diag(a) if a.ndim == 1 else a

    def get_sigma_total(self, E, spin=None, matrix_size=None):
        if self.energy_dependent:
            total = self.sig1.sigmaTot(E)
        else:
            a1, a2 = np.asarray(self.sig1), np.asarray(self.sig2)
            total = np.diag(a1 + a2) if a1.ndim == 1 else a1 + a2
        return self._expand(total, spin, matrix_size)

    def get_sigma(self, E, contact_index, spin=None, matrix_size=None):
        if self.energy_dependent:
            sigma = self.sig1.sigma(E, contact_index)
        else:
            if contact_index == 0:
                sigma = self._static(self.sig1)
            elif contact_index == -1 or contact_index == 1:
                sigma = self._static(self.sig2)
            else:
                raise ValueError(f"Invalid contact_index {contact_index}")
        return self._expand(sigma, spin, matrix_size)

    def get_gamma(self, E, contact_index, spin=None, matrix_size=None):
        sigma = self.get_sigma(E, contact_index, spin, matrix_size)
        return 1j * (sigma - np.conj(sigma).T)

    # ---- engine lowering ---------------------------------------------------
    def _const_handle(self, engine, what, spin, matrix_size):
        """Device-side CONST provider of the static self-energies, created once and kept with this object
        (creating and freeing it per call costs several device allocations and frees -- 20 ms on some hosts
        against 7 ms of kernels for 1000 energies at N = 200).  ``what``: "LR" = the two contacts, "tot" =
        their sum as a single contact (DOS).  The entry is keyed on the engine generation (a change of the
        matrix dimension drops every provider in the library) and on a checksum of the arrays, which the
        caller owns and may change between calls."""
        from .engine import fingerprint
        a1 = np.ascontiguousarray(self._static(self.sig1))
        a2 = np.ascontiguousarray(self._static(self.sig2))
        stamp = (a1.shape, a2.shape, fingerprint(a1), fingerprint(a2))
        cache = self.__dict__.setdefault("_lowered", {})
        key = (id(engine), getattr(engine, "generation", 0), what, spin if spin in ('u', 'ro', 'g') else 'r', matrix_size)
        hit = cache.get(key)
        if hit is not None and hit[2] == stamp:
            return hit[1]
        if hit is not None:
            hit[0].sigma_free(hit[1])
        for k in [k for k in cache if k[1] != key[1]]:          # older generations: handles already dropped by the library
            cache.pop(k)
        s1 = self._expand(a1, spin, matrix_size)
        s2 = self._expand(a2, spin, matrix_size)
        h = engine.sigma_const([s1, s2]) if what == "LR" else engine.sigma_const([np.asarray(s1) + np.asarray(s2)])
        cache[key] = (engine, h, stamp)
        return h

    def _release(self):
        for eng, h, _ in self.__dict__.get("_lowered", {}).values():
            eng.sigma_free(h)               # (a handle the library already dropped is a no-op there)
        self.__dict__.get("_lowered", {}).clear()

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _lower(self, engine, energies, spin, matrix_size):
        """Provider handle serving Sigma_tot, Sigma_L (contact 0) and Sigma_R (contact -1)
        for ``energies``.  Returns (handle, temporary)."""
        if not self.energy_dependent:
            return self._const_handle(engine, "LR", spin, matrix_size), False
        g = self.sig1
        native = hasattr(g, "_negf_lower")
        sig_size = getattr(g, "F", np.zeros((matrix_size, matrix_size))).shape[0] if native else None
        if native and sig_size == matrix_size and getattr(g, "num_contacts", 2) >= 1:
            return g._negf_lower(engine), False
        # spin-expanded or foreign provider: evaluate the three matrices per energy and
        # stage them (expansion is index bookkeeping; the Green's functions stay on the GPU)
        tot = np.stack([np.asarray(self.get_sigma_total(E, spin, matrix_size)) for E in energies])
        sL = np.stack([np.asarray(self.get_sigma(E, 0, spin, matrix_size)) for E in energies])
        sR = np.stack([np.asarray(self.get_sigma(E, -1, spin, matrix_size)) for E in energies])
        return engine.sigma_precomputed(tot, np.stack([sL, sR], axis=1)), True


# --------------------------------------------------------------------------- #
# per-energy kernels with explicit matrices (names imported by reference users,
# tests/jax_optimization_suite.py:36-37)
# --------------------------------------------------------------------------- #
def _explicit(E, F, S, sigma_total, gammas=None):
    eng = get_engine()
    eng.set_system(F, S)
    st = np.asarray(sigma_total)[None]
    gm = None if gammas is None else np.stack([np.asarray(x) for x in gammas])[None]
    return eng, eng.sigma_precomputed(st, gammas=gm)


def _transmission_kernel_restricted(E, F, S, sigma_total, gamma1, gamma2):
    """Re Tr[gamma1 G gamma2 G^H] (transport.py:150-157)."""
    eng, h = _explicit(E, F, S, sigma_total, (gamma1, gamma2))
    try:
        return float(eng.transmission(h, 0, 1, [E])[0])
    finally:
        eng.sigma_free(h)


def _transmission_kernel_spin_block(E, F, S, sigma_total, gamma1, gamma2):
    """(sum, [uu, ud, du, dd]) for 2N x 2N block-form matrices (transport.py:159-181)."""
    eng, h = _explicit(E, F, S, sigma_total, (gamma1, gamma2))
    try:
        T, Ts = eng.transmission(h, 0, 1, [E], spin_block=True)
        return float(T[0]), Ts[0]
    finally:
        eng.sigma_free(h)


def _dos_kernel(E, F, S, sigma_total):
    """(total, per-site) DOS = -Im diag(G)/pi (transport.py:183-190)."""
    eng, h = _explicit(E, F, S, sigma_total)
    try:
        tot, site = eng.dos(h, [E])
        return float(tot[0]), site[0]
    finally:
        eng.sigma_free(h)


# --------------------------------------------------------------------------- #
# batched evaluation used by the front-ends
# --------------------------------------------------------------------------- #
SPIN_BLOCK_SPLIT = True      # False: always invert the full 2N x 2N matrix, as the reference does
def _spinor_perm(N):
    # spinor [a0,b0,a1,b1,...] -> block [a0,a1,...,b0,b1,...] (transport.py:255)
    return np.concatenate([np.arange(0, 2 * N, 2), np.arange(1, 2 * N, 2)])


def _spin_diagonal_blocks(F, S):
    """(F_uu, S_uu, F_dd, S_dd) when the 2N x 2N block-form matrices are EXACTLY block diagonal (the layout
    scf.py:177-180 builds for 'u' / 'ro': blockdiag(alpha, beta)), else None.  The blocks come from the same cache as the
    integrals' (integrate._split_blocks: contiguous read-only copies, recognised by identity and checksum), so that
    GrLessInt and calculate_transmission on one system share them and their complex conversions."""
    n2 = F.shape[0]
    if n2 % 2:
        return None
    from .integrate import _split_blocks
    return _split_blocks(F, S, n2 // 2)


def _sigma_is_spin_expanded(sigma_calc, size):
    """True when get_sigma* expand an N x N self-energy with kron(I2, .) for a 2N x 2N system
    (transport.py:96-104): both spin blocks then see the same N x N self-energy."""
    if sigma_calc.energy_dependent:
        g = sigma_calc.sig1
        n_sig = getattr(g, "F", None)
        return n_sig is not None and 2 * np.asarray(n_sig).shape[0] == size
    return 2 * SigmaCalculator._static(sigma_calc.sig1).shape[0] == size


def _transmission_batch(F, S, sigma_calc, energies, spin):
    """T(E) for all ``energies`` on the GPU: array [m] ('r') or ([m], [m,4])."""
    if spin not in ('r', 'u', 'ro', 'g'):
        raise ValueError(f"Unknown spin configuration '{spin}'. Use 'r', 'u', 'ro', or 'g'")
    energies = np.asarray(energies)
    F = np.asarray(F)
    S = np.asarray(S)
    eng = get_engine()
    size = F.shape[0]
    if spin in ('u', 'ro') and SPIN_BLOCK_SPLIT and _sigma_is_spin_expanded(sigma_calc, size):
        blocks = _spin_diagonal_blocks(F, S)
        if blocks is not None:
            # Spin-polarised system without spin mixing: G = blockdiag(G_uu, G_dd), so the four block traces
            # of transport.py:166-177 are T_uu, 0, 0, T_dd with T_ss = Re Tr[G1 G_ss G2 G_ss^H] of the N x N
            # spin block -- two N-sized solves instead of one 2N-sized one (a quarter of the flops).  The sum
            # keeps the reference's order ((uu + ud) + du) + dd.
            Tuu = _transmission_batch(blocks[0], blocks[1], sigma_calc, energies, 'r')
            Tdd = _transmission_batch(blocks[2], blocks[3], sigma_calc, energies, 'r')
            Ts = np.stack([Tuu, np.zeros_like(Tuu), np.zeros_like(Tuu), Tdd], axis=1)
            return ((Ts[:, 0] + Ts[:, 1]) + Ts[:, 2]) + Ts[:, 3], Ts
    if spin == 'g':
        # shuffle everything to block form, as the reference does before its kernel
        perm = _spinor_perm(size // 2)
        ix = np.ix_(perm, perm)
        tot = np.stack([np.asarray(sigma_calc.get_sigma_total(E, spin, size))[ix] for E in energies])
        sL = np.stack([np.asarray(sigma_calc.get_sigma(E, 0, spin, size))[ix] for E in energies])
        sR = np.stack([np.asarray(sigma_calc.get_sigma(E, -1, spin, size))[ix] for E in energies])
        eng.set_system(F[ix], S[ix])
        h, temp = eng.sigma_precomputed(tot, np.stack([sL, sR], axis=1)), True
    else:
        eng.set_system(F, S)
        h, temp = sigma_calc._lower(eng, energies, spin, size)
    try:
        if spin == 'r':
            return eng.transmission(h, 0, -1, energies)
        return eng.transmission(h, 0, -1, energies, spin_block=True)
    finally:
        if temp:
            eng.sigma_free(h)


def _channels_batch(F, S, sigma_calc, energies, spin, nchan):
    """Transmission eigenchannels [m, nchan] ('r') or (up, down) for all ``energies`` on the GPU."""
    if spin not in ('r', 'u', 'ro', 'g'):
        raise ValueError(f"Unknown spin configuration '{spin}'. Use 'r', 'u', 'ro', or 'g'")
    energies = np.asarray(energies)
    F = np.asarray(F)
    S = np.asarray(S)
    size = F.shape[0]
    if spin == 'g':
        raise NotImplementedError("transmission eigenchannels: the spinor ('g') layout mixes spins inside each contact "
                                  "block; channels are served for 'r' and for spin-diagonal 'u' / 'ro' systems only")
    if spin in ('u', 'ro'):
        blocks = _spin_diagonal_blocks(F, S) if _sigma_is_spin_expanded(sigma_calc, size) else None
        if blocks is None:
            raise NotImplementedError("transmission eigenchannels with spin 'u' / 'ro' need an exactly block-diagonal "
                                      "(spin-diagonal) F, S and a spin-expanded N x N self-energy; spin mixing is not served")
        return (_channels_batch(blocks[0], blocks[1], sigma_calc, energies, 'r', nchan),
                _channels_batch(blocks[2], blocks[3], sigma_calc, energies, 'r', nchan))
    eng = get_engine()
    eng.set_system(F, S)
    if sigma_calc.energy_dependent and not hasattr(sigma_calc.sig1, "_negf_lower"):
        raise NotImplementedError("transmission eigenchannels need a provider the engine lowers itself (surfGTest, "
                                  "surfG, surfGB or static matrices); this self-energy object is evaluated on the host")
    h, temp = sigma_calc._lower(eng, energies, spin, size)
    try:
        if temp:
            raise NotImplementedError("transmission eigenchannels: this self-energy is staged per energy (no contact "
                                      "orbital lists); use static matrices or a native surfG / surfGB / surfGTest object")
        return eng.transmission_channels(h, 0, -1, energies, nchan)
    finally:
        if temp:
            eng.sigma_free(h)


def _channel_count(F, S, sigma_calc, spin):
    """Number of channels calculate_transmission_channels reports by default (min(K_L, K_R) of the lowered provider)."""
    F = np.asarray(F)
    S = np.asarray(S)
    if spin in ('u', 'ro'):
        blocks = _spin_diagonal_blocks(F, S) if _sigma_is_spin_expanded(sigma_calc, F.shape[0]) else None
        if blocks is None:
            raise NotImplementedError("transmission eigenchannels with spin 'u' / 'ro' need an exactly block-diagonal "
                                      "(spin-diagonal) F, S and a spin-expanded N x N self-energy; spin mixing is not served")
        F, S = blocks[0], blocks[1]
    elif spin == 'g':
        raise NotImplementedError("transmission eigenchannels: the spinor ('g') layout mixes spins inside each contact "
                                  "block; channels are served for 'r' and for spin-diagonal 'u' / 'ro' systems only")
    if sigma_calc.energy_dependent and not hasattr(sigma_calc.sig1, "_negf_lower"):
        raise NotImplementedError("transmission eigenchannels need a provider the engine lowers itself (surfGTest, "
                                  "surfG, surfGB or static matrices); this self-energy object is evaluated on the host")
    eng = get_engine()
    eng.set_system(F, S)
    h, temp = sigma_calc._lower(eng, np.zeros(0), 'r', F.shape[0])
    try:
        if temp:
            raise NotImplementedError("transmission eigenchannels: this self-energy is staged per energy (no contact "
                                      "orbital lists)")
        return eng.channel_count(h, 0, -1)
    finally:
        if temp:
            eng.sigma_free(h)


def _channel_states_run(F, S, sigma_calc, energies, spin, fn):
    """What _channels_batch and _channel_count do around their engine call, for the scattering states: the same spin
    and provider restrictions with the same messages; ``fn(engine, handle)`` on the lowered provider of an 'r' system,
    a pair of such results for a spin-diagonal 'u' / 'ro' one."""
    if spin not in ('r', 'u', 'ro', 'g'):
        raise ValueError(f"Unknown spin configuration '{spin}'. Use 'r', 'u', 'ro', or 'g'")
    F = np.asarray(F)
    S = np.asarray(S)
    size = F.shape[0]
    if spin == 'g':
        raise NotImplementedError("transmission eigenchannels: the spinor ('g') layout mixes spins inside each contact "
                                  "block; channels are served for 'r' and for spin-diagonal 'u' / 'ro' systems only")
    if spin in ('u', 'ro'):
        blocks = _spin_diagonal_blocks(F, S) if _sigma_is_spin_expanded(sigma_calc, size) else None
        if blocks is None:
            raise NotImplementedError("transmission eigenchannels with spin 'u' / 'ro' need an exactly block-diagonal "
                                      "(spin-diagonal) F, S and a spin-expanded N x N self-energy; spin mixing is not served")
        return (_channel_states_run(blocks[0], blocks[1], sigma_calc, energies, 'r', fn),
                _channel_states_run(blocks[2], blocks[3], sigma_calc, energies, 'r', fn))
    eng = get_engine()
    eng.set_system(F, S)
    if sigma_calc.energy_dependent and not hasattr(sigma_calc.sig1, "_negf_lower"):
        raise NotImplementedError("transmission eigenchannels need a provider the engine lowers itself (surfGTest, "
                                  "surfG, surfGB or static matrices); this self-energy object is evaluated on the host")
    h, temp = sigma_calc._lower(eng, energies, 'r', size)
    try:
        if temp:
            raise NotImplementedError("transmission eigenchannels: this self-energy is staged per energy (no contact "
                                      "orbital lists); use static matrices or a native surfG / surfGB / surfGTest object")
        return fn(eng, h)
    finally:
        if temp:
            eng.sigma_free(h)


def _channel_states_batch(F, S, sigma_calc, energies, spin, nchan, source):
    """(T [m, nchan], psi [m, nchan, N]) ('r') or ((T, psi) up, (T, psi) down) for all ``energies`` on the GPU."""
    energies = np.asarray(energies)
    dest = -1 if source == 0 else 0
    return _channel_states_run(F, S, sigma_calc, energies, spin,
                               lambda eng, h: eng.channel_states(h, source, dest, energies, nchan))


def _channel_states_count(F, S, sigma_calc, spin, source):
    """Number of states calculate_channel_states reports by default (K_s of the lowered provider's source contact)."""
    res = _channel_states_run(F, S, sigma_calc, np.zeros(0), spin, lambda eng, h: eng.channel_states_count(h, source))
    return res[0] if spin in ('u', 'ro') else res


def _bond_layout(F, S, sigma_calc, spin):
    """How the local transmission of (F, S, spin) is evaluated: [(F, S, perm)] -- one system for 'r' (perm None), the two
    N x N spin blocks for a spin-diagonal 'u' / 'ro' system with a spin-expanded self-energy, and otherwise the whole
    2N x 2N system: as it is for 'u' / 'ro' with spin mixing, shuffled to block form (perm) for 'g'."""
    if spin not in ('r', 'u', 'ro', 'g'):
        raise ValueError(f"Unknown spin configuration '{spin}'. Use 'r', 'u', 'ro', or 'g'")
    F = np.asarray(F)
    S = np.asarray(S)
    size = F.shape[0]
    if spin in ('u', 'ro') and SPIN_BLOCK_SPLIT and _sigma_is_spin_expanded(sigma_calc, size):
        blocks = _spin_diagonal_blocks(F, S)
        if blocks is not None:
            return [(blocks[0], blocks[1], None), (blocks[2], blocks[3], None)]
    if spin == 'g':
        return [(F, S, _spinor_perm(size // 2))]
    return [(F, S, None)]


def _bond_handle(eng, F, S, perm, sigma_calc, energies, spin):
    """Make (F, S) the resident system and lower the self-energy the way _transmission_batch does; (handle, temporary)."""
    size = F.shape[0]
    if perm is not None:
        ix = np.ix_(perm, perm)
        tot = np.stack([np.asarray(sigma_calc.get_sigma_total(E, spin, size))[ix] for E in energies])
        sL = np.stack([np.asarray(sigma_calc.get_sigma(E, 0, spin, size))[ix] for E in energies])
        sR = np.stack([np.asarray(sigma_calc.get_sigma(E, -1, spin, size))[ix] for E in energies])
        eng.set_system(F[ix], S[ix])
        return eng.sigma_precomputed(tot, np.stack([sL, sR], axis=1)), True
    eng.set_system(F, S)
    # (a spin block of a 'u' / 'ro' system sees the N x N self-energy: lowered as a restricted system)
    return sigma_calc._lower(eng, energies, spin if size != _sigma_size(sigma_calc) else 'r', size)


def _sigma_size(sigma_calc):
    if sigma_calc.energy_dependent:
        f = getattr(sigma_calc.sig1, "F", None)
        return None if f is None else np.asarray(f).shape[0]
    return SigmaCalculator._static(sigma_calc.sig1).shape[0]


def _check_contact(contact):
    if contact not in (0, 1, -1):
        raise ValueError(f"contact must be 0 (the first contact) or 1 / -1 (the second), got {contact!r}")
    return int(contact)


def _local_batch(layout, sigma_calc, energies, spin, groups, n_groups, contact):
    """Local transmission tables of all ``energies``: [len(layout), m, n_g, n_g]."""
    energies = np.asarray(energies)
    eng = get_engine()
    out = []
    for F, S, perm in layout:
        g = groups
        if perm is not None:                       # block form: position q holds the caller's orbital perm[q]
            g = (np.arange(F.shape[0]) if groups is None else np.asarray(groups))[perm]
        h, temp = _bond_handle(eng, F, S, perm, sigma_calc, energies, spin)
        try:
            out.append(eng.local_transmission(h, contact, energies, g, n_groups))
        finally:
            if temp:
                eng.sigma_free(h)
    return np.stack(out)


def _bond_int_batch(layout, sigma_calc, energies, weights, spin, contact):
    """sum_k w_k flow(E_k) per system of the layout, in the caller's orbital order: [len(layout), n, n]."""
    energies = np.asarray(energies)
    eng = get_engine()
    out = []
    for F, S, perm in layout:
        h, temp = _bond_handle(eng, F, S, perm, sigma_calc, energies, spin)
        try:
            flow = eng.bond_int(h, contact, energies, weights)
        finally:
            if temp:
                eng.sigma_free(h)
        if perm is not None:
            back = np.empty_like(flow)
            back[np.ix_(perm, perm)] = flow
            flow = back
        out.append(flow)
    return np.stack(out)


def _group_count(groups, n):
    if groups is None:
        return n
    g = np.asarray(groups).ravel()
    if g.size != n:
        raise ValueError(f"groups must map each of the {n} orbitals to a group, got {g.size} entries")
    if not np.issubdtype(g.dtype, np.integer) or g.min() < 0:
        raise ValueError("groups must be non-negative integers")
    return int(g.max()) + 1


def _pop_ind(contact):
    """contact=None: the retarded form; 0 / 1 / -1: that contact's share."""
    from .engine import Engine
    return Engine.RETARDED if contact is None else _check_contact(contact)


def _pop_batch(layout, sigma_calc, energies, spin, call):
    """call(engine, handle, pos, perm) -> [m, ...] for system ``pos`` of the layout, stacked: [len(layout), m, ...]."""
    energies = np.asarray(energies)
    eng = get_engine()
    out = []
    for pos, (F, S, perm) in enumerate(layout):
        h, temp = _bond_handle(eng, F, S, perm, sigma_calc, energies, spin)
        try:
            out.append(call(eng, h, pos, perm))
        finally:
            if temp:
                eng.sigma_free(h)
    return np.stack(out)


def _pop_population(eng, h, ind, energies, op, groups, n_g, perm, rows):
    """Engine.population for a system staged in block form (position q holds the caller's orbital perm[q]; perm None: as
    it is): a group map is handed over in the staged order; without one the per-orbital kernels run as they are and the
    result is put back into the caller's order here."""
    if perm is None:
        return eng.population(h, ind, energies, op, groups, n_g, rows=rows)
    if groups is not None:
        return eng.population(h, ind, energies, op, np.asarray(groups)[perm], n_g, rows=rows)
    out = eng.population(h, ind, energies, op, rows=rows)
    back = np.empty_like(out)
    if rows:
        back[:, perm] = out
    else:
        back[:, perm[:, None], perm[None, :]] = out
    return back


def _pop_sharded(layout, m, shape, run):
    """run(idx) -> [len(layout), len(idx), *shape], sharded over the energies; one array, or (up, down) for two systems."""
    k = len(layout)
    flat = int(np.prod(shape))
    res = _dist.sharded_map(lambda idx: np.moveaxis(run(idx), 0, 1).reshape(-1, k * flat), m, (k * flat,))
    res = np.asarray(res).reshape((m, k) + tuple(shape))
    return res[:, 0] if k == 1 else (res[:, 0], res[:, 1])


def fragment_orbitals(F, S, indices):
    """Molecular orbitals of the fragment ``indices``: the generalised eigenproblem F_ff c = e S_ff c of the fragment's
    blocks, solved on the host (Cholesky of S_ff, then a Hermitian eigenproblem).  Returns (energies [k] ascending,
    C [n, k]): the eigenvectors embedded in the full basis (zero outside the fragment) and S-normalised, C^H S C = 1."""
    F = np.asarray(F)
    S = np.asarray(S)
    idx = np.asarray(indices, dtype=int).ravel()
    if idx.size == 0 or np.unique(idx).size != idx.size or idx.min() < 0 or idx.max() >= F.shape[0]:
        raise ValueError("fragment must be a non-empty list of distinct orbital indices")
    Fff = F[np.ix_(idx, idx)].astype(complex)
    Sff = S[np.ix_(idx, idx)].astype(complex)
    Linv = np.linalg.inv(np.linalg.cholesky((Sff + Sff.conj().T) / 2))
    A = Linv @ ((Fff + Fff.conj().T) / 2) @ Linv.conj().T
    e, V = np.linalg.eigh((A + A.conj().T) / 2)
    C = np.zeros((F.shape[0], idx.size), dtype=complex)
    C[idx] = Linv.conj().T @ V
    return e, C


def _dos_batch(F, S, sigma_calc, energies, spin):
    F = np.asarray(F)
    S = np.asarray(S)
    eng = get_engine()
    eng.set_system(F, S)
    size = F.shape[0]
    if sigma_calc.energy_dependent and hasattr(sigma_calc.sig1, "_negf_lower") and \
            getattr(sigma_calc.sig1, "F", F).shape[0] == size:
        h, temp = sigma_calc.sig1._negf_lower(eng), False
    elif not sigma_calc.energy_dependent:
        h, temp = sigma_calc._const_handle(eng, "tot", spin, size), False
    else:
        tot = np.stack([np.asarray(sigma_calc.get_sigma_total(E, spin, size)) for E in energies])
        h, temp = eng.sigma_precomputed(tot), True
    try:
        return eng.dos(h, energies)
    finally:
        if temp:
            eng.sigma_free(h)


def transmission_single_energy(E, F_jax, S_jax, sigma_calc, spin=None):
    """transport.py:193-271: float for 'r', (total, [4]) otherwise."""
    if spin is None:
        spin = 'r'
    res = _transmission_batch(F_jax, S_jax, sigma_calc, np.array([E]), spin)
    if spin == 'r':
        return float(res[0])
    return float(res[0][0]), res[1][0].tolist()


def dos_single_energy(E, F_jax, S_jax, sigma_calc, spin=None):
    """transport.py:273-373."""
    if spin is None:
        spin = 'r'
    if spin not in ('r', 'u', 'ro', 'g'):
        raise ValueError(f"Unknown spin configuration '{spin}'. Use 'r', 'u', 'ro', or 'g'")
    tot, site = _dos_batch(F_jax, S_jax, sigma_calc, np.array([E]), spin)
    return _dos_result(float(tot[0]), site[0], spin)


def _dos_result(total, per_site, spin):
    if spin == 'r':
        return total, np.array(per_site)
    N = per_site.shape[0] // 2
    if spin in ('u', 'ro'):
        up, down = per_site[:N], per_site[N:]
        per = np.concatenate([up, down])
        return np.sum(up) + np.sum(down), per, up, down
    up, down = per_site[0::2], per_site[1::2]          # 'g': alpha / beta spinor components
    return np.sum(per_site), per_site, up, down


# --------------------------------------------------------------------------- #
# front-ends with the reference's checkpoint semantics
# --------------------------------------------------------------------------- #
def _write_checkpoint(path, **arrays):
    """One writer (rank 0 when the energy grid is sharded over ranks), through a temporary file and an
    atomic rename: a reader -- this run's resume, or another rank -- never sees a torn .npz."""
    if _dist.rank_world()[0] != 0:
        return
    target = path if path.endswith(".npz") else path + ".npz"       # np.savez appends the suffix
    tmp = target + ".tmp.npz"
    np.savez(tmp, **arrays)
    os.replace(tmp, target)


def _chunks(remaining, checkpoint_file, checkpoint_interval):
    if not checkpoint_file:
        return [remaining] if len(remaining) else []
    step = max(int(checkpoint_interval), 1)
    step = ((GPU_CHUNK + step - 1) // step) * step       # a multiple of the save interval
    return [remaining[a:a + step] for a in range(0, len(remaining), step)]


def calculate_transmission(F, S, sigma_calculator, energy_list, spin=None, checkpoint_file=None,
                           checkpoint_interval=10):
    """T(E) over ``energy_list`` with ``.npz`` checkpointing (transport.py:376-483):
    -1 marks uncalculated energies; an existing checkpoint whose energy list matches
    (rtol 1e-10) is resumed; keys ``transmission``, ``spin_transmission``, ``energy_list``."""
    energy_list = np.asarray(energy_list)
    n_energies = len(energy_list)
    if spin is None:
        spin = 'r'
    spin_open = spin in ['u', 'ro', 'g']

    transmission = -1 * np.ones(n_energies)
    spin_trans = -1 * np.ones((n_energies, 4)) if spin_open else None
    if checkpoint_file and os.path.exists(checkpoint_file):
        data = np.load(checkpoint_file, allow_pickle=True)
        if 'energy_list' in data:
            if not np.allclose(data['energy_list'], energy_list, rtol=1e-10):
                # (the reference leaves spin_transmission unallocated on this branch and then
                # fails at :459 for open-shell spins; a fresh start is what its message says)
                print("Warning: energy_list in checkpoint doesn't match. Starting fresh.")
            else:
                if 'transmission' in data:
                    transmission = data['transmission']
                if spin_open and 'spin_transmission' in data:
                    spin_trans = data['spin_transmission']

    def save():
        if spin_trans is not None:
            _write_checkpoint(checkpoint_file, transmission=transmission, spin_transmission=spin_trans,
                              energy_list=energy_list)
        else:
            _write_checkpoint(checkpoint_file, transmission=transmission, energy_list=energy_list)

    remaining = np.where(transmission == -1)[0]
    for chunk in _chunks(remaining, checkpoint_file, checkpoint_interval):
        E = energy_list[chunk]
        if spin == 'r':
            transmission[chunk] = _dist.sharded_map(
                lambda idx: _transmission_batch(F, S, sigma_calculator, E[idx], spin), len(chunk))
        else:
            def both(idx):
                T, Ts = _transmission_batch(F, S, sigma_calculator, E[idx], spin)
                return np.concatenate([T[:, None], Ts], axis=1)
            res = _dist.sharded_map(both, len(chunk), (5,))
            transmission[chunk] = res[:, 0]
            spin_trans[chunk] = res[:, 1:]
        if checkpoint_file:
            save()
    if checkpoint_file:
        save()
    if spin_trans is not None:
        return transmission, spin_trans
    return transmission


def calculate_transmission_channels(F, S, sigma_calculator, energy_list, spin=None, nchan=None):
    """Transmission eigenchannels: T(E) = sum_n T_n(E), T_n the eigenvalues of t^H t with t = Gamma_R^{1/2} G_RL
    Gamma_L^{1/2} -- how many channels conduct and how much each carries.  Returns [m, nchan] for spin 'r', and
    (up, down) for 'u' / 'ro' on a spin-diagonal system with a spin-expanded self-energy.  Each row is descending,
    exact zeros beyond the numerical rank of the smaller contact's coupling; sum_n T_n(E) equals
    calculate_transmission.  ``nchan`` defaults to min(K_L, K_R), the contacts' orbital counts (at most 96).
    Served for self-energies confined to contact orbital lists (static matrices, surfGTest, surfG, surfGB without
    the Xi Sigma Xi transform); others, 'g' and spin mixing raise NotImplementedError.  A contact's orbital list is the
    support of its Sigma: formSigma (and so surfGTest) adds -1e-9 i S on every orbital, which makes K_L = K_R = N --
    N channels, most of them the ~1e-9 background (it is above the 1e-14 relative rank cut), and NotImplementedError
    for N > 96.  Static matrices that vanish outside the contact orbitals give K_c = the contact's orbital count."""
    energy_list = np.asarray(energy_list)
    if spin is None:
        spin = 'r'
    if spin not in ('r', 'u', 'ro', 'g'):
        raise ValueError(f"Unknown spin configuration '{spin}'. Use 'r', 'u', 'ro', or 'g'")
    if nchan is None:
        nchan = _channel_count(F, S, sigma_calculator, spin)
    nchan = int(nchan)
    m = len(energy_list)
    if spin == 'r':
        return _dist.sharded_map(lambda idx: _channels_batch(F, S, sigma_calculator, energy_list[idx], spin, nchan),
                                 m, (nchan,))

    def both(idx):
        up, down = _channels_batch(F, S, sigma_calculator, energy_list[idx], spin, nchan)
        return np.concatenate([up, down], axis=1)
    res = _dist.sharded_map(both, m, (2 * nchan,))
    return res[:, :nchan], res[:, nchan:]


def calculate_channel_states(F, S, sigma_calculator, energy_list, source=0, spin=None, nchan=None):
    """Eigenchannel scattering states: WHICH orbitals carry channel n.  With Gamma_s = L L^H the coupling of the source
    contact (``source`` = 0 or -1; the destination d is the other end) on its orbitals I_s, T_n and u_n the eigenpairs of
    H = L^H G[I_d, I_s]^H Gamma_d G[I_d, I_s] L, and psi_n = G[:, I_s] L u_n: the state the retarded G injects from the
    source in channel n, normalised to unit incoming flux.  Returns (T [m, nchan], psi [m, nchan, N]) for spin 'r' and
    ((T_up, psi_up), (T_down, psi_down)) for 'u' / 'ro' on a spin-diagonal system with a spin-expanded self-energy.
    T is descending per energy and equals calculate_transmission_channels' nonzero values; psi_a^H Gamma_d psi_b =
    T_a delta_ab; with all channels sum_n psi_n psi_n^H = G Gamma_s G^H, the source's spectral function.  Closed
    channels have well-defined states (nothing is divided by sqrt(T_n)).  Each psi_n carries the phase that makes its
    component of largest modulus real and positive (lowest index on ties); the states of a degenerate cluster of T_n
    are an arbitrary orthogonal basis of that cluster.  Columns beyond the rank of Gamma_s are exact zeros, rows of
    singular energies NaN.  ``nchan`` defaults to K_s, the source contact's orbital count (at most 96; K_d is not
    limited).  Providers, 'g' and spin mixing as calculate_transmission_channels."""
    energy_list = np.asarray(energy_list)
    if spin is None:
        spin = 'r'
    if spin not in ('r', 'u', 'ro', 'g'):
        raise ValueError(f"Unknown spin configuration '{spin}'. Use 'r', 'u', 'ro', or 'g'")
    if source not in (0, -1):
        raise ValueError("source must be 0 (the first contact) or -1 (the last one)")
    if nchan is None:
        nchan = _channel_states_count(F, S, sigma_calculator, spin, source)
    nchan = int(nchan)
    m = len(energy_list)
    N = np.asarray(F).shape[0] // (2 if spin in ('u', 'ro') else 1)
    row = nchan * (1 + 2 * N)                                # T | Re, Im of psi: one row of doubles per energy

    def pack(T, psi):
        return np.concatenate([T, np.ascontiguousarray(psi).view(np.float64).reshape(len(T), -1)], axis=1)

    def unpack(rows):
        rows = np.ascontiguousarray(rows)
        return rows[:, :nchan].copy(), rows[:, nchan:].copy().view(np.complex128).reshape(len(rows), nchan, N)

    if spin == 'r':
        return unpack(_dist.sharded_map(
            lambda idx: pack(*_channel_states_batch(F, S, sigma_calculator, energy_list[idx], spin, nchan, source)), m, (row,)))

    def both(idx):
        up, down = _channel_states_batch(F, S, sigma_calculator, energy_list[idx], spin, nchan, source)
        return np.concatenate([pack(*up), pack(*down)], axis=1)
    res = _dist.sharded_map(both, m, (2 * row,))
    return unpack(res[:, :row]), unpack(res[:, row:])


def calculate_local_transmission(F, S, sigma_calculator, energy_list, groups=None, contact=0, spin=None):
    """Local (bond) transmission: WHERE the transmission injected by ``contact`` flows.  Per energy, with K = E S - F
    (no self-energies) and A = G Gamma_c G^H, flow[i, j] = 2 Im[K_ij A_ji] is the transmission flowing from orbital i to
    orbital j; with ``groups`` (orbital -> atom / fragment labels, one per orbital) the table is summed over the orbital
    pairs of each pair of groups.  Returns [m, n_g, n_g] (n_g = N without groups): real, antisymmetric, and for every split
    of the groups into a side holding the injecting contact and a side holding the other one the entries across the cut
    sum to calculate_transmission's T(E); rows of groups outside all contacts sum to zero.
    spin 'r': as is.  'u' / 'ro' on a spin-diagonal system with a spin-expanded N x N self-energy: (up, down), ``groups``
    of length N.  'g', and 'u' / 'ro' with spin mixing: the total over the 2N x 2N system, ``groups`` of length 2N in the
    caller's orbital order; its cuts sum to the full trace Tr[Gamma_L G Gamma_R G^H] of the 2N system, which the
    spin-block sum of calculate_transmission (the reference's pairing of G_ud with (G^H)_ud) equals only without spin
    mixing.  Explicit coupling matrices (non-Hermitian in general) are not served."""
    energy_list = np.asarray(energy_list)
    if spin is None:
        spin = 'r'
    contact = _check_contact(contact)
    layout = _bond_layout(F, S, sigma_calculator, spin)
    n_g = _group_count(groups, layout[0][0].shape[0])
    k = len(layout)
    res = _dist.sharded_map(
        lambda idx: np.moveaxis(_local_batch(layout, sigma_calculator, energy_list[idx], spin, groups, n_g, contact), 0, 1)
        .reshape(-1, k * n_g, n_g), len(energy_list), (k * n_g, n_g))
    res = np.asarray(res).reshape(len(energy_list), k, n_g, n_g)
    return res[:, 0] if k == 1 else (res[:, 0], res[:, 1])


def calculate_bond_currents(F, S, sigma_calculator, fermi, qV, T=TEMPERATURE, groups=None, spin=None, dE=ENERGY_STEP):
    """Bond currents in amperes [n_g, n_g]: the local transmission integrated over calculate_current's grid with its
    occupation factor, trapezoid weights (signed step for qV < 0), e/h and the factor 2 of spin 'r' -- in ONE pass over
    the grid (Engine.bond_int) --, so that every cut separating the first contact from the second sums to
    calculate_current of the same arguments, sign included.  ``groups`` and spin as calculate_local_transmission
    ((up, down) for a spin-diagonal 'u' / 'ro' system: the cuts equal the uu and dd entries of calculate_current's
    spin list).  qV ~ 0 returns zeros."""
    if fermi is None or qV is None:
        raise ValueError("fermi and qV must be provided for current calculations")
    if spin is None:
        spin = 'r'
    layout = _bond_layout(F, S, sigma_calculator, spin)
    n = layout[0][0].shape[0]
    n_g = _group_count(groups, n)
    k = len(layout)
    if np.allclose(0, qV):
        z = np.zeros((n_g, n_g))
        return z if k == 1 else (z, z.copy())
    energies, muL, muR = current_grid(fermi, qV, T, dE)
    if len(energies) == 0:
        raise ValueError("No energies in integration window. Check fermi, qV, and dE.")
    # trapezoid(y * occupation, energies) = sum_k w_k y_k
    w = np.zeros(len(energies))
    if len(energies) > 1:
        d = np.diff(energies)
        w[:-1] += d / 2
        w[1:] += d / 2
    if T != 0:
        w = w * np.abs(1 / (np.exp((energies - muR) / (kB * T)) + 1) - 1 / (np.exp((energies - muL) / (kB * T)) + 1))
    flow = _dist.sharded_sum(lambda idx: _bond_int_batch(layout, sigma_calculator, energies[idx], w[idx], spin, 0),
                             len(energies))
    flow = eoverh * np.asarray(flow)
    if spin == 'r':
        flow = flow * 2
    if groups is not None:
        onehot = np.zeros((n, n_g))
        onehot[np.arange(n), np.asarray(groups).ravel()] = 1.0
        flow = np.stack([onehot.T @ f @ onehot for f in flow])
    return flow[0] if k == 1 else (flow[0], flow[1])


def calculate_pdos(F, S, sigma_calculator, energy_list, groups=None, contact=None, spin=None):
    """Projected DOS in a non-orthogonal basis [m, n_g]: the Mulliken population per energy of every orbital
    (``groups=None``) or of every group of orbitals (atoms, fragments), row a = sum_{i in a} -Im (G S)_ii / pi; the rows
    of an energy sum to -Im Tr(G S) / pi.  ``contact=None``: the retarded form above; 0 or 1 / -1: the share injected by
    that contact, sum_{i in a} (G Gamma_c G^H S)_ii / 2pi -- for real energies the contacts' shares add up to the rows of the
    symmetrised table (pop + pop^T) / 2, and their grand total to the retarded form's, -Im Tr(G S) / pi.  One pass over G (or G Gamma_c G^H) per energy on the GPU; the [n_g, n_g] table is never formed.
    This -- not calculate_dos, which keeps the reference's -Im diag G / pi and ignores S -- is the DOS a user with a
    non-orthogonal (Gaussian) basis wants.  spin as calculate_local_transmission: (up, down) for a spin-diagonal
    'u' / 'ro' system with a spin-expanded self-energy, otherwise the 2N system with ``groups`` of length 2N."""
    energy_list = np.asarray(energy_list)
    if spin is None:
        spin = 'r'
    ind = _pop_ind(contact)
    layout = _bond_layout(F, S, sigma_calculator, spin)
    n_g = _group_count(groups, layout[0][0].shape[0])
    return _pop_sharded(layout, len(energy_list), (n_g,), lambda idx: _pop_batch(
        layout, sigma_calculator, energy_list[idx], spin,
        lambda eng, h, pos, perm: _pop_population(eng, h, ind, energy_list[idx], 'S', groups, n_g, perm, True)))


def calculate_overlap_population(F, S, sigma_calculator, energy_list, op='S', groups=None, contact=None, spin=None):
    """Energy-resolved overlap (``op='S'``, COOP) or Hamilton (``op='F'``, COHP) populations [m, n_g, n_g]:
    entry [k, a, b] = sum_{i in a, j in b} -(1/pi) Im[G_ij X_ji](E_k), X = S or F; with ``contact`` 0 or 1 / -1 that
    contact's share (1/2pi) Re[(G Gamma_c G^H)_ij X_ji].  The rows of the S table sum to calculate_pdos; for real energies
    the contacts' shares add up to the symmetrised retarded table.  ``groups``, spin as calculate_pdos."""
    energy_list = np.asarray(energy_list)
    if spin is None:
        spin = 'r'
    if op not in ('S', 'F'):
        raise ValueError(f"op must be 'S' or 'F', got {op!r}")
    ind = _pop_ind(contact)
    layout = _bond_layout(F, S, sigma_calculator, spin)
    n_g = _group_count(groups, layout[0][0].shape[0])
    return _pop_sharded(layout, len(energy_list), (n_g, n_g), lambda idx: _pop_batch(
        layout, sigma_calculator, energy_list[idx], spin,
        lambda eng, h, pos, perm: _pop_population(eng, h, ind, energy_list[idx], op, groups, n_g, perm, False)))


def calculate_projected_dos(F, S, sigma_calculator, energy_list, orbitals=None, fragment=None, contact=None, spin=None):
    """DOS projected on orbitals |phi_a> = sum_i c_ia |i> of the non-orthogonal basis [m, k]:
    p_a(E) = -(1/pi) Im <phi_a|G|phi_a> = -(1/pi) Im[c_a^H S G S c_a]; with ``contact`` 0 or 1 / -1 the share injected by
    that contact, (1/2pi) Re[c_a^H S G Gamma_c G^H S c_a].  Give either ``orbitals`` = C [n, k] (columns; S-normalise them
    for a DOS) or ``fragment`` = orbital indices: the fragment's molecular orbitals (fragment_orbitals) are projected on,
    and the result is (p [m, k], energies [k]).  A complete S-orthonormal set sums to calculate_pdos's total.
    spin as calculate_pdos: (up, down) -- and with ``fragment`` ((p_up, p_down), (e_up, e_down)) -- for a spin-diagonal
    'u' / 'ro' system (C has the N rows of a spin block there), otherwise C has the 2N rows of the whole system."""
    energy_list = np.asarray(energy_list)
    if spin is None:
        spin = 'r'
    if (orbitals is None) == (fragment is None):
        raise ValueError("give either orbitals=C [n, k] or fragment=indices")
    ind = _pop_ind(contact)
    layout = _bond_layout(F, S, sigma_calculator, spin)
    Ws, es = [], []
    for Fs, Ss, perm in layout:
        n = Fs.shape[0]
        if fragment is not None:
            e, Cmat = fragment_orbitals(Fs, Ss, fragment)
            es.append(e)
        else:
            Cmat = np.asarray(orbitals)
            if Cmat.ndim == 1:
                Cmat = Cmat[:, None]
            if Cmat.ndim != 2 or Cmat.shape[0] != n or not 1 <= Cmat.shape[1] <= n:
                raise ValueError(f"orbitals must be [n, k] with n = {n} rows and 1 <= k <= n, got {Cmat.shape}")
        W = (np.asarray(Ss) @ Cmat).T
        if perm is not None:                       # block form: position q holds the caller's orbital perm[q]
            W = W[:, perm]
        Ws.append(np.ascontiguousarray(W))
    k = Ws[0].shape[0]

    p = _pop_sharded(layout, len(energy_list), (k,), lambda idx: _pop_batch(
        layout, sigma_calculator, energy_list[idx], spin,
        lambda eng, h, pos, perm: eng.projected_dos(h, ind, energy_list[idx], Ws[pos])))
    if fragment is None:
        return p
    return p, (es[0] if len(es) == 1 else tuple(es))


def calculate_dos(F, S, sigma_calculator, energy_list, spin=None, checkpoint_file=None,
                  checkpoint_interval=10):
    """DOS over ``energy_list`` with checkpointing (transport.py:486-607): keys ``dos_total``,
    ``dos_per_site``, ``dos_spin``, ``energy_list``.  This is the reference's -Im diag G / pi, kept for parity: it ignores
    the overlap matrix.  In a non-orthogonal basis use calculate_pdos (populations, -Im (G S)_ii / pi)."""
    energy_list = np.asarray(energy_list)
    n_energies = len(energy_list)
    n_sites = F.shape[0]
    if spin is None:
        spin = 'r'
    if spin not in ('r', 'u', 'ro', 'g'):
        raise ValueError(f"Unknown spin configuration '{spin}'. Use 'r', 'u', 'ro', or 'g'")
    spin_open = spin in ['u', 'ro', 'g']

    dos_total = -1 * np.ones(n_energies)
    dos_per_site = -1 * np.ones((n_energies, n_sites))
    dos_spin = -1 * np.ones((n_energies, 2)) if spin_open else None
    if checkpoint_file and os.path.exists(checkpoint_file):
        data = np.load(checkpoint_file, allow_pickle=True)
        if 'energy_list' in data:
            if not np.allclose(data['energy_list'], energy_list, rtol=1e-10):
                print("Warning: energy_list in checkpoint doesn't match. Starting fresh.")
            else:
                if 'dos_total' in data:
                    dos_total = data['dos_total']
                if 'dos_per_site' in data:
                    dos_per_site = data['dos_per_site']
                if spin_open and 'dos_spin' in data:
                    dos_spin = data['dos_spin']

    def save():
        if dos_spin is not None:
            _write_checkpoint(checkpoint_file, dos_total=dos_total, dos_per_site=dos_per_site, dos_spin=dos_spin,
                              energy_list=energy_list)
        else:
            _write_checkpoint(checkpoint_file, dos_total=dos_total, dos_per_site=dos_per_site,
                              energy_list=energy_list)

    remaining = np.where(dos_total == -1)[0]
    for chunk in _chunks(remaining, checkpoint_file, checkpoint_interval):
        E = energy_list[chunk]

        def both(idx):
            tot, site = _dos_batch(F, S, sigma_calculator, E[idx], spin)
            return np.concatenate([tot[:, None], site], axis=1)
        res = _dist.sharded_map(both, len(chunk), (n_sites + 1,))
        for row, i in zip(res, chunk):
            out = _dos_result(row[0], row[1:], spin)
            dos_total[i] = out[0]
            dos_per_site[i] = np.asarray(out[1])
            if len(out) == 4:
                dos_spin[i, 0] = np.sum(out[2])
                dos_spin[i, 1] = np.sum(out[3])
        if checkpoint_file:
            save()
    if checkpoint_file:
        save()
    if dos_spin is not None:
        return dos_total, dos_per_site, dos_spin
    return dos_total, dos_per_site


def current_grid(fermi, qV, T=TEMPERATURE, dE=ENERGY_STEP):
    """Integration energies of calculate_current (transport.py:652-672): ``np.arange``
    (end-exclusive) from muL to muR, padded by 10 kT when T > 0; the step takes the
    sign of qV.  Returns (energies, muL, muR)."""
    dE = -1 * abs(dE) if qV < 0 else abs(dE)
    muL = fermi - qV / 2
    muR = fermi + qV / 2
    if T == 0:
        energies = np.arange(muL, muR, dE)
    else:
        spread = np.sign(dE) * N_KT * kB * T
        energies = np.arange(muL - spread, muR + spread, dE)
    return energies, muL, muR


def calculate_current(F, S, sigma_calculator, fermi, qV, T=TEMPERATURE, spin=None, dE=ENERGY_STEP,
                      **kwargs):
    """Landauer current at bias qV (transport.py:610-720)."""
    if fermi is None or qV is None:
        raise ValueError("fermi and qV must be provided for current calculations")
    if spin is None:
        spin = 'r'
    if np.allclose(0, qV):
        return 0.0 if spin == 'r' else [0.0, 0.0, 0.0, 0.0]
    integration_energies, muL, muR = current_grid(fermi, qV, T, dE)
    if len(integration_energies) == 0:
        raise ValueError("No energies in integration window. Check fermi, qV, and dE.")

    result = calculate_transmission(F, S, sigma_calculator, integration_energies, spin=spin, **kwargs)
    if isinstance(result, tuple):
        transmissions, spin_transmissions = np.asarray(result[0]), np.asarray(result[1])
    else:
        transmissions, spin_transmissions = np.asarray(result), None

    if T == 0:
        occupation = 1.0
    else:
        occupation = np.abs(1 / (np.exp((integration_energies - muR) / (kB * T)) + 1) -
                            1 / (np.exp((integration_energies - muL) / (kB * T)) + 1))
    if spin_transmissions is not None:
        if T == 0:
            current_spin = [eoverh * trapezoid(spin_transmissions[:, i], integration_energies)
                            for i in range(4)]
        else:
            current_spin = [eoverh * trapezoid(spin_transmissions[:, i] * occupation, integration_energies)
                            for i in range(4)]
        return sum(current_spin), current_spin
    if T == 0:
        current_total = eoverh * trapezoid(transmissions, integration_energies)
    else:
        current_total = eoverh * trapezoid(transmissions * occupation, integration_energies)
    if spin == 'r':
        current_total *= 2
    return current_total


# --------------------------------------------------------------------------- #
# multi-terminal transmission matrix and dephasing probes
# --------------------------------------------------------------------------- #
TMAT_CALL_DOUBLES = 1 << 27     # one engine call returns at most this many doubles (1 GiB)


def dephasing_probes(S, groups, gamma):
    """Buettiker / D'Amato-Pastawski dephasing probes for Engine.transmission_matrix and the front ends below: the list
    of (indices, block) with  Sigma_p = -(i gamma_p / 2) S[I_p, I_p],  hence Gamma_p = gamma_p S_pp -- positive definite
    in the non-orthogonal basis, and -i gamma / 2 for S = 1.  ``groups``: an orbital -> probe label map of length n
    (negative: no probe on that orbital; probe p takes the orbitals labelled p, in ascending order; labels without an
    orbital are skipped) or a list of index lists.  ``gamma``: a scalar or one value per probe."""
    S = np.asarray(S)
    n = S.shape[0]
    if len(groups) > 0 and np.ndim(groups[0]) > 0:
        lists = [np.asarray(g, dtype=int).ravel() for g in groups]
    else:
        g = np.asarray(groups).ravel()
        if g.size != n or not np.issubdtype(g.dtype, np.integer):
            raise ValueError(f"groups must be an integer label per orbital (length {n}) or a list of index lists")
        lists = [np.nonzero(g == lab)[0] for lab in range(int(g.max()) + 1 if g.size else 0)]
        lists = [ix for ix in lists if ix.size]
    gam = np.broadcast_to(np.asarray(gamma, dtype=float), (len(lists),)) if np.ndim(gamma) == 0 else np.asarray(gamma, dtype=float).ravel()
    if gam.size != len(lists):
        raise ValueError(f"gamma must be a scalar or one value per probe ({len(lists)}), got {gam.size}")
    out = []
    for ix, gp in zip(lists, gam):
        if ix.size == 0 or ix.min() < 0 or ix.max() >= n or np.unique(ix).size != ix.size:
            raise ValueError(f"a probe must be a non-empty list of distinct orbital indices in [0, {n})")
        out.append((ix, -0.5j * gp * S[np.ix_(ix, ix)].astype(complex)))
    return out


def effective_transmission(T, n_real, source=0, drain=-1):
    """T_eff [m] between the real terminals ``drain`` and ``source`` of transmission matrices T [m, C, C] whose
    terminals n_real .. C - 1 are probes that float at every energy (no net current):
        To = T with zero diagonal,  W_pp = sum_{c != p} To[p][c] (c over ALL terminals),  W_pq = -To[p][q],
        P' = probes with W_pp > 0 (decoupled probes drop out),
        T_eff[d][s] = To[d][s] + To[d][P'] W^-1 To[P'][s].
    One numpy.linalg.solve batched over the energies; NaN matrices (singular energies) give NaN."""
    T = np.asarray(T, dtype=float)
    m, C = T.shape[0], T.shape[1]
    d = drain + n_real if drain < 0 else drain
    s_ = source + n_real if source < 0 else source
    if not (0 <= d < n_real and 0 <= s_ < n_real) or d == s_:
        raise ValueError(f"source and drain must be two different real terminals (0 .. {n_real - 1})")
    To = T.copy()
    To[:, np.arange(C), np.arange(C)] = 0.0
    coh = To[:, d, s_].copy()
    npr = C - n_real
    if npr == 0 or m == 0:
        return coh
    bad = ~np.isfinite(To).all(axis=(1, 2))
    To[bad] = 0.0
    Wd = To[:, n_real:, :].sum(axis=2)                       # [m, npr]
    on = Wd > 0
    W = -To[:, n_real:, n_real:]
    W = W * (on[:, :, None] & on[:, None, :])
    ar = np.arange(npr)
    W[:, ar, ar] = np.where(on, Wd, 1.0)
    rhs = np.where(on, To[:, n_real:, s_], 0.0)
    row = np.where(on, To[:, d, n_real:], 0.0)
    x = np.linalg.solve(W, rhs[:, :, None])[:, :, 0]
    out = coh + np.einsum("mp,mp->m", row, x)
    out[bad] = np.nan
    return out


def probe_response(T, n_real):
    """R [m, P, n_real]: the response of the floating probes (terminals n_real .. C - 1) to the real terminals, from
    transmission matrices T [m, C, C] -- the host form of Engine.probe_response, next to effective_transmission and with
    its masking:
        To = T with zero diagonal,  W_pp = sum_{c != p} To[p][c] (c over ALL terminals),  W_pq = -To[p][q],
        P' = probes with W_pp > 0,  R[P', :] = W^-1 To[P', 0:n_real];  rows of decoupled probes are exact zeros.
    Probe p's occupation is f_p = sum_c R[p][c] f_c; for real energies every row over P' sums to 1 and 0 <= R <= 1 to
    rounding.  One numpy.linalg.solve batched over the energies; NaN matrices (singular energies) give NaN, and so does
    an energy whose W is singular (probes without a path to any contact)."""
    T = np.asarray(T, dtype=float)
    m, C = T.shape[0], T.shape[1]
    npr = C - n_real
    if not 0 < n_real <= C:
        raise ValueError(f"n_real must lie in 1 .. {C}")
    if npr == 0 or m == 0:
        return np.zeros((m, npr, n_real))
    To = T.copy()
    To[:, np.arange(C), np.arange(C)] = 0.0
    bad = ~np.isfinite(To).all(axis=(1, 2))
    To[bad] = 0.0
    Wd = To[:, n_real:, :].sum(axis=2)                       # [m, npr]
    on = Wd > 0
    W = -To[:, n_real:, n_real:]
    W = W * (on[:, :, None] & on[:, None, :])
    ar = np.arange(npr)
    W[:, ar, ar] = np.where(on, Wd, 1.0)
    rhs = np.where(on[:, :, None], To[:, n_real:, :n_real], 0.0)
    try:
        R = np.linalg.solve(W, rhs)
    except np.linalg.LinAlgError:
        # probes without a path to any contact (a cluster that sees only itself) make W singular at that energy: NaN
        # for it, as the device form gives, and the other energies one by one
        R = np.full(rhs.shape, np.nan)
        for k in range(m):
            try:
                R[k] = np.linalg.solve(W[k], rhs[k])
            except np.linalg.LinAlgError:
                on[k] = True
    R[~on] = 0.0
    R[bad] = np.nan
    return R


def _tmat_contacts(sigma_calc):
    if not sigma_calc.energy_dependent:
        return 2
    nc = getattr(sigma_calc.sig1, "num_contacts", 2)
    return int(nc() if callable(nc) else nc)


def _tmat_layout(F, S, sigma_calc, spin):
    """[(F, S, perm, static)] as _bond_layout; static: the system is 2N-sized with spin mixing or in the spinor layout
    and is served for static (sig1, sig2) only, lowered as a CONST provider."""
    layout = _bond_layout(F, S, sigma_calc, spin)
    size = np.asarray(F).shape[0]
    big = spin in ('u', 'ro', 'g') and len(layout) == 1 and size != _sigma_size(sigma_calc)
    if (spin == 'g' or big) and sigma_calc.energy_dependent:
        raise NotImplementedError("transmission matrix: the spinor ('g') layout and 'u' / 'ro' systems with spin mixing are "
                                  "served for static (sig1, sig2) only; energy-dependent providers need 'r' or a "
                                  "spin-diagonal 'u' / 'ro' system with a spin-expanded N x N self-energy")
    return [(f, s_, perm, spin == 'g' or big) for f, s_, perm in layout]


def _tmat_batch(layout, sigma_calc, energies, spin, probes, run=None):
    """Transmission matrices of all ``energies``: [len(layout), m, C, C]; or, per system, what
    ``run(engine, handle, probes, energies)`` returns (the floating-probe front ends)."""
    energies = np.asarray(energies)
    eng = get_engine()
    out = []
    for F, S, perm, static in layout:
        size = F.shape[0]
        pr = probes
        if sigma_calc.energy_dependent and not hasattr(sigma_calc.sig1, "_negf_lower"):
            raise NotImplementedError("transmission matrix needs a provider the engine lowers itself (surfGTest, surfG, "
                                      "surfGB or static matrices); this self-energy object is evaluated on the host")
        if perm is not None:
            # block form: position q holds the caller's orbital perm[q]; the probes' indices follow
            ix = np.ix_(perm, perm)
            inv = np.empty(size, dtype=int); inv[perm] = np.arange(size)
            eng.set_system(F[ix], S[ix])
            sig = [np.asarray(sigma_calc.get_sigma(None, k, spin, size))[ix] for k in (0, -1)]
            h, temp = eng.sigma_const(sig), True
            pr = None if not probes else [(inv[np.asarray(i, dtype=int).ravel()], b) for i, b in probes]
        else:
            h, temp = _bond_handle(eng, F, S, None, sigma_calc, energies, spin)
        try:
            if temp and perm is None:
                raise NotImplementedError("transmission matrix: this self-energy is staged per energy (no contact orbital "
                                          "lists); use static matrices or a native surfG / surfGB / surfGTest object")
            if run is not None:
                out.append(run(eng, h, pr, energies))
                continue
            Cn = eng.terminal_count(h, pr)
            step = max(1, TMAT_CALL_DOUBLES // (Cn * Cn))
            parts = [eng.transmission_matrix(h, energies[k:k + step], pr) for k in range(0, len(energies), step)]
            out.append(np.concatenate(parts) if parts else np.zeros((0, Cn, Cn)))
        finally:
            if temp:
                eng.sigma_free(h)
    return np.stack(out)


def calculate_transmission_matrix(F, S, sigma_calculator, energy_list, probes=None, spin=None):
    """Transmission matrix [m, C, C] between all terminals of the junction, one inverse per energy on the GPU
    (Engine.transmission_matrix): T[k, a, b] = Re Tr[Gamma_a G Gamma_b G^H](E_k), the transmission from b into a.  The
    terminals are the contacts of ``sigma_calculator`` followed by ``probes``, a list of (indices, block) -- see
    dephasing_probes.  T[k, 0, -1] without probes is calculate_transmission's T(E_k).
    spin: 'r' as is; 'u' / 'ro' on a spin-diagonal system with a spin-expanded N x N self-energy: (up, down), with the
    probes given on the N orbitals; 'g', and 'u' / 'ro' with spin mixing: static (sig1, sig2) only, on the 2N system
    with the probes' indices in the caller's orbital order.  Energies are sharded over the ranks."""
    energy_list = np.asarray(energy_list)
    if spin is None:
        spin = 'r'
    layout = _tmat_layout(F, S, sigma_calculator, spin)
    Cn = _tmat_contacts(sigma_calculator) + (len(probes) if probes else 0)
    return _pop_sharded(layout, len(energy_list), (Cn, Cn),
                        lambda idx: _tmat_batch(layout, sigma_calculator, energy_list[idx], spin, probes))


def calculate_effective_transmission(F, S, sigma_calculator, energy_list, probes, source=0, drain=-1, spin=None):
    """(T_eff [m], T_coherent [m]) between the contacts ``source`` and ``drain`` with the ``probes`` floating at every
    energy (effective_transmission on calculate_transmission_matrix's result; the solve runs on the host).  T_coherent
    is the direct term T[drain][source] in the presence of the probes; T_eff = T_coherent for probes of zero strength.
    A spin-diagonal 'u' / 'ro' system gives the sums over the two spin blocks."""
    T = calculate_transmission_matrix(F, S, sigma_calculator, energy_list, probes=probes, spin=spin)
    n_real = _tmat_contacts(sigma_calculator)
    parts = T if isinstance(T, tuple) else (T,)
    eff = sum(effective_transmission(t, n_real, source, drain) for t in parts)
    d = drain + n_real if drain < 0 else drain
    s_ = source + n_real if source < 0 else source
    coh = sum(t[:, d, s_] for t in parts)
    return eff, coh


def calculate_effective_current(F, S, sigma_calculator, fermi, qV, probes, T=TEMPERATURE, spin=None, dE=ENERGY_STEP):
    """Current at bias qV with dephasing probes: calculate_current's grid, occupation factor, trapezoid rule, e/h and
    spin factor, applied to calculate_effective_transmission's T_eff."""
    if fermi is None or qV is None:
        raise ValueError("fermi and qV must be provided for current calculations")
    if spin is None:
        spin = 'r'
    if np.allclose(0, qV):
        return 0.0
    energies, muL, muR = current_grid(fermi, qV, T, dE)
    if len(energies) == 0:
        raise ValueError("No energies in integration window. Check fermi, qV, and dE.")
    t_eff, _ = calculate_effective_transmission(F, S, sigma_calculator, energies, probes, spin=spin)
    if T == 0:
        total = eoverh * trapezoid(t_eff, energies)
    else:
        occupation = np.abs(1 / (np.exp((energies - muR) / (kB * T)) + 1) - 1 / (np.exp((energies - muL) / (kB * T)) + 1))
        total = eoverh * trapezoid(t_eff * occupation, energies)
    if spin == 'r':
        total *= 2
    return total


def _deph_layout(F, S, sigma_calc, spin):
    layout = _tmat_layout(F, S, sigma_calc, spin)
    if any(static for *_, static in layout):
        raise NotImplementedError("floating probes: the spinor ('g') layout and 'u' / 'ro' systems with spin mixing are not "
                                  "served; use 'r' or a spin-diagonal 'u' / 'ro' system with a spin-expanded N x N self-energy")
    return layout


def calculate_probe_response(F, S, sigma_calculator, energy_list, probes, spin=None):
    """R [m, P, n_c]: the response of the floating ``probes`` to the contacts at every energy, solved on the GPU behind
    the transmission matrices (Engine.probe_response; the host form is probe_response on
    calculate_transmission_matrix's result).  Probe p's occupation is sum_c R[k, p, c] f_c(E_k).
    spin: 'r' as is; 'u' / 'ro' on a spin-diagonal system with a spin-expanded N x N self-energy: (up, down), with the
    probes given on the N orbitals.  'g' and spin mixing raise NotImplementedError.  Energies are sharded over the ranks."""
    energy_list = np.asarray(energy_list)
    if spin is None:
        spin = 'r'
    layout = _deph_layout(F, S, sigma_calculator, spin)
    nc = _tmat_contacts(sigma_calculator)
    P = len(probes) if probes else 0
    return _pop_sharded(layout, len(energy_list), (P, nc),
                        lambda idx: _tmat_batch(layout, sigma_calculator, energy_list[idx], spin, probes,
                                                run=lambda eng, h, pr, E: eng.probe_response(h, E, pr)))


def calculate_probe_occupations(F, S, sigma_calculator, energy_list, probes, fermi, qV, T=TEMPERATURE, spin=None):
    """f_p(E) [m, P]: the occupations the floating ``probes`` take at bias qV -- the local chemical-potential profile of a
    dephased junction -- f_p = R[p][0] f_L + R[p][-1] f_R with calculate_current's muL = fermi + qV / 2,
    muR = fermi - qV / 2 and Fermi functions (step functions at T = 0).  A probe that is the only path between two parts
    of a device takes the occupation of the side that feeds it.  (up, down) for a spin-diagonal 'u' / 'ro' system."""
    if fermi is None or qV is None:
        raise ValueError("fermi and qV must be provided for probe occupations")
    energy_list = np.asarray(energy_list)
    if _tmat_contacts(sigma_calculator) != 2:
        raise NotImplementedError("probe occupations at a bias are defined for two contacts; use calculate_probe_response "
                                  "with your own occupations for more")
    R = calculate_probe_response(F, S, sigma_calculator, energy_list, probes, spin=spin)
    muL, muR = fermi + qV / 2, fermi - qV / 2
    E = np.real(energy_list).astype(float)

    def occ(mu):
        if T == 0:
            return (E < mu).astype(float) + 0.5 * (E == mu)
        return 1 / (np.exp((E - mu) / (kB * T)) + 1)
    f = np.stack([occ(muL), occ(muR)], axis=1)                # [m, 2]
    one = lambda r: np.einsum("mpc,mc->mp", r, f)
    return tuple(one(r) for r in R) if isinstance(R, tuple) else one(R)


# --------------------------------------------------------------------------- #
# Legacy wrappers (gauNEGF/transport.py:724-1107): thin adapters kept so that existing
# user scripts run unchanged; each one builds a SigmaCalculator and forwards to the
# batch front-ends above (i.e. to the GPU engine).
# --------------------------------------------------------------------------- #
def _static_calc(sig1, sig2):
    return SigmaCalculator(sig1, sig2, energy_dependent=False)


def _dynamic_calc(g):
    return SigmaCalculator(g, energy_dependent=True)


def current(F, S, sig1, sig2, fermi, qV, T=TEMPERATURE, spin="r", dE=ENERGY_STEP):
    """Coherent current, energy-independent self-energies (transport.py:724-770)."""
    return calculate_current(F, S, _static_calc(sig1, sig2), fermi=fermi, qV=qV, T=T, spin=spin, dE=dE)


def currentSpin(F, S, sig1, sig2, fermi, qV, T=TEMPERATURE, spin="r", dE=ENERGY_STEP):
    """Spin currents [uu, ud, du, dd]; zeros for a restricted calculation (transport.py:772-812)."""
    result = calculate_current(F, S, _static_calc(sig1, sig2), fermi=fermi, qV=qV, T=T, spin=spin, dE=dE)
    return result[1] if isinstance(result, tuple) else [0, 0, 0, 0]


def currentE(F, S, g, fermi, qV, T=TEMPERATURE, spin="r", dE=ENERGY_STEP):
    """Coherent current with an energy-dependent provider ``g`` (transport.py:815-845)."""
    return calculate_current(F, S, _dynamic_calc(g), fermi=fermi, qV=qV, T=T, spin=spin, dE=dE)


def currentF(fn, dE=ENERGY_STEP, T=TEMPERATURE):
    """Current from a saved SCF ``.mat`` file with keys F, S, sig1, sig2, fermi, qV, spin
    (transport.py:847-875)."""
    import scipy.io as io
    m = io.loadmat(fn)
    return current(m["F"], m["S"], m["sig1"], m["sig2"], m["fermi"][0, 0], m["qV"][0, 0], T, m["spin"][0], dE=dE)


def _report(Elist, values, label, extra=None):
    for i, E in enumerate(Elist):
        if extra is None:
            print("Energy:", E, f"eV, {label}=", values[i])
        else:
            print("Energy:", E, f"eV, {label}=", values[i], ", Tspin=", extra[i])


def cohTrans(Elist, F, S, sig1, sig2):
    """T(E) list, energy-independent self-energies (transport.py:878-912)."""
    T_ = calculate_transmission(F, S, _static_calc(sig1, sig2), Elist, spin='r')
    _report(Elist, T_, "Transmission")
    return T_.tolist()


def cohTransChannels(Elist, F, S, sig1, sig2, nchan=None):
    """Transmission eigenchannels [M, nchan] with energy-independent self-energies (next to cohTrans); each row sums
    to cohTrans's T(E)."""
    return calculate_transmission_channels(F, S, _static_calc(sig1, sig2), Elist, spin='r', nchan=nchan)


def cohTransChannelsE(Elist, F, S, g, nchan=None):
    """Transmission eigenchannels [M, nchan] with an energy-dependent provider ``g`` (next to cohTransE)."""
    return calculate_transmission_channels(F, S, _dynamic_calc(g), Elist, spin='r', nchan=nchan)


def cohTransChannelStates(Elist, F, S, sig1, sig2, nchan=None, source=0):
    """(T [M, nchan], psi [M, nchan, N]): eigenchannels and their scattering states with energy-independent
    self-energies (next to cohTransChannels); ``source`` = 0 injects from sig1's contact, -1 from sig2's."""
    return calculate_channel_states(F, S, _static_calc(sig1, sig2), Elist, source=source, spin='r', nchan=nchan)


def cohTransChannelStatesE(Elist, F, S, g, nchan=None, source=0):
    """(T, psi) with an energy-dependent provider ``g`` (next to cohTransChannelsE)."""
    return calculate_channel_states(F, S, _dynamic_calc(g), Elist, source=source, spin='r', nchan=nchan)


def cohTransMatrix(Elist, F, S, sig1, sig2, probes=None):
    """Transmission matrix [M, C, C] with energy-independent self-energies (next to cohTrans): the two contacts followed
    by ``probes``."""
    return calculate_transmission_matrix(F, S, _static_calc(sig1, sig2), Elist, probes=probes, spin='r')


def cohTransMatrixE(Elist, F, S, g, probes=None):
    """Transmission matrix [M, C, C] with an energy-dependent provider ``g`` (next to cohTransE)."""
    return calculate_transmission_matrix(F, S, _dynamic_calc(g), Elist, probes=probes, spin='r')


def cohTransDephased(Elist, F, S, sig1, sig2, probes):
    """Effective T(E) list with floating dephasing probes, energy-independent self-energies (next to cohTrans)."""
    T_, _ = calculate_effective_transmission(F, S, _static_calc(sig1, sig2), Elist, probes, spin='r')
    _report(Elist, T_, "Effective transmission")
    return T_.tolist()


def cohTransDephasedE(Elist, F, S, g, probes):
    """Effective T(E) list with floating dephasing probes and an energy-dependent provider ``g`` (next to cohTransE)."""
    T_, _ = calculate_effective_transmission(F, S, _dynamic_calc(g), Elist, probes, spin='r')
    _report(Elist, T_, "Effective transmission")
    return T_.tolist()


def probeOccupations(Elist, F, S, sig1, sig2, probes, fermi, qV, T=TEMPERATURE):
    """Occupations f_p(E) [M, P] of floating dephasing probes, energy-independent self-energies (next to cohTransDephased)."""
    return calculate_probe_occupations(F, S, _static_calc(sig1, sig2), Elist, probes, fermi, qV, T=T, spin='r')


def probeOccupationsE(Elist, F, S, g, probes, fermi, qV, T=TEMPERATURE):
    """Occupations f_p(E) [M, P] of floating dephasing probes with an energy-dependent provider ``g``."""
    return calculate_probe_occupations(F, S, _dynamic_calc(g), Elist, probes, fermi, qV, T=T, spin='r')


def localTrans(Elist, F, S, sig1, sig2, groups=None):
    """Local (bond) transmission tables [M, n_g, n_g] with energy-independent self-energies (next to cohTrans); every cut
    between the contacts sums to cohTrans's T(E)."""
    return calculate_local_transmission(F, S, _static_calc(sig1, sig2), Elist, groups=groups, spin='r')


def localTransE(Elist, F, S, g, groups=None):
    """Local (bond) transmission tables [M, n_g, n_g] with an energy-dependent provider ``g`` (next to cohTransE)."""
    return calculate_local_transmission(F, S, _dynamic_calc(g), Elist, groups=groups, spin='r')


def _spin_trans(Elist, F, S, calc, spin):
    result = calculate_transmission(F, S, calc, Elist, spin=spin)
    if isinstance(result, tuple):
        T_, Ts = result
        _report(Elist, T_, "Transmission", Ts)
        return (T_.tolist(), Ts)
    _report(Elist, result, "Transmission")
    return (result.tolist(), np.zeros((len(Elist), 4)))


def cohTransSpin(Elist, F, S, sig1, sig2, spin='u'):
    """(T list, [M,4] spin-resolved T) (transport.py:914-966)."""
    return _spin_trans(Elist, F, S, _static_calc(sig1, sig2), spin)


def DOS(Elist, F, S, sig1, sig2):
    """(DOS list, per-site DOS [M,N]) (transport.py:969-997)."""
    tot, site = calculate_dos(F, S, _static_calc(sig1, sig2), Elist, spin='r')
    return tot.tolist(), site


def PDOS(Elist, F, S, sig1, sig2, groups=None):
    """(total list, projected DOS [M, n_g]) in a non-orthogonal basis with energy-independent self-energies (next to DOS,
    which ignores S): calculate_pdos and its sum over the groups, -Im Tr(G S) / pi."""
    pd = calculate_pdos(F, S, _static_calc(sig1, sig2), Elist, groups=groups, spin='r')
    return pd.sum(axis=1).tolist(), pd


def cohTransE(Elist, F, S, g):
    """T(E) list with an energy-dependent provider (transport.py:1001-1034)."""
    T_ = calculate_transmission(F, S, _dynamic_calc(g), Elist, spin='r')
    _report(Elist, T_, "Transmission")
    return T_.tolist()


def cohTransSpinE(Elist, F, S, g, spin='u'):
    """Spin-resolved T(E) with an energy-dependent provider (transport.py:1036-1075)."""
    return _spin_trans(Elist, F, S, _dynamic_calc(g), spin)


def DOSE(Elist, F, S, g):
    """DOS with an energy-dependent provider (transport.py:1077-1107)."""
    tot, site = calculate_dos(F, S, _dynamic_calc(g), Elist, spin='r')
    _report(Elist, tot, "DOS")
    return tot.tolist(), site


def PDOSE(Elist, F, S, g, groups=None):
    """(total list, projected DOS [M, n_g]) with an energy-dependent provider ``g`` (next to DOSE)."""
    pd = calculate_pdos(F, S, _dynamic_calc(g), Elist, groups=groups, spin='r')
    tot = pd.sum(axis=1)
    _report(Elist, tot, "PDOS")
    return tot.tolist(), pd
