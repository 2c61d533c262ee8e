"""
Layered (block-tridiagonal) devices on the recursive Green's function path of the engine.

A long wire, an oligomer between two chain leads or a molecule with several principal layers of electrode attached
couples only neighbouring layers; only the two end layers carry a self-energy.  ``LayeredSystem`` holds the blocks,
``partition`` finds a layering of a dense (F, S), ``Lead`` describes a terminal, and the front ends follow their dense
namesakes in transport.py / integrate.py:

    calculate_transmission_layered(system, leads, energy_list)      -> T [m]
    calculate_dos_layered(system, leads, energy_list)               -> (dos_total [m], dos_per_site [m, N])
    calculate_pdos_layered(system, leads, energy_list, groups=None) -> [m, n_g]      (Mulliken, -Im (G S)_ii / pi)
    GrIntLayered(system, leads, Elist, weights)                     -> (diag, up, low) block lists of sum_m w_m G(E_m)
    GrLessIntLayered(system, leads, Elist, weights, ind=None)       -> the same lists of sum_m w_m G Gamma G^H (E_m)
    calculate_contact_pdos_layered(system, leads, energy_list, contact, groups=None) -> [m, n_g]   (a lead's share)
    calculate_transmission_matrix_layered(system, leads, energy_list, probes=None)   -> T [m, C, C], probes on any layer
    dephasing_probes_layered(system, groups, gamma)                 -> the probes' (indices, block) list
    calculate_effective_transmission_layered(system, leads, energy_list, probes)     -> (T_eff [m], T_coherent [m])
    calculate_effective_current_layered(system, leads, fermi, qV, probes)            -> the current with floating probes
    calculate_probe_response_layered(system, leads, energy_list, probes)             -> R [m, P, n_leads] of the floating probes
    calculate_probe_occupations_layered(system, leads, energy_list, probes, f)       -> f_p(E) [m, P]
    GrLessIntProbesLayered(system, leads, Elist, weights, probes, ind=None)          -> block lists of sum_m w_m G D_s G^H (E_m)
    GrIntProbesLayered(system, leads, Elist, weights, probes)                        -> block lists of sum_m w_m G(E_m), probes in A
    calculate_bond_transmission_layered(system, leads, energy_list, contact=0, groups=None)
                                                                    -> (diag, up, low, labels): where the transmission flows
    calculate_bond_currents_layered(system, leads, fermi, qV, contact=0, groups=None) -> the same in amperes, integrated
    calculate_interlayer_transmission(system, leads, energy_list, contact=0)         -> [m, L - 1] flow across each boundary
    calculate_eigenchannels_layered(system, leads, energy_list, pair=(0, 1), nchan=None) -> T_n [m, nchan], leads up to 512 wide
    channel_count_layered(system, leads, pair=(0, 1))               -> min(K_a, K_b)

Per energy the work is L inverses and a handful of products of layer size instead of one N x N inverse.
G Gamma_c G^H is formed on the pattern of S only -- what Tr[P S], a tight-binding Fock builder and the Mulliken populations
read -- from the columns of G on the lead's orbitals, which the two sweeps yield at a few n^2 K products per layer.
The transmission matrix between all terminals, with Buettiker / D'Amato-Pastawski probes on ANY layer, comes from column
strips of G on the terminals' orbitals that the backward sweep carries from layer to layer, one pass over the layers
as they are and one in reverse order; no block of G between distant layers is formed.  With the probes FLOATING, their
response R and G D_s G^H (D_s = Gamma_s + sum_p R_ps Gamma_p, block diagonal over the layers) come from the same two passes
with the strips of all layers kept until R is known.
The local (bond) transmission flow[i, j] = 2 Im[K_ij A_ji], K = E S - F, vanishes wherever S and F do: the complete
orbital-resolved flow map lives on the pattern of S and costs one more pass over the blocks of G Gamma G^H.
The transmission eigenchannels of a pair of terminals on opposite ends need the corner block of G alone, which the
transmission already forms: the dense channel call's products on it, and for lists of 97 to 512 orbitals a wide pivoted
Cholesky and a Householder / bisection eigensolver (values only; scattering states need the leads' columns of G).
Everything that needs more of G than that raises instead of guessing: channel states, flows with floating probes, spin layouts other than 'r', sharding over ranks and checkpoint files.  The layering itself (``from_dense``, ``partition``)
is host-side numpy.
"""
import numpy as np

from .config import (ETA, SURFACE_DOUBLING_MAX_STEPS, SURFACE_DOUBLING_TOL, SURFACE_GREEN_CONVERGENCE,
                     SURFACE_GREEN_MAX_ITER, SURFACE_GREEN_SOLVER, SURFACE_RELAXATION_FACTOR)


def _worst_outside(M, offs, atol):
    """(|value|, i, j) of the largest entry of M outside the block-tridiagonal pattern given by the layer offsets that
    exceeds atol, or None."""
    L = len(offs) - 1
    layer = np.repeat(np.arange(L), np.diff(offs))
    out = np.abs(layer[:, None] - layer[None, :]) > 1
    A = np.where(out, np.abs(M), 0.0)
    k = int(np.argmax(A))
    i, j = divmod(k, M.shape[1])
    return (float(A[i, j]), i, j) if A[i, j] > atol else None


class LayeredSystem:
    """L >= 2 diagonal blocks F_ii, S_ii (n_i x n_i) and L - 1 upper blocks F_{i,i+1}, S_{i,i+1} (n_i x n_{i+1}); the
    lower blocks are their conjugate transposes (F, S Hermitian, real or complex).  The sizes are arbitrary."""

    def __init__(self, F_diag, F_up, S_diag, S_up):
        self.F_diag = [np.array(b) for b in F_diag]
        self.F_up = [np.array(b) for b in F_up]
        self.S_diag = [np.array(b) for b in S_diag]
        self.S_up = [np.array(b) for b in S_up]
        L = len(self.F_diag)
        if L < 2:
            raise ValueError(f"a layered system needs at least two layers, got {L}")
        if len(self.S_diag) != L or len(self.F_up) != L - 1 or len(self.S_up) != L - 1:
            raise ValueError("expected L diagonal blocks and L - 1 upper blocks of F and of S")
        self.sizes = tuple(int(b.shape[0]) for b in self.F_diag)
        for i in range(L):
            n = self.sizes[i]
            if n < 1 or self.F_diag[i].shape != (n, n) or self.S_diag[i].shape != (n, n):
                raise ValueError(f"diagonal block {i}: F {self.F_diag[i].shape}, S {self.S_diag[i].shape}")
        for i in range(L - 1):
            want = (self.sizes[i], self.sizes[i + 1])
            if self.F_up[i].shape != want or self.S_up[i].shape != want:
                raise ValueError(f"upper block {i}: expected {want}, got F {self.F_up[i].shape}, S {self.S_up[i].shape}")

    @property
    def n_layers(self):
        return len(self.sizes)

    @property
    def n(self):
        return int(sum(self.sizes))

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.sizes)]).astype(int)

    @classmethod
    def from_dense(cls, F, S, sizes, atol=0.0):
        """Cut (F, S) into layers of the given sizes.  Raises ValueError, naming the largest entry it would drop, when F
        or S exceeds ``atol`` outside the block-tridiagonal pattern."""
        F = np.asarray(F); S = np.asarray(S)
        sizes = [int(s) for s in sizes]
        if F.ndim != 2 or F.shape[0] != F.shape[1] or S.shape != F.shape:
            raise ValueError(f"F and S must be square matrices of one shape, got {F.shape} and {S.shape}")
        if len(sizes) < 2 or min(sizes) < 1 or sum(sizes) != F.shape[0]:
            raise ValueError(f"layer sizes {sizes} do not split {F.shape[0]} orbitals into at least two layers")
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        for name, M in (("F", F), ("S", S)):
            bad = _worst_outside(M, offs, atol)
            if bad is not None:
                raise ValueError(f"{name}[{bad[1]}, {bad[2]}] = {M[bad[1], bad[2]]!r} (|.| = {bad[0]:.3g} > atol = {atol:g}) "
                                 f"lies outside the layer pattern {tuple(sizes)}: it would be dropped")
        L = len(sizes)
        sl = [slice(offs[i], offs[i + 1]) for i in range(L)]
        return cls([F[sl[i], sl[i]] for i in range(L)], [F[sl[i], sl[i + 1]] for i in range(L - 1)],
                   [S[sl[i], sl[i]] for i in range(L)], [S[sl[i], sl[i + 1]] for i in range(L - 1)])

    def to_dense(self):
        """(F, S) as N x N matrices, lower blocks = conjugate transposes of the upper ones."""
        offs = self.offsets
        out = []
        for diag, up in ((self.F_diag, self.F_up), (self.S_diag, self.S_up)):
            M = np.zeros((self.n, self.n), dtype=np.result_type(*diag, *up))
            for i, b in enumerate(diag):
                M[offs[i]:offs[i + 1], offs[i]:offs[i + 1]] = b
            for i, b in enumerate(up):
                M[offs[i]:offs[i + 1], offs[i + 1]:offs[i + 2]] = b
                M[offs[i + 1]:offs[i + 2], offs[i]:offs[i + 1]] = b.conj().T
            out.append(M)
        return out[0], out[1]

    def locate(self, orbitals):
        """(layer, indices inside it) of a list of orbitals that must all lie in one layer."""
        orb = np.asarray(orbitals, dtype=int).ravel()
        offs = self.offsets
        if orb.size == 0 or orb.min() < 0 or orb.max() >= self.n:
            raise ValueError(f"orbital list outside 0 .. {self.n - 1}")
        layer = np.searchsorted(offs, orb, side='right') - 1
        if np.any(layer != layer[0]):
            raise ValueError("the orbitals of a lead must lie in one layer")
        return int(layer[0]), orb - offs[layer[0]]


def partition(F, S, left, right, atol=0.0):
    """The finest layering of (F, S): a breadth-first walk of the graph of |F| + |S| > atol that starts from the orbitals
    ``left`` -- layer k holds the orbitals k steps away.  Trailing layers are merged until the last one contains all of
    ``right``.  Returns (system, perm): the LayeredSystem of the permuted matrices and the permutation, layer by layer
    (``F[np.ix_(perm, perm)]`` is ``system.to_dense()[0]``).  Raises ValueError when no layering exists: part of the system
    is not connected to ``left``, or ``right`` is reached in fewer than two steps -- the only split left is then
    {left | everything else}, which puts the device and the right lead into one layer with the leads touching (a fully
    coupled matrix is the extreme case)."""
    F = np.asarray(F); S = np.asarray(S)
    n = F.shape[0]
    left = np.unique(np.asarray(left, dtype=int)); right = np.unique(np.asarray(right, dtype=int))
    if left.size == 0 or right.size == 0 or left.min() < 0 or right.min() < 0 or max(left.max(), right.max()) >= n:
        raise ValueError("left and right must be non-empty orbital lists inside the system")
    adj = (np.abs(F) + np.abs(S)) > atol
    adj = adj | adj.T
    dist = np.full(n, -1)
    dist[left] = 0
    frontier, d = left, 0
    while frontier.size:
        d += 1
        reach = np.any(adj[frontier], axis=0) & (dist < 0)
        frontier = np.nonzero(reach)[0]
        dist[frontier] = d
    if np.any(dist < 0):
        raise ValueError(f"no layering: {int(np.sum(dist < 0))} orbitals are not connected to the left lead "
                         f"(first: {int(np.nonzero(dist < 0)[0][0])})")
    last = int(dist[right].min())              # every layer from here on is merged into the last one
    if last < 2:
        # (the split {left | everything else} always exists, and is no layering: the device and the right lead share a
        # layer, the two leads touch, and the sweep costs more than the dense inverse)
        raise ValueError("no layering with two or more layers exists that keeps the leads apart: orbitals of the right "
                         "lead couple directly to, or are among, the left lead's (a fully coupled system belongs on "
                         "the dense engine)")
    dist = np.minimum(dist, last)
    perm = np.argsort(dist, kind='stable')
    sizes = np.bincount(dist, minlength=last + 1)
    system = LayeredSystem.from_dense(F[np.ix_(perm, perm)], S[np.ix_(perm, perm)], sizes, atol=atol)
    return system, perm


class Lead:
    """A terminal of a layered system: a self-energy block on the orbitals ``inds`` (numbered in the whole system, all
    inside layer 0 or the last layer)."""

    def __init__(self, kind, inds, **kw):
        self.kind = kind
        self.inds = np.asarray(inds, dtype=int).ravel()
        self.kw = kw

    @classmethod
    def const(cls, inds, sigma):
        """An energy-independent K x K block."""
        return cls('const', inds, sigma=np.asarray(sigma))

    @classmethod
    def chain(cls, inds, alpha, Salpha, beta, Sbeta, tau=None, Stau=None, eta=ETA, solver=SURFACE_GREEN_SOLVER,
              conv=SURFACE_GREEN_CONVERGENCE, relFactor=SURFACE_RELAXATION_FACTOR, max_iter=SURFACE_GREEN_MAX_ITER,
              tol=SURFACE_DOUBLING_TOL, max_steps=SURFACE_DOUBLING_MAX_STEPS):
        """A 1-D chain lead with unit cell (alpha, Salpha), hopping (beta, Sbeta) and coupling (tau, Stau) to the device
        (default: the lead's own hopping); ``solver`` 'fixed-point' or 'doubling'."""
        return cls('chain', inds, alpha=alpha, Salpha=Salpha, beta=beta, Sbeta=Sbeta,
                   tau=beta if tau is None else tau, Stau=Sbeta if Stau is None else Stau, eta=eta, solver=solver,
                   conv=conv, relFactor=relFactor, max_iter=max_iter, tol=tol, max_steps=max_steps)

    @classmethod
    def blocks(cls, inds, sigma):
        """Blocks [m, K, K] evaluated by the caller for exactly the energies of the calls that follow (Bethe lattices,
        foreign self-energies); a call with more energies is refused."""
        return cls('blocks', inds, sigma=np.asarray(sigma))


class _Bound:
    """A system with its leads on the engine, freed when the call is over."""

    def __init__(self, system, leads, engine=None):
        from .engine import get_engine
        if not isinstance(system, LayeredSystem):
            raise TypeError("expected a LayeredSystem (LayeredSystem.from_dense / partition make one)")
        self.eng = engine if engine is not None else get_engine()
        self.system = system
        placed = []
        for lead in leads:
            layer, local = system.locate(lead.inds)
            if layer not in (0, system.n_layers - 1):
                raise ValueError(f"a lead on layer {layer}: terminals sit on the first or the last layer only")
            placed.append((lead, layer, local))
        self.h = self.eng.layered_create(system.F_diag, system.F_up, system.S_diag, system.S_up)
        self.terms = []
        try:
            for lead, layer, local in placed:
                if lead.kind == 'const':
                    t = self.eng.layered_terminal_const(self.h, layer, local, lead.kw['sigma'])
                elif lead.kind == 'blocks':
                    t = self.eng.layered_terminal_blocks(self.h, layer, local, lead.kw['sigma'])
                else:
                    t = self.eng.layered_terminal_chain(self.h, layer, local, **lead.kw)
                self.terms.append(t)
        except Exception:
            self.close()
            raise

    def term_of(self, ind):
        """the engine's terminal number of lead ``ind`` (negative: from the end), None: all"""
        if ind is None:
            return None
        if not -len(self.terms) <= int(ind) < len(self.terms):
            raise ValueError(f"lead {ind} of {len(self.terms)}")
        return self.terms[int(ind)]

    def close(self):
        if self.h is not None:
            self.eng.layered_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _only_restricted(spin):
    if spin not in (None, 'r'):
        raise NotImplementedError(f"layered systems serve spin='r' only, got {spin!r}")


def _no_checkpoint(checkpoint_file):
    if checkpoint_file:
        raise NotImplementedError("checkpoint files are not written for layered systems")


def calculate_transmission_layered(system, leads, energy_list, spin=None, checkpoint_file=None, pair=(0, 1),
                                   engine=None):
    """T(E) [m] = Re Tr[Gamma_a G_ab Gamma_b G_ab^H] for ``pair`` = (a, b), indices into ``leads`` that sit on opposite
    end layers (calculate_transmission's contacts 0 and 1)."""
    _only_restricted(spin); _no_checkpoint(checkpoint_file)
    with _Bound(system, leads, engine) as b:
        return b.eng.layered_transmission(b.h, b.terms[pair[0]], b.terms[pair[1]], np.asarray(energy_list))


def calculate_dos_layered(system, leads, energy_list, spin=None, checkpoint_file=None, engine=None):
    """(dos_total [m], dos_per_site [m, N]): the reference's -Im diag G / pi, as calculate_dos; orbitals in layer order."""
    _only_restricted(spin); _no_checkpoint(checkpoint_file)
    with _Bound(system, leads, engine) as b:
        return b.eng.layered_dos(b.h, np.asarray(energy_list), mulliken=False)


def calculate_pdos_layered(system, leads, energy_list, groups=None, contact=None, spin=None, engine=None):
    """Mulliken projected DOS [m, n_g], row a = sum_{i in a} -Im (G S)_ii / pi, as calculate_pdos with contact=None;
    ``groups`` maps the N orbitals (layer order) to groups, None: every orbital its own."""
    _only_restricted(spin)
    if contact is not None:
        raise NotImplementedError("the contact-resolved populations are calculate_contact_pdos_layered's")
    with _Bound(system, leads, engine) as b:
        _, site = b.eng.layered_dos(b.h, np.asarray(energy_list), mulliken=True)
    return _grouped(system, site, groups)


def _grouped(system, site, groups):
    if groups is None:
        return site
    groups = np.asarray(groups, dtype=int).ravel()
    if groups.size != system.n or groups.min() < 0:
        raise ValueError(f"groups must map the {system.n} orbitals to non-negative group numbers")
    out = np.zeros((site.shape[0], int(groups.max()) + 1))
    for g in range(out.shape[1]):                 # orbitals of a group in ascending order
        out[:, g] = site[:, groups == g].sum(axis=1)
    return out


def calculate_contact_pdos_layered(system, leads, energy_list, contact, groups=None, spin=None, engine=None):
    """The share of lead ``contact`` (an index into ``leads``, None: all of them) in the Mulliken projected DOS [m, n_g],
    row a = sum_{i in a} (1/2pi) Re sum_j (G Gamma_c G^H)_ij conj(S_ij), as calculate_pdos with a contact; ``groups`` as
    calculate_pdos_layered's."""
    _only_restricted(spin)
    with _Bound(system, leads, engine) as b:
        _, site = b.eng.layered_contact_dos(b.h, b.term_of(contact), np.asarray(energy_list))
    return _grouped(system, site, groups)


def GrIntLayered(system, leads, Elist, weights, engine=None):
    """sum_m w_m G(E_m) on the pattern of S, as GrInt: (diagonal blocks, upper blocks G_{i,i+1}, lower blocks G_{i+1,i})."""
    with _Bound(system, leads, engine) as b:
        return b.eng.layered_gr_int(b.h, np.asarray(Elist), np.asarray(weights))


def GrLessIntLayered(system, leads, Elist, weights, ind=None, engine=None):
    """sum_m w_m G Gamma G^H (E_m) on the pattern of S, as GrLessInt: (diagonal blocks, upper blocks (i, i+1), lower blocks
    (i+1, i)); ``ind`` indexes ``leads``, None: Gamma of all of them."""
    with _Bound(system, leads, engine) as b:
        return b.eng.layered_gless_int(b.h, b.term_of(ind), np.asarray(Elist), np.asarray(weights))


def calculate_transmission_matrix_layered(system, leads, energy_list, probes=None, spin=None, checkpoint_file=None,
                                          engine=None):
    """T [m, C, C] between all terminals: T[k, a, b] = Re Tr[Gamma_a G Gamma_b G^H](E_k), the transmission from b into a, as
    calculate_transmission_matrix.  The terminals are ``leads`` in their order, then ``probes``: a list of (indices,
    block) -- orbitals numbered in the whole system in layer order, each probe inside one layer, any layer (see
    dephasing_probes_layered).  Without probes: the matrix over the leads, pairs on the same end included."""
    _only_restricted(spin); _no_checkpoint(checkpoint_file)
    with _Bound(system, leads, engine) as b:
        return b.eng.layered_transmission_matrix(b.h, np.asarray(energy_list), probes)


def dephasing_probes_layered(system, groups, gamma):
    """Buettiker / D'Amato-Pastawski probes on a layered system, as transport.dephasing_probes: the list of (indices,
    block) with Sigma_p = -(i gamma_p / 2) S[I_p, I_p], S taken from the system's own diagonal blocks.  ``groups``: an
    orbital -> probe label map of length N (negative: no probe; labels without an orbital are skipped) or a list of index
    lists, orbitals numbered in layer order; ``gamma``: a scalar or one value per probe.  Raises ValueError when a group
    spans layers."""
    if not isinstance(system, LayeredSystem):
        raise TypeError("expected a LayeredSystem (LayeredSystem.from_dense / partition make one)")
    n = system.n
    if len(groups) > 0 and np.ndim(groups[0]) > 0:
        lists = [np.asarray(g, dtype=int).ravel() for g in groups]
    else:
        g = np.asarray(groups).ravel()
        if g.size != n or not np.issubdtype(g.dtype, np.integer):
            raise ValueError(f"groups must be an integer label per orbital (length {n}) or a list of index lists")
        lists = [np.nonzero(g == lab)[0] for lab in range(int(g.max()) + 1 if g.size else 0)]
        lists = [ix for ix in lists if ix.size]
    gam = (np.broadcast_to(np.asarray(gamma, dtype=float), (len(lists),)) if np.ndim(gamma) == 0
           else np.asarray(gamma, dtype=float).ravel())
    if gam.size != len(lists):
        raise ValueError(f"gamma must be a scalar or one value per probe ({len(lists)}), got {gam.size}")
    offs = system.offsets
    out = []
    for q, (ix, gp) in enumerate(zip(lists, gam)):
        if ix.size == 0 or ix.min() < 0 or ix.max() >= n or np.unique(ix).size != ix.size:
            raise ValueError(f"a probe must be a non-empty list of distinct orbital indices in [0, {n})")
        layer = np.searchsorted(offs, ix, side='right') - 1
        if layer.min() != layer.max():
            raise ValueError(f"probe group {q} spans layers {int(layer.min())} and {int(layer.max())}: a probe of a layered "
                             "system lies inside one layer")
        loc = ix - offs[layer[0]]
        out.append((ix, -0.5j * gp * np.asarray(system.S_diag[layer[0]])[np.ix_(loc, loc)].astype(complex)))
    return out


def calculate_effective_transmission_layered(system, leads, energy_list, probes, source=0, drain=-1, spin=None, engine=None):
    """(T_eff [m], T_coherent [m]) between the leads ``source`` and ``drain`` with the ``probes`` floating at every energy,
    as calculate_effective_transmission: transport.effective_transmission on calculate_transmission_matrix_layered's
    result (the solve runs on the host); T_coherent is the direct term T[drain][source] in the presence of the probes."""
    from .transport import effective_transmission
    T = calculate_transmission_matrix_layered(system, leads, energy_list, probes=probes, spin=spin, engine=engine)
    n_real = len(leads)
    eff = effective_transmission(T, n_real, source, drain)
    d = drain + n_real if drain < 0 else drain
    s_ = source + n_real if source < 0 else source
    return eff, T[:, d, s_]


def calculate_probe_response_layered(system, leads, energy_list, probes, spin=None, checkpoint_file=None, engine=None):
    """R [m, P, n_leads]: the response of the floating ``probes`` to the leads, solved on the device, as
    calculate_probe_response: probe p's occupation at E_k is sum_c R[k, p, c] f_c(E_k).  ``probes`` as
    calculate_transmission_matrix_layered takes them (dephasing_probes_layered makes them)."""
    _only_restricted(spin); _no_checkpoint(checkpoint_file)
    with _Bound(system, leads, engine) as b:
        return b.eng.layered_probe_response(b.h, np.asarray(energy_list), probes)


def calculate_probe_occupations_layered(system, leads, energy_list, probes, f, spin=None, checkpoint_file=None, engine=None):
    """f_p(E_k) [m, P] = sum_c R[k, p, c] f_c(E_k) of the floating probes; ``f``: the leads' occupations, [n_leads] (the
    same at every energy) or [m, n_leads].  The sum over the leads runs on the host."""
    R = calculate_probe_response_layered(system, leads, energy_list, probes, spin=spin, checkpoint_file=checkpoint_file,
                                         engine=engine)
    f = np.asarray(f, dtype=float)
    if f.shape not in ((R.shape[2],), (R.shape[0], R.shape[2])):
        raise ValueError(f"f must be [{R.shape[2]}] or [{R.shape[0]}, {R.shape[2]}], got {f.shape}")
    return np.einsum('kpc,kc->kp', R, np.broadcast_to(f, (R.shape[0], R.shape[2])))


def GrLessIntProbesLayered(system, leads, Elist, weights, probes, ind=None, spin=None, checkpoint_file=None, engine=None):
    """sum_m w_m G D_s G^H (E_m) on the pattern of S with the ``probes`` floating at every energy, as GrLessIntProbes: D_s =
    Gamma_s + sum_p R_ps Gamma_p, the non-equilibrium density's integrand with dephasing.  ``ind`` indexes ``leads``, None:
    Gamma of all terminals.  Returns GrLessIntLayered's (diagonal blocks, upper blocks, lower blocks)."""
    _only_restricted(spin); _no_checkpoint(checkpoint_file)
    with _Bound(system, leads, engine) as b:
        return b.eng.layered_gless_int_probes(b.h, b.term_of(ind), np.asarray(Elist), np.asarray(weights), probes)


def GrIntProbesLayered(system, leads, Elist, weights, probes, spin=None, checkpoint_file=None, engine=None):
    """sum_m w_m G(E_m) on the pattern of S with the ``probes`` in E S - F - Sigma, as GrIntProbes: GrIntLayered's block lists."""
    _only_restricted(spin); _no_checkpoint(checkpoint_file)
    with _Bound(system, leads, engine) as b:
        return b.eng.layered_gr_int_probes(b.h, np.asarray(Elist), np.asarray(weights), probes)


def calculate_effective_current_layered(system, leads, fermi, qV, probes, T=None, spin=None, dE=None, engine=None):
    """Current at bias qV with dephasing probes, as calculate_effective_current: transport.current_grid's energies, its
    occupation factor, trapezoid rule, e/h and the factor 2 of spin 'r', applied to
    calculate_effective_transmission_layered's T_eff."""
    from . import transport as tp
    _only_restricted(spin)
    T = tp.TEMPERATURE if T is None else T
    dE = tp.ENERGY_STEP if dE is None else dE
    if fermi is None or qV is None:
        raise ValueError("fermi and qV must be provided for current calculations")
    if np.allclose(0, qV):
        return 0.0
    energies, muL, muR = tp.current_grid(fermi, qV, T, dE)
    if len(energies) == 0:
        raise ValueError("No energies in integration window. Check fermi, qV, and dE.")
    t_eff, _ = calculate_effective_transmission_layered(system, leads, energies, probes, engine=engine)
    if T == 0:
        total = tp.eoverh * tp.trapezoid(t_eff, energies)
    else:
        occupation = np.abs(1 / (np.exp((energies - muR) / (tp.kB * T)) + 1) - 1 / (np.exp((energies - muL) / (tp.kB * T)) + 1))
        total = tp.eoverh * tp.trapezoid(t_eff * occupation, energies)
    return 2 * total


def _layer_groups(system, groups):
    """``groups``: an integer label >= 0 per orbital of the whole system.  Returns (groups_per_layer [L], group_of [N]: the
    position of each orbital's label among the ascending labels of its own layer, labels_per_layer); (None, None, None)
    without groups.  Raises ValueError for a wrong length, a negative label, and a label whose orbitals span two layers."""
    if not isinstance(system, LayeredSystem):
        raise TypeError("expected a LayeredSystem (LayeredSystem.from_dense / partition make one)")
    if groups is None:
        return None, None, None
    g = np.asarray(groups).ravel()
    if g.size != system.n or not np.issubdtype(g.dtype, np.integer):
        raise ValueError(f"groups must be an integer label per orbital (length {system.n}), got {g.size} entries of {g.dtype}")
    if g.min() < 0:
        raise ValueError(f"group labels must be non-negative, got {int(g.min())}")
    offs = system.offsets
    layer = np.repeat(np.arange(system.n_layers), system.sizes)
    first = {}
    for lab, lay in zip(g.tolist(), layer.tolist()):
        if first.setdefault(lab, lay) != lay:
            raise ValueError(f"group label {lab} spans layers {first[lab]} and {lay}: a group of a layered system lies "
                             "inside one layer")
    labels, group_of = [], np.zeros(system.n, dtype=np.int32)
    for i in range(system.n_layers):
        lab, inv = np.unique(g[offs[i]:offs[i + 1]], return_inverse=True)          # ascending
        labels.append(lab)
        group_of[offs[i]:offs[i + 1]] = inv
    return np.array([len(lab) for lab in labels], dtype=np.int32), group_of, labels


def calculate_bond_transmission_layered(system, leads, energy_list, contact=0, groups=None, spin=None, engine=None):
    """Local (bond) transmission on a layered system, as calculate_local_transmission: WHERE the transmission injected by
    lead ``contact`` (an index into ``leads``, None: all of them) flows.  flow[i, j] = 2 Im[K_ij A_ji] with K = E S - F and
    A = G Gamma_c G^H is zero wherever S and F are, so the complete map lives on the pattern of S: returns (diag, upper,
    lower, labels_per_layer), block lists with entries [m, g_i, g_j] -- the flow inside layer i, from layer i into layer
    i + 1, and from layer i + 1 into layer i.  ``groups``: an integer label >= 0 per orbital of the whole system (atoms,
    fragments), each label inside ONE layer; the labels of a layer are taken in ascending order (labels_per_layer[i][a] is
    the label of row a of layer i's blocks).  None: per orbital pair (g_i = n_i, labels_per_layer None).
    pattern_to_dense(...) assembles an [m, G, G] table for small systems."""
    _only_restricted(spin)
    gpl, group_of, labels = _layer_groups(system, groups)
    with _Bound(system, leads, engine) as b:
        d, u, l = b.eng.layered_local_transmission(b.h, b.term_of(contact), np.asarray(energy_list), gpl, group_of)
    return d, u, l, labels


def calculate_interlayer_transmission(system, leads, energy_list, contact=0, spin=None, engine=None):
    """[m, L - 1]: the flow from layer i into layer i + 1 of the transmission injected by lead ``contact`` -- the sum of the
    upper block i of calculate_bond_transmission_layered, obtained with one group per layer (nothing orbital-sized comes
    back).  For one injecting lead at real energies every column equals the transmission into the leads of the other
    end (with the sign of the direction): the current is conserved from boundary to boundary."""
    _only_restricted(spin)
    if not isinstance(system, LayeredSystem):
        raise TypeError("expected a LayeredSystem (LayeredSystem.from_dense / partition make one)")
    gpl = np.ones(system.n_layers, dtype=np.int32)
    with _Bound(system, leads, engine) as b:
        _, u, _ = b.eng.layered_local_transmission(b.h, b.term_of(contact), np.asarray(energy_list), gpl,
                                                   np.zeros(system.n, dtype=np.int32))
    return np.stack([blk[:, 0, 0] for blk in u], axis=1)


def calculate_bond_currents_layered(system, leads, fermi, qV, T=None, contact=0, groups=None, dE=None, spin=None,
                                    engine=None):
    """Bond currents in amperes on the pattern of S, as calculate_bond_currents: the local transmission of lead
    ``contact`` integrated over transport.current_grid's energies with its occupation factor, trapezoid weights (signed
    step for qV < 0), e/h and the factor 2 of spin 'r', in ONE pass over the grid (Engine.layered_bond_int).  Returns
    (diag, upper, lower, labels_per_layer) with [g_i, g_j] blocks; ``groups`` as calculate_bond_transmission_layered's, summed
    on the host with the orbitals of a group in ascending order.  qV ~ 0 returns zeros."""
    from . import transport as tp
    _only_restricted(spin)
    T = tp.TEMPERATURE if T is None else T
    dE = tp.ENERGY_STEP if dE is None else dE
    if fermi is None or qV is None:
        raise ValueError("fermi and qV must be provided for current calculations")
    gpl, group_of, labels = _layer_groups(system, groups)
    sizes = system.sizes
    if np.allclose(0, qV):
        g = sizes if gpl is None else tuple(int(x) for x in gpl)
        return ([np.zeros((a, a)) for a in g], [np.zeros((a, c)) for a, c in zip(g[:-1], g[1:])],
                [np.zeros((c, a)) for a, c in zip(g[:-1], g[1:])], labels)
    energies, muL, muR = tp.current_grid(fermi, qV, T, dE)
    if len(energies) == 0:
        raise ValueError("No energies in integration window. Check fermi, qV, and dE.")
    # trapezoid(y * occupation, energies) = sum_k w_k y_k
    w = np.zeros(len(energies))
    if len(energies) > 1:
        d = np.diff(energies)
        w[:-1] += d / 2
        w[1:] += d / 2
    if T != 0:
        w = w * np.abs(1 / (np.exp((energies - muR) / (tp.kB * T)) + 1) - 1 / (np.exp((energies - muL) / (tp.kB * T)) + 1))
    with _Bound(system, leads, engine) as b:
        blocks = b.eng.layered_bond_int(b.h, b.term_of(contact), energies, w)
    blocks = [[2 * tp.eoverh * blk for blk in kind] for kind in blocks]
    if gpl is not None:
        offs = system.offsets
        loc = [group_of[offs[i]:offs[i + 1]] for i in range(system.n_layers)]

        def summed(blk, i, j):
            out = np.zeros((gpl[i], gpl[j]))
            for a in range(gpl[i]):
                rows = blk[loc[i] == a]                                       # ascending orbitals
                for c in range(gpl[j]):
                    out[a, c] = rows[:, loc[j] == c].sum()
            return out
        L = system.n_layers
        blocks = [[summed(blocks[0][i], i, i) for i in range(L)], [summed(blocks[1][i], i, i + 1) for i in range(L - 1)],
                  [summed(blocks[2][i], i + 1, i) for i in range(L - 1)]]
    return blocks[0], blocks[1], blocks[2], labels


def pattern_to_dense(sizes, diag, upper, lower):
    """The block lists of a result on the pattern of S (blocks [..., n_i, n_j], any leading axes) as one [..., N, N] array,
    zero outside the pattern -- for small systems and tests."""
    sizes = [int(n) for n in sizes]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    if len(diag) != len(sizes) or len(upper) != len(sizes) - 1 or len(lower) != len(sizes) - 1:
        raise ValueError("expected L diagonal blocks and L - 1 upper and lower blocks")
    lead = np.shape(diag[0])[:-2]
    out = np.zeros(lead + (offs[-1], offs[-1]), dtype=np.result_type(*diag, *upper, *lower))
    for i, blk in enumerate(diag):
        out[..., offs[i]:offs[i + 1], offs[i]:offs[i + 1]] = blk
    for i in range(len(sizes) - 1):
        out[..., offs[i]:offs[i + 1], offs[i + 1]:offs[i + 2]] = upper[i]
        out[..., offs[i + 1]:offs[i + 2], offs[i]:offs[i + 1]] = lower[i]
    return out


# ----------------------------------------------------------------------------- transmission eigenchannels
# The entry points of include/negf_layered_channels.h (_lib.SIGNATURES_LAYERED_CHANNELS), reached through the engine's
# own way into the library (Engine._call / _counted / _host): module-level functions, the engine as an argument.
EIG_WIDE_KMAX = 512


def _engine(engine):
    from .engine import get_engine
    return engine if engine is not None else get_engine()


def set_channel_algo(algo, engine=None):
    """Which kernels the layered channel call runs: 0 by size (min(K_a, K_b) <= 96 the kernels of the dense channel call,
    above that the wide ones; default), 1 the wide kernels at every size (tests)."""
    _engine(engine)._call("negf_set_channel_algo", int(algo))


def eigvalsh_wide(A, engine=None):
    """Ascending eigenvalues [m, K] of the Hermitian matrices A [m, K, K] (or one [K, K] -> [K]), 1 <= K <= 512, read from
    their lower triangles like numpy.linalg.eigvalsh: the WIDE kernel alone (Householder tridiagonalisation, bisection),
    a diagnostic (negf_eigvalsh_wide_batched).  A row whose input is not finite is NaN; the engine's ``last_info`` holds
    the per-matrix flags (1: non-finite)."""
    import warnings
    from . import _lib
    from .engine import _ptr, _first_bad
    eng = _engine(engine)
    A = np.ascontiguousarray(A, dtype=np.complex128)
    single = A.ndim == 2
    if single:
        A = A[None]
    if A.ndim != 3 or A.shape[1] != A.shape[2]:
        raise ValueError(f"eigvalsh_wide: expected [m, K, K] or [K, K], got {A.shape}")
    m, K = A.shape[0], A.shape[1]
    if not 1 <= K <= EIG_WIDE_KMAX:
        raise ValueError(f"eigvalsh_wide: K = {K} outside 1 .. {EIG_WIDE_KMAX}")
    w = np.zeros((m, K), dtype=np.float64)
    info = np.zeros(max(m, 1), dtype=np.int32)
    rc = eng._call("negf_eigvalsh_wide_batched", K, m, _ptr(A), _ptr(w), _ptr(info))
    eng.last_info = info[:m]
    if rc == _lib.NEGF_ESINGULAR:
        warnings.warn(f"eigvalsh_wide: non-finite input for matrices {_first_bad(np.nonzero(info[:m])[0])}", RuntimeWarning)
    return w[0] if single else w


def layered_channel_count(eng, handle, term_a, term_b):
    """min(K_a, K_b) of two terminals of an engine-side layered system; ValueError for a pair on the same end layer or
    more than 512 channels."""
    import ctypes as C
    nc = C.c_int(0)
    eng._call("negf_layered_channel_count", int(handle), int(term_a), int(term_b), C.byref(nc))
    return nc.value


def layered_transmission_channels(eng, handle, term_a, term_b, E, nchan=None):
    """T_n(E) [m, nchan] of two terminals of an engine-side layered system, descending per energy
    (negf_layered_transmission_channels); nchan defaults to layered_channel_count().  Rows of singular energies are NaN
    (with a warning, as layered_transmission); ``eng.last_info`` holds the per-energy info, the eigensolver's flags
    negative."""
    import warnings
    from . import _lib
    from .engine import _ptr, _first_bad
    nchan = layered_channel_count(eng, handle, term_a, term_b) if nchan is None else int(nchan)
    if nchan < 1:
        raise ValueError("nchan must be at least 1")
    E, _ = eng._grid(E)
    T = np.zeros((E.size, nchan), dtype=np.float64)
    where = "layered_transmission_channels"
    info = eng._host(where, E.size, int(handle), int(term_a), int(term_b), E.size, _ptr(E), nchan, _ptr(T), raw=True)
    # info > 0: a singular layer (pivot column in the whole system); < 0: the eigensolver's flags on H -- reported apart
    eng._numerical(_lib.NEGF_ESINGULAR if np.any(info > 0) else 0, np.where(info > 0, info, 0), where)
    eng.last_info = info
    bad = np.nonzero(info < 0)[0]
    if bad.size:
        what = {-1: "non-finite H", -2: "Jacobi not converged within its sweep limit"}
        kinds = sorted({what.get(int(v), str(int(v))) for v in info[bad]})
        warnings.warn(f"{where}: eigensolver flags ({', '.join(kinds)}) at energy indices {_first_bad(bad)}", RuntimeWarning)
    return T


def layered_transmission_channels_dev(eng, handle, term_a, term_b, m, E_ptr, nchan, T_ptr):
    """The device-resident form: E_ptr [m] complex128 and T_ptr [m, nchan] float64 are device addresses; the stream
    contract of Engine.set_stream holds (T is overwritten, nothing waits for the host on a warm call)."""
    from .engine import _p
    eng._counted(m)("negf_layered_transmission_channels_dev", int(handle), int(term_a), int(term_b), int(m), _p(E_ptr),
                    int(nchan), _p(T_ptr))


def _opposite_pair(b, pair):
    """the engine's terminal numbers of ``pair`` = (a, b), indices into the leads; ValueError unless they sit on opposite
    end layers"""
    ta, tb = b.term_of(pair[0]), b.term_of(pair[1])
    if ta is None or tb is None:
        raise ValueError("pair must name two leads")
    return ta, tb


def channel_count_layered(system, leads, pair=(0, 1), engine=None):
    """min(K_a, K_b): the number of transmission eigenchannels of ``pair`` = (a, b), indices into ``leads`` on opposite end
    layers; ValueError for a pair on one end and for more than 512 channels."""
    with _Bound(system, leads, engine) as b:
        return layered_channel_count(b.eng, b.h, *_opposite_pair(b, pair))


def calculate_eigenchannels_layered(system, leads, energy_list, pair=(0, 1), nchan=None, spin=None, checkpoint_file=None,
                                    engine=None):
    """Transmission eigenchannels T_n(E) [m, nchan] of a layered system, descending per energy: the eigenvalues of t^H t,
    t = Gamma_a^{1/2} G_ab Gamma_b^{1/2}, for ``pair`` = (a, b) read as calculate_transmission_layered reads it (indices into
    ``leads`` on opposite end layers) -- their sum is calculate_transmission_layered's T(E).  The eigenproblem lives on the
    shorter of the two orbital lists, at most 512 orbitals (up to 96 the kernels of calculate_transmission_channels, above
    that a Householder / bisection solver); ``nchan`` defaults to channel_count_layered().  Exact zeros beyond the rank of
    the factored Gamma; rows of singular energies are NaN, with a warning.  Values only."""
    _only_restricted(spin); _no_checkpoint(checkpoint_file)
    with _Bound(system, leads, engine) as b:
        ta, tb = _opposite_pair(b, pair)
        return layered_transmission_channels(b.eng, b.h, ta, tb, np.asarray(energy_list), nchan)


def _not_served(name, why):
    def fn(*args, **kwargs):
        raise NotImplementedError(f"{name} is not served on layered systems: {why}")
    fn.__name__ = name
    return fn


calculate_transmission_channels_layered = _not_served(
    "calculate_transmission_channels_layered",
    "the eigenchannel values of a layered system are calculate_eigenchannels_layered's (pair= instead of two contact "
    "numbers, leads up to 512 orbitals wide); channel states need the leads' columns of G and stay with the dense engine "
    "on system.to_dense()")
calculate_local_transmission_layered = _not_served(
    "calculate_local_transmission_layered",
    "the local transmission of a layered system lives on the pattern of S and is calculate_bond_transmission_layered's "
    "(block lists instead of an N x N table; pattern_to_dense assembles one)")
