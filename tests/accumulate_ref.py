"""
The weighted sum behind GrInt / GrIntSegments / gr_int_refine, out_ij = acc_ij + sum_b w_b X_b,ij
(gaunegf_amd/csrc/k_elementwise.hip: accumulate_partial_kernel, accumulate_perm_rows_kernel, accumulate_perm_partial_kernel,
accumulate_final_kernel, accumulate_final_seg_kernel), held ENTRY BY ENTRY to an extended-precision truth.

Truth: the sum formed in np.clongdouble (64-bit significand) from the float64 operands.  Its own error is k * 2^-64 of the
bar's sum, 2^-11 of the bar below: ignored.

Bar (derived, not measured).  The kernels cut a segment's share of a workspace batch into chunks of ACC_CHUNK = 32 matrices,
add a chunk from zero with cfma (a.x + w.x x.x - w.y x.y: a product is rounded once, then takes part in two additions per
later matrix of its chunk at the most), and add the C chunk records of the segment -- over all workspace batches -- to the
result in order.  A product therefore takes part in at most

    k = 2 * min(len, 32) + C + 2

roundings (len: the longest share of the segment in one batch), and with u = 2^-53, gamma_k = k u / (1 - k u) (Higham,
Accuracy and Stability of Numerical Algorithms, Lemma 3.1 and section 4.2: any order of additions)

    |Re err_ij| <= gamma_k sum_b (|Re w_b| |Re X_b,ij| + |Im w_b| |Im X_b,ij|)
    |Im err_ij| <= gamma_k sum_b (|Re w_b| |Im X_b,ij| + |Im w_b| |Re X_b,ij|)

whether the compiler contracts a product and an addition into one fma (one rounding fewer) or not.  A float64 model of the
kernels' order (model_segments below) stays below half of the bar (tests/test_accumulate_host.py), so the bar is within
about a decade of tight; a dropped, doubled or misplaced term misses it by ten orders of magnitude.
"""
import numpy as np

ACC_CHUNK = 32
U = 2.0 ** -53
LD = np.longdouble
CLD = np.clongdouble


# ------------------------------------------------------------------ the host rules, restated
def batch_shares(seg_end, m0, nb):
    """[(lo, hi, slot)]: the energies [lo, hi) of the batch [m0, m0 + nb), counted from its first one, that belong to
    segment slot; empty shares left out (batch_shares, negf_api.hip)."""
    out, start = [], 0
    for sg, end in enumerate(seg_end):
        lo, hi = max(start, m0), min(end, m0 + nb)
        if hi > lo:
            out.append((lo - m0, hi - m0, sg))
        start = end
    return out


def shares_of(seg_end, m, batch):
    """Per segment, the list of its share lengths over the batches of a grid of m energies swept `batch` at a time."""
    per = [[] for _ in seg_end]
    for m0 in range(0, m, batch):
        for lo, hi, sg in batch_shares(seg_end, m0, min(batch, m - m0)):
            per[sg].append(hi - lo)
    return per


def k_of(shares):
    """k of the bar from one segment's shares per batch: 2 * min(longest share, 32) + (chunk records) + 2."""
    shares = [int(s) for s in shares if s > 0]
    if not shares:
        return 0
    records = sum((s + ACC_CHUNK - 1) // ACC_CHUNK for s in shares)
    return 2 * min(max(shares), ACC_CHUNK) + records + 2


ACC_TAB_SEGS, ACC_TAB_CHUNKS, APR_MAXN = 32, 96, 2048


def one_table_serves(n, perm, shares):
    """launch_accumulate_ranges' rule for the shares (lo, hi, slot) of one batch: True when one chunk table serves them
    all, False when gr_seg_core launches range by range (more than 32 ranges, more than 96 chunks, or the permuted read
    above the row form's n)."""
    if len(shares) > ACC_TAB_SEGS or (perm and n > APR_MAXN):
        return False
    return sum((hi - lo + ACC_CHUNK - 1) // ACC_CHUNK for lo, hi, _ in shares) <= ACC_TAB_CHUNKS


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------ truth and bar
def reference(w, X, rows=None):
    """sum_b w_b X_b in np.clongdouble (the rows `rows` of every matrix, all of them by default)."""
    w = np.asarray(w, dtype=np.complex128).ravel()
    sel = slice(None) if rows is None else np.asarray(rows)
    ref = None
    for b in range(w.size):
        t = CLD(w[b]) * np.asarray(X[b][sel], dtype=np.complex128).astype(CLD)
        ref = t if ref is None else ref + t
    return ref


def bar_sums(w, X, rows=None):
    """(sum_b |Re w||Re X| + |Im w||Im X|, sum_b |Re w||Im X| + |Im w||Re X|) in long double."""
    w = np.asarray(w, dtype=np.complex128).ravel()
    sel = slice(None) if rows is None else np.asarray(rows)
    sr = si = None
    for b in range(w.size):
        x = np.asarray(X[b][sel], dtype=np.complex128)
        xr, xi = np.abs(x.real).astype(LD), np.abs(x.imag).astype(LD)
        wr, wi = LD(abs(w[b].real)), LD(abs(w[b].imag))
        tr, ti = wr * xr + wi * xi, wr * xi + wi * xr
        sr, si = (tr, ti) if sr is None else (sr + tr, si + ti)
    return sr, si


def ratio(got, w, X, k, rows=None, block=256):
    """The worst of |error| / bar over all entries and both components (inf where an entry with a zero bar is not exact,
    or where `got` is not finite).  `rows`: compare these rows only.  Worked through in blocks of rows: the long double
    copies of a 2049 x 2049 batch are hundreds of megabytes each."""
    got = np.asarray(got)
    idx = np.arange(got.shape[0]) if rows is None else np.asarray(rows)
    g, worst = LD(gamma(k)), 0.0
    for s in range(0, idx.size, block):
        r = idx[s:s + block]
        ref = reference(w, X, r)
        sr, si = bar_sums(w, X, r)
        gt = got[r]
        for err, bar in ((np.abs(gt.real.astype(LD) - ref.real), g * sr), (np.abs(gt.imag.astype(LD) - ref.imag), g * si)):
            if not np.all(np.isfinite(err)):
                return np.inf
            if np.any((bar == 0) & (err != 0)):
                return np.inf
            q = np.divide(err, bar, out=np.zeros_like(err), where=bar > 0)
            worst = max(worst, float(q.max()))
    return worst


# ------------------------------------------------------------------ inputs shared by the host and the GPU tests
def const_system(N, seed, gamma_c=0.1):
    """(F, S, [Sigma_left, Sigma_right]): helpers.random_system with the constant contacts of test_small_fused_gpu._const
    (-i gamma on the first / last N // 10 orbitals over -i 1e-9 S), plus a seeded NON-symmetric block of a tenth of that
    size on the contact orbitals.  With F, S and Sigma all symmetric G(E) is complex symmetric, and a kernel that read a
    matrix transposed -- rows and columns of the permuted read exchanged consistently -- would pass every check."""
    from helpers import const_sigma_pair, random_system
    F, S = random_system(N, seed)
    nc = max(1, N // 10)
    inds, sl, sr = const_sigma_pair(N, S, nc, gamma_c)
    rng = np.random.default_rng(seed + 7919)
    for sig, ix in zip((sl, sr), inds):
        V = rng.standard_normal((nc, nc)) + 1j * rng.standard_normal((nc, nc))
        sig[np.ix_(ix, ix)] += 0.1 * gamma_c * V / np.sqrt(nc)
    return F, S, [sl, sr]


def grid(M, seed):
    """M energies with Im E in [0.02, 1] (every G(E) of comparable size) and complex weights of mixed signs."""
    rng = np.random.default_rng(seed)
    E = rng.uniform(-2.5, 2.5, M) + 1j * rng.uniform(0.02, 1.0, M)
    w = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    return E, w


def segment_sizes(which):
    """The segment tables of the tests: 'forty' = 40 segments of 1 - 3 energies, two of them empty (more than the 32
    ranges one table holds); 'long' = 3104 energies (97 chunks, more than the table's 96) between two short segments."""
    if which == "forty":
        rng = np.random.default_rng(40)
        sizes = [int(s) for s in rng.integers(1, 4, 40)]
        sizes[7] = sizes[31] = 0
        return sizes
    if which == "long":
        return [3, 97 * ACC_CHUNK, 2]
    raise KeyError(which)


# ------------------------------------------------------------------ float64 model of the kernels' order
def _cfma(ar, ai, w, x):
    """cfma(a, w, x) of negf_common.h without contraction: (a.x + w.x x.x) - w.y x.y, (a.y + w.x x.y) + w.y x.x"""
    ar = ar + w.real * x.real
    ar = ar - w.imag * x.imag
    ai = ai + w.real * x.imag
    ai = ai + w.imag * x.real
    return ar, ai


DEFECTS = ("drop_last_of_chunk", "weight_of_the_next", "unroll_tail_skipped", "record_twice", "record_to_neighbour",
           "one_matrix_transposed", "colof_pivrow_exchanged")


def model_segments(w, X, seg_end, batch, defect=None, perm_seed=1):
    """out [nseg][n][n] as gr_seg_core forms it, in float64 and in the kernels' order: batches of `batch` energies, every
    segment's share cut into chunks of 32, a chunk added from zero with cfma in ascending b, the chunk records added to the
    segment's slot in order.  `defect` plants one of DEFECTS into the FIRST chunk of the first non-empty segment (the
    neighbour defect: its record goes to the next slot).  The matrices are read through a row / column permutation as the
    permuted kernels do (G[i][j] = W[pivrow[i]][colof[j]]); only the exchanged-tables defect makes that visible."""
    w = np.asarray(w, dtype=np.complex128).ravel()
    m, n = w.size, X[0].shape[0]
    nseg = len(seg_end)
    out = np.zeros((nseg, n, n), dtype=np.complex128)
    rng = np.random.default_rng(perm_seed)
    hit = False                                       # the defect has been planted
    for m0 in range(0, m, batch):
        nb = min(batch, m - m0)
        for lo, hi, slot in batch_shares(seg_end, m0, nb):
            records = []
            for b0 in range(lo, hi, ACC_CHUNK):
                b1 = min(hi, b0 + ACC_CHUNK)
                plant = defect if not hit else None
                hit = True
                ar = np.zeros((n, n)); ai = np.zeros((n, n))
                stop = b1
                if plant == "drop_last_of_chunk":
                    stop = b1 - 1
                if plant == "unroll_tail_skipped":
                    stop = b0 + 4 * ((b1 - b0) // 4)
                for b in range(b0, stop):
                    g = m0 + b
                    x = np.asarray(X[g], dtype=np.complex128)
                    wb = w[g]
                    if plant == "weight_of_the_next":
                        wb = w[(g + 1) % m]
                    if plant == "one_matrix_transposed" and b == b0:
                        x = x.T
                    if plant == "colof_pivrow_exchanged" and b == b0:
                        pr, cf = rng.permutation(n), rng.permutation(n)
                        W = np.empty_like(x)
                        W[np.ix_(pr, cf)] = x            # W[pivrow[i]][colof[j]] = G[i][j]
                        x = W[np.ix_(cf, pr)]            # read as W[colof[i]][pivrow[j]]
                    ar, ai = _cfma(ar, ai, wb, x)
                rec = ar + 1j * ai
                where = slot
                if plant == "record_to_neighbour":
                    where = (slot + 1) % nseg
                records.append((where, rec))
                if plant == "record_twice":
                    records.append((where, rec))
            for where, rec in records:
                out[where] = out[where] + rec
    return out


# ------------------------------------------------------------------ float64 model of the grid-chunked sum with carry
GRID_DEFECTS = ("carry_dropped", "carry_twice", "chunk_from_sweep", "open_chunk_closed_early", "weight_from_sweep_start")


def model_grid_sum(w, X, batch, defect=None):
    """out [n][n] as negf_gless_int_probes forms its weighted sum (launch_accumulate_grid, k_elementwise.hip; the order of
    launch_bond_int), in float64: the grid is swept `batch` energies at a time, but chunk c is the energies [32 c, 32 c + 32)
    OF THE GRID, added from zero with cfma in ascending order, and out receives the chunk sums in ascending chunk order.  A
    chunk that a sweep boundary cuts waits in `carry` and the next sweep continues it.  `defect` plants one of GRID_DEFECTS
    at every place it can act:
        carry_dropped            the continued chunk starts from zero
        carry_twice              the open chunk's running sum goes to the carry AND to out
        chunk_from_sweep         chunks are counted from the sweep's first energy (launch_accumulate per sweep: no carry)
        open_chunk_closed_early  the open last chunk is added to out as if finished; the carry keeps what it held
        weight_from_sweep_start  w[m0 + b] read as w[b]"""
    w = np.asarray(w, dtype=np.complex128).ravel()
    m, n = w.size, X[0].shape[0]
    out = np.zeros((n, n), dtype=np.complex128)
    carry = np.zeros((n, n), dtype=np.complex128)
    for m0 in range(0, m, batch):
        nb = min(batch, m - m0)
        if defect == "chunk_from_sweep":
            cuts = [(b0, min(m0 + nb, b0 + ACC_CHUNK), False, False) for b0 in range(m0, m0 + nb, ACC_CHUNK)]
        else:
            cuts = []
            for c in range(m0 // ACC_CHUNK, (m0 + nb - 1) // ACC_CHUNK + 1):
                g0, g1 = max(c * ACC_CHUNK, m0), min((c + 1) * ACC_CHUNK, m0 + nb)
                continued = c * ACC_CHUNK < m0
                is_open = g1 == m0 + nb and g1 < m and g1 % ACC_CHUNK != 0
                cuts.append((g0, g1, continued, is_open))
        for g0, g1, continued, is_open in cuts:
            if continued and defect != "carry_dropped":
                ar, ai = carry.real.copy(), carry.imag.copy()
            else:
                ar = np.zeros((n, n)); ai = np.zeros((n, n))
            for g in range(g0, g1):
                wb = w[g - m0] if defect == "weight_from_sweep_start" else w[g]
                ar, ai = _cfma(ar, ai, wb, np.asarray(X[g], dtype=np.complex128))
            rec = ar + 1j * ai
            if is_open and defect == "open_chunk_closed_early":
                out = out + rec
            elif is_open:
                carry = rec
                if defect == "carry_twice":
                    out = out + rec
            else:
                out = out + rec
    return out


def sweeps_of(m, batch):
    """[(m0, nb)]: the sweeps of a grid of m energies under a workspace of `batch`."""
    return [(m0, min(batch, m - m0)) for m0 in range(0, m, batch)]
