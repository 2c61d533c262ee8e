"""
The bar of tests/accumulate_ref.py without a GPU: a float64 model of the accumulate kernels' order of operations stays
below it on the grids, segment tables and batch sizes of tests/test_accumulate_gpu.py (numpy inverses in place of the
device's G; the bound does not depend on n, so the model runs at n = 24), every planted defect of the model misses it by
orders of magnitude, and k_of counts what a brute-force walk over the chunks counts.
"""
import numpy as np
import pytest

import accumulate_ref as R

N_HOST = 24

# (name, segment sizes, batch; None = the whole grid in one batch) -- the grids of test_accumulate_gpu.py
PLAIN = [(f"M{M}", [M], None) for M in (1, 3, 4, 5, 31, 32, 33, 64, 65)]
CASES = PLAIN + [
    ("M7 in batches of 3", [7], 3),
    ("M6", [6], None),
    ("M34", [34], None),
    ("M34 in batches of 12", [34], 12),
    ("forty segments", R.segment_sizes("forty"), None),
    ("forty segments in batches of 7", R.segment_sizes("forty"), 7),
    ("97 chunks between two short segments", R.segment_sizes("long"), None),
    ("2, 0, 3", [2, 0, 3], None),
]


_G = {}


def _inputs(sizes, seed=5):
    """(w, G [m][n][n], seg_end) of a table: G(E) = (E S - F - Sigma)^-1 by numpy, shared between the tests."""
    m = int(sum(sizes))
    if m not in _G:
        F, S, sig = R.const_system(N_HOST, 100 + N_HOST)
        E, w = R.grid(m, seed)
        A = E[:, None, None] * S[None] - F[None] - (sig[0] + sig[1])[None]
        G = np.linalg.inv(A)
        G.setflags(write=False)
        _G[m] = (w, G)
    w, G = _G[m]
    return w, G, list(np.cumsum(sizes))


def _worst(out, w, G, sizes, batch):
    """worst ratio over the segments of a table, every segment against its own k"""
    ends = list(np.cumsum(sizes))
    shares = R.shares_of(ends, int(sum(sizes)), batch)
    worst, start = 0.0, 0
    for sg, end in enumerate(ends):
        if end == start:
            assert not np.any(out[sg])
            continue
        worst = max(worst, R.ratio(out[sg], w[start:end], G[start:end], R.k_of(shares[sg])))
        start = end
    return worst


def test_the_inputs_are_not_symmetric():
    """G(E) of a symmetric F, S, Sigma is complex symmetric, which would hide a transposed read: the contacts carry a
    non-symmetric block, and G differs from its transpose in the bulk of its entries."""
    w, G, _ = _inputs([5])
    d = np.abs(G[0] - G[0].T)
    assert np.median(d[np.triu_indices(N_HOST, 1)]) > 1e-6 * np.abs(G[0]).max()


def test_model_of_the_kernel_order_is_below_the_bar(capsys):
    worst = {}
    for name, sizes, batch in CASES:
        w, G, ends = _inputs(sizes)
        b = batch or int(sum(sizes))
        worst[name] = _worst(R.model_segments(w, G, ends, b), w, G, sizes, b)
    with capsys.disabled():
        print("\nACC acc model: " + "; ".join(f"{k}: {v:.3f}" for k, v in worst.items()))
        print(f"ACC acc model: worst ratio {max(worst.values()):.3f}")
    assert max(worst.values()) < 1.0, worst


def test_the_model_sums_what_numpy_sums():
    """the model is a sum at all: against numpy's einsum to a rounding-level relative Frobenius distance"""
    for name, sizes, batch in CASES[-4:]:
        w, G, ends = _inputs(sizes)
        out = R.model_segments(w, G, ends, batch or int(sum(sizes)))
        start = 0
        for sg, end in enumerate(ends):
            ref = np.einsum("b,bij->ij", w[start:end], G[start:end])
            assert np.linalg.norm(out[sg] - ref) <= 1e-13 * max(np.linalg.norm(ref), 1e-300), (name, sg)
            start = end


# the tables a defect is planted into (its first chunk has to show it): a tail of 1 behind an unroll of 4; three
# batches; a chunk of 2 in front of an empty segment; the 40-segment table
PLANT_INTO = [("M5", [5], None), ("M7 in batches of 3", [7], 3), ("2, 0, 3", [2, 0, 3], None),
              ("forty segments in batches of 7", R.segment_sizes("forty"), 7), ("M34", [34], None)]


def test_planted_defects_miss_the_bar_by_a_wide_margin(capsys):
    smallest = {}
    for defect in R.DEFECTS:
        for name, sizes, batch in PLANT_INTO:
            ends = list(np.cumsum(sizes))
            first = next(s for s in sizes if s)
            first = min(first, batch or first, R.ACC_CHUNK)               # length of the first chunk
            if defect == "record_to_neighbour" and len(sizes) == 1:
                continue
            if defect == "unroll_tail_skipped" and first % 4 == 0:
                continue
            if defect == "weight_of_the_next" and sum(sizes) == 1:
                continue
            w, G, _ = _inputs(sizes)
            b = batch or int(sum(sizes))
            out = R.model_segments(w, G, ends, b, defect=defect)
            # (a record in the neighbour's slot may land in an empty segment: the sum it was taken from shows it)
            shares = R.shares_of(ends, int(sum(sizes)), b)
            sg = next(i for i, s in enumerate(sizes) if s)
            r = R.ratio(out[sg], w[:ends[sg]][ends[sg] - sizes[sg]:], G[ends[sg] - sizes[sg]:ends[sg]], R.k_of(shares[sg]))
            smallest[defect] = min(smallest.get(defect, np.inf), r)
    assert set(smallest) == set(R.DEFECTS)
    with capsys.disabled():
        print("\nACC acc planted: " + "; ".join(f"{k}: {v:.3g}" for k, v in smallest.items()))
        print(f"ACC acc planted: smallest ratio {min(smallest.values()):.3g}")
    assert min(smallest.values()) > 1e6, smallest


def test_the_bar_sees_a_term_dropped_from_a_small_entry():
    """What the relative Frobenius bars of the older tests (1e-12 against another device call, 1e-8 against the oracle)
    cannot see: one term dropped from an entry that is 1e-9 of the matrix norm."""
    rng = np.random.default_rng(3)
    M, n = 9, 8
    X = rng.standard_normal((M, n, n)) + 1j * rng.standard_normal((M, n, n))
    X[:, 2, 5] *= 1e-9
    w = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    good = R.model_segments(w, X, [M], M)[0]
    bad = good.copy()
    bad[2, 5] -= w[4] * X[4, 2, 5]
    k = R.k_of([M])
    assert R.ratio(good, w, X, k) < 1.0
    assert np.linalg.norm(bad - good) / np.linalg.norm(good) < 1e-9            # passes a Frobenius bar of 1e-8
    assert R.ratio(bad, w, X, k) > 1e6
    assert R.ratio(np.full_like(good, np.nan), w, X, k) == np.inf


def test_the_tables_of_the_gpu_tests_leave_the_one_table_path():
    """launch_accumulate_ranges' rule restated (one_table_serves): which of the GPU tests' tables go range by range."""
    forty = R.segment_sizes("forty")
    ends = list(np.cumsum(forty))
    m = ends[-1]
    assert len(R.batch_shares(ends, 0, m)) == 38 and not R.one_table_serves(130, False, R.batch_shares(ends, 0, m))
    assert all(R.one_table_serves(300, True, R.batch_shares(ends, m0, min(7, m - m0))) for m0 in range(0, m, 7))
    long_ends = list(np.cumsum(R.segment_sizes("long")))
    shares = R.batch_shares(long_ends, 0, long_ends[-1])
    assert sum(-(-(hi - lo) // R.ACC_CHUNK) for lo, hi, _ in shares) == 99 and not R.one_table_serves(40, False, shares)
    assert R.one_table_serves(40, False, [(0, 96 * R.ACC_CHUNK, 0)]) and not R.one_table_serves(40, False, [(0, 96 * R.ACC_CHUNK + 1, 0)])
    assert R.one_table_serves(2048, True, [(0, 2, 0), (2, 5, 2)]) and not R.one_table_serves(2049, True, [(0, 2, 0), (2, 5, 2)])
    assert R.one_table_serves(2049, False, [(0, 2, 0), (2, 5, 2)])


def test_k_of_equals_a_brute_force_count():
    """k_of against a walk over the batches, shares and chunks that counts, for the first product of the longest chunk, one
    rounding for the product, two additions per matrix of its chunk, one addition per chunk record of the segment, plus
    one (the bar's slack)."""
    rng = np.random.default_rng(11)
    for trial in range(200):
        nseg = int(rng.integers(1, 45))
        sizes = [int(s) for s in rng.integers(0, rng.choice([4, 40, 200]), nseg)]
        m = int(sum(sizes))
        if m == 0:
            continue
        batch = int(rng.choice([1, 3, 7, 31, 32, 33, 64, 100, m]))
        ends = list(np.cumsum(sizes))
        shares = R.shares_of(ends, m, batch)
        # brute force: label every energy with (segment, batch), cut runs of equal labels into chunks of 32
        seg_of = np.repeat(np.arange(nseg), sizes)
        chunks = {sg: [] for sg in range(nseg)}
        for m0 in range(0, m, batch):
            b = m0
            while b < min(m, m0 + batch):
                e = b
                while e < min(m, m0 + batch) and seg_of[e] == seg_of[b] and e - b < R.ACC_CHUNK:
                    e += 1
                chunks[int(seg_of[b])].append(e - b)
                b = e
        for sg in range(nseg):
            if sizes[sg] == 0:
                assert R.k_of(shares[sg]) == 0 and not chunks[sg]
                continue
            assert sum(chunks[sg]) == sizes[sg] == sum(shares[sg])
            want = 1 + 2 * max(chunks[sg]) + len(chunks[sg]) + 1
            assert R.k_of(shares[sg]) == want, (sizes, batch, sg)
