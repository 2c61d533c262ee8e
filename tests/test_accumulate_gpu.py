"""
The reduction behind GrInt, GrIntSegments and gr_int_refine on the GPU (gaunegf_amd/csrc/k_elementwise.hip:
accumulate_partial_kernel, accumulate_perm_rows_kernel, accumulate_perm_partial_kernel, accumulate_final_kernel,
accumulate_final_seg_kernel; the host rules launch_accumulate_ranges, launch_accumulate_perm and gr_seg_core), entry by
entry against the extended-precision sum and the derived bar of tests/accumulate_ref.py.

The operands of the truth are the device's own G(E) (Engine.gr_batch under the same negf_set_batch), so the inverse is not
part of what is measured; a bridge test shows that a weighted sum reads the numbers gr_batch hands out, bit for bit, where
it reads the windowed inverse through its pivot bookkeeping instead of the gathered G.  Every case prints an `ACC acc`
line: n, the grid, the form the host rules take, the worst error / bar.
"""
import warnings

import numpy as np
import pytest

import accumulate_ref as R
from helpers import rel_fro

pytestmark = pytest.mark.gpu
TOL = 1e-8                                            # test_small_fused_gpu.TOL


class _System:
    """const_system(n) resident on the engine with its constant provider; `batch`: negf_set_batch for the block."""

    def __init__(self, engine, n, batch=0, small_algo=0):
        self.engine, self.n, self.batch, self.small_algo = engine, n, batch, small_algo

    def __enter__(self):
        F, S, sig = R.const_system(self.n, 500 + self.n)
        if self.batch:
            # a system of another size drops the workspace, so the next one is built to the limit whatever stood before
            # (a workspace above the limit is rebuilt by the library itself; one below it but above the grid is kept);
            # swept() holds the call to it.
            self.engine.set_system(np.eye(2), np.eye(2))
        self.engine.set_system(F, S)
        self.h = self.engine.sigma_const(sig)
        self.engine.set_batch(self.batch)
        self.engine.set_small_algo(self.small_algo)
        return self

    def __exit__(self, *exc):
        self.engine.set_batch(0)
        self.engine.set_small_algo(0)
        self.engine.sigma_free(self.h)

    def swept(self, m):
        """energies per sweep of the workspace in the call just made over m energies"""
        b = self.engine.get_batch()
        if self.batch:
            assert min(b, m) == min(self.batch, m), (b, self.batch, m)   # the limit is in force, not a larger workspace in place
        return min(b, m)


def _Engine():
    from gaunegf_amd.engine import Engine
    return Engine


def _form(n, M, batch):
    """(inverse plan of one sweep, the kernels its weighted sum takes)"""
    plan = _Engine().inverse_plan(n, min(M, batch), defer=True)
    return plan, ("plain" if not plan["deferred"] else "rows" if n <= R.APR_MAXN else "elements")


def _one_sum(engine, n, M, batch, form, cls=None, rows=None):
    """gr_int over the grid (M, seed n + M) against the truth formed from gr_batch's G under the same batch; returns the
    worst ratio after printing the case's line and checking the form the inverse plan promises"""
    E, w = R.grid(M, 1000 * n + M)
    with _System(engine, n, batch) as s:
        X = engine.gr_batch(s.h, E)
        b0 = s.swept(M)
        got = engine.gr_int(s.h, E, w)
        b = s.swept(M)
    assert b == b0
    plan, taken = _form(n, M, b)
    assert taken == form, (n, M, b, plan)
    if cls is not None:
        assert plan["cls"] == cls, plan
    k = R.k_of(R.shares_of([M], M, b)[0])
    r = R.ratio(got, w, X, k, rows=rows)
    print(f"ACC acc n={n} M={M} batch={b} form={taken} class={plan['cls']} k={k}"
          f"{'' if rows is None else f' rows={len(rows)}'}: worst ratio {r:.3f}")
    return r


# ------------------------------------------------------------------ bridge
@pytest.mark.parametrize("n,nb,ps,form", [(300, 7, (0, 3, 6), "rows"), (2049, 3, (0, 2), "elements")])
def test_one_hot_weight_returns_the_matrix_gr_batch_returns(engine, n, nb, ps, form):
    """A sum of exact zeros and 1 * x is exact: gr_int with a one-hot weight at p IS gr_batch(...)[p], bit for bit, also
    where the sum reads the windowed inverse through (pivrow, colof) and gr_batch reads the gathered G."""
    plan, taken = _form(n, nb, nb)
    assert plan["deferred"] and taken == form
    E, _ = R.grid(nb, 1000 * n + nb)
    with _System(engine, n, nb) as s:
        X = engine.gr_batch(s.h, E)
        assert s.swept(nb) == nb
        for p in ps:
            w = np.zeros(nb, dtype=np.complex128)
            w[p] = 1.0
            got = engine.gr_int(s.h, E, w)
            assert np.all(np.isfinite(X[p].view(np.float64)))
            assert np.array_equal(got, X[p]), (n, p, np.abs(got - X[p]).max())
    print(f"ACC acc n={n} nb={nb} form={taken}: one-hot sums at {ps} equal gr_batch bitwise")


# ------------------------------------------------------------------ one sum
@pytest.mark.parametrize("M,batch", [(1, 0), (3, 0), (4, 0), (5, 0), (31, 0), (32, 0), (33, 0), (64, 0), (65, 0), (7, 3)])
def test_plain_form(engine, M, batch):
    """launch_accumulate on the gathered G (n = 130: n^2 = 16900 is no multiple of the 256 threads): the unroll of four
    and its tails, one chunk, chunk edges, three chunks; acc carried over three workspace batches."""
    assert _one_sum(engine, 130, M, batch, "plain") <= 1.0


@pytest.mark.parametrize("n,M,cls", [(257, 33, None), (1030, 5, None), (2048, 5, (8, 4))])
def test_row_form(engine, n, M, cls):
    """accumulate_perm_rows_kernel: two of the eight column slots per thread live and two chunks (n = 257), a last slot
    cut by n (1030), every slot live with the 64 KiB of LDS the form may ask for (2048, the (8, 4) class)."""
    assert _one_sum(engine, n, M, 0, "rows", cls) <= 1.0


@pytest.mark.parametrize("M,batch", [(6, 0), (7, 3), (34, 0)])
def test_element_form(engine, M, batch):
    """accumulate_perm_partial_kernel (n > 2048): the unroll and a tail of two, acc over three batches, a full chunk and
    a chunk of two (M = 34: 2.2 GB of G; 64 seeded rows, the first and the last are compared)."""
    n, rows = 2049, None
    if M == 34:
        rng = np.random.default_rng(34)
        rows = np.unique(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), 64, replace=False)]))
    assert _one_sum(engine, n, M, batch, "elements", (4, 8), rows) <= 1.0


# ------------------------------------------------------------------ segment tables
def _segments(engine, n, sizes, batch=0, small_algo=0, seed=0):
    """gr_int_seg over a table against the truth per segment; returns (worst ratio, forms taken per batch)"""
    m = int(sum(sizes))
    E, w = R.grid(m, 1000 * n + m + seed)
    ends = list(np.cumsum(sizes))
    segs = [(E[e - k:e], w[e - k:e]) for k, e in zip(sizes, ends)]
    with _System(engine, n, batch, small_algo) as s:
        X = engine.gr_batch(s.h, E)
        b0 = s.swept(m)
        got = engine.gr_int_seg(s.h, segs)
        b = s.swept(m)
    assert b == b0 and len(got) == len(sizes)
    plan = _Engine().inverse_plan(n, b, defer=True)
    perm = plan["deferred"]
    forms = [R.one_table_serves(n, perm, R.batch_shares(ends, m0, min(b, m - m0))) for m0 in range(0, m, b)]
    shares = R.shares_of(ends, m, b)
    worst = 0.0
    for sg, (k, e) in enumerate(zip(sizes, ends)):
        if k == 0:
            assert not np.any(got[sg].view(np.float64)), sg           # an empty segment: exact zeros
            continue
        worst = max(worst, R.ratio(got[sg], w[e - k:e], X[e - k:e], R.k_of(shares[sg])))
    taken = "+".join(sorted({"table" if f else "range by range" for f in forms}))
    print(f"ACC acc n={n} segments={len(sizes)} m={m} batch={b} ({len(forms)} sweeps) "
          f"{'permuted' if perm else 'plain'} form={taken}: worst ratio {worst:.3f}")
    return worst, forms, perm


@pytest.mark.parametrize("n", [130, 300])
def test_more_ranges_than_the_table_holds(engine, n):
    """40 segments of 1 - 3 energies, two of them empty, in one sweep: 38 ranges against ACC_TAB_SEGS = 32, so
    gr_seg_core launches range by range (the plain kernels at n = 130, the row form at n = 300)."""
    worst, forms, perm = _segments(engine, n, R.segment_sizes("forty"))
    assert forms == [False] and perm == (n == 300)
    assert worst <= 1.0


def test_more_chunks_than_the_table_holds(engine):
    """One segment of 3104 energies between two short ones: 1 + 97 + 1 chunks against ACC_TAB_CHUNKS = 96 (n = 40 through
    the kernel sequence)."""
    worst, forms, perm = _segments(engine, 40, R.segment_sizes("long"), small_algo=1)
    assert forms == [False] and not perm
    assert worst <= 1.0


def test_segments_on_the_element_form(engine):
    """Segments of 2, 0 and 3 energies at n = 2049: the permuted read above the row form's n goes range by range."""
    worst, forms, perm = _segments(engine, 2049, [2, 0, 3])
    assert forms == [False] and perm
    assert worst <= 1.0


def test_segments_straddling_workspace_batches(engine):
    """The 40-segment table at n = 300 swept seven energies at a time (every sweep's ranges fit one table; segments
    cut by a sweep's edge continue in their slot), and twice that table swept 70 at a time: more than 32 ranges in a
    sweep AND segments cut by its edge."""
    forty = R.segment_sizes("forty")
    worst, forms, perm = _segments(engine, 300, forty, batch=7)
    assert perm and all(forms) and len(forms) > 5
    assert worst <= 1.0
    worst, forms, perm = _segments(engine, 300, forty + forty, batch=70, seed=1)
    assert perm and len(forms) > 1 and not forms[0]
    assert worst <= 1.0


def test_default_small_path_hands_a_long_grid_to_the_kernel_sequence(engine):
    """n = 12 in the default small mode, segments of 4000 and 100 energies: above 4096 energies the fused path of
    gr_seg_core hands over to the kernel sequence.  Every segment against gr_int on that segment alone (the fused kernel:
    another inverse, another order) at the 1e-12 relative Frobenius bar of test_small_fused_gpu.py."""
    n, sizes = 12, [4000, 100]
    E, w = R.grid(sum(sizes), 12)
    segs = [(E[:4000], w[:4000]), (E[4000:], w[4000:])]
    with _System(engine, n) as s:
        got = engine.gr_int_seg(s.h, segs)
        for a, (e, ww) in zip(got, segs):
            d = rel_fro(a, engine.gr_int(s.h, e, ww))
            print(f"ACC acc n={n} segment of {e.size} in a grid of {E.size}: kernel sequence against the fused path {d:.2e}")
            assert d < 1e-12


# ------------------------------------------------------------------ a dead matrix in the element form
def test_dead_matrix_in_the_element_form(engine):
    """F = S = 1, Sigma = 0 at n = 2049: E = 1 gives the zero matrix.  Its NaN reaches every entry of the sum it is in (the
    element form substitutes NaN for a matrix whose bookkeeping is not an index) and no other sum."""
    n = 2049
    I = np.eye(n)
    E = np.array([0.5 + 0.1j, 1.0 + 0j, 2.0 + 0.1j])
    one = np.ones(1, dtype=np.complex128)
    assert _Engine().inverse_plan(n, 3, defer=True)["deferred"]
    engine.set_system(I, I)
    h = engine.sigma_precomputed(np.zeros((3, n, n), dtype=np.complex128))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out = engine.gr_int(h, E, np.ones(3))
            info = np.array(engine.last_info)
            segs = engine.gr_int_seg(h, [(E[k:k + 1], one) for k in range(3)])
            info_seg = np.array(engine.last_info)
    finally:
        engine.sigma_free(h)
    assert np.all(np.isnan(out.real)) and np.all(np.isnan(out.imag))
    assert list(np.nonzero(info)[0]) == [1] and list(np.nonzero(info_seg)[0]) == [1]
    assert np.all(np.isnan(segs[1].real)) and np.all(np.isnan(segs[1].imag))
    for k in (0, 2):
        assert rel_fro(segs[k], I / (E[k] - 1)) < TOL, k


# ------------------------------------------------------------------ refinement with a NaN level
@pytest.mark.parametrize("n", [24, 730])         # refine_levels_kernel (one workgroup per integral); refine_wide_kernel (a launch per level)
def test_refinement_never_converges_on_a_nan(engine, n):
    """The NaN rule of negf_gr_int_refine: a NaN anywhere in a level makes its maxDP NaN (numpy's max), which is below no
    tolerance -- the integration does not converge, whatever is asked, and hands back NaN; a second integral in the same
    call is not touched by it and converges at the level and to the bits the host refinement of its level sums gives."""
    from helpers import random_system
    _, S = random_system(n, 60 + n)
    engine.set_system(S, S)                                              # E = 1: E S - F is the zero matrix
    h = engine.sigma_const([np.zeros((n, n), dtype=np.complex128)])
    rng = np.random.default_rng(n)
    counts = [2, 3, 2]
    Ebad = np.array([0.5 + 0.1j, 2.0 + 0.1j, 1.0 + 0j, 3.0 + 0.2j, -1.0 + 0.3j, 0.2 + 0.5j, 1.5 + 0.4j])
    Eok = rng.uniform(-2, 3, 7) + 1j * rng.uniform(0.05, 0.5, 7)
    wbad = rng.standard_normal(7) + 1j * rng.standard_normal(7)
    wok = rng.standard_normal(7) + 1j * rng.standard_normal(7)
    ratios = [None, 0.5, 0.25]
    ends = np.cumsum(counts)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            sums = engine.gr_int_seg(h, [(E[e - c:e], w[e - c:e]) for E, w in ((Ebad, wbad), (Eok, wok)) for c, e in zip(counts, ends)])
            assert all(np.all(np.isfinite(a.view(np.float64))) for a in sums[3:]) and np.all(np.isnan(sums[1].real))
            for tol in (1e-30, 1e-3, 1e30):
                P, conv, dps = sums[3].copy(), -1, [np.nan]
                for j in (1, 2):
                    new_P = P * ratios[j]
                    new_P += sums[3 + j]
                    dps.append(np.max(np.abs(new_P - P)))
                    P = new_P
                    if dps[-1] < tol:
                        conv = j
                        break
                got = engine.gr_int_refine(h, [(Ebad, wbad, counts, ratios, None), (Eok, wok, counts, ratios, None)], tol)
                assert list(np.nonzero(engine.last_info)[0]) == [2]
                Pb, convb, dpb = got[0]
                assert convb == -1 and np.all(np.isnan(dpb)), (tol, convb, dpb)
                assert np.all(np.isnan(Pb.real)) and np.all(np.isnan(Pb.imag))
                Pd, convd, dpd = got[1]
                assert convd == conv and np.array_equal(Pd, P), (tol, convd, conv)
                assert np.isnan(dpd[0]) and np.allclose(dpd[1:len(dps)], dps[1:], rtol=1e-14, atol=0) and np.all(np.isnan(dpd[len(dps):]))
            assert conv == 1                                             # (the last tolerance: 1e30 stops the clean integral at once)
    finally:
        engine.sigma_free(h)
