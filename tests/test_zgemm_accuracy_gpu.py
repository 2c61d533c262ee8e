"""The three product kernels of k_zgemm.hip on the GPU, called directly (Engine.zgemm -> negf_zgemm_batched) on the
operands, truths and bars of tests/xprec_zgemm.py: kernel 1 = zgemm_mfma_kernel (64 x 64 blocks), 2 = zgemm_flex_kernel
(balanced blocks), 3 = zgemm_valu_kernel (four products on the vector unit), 0 = the production rule.

  * Z1 (integer operands): every kernel, every opB and store mode returns the int64 product exactly; in the same
    calls nothing outside the M x N (bit 2: N x M) window of C changes and the NaN padding of A and B never enters;
  * Z2 / Z3: kernels 1 and 2 (and 3) stay within the per-element bars and the gamma_{K+4} ceiling; kernel 3 also meets
    the four-product bound on the tiny-imaginary case, where the 3M kernels' ratio is reported, not asserted;
  * kernel 0 returns bitwise what the kernel named by negf_zgemm_plan returns; kernels 1 and 2 agree bitwise wherever
    both compute an element directly (everywhere without the Hermitian promise, the upper triangle with it);
  * Hermitian launches: blocks above the diagonal and diagonal blocks are bitwise those of the full product, the mirror
    images are their exact conjugate transposes, kernel 3 ignores the promise;
  * batches: every member of a batch is bitwise its own single launch, a shared operand behaves as nb copies, a NaN /
    Inf in one member's operand stays in its row / column of that member;
  * power-of-two scaling commutes bitwise; the Hermitian bit is dropped where negf_zgemm_plan says; K = 0 gives zeros;
    invalid arguments are refused.
Each line 'ACC zgemm ...' reports the worst ratio error / bar of one kernel and case family.
"""
import functools

import numpy as np
import pytest

import xprec_zgemm as xz
from gaunegf_amd import _lib

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=48)
def _ops(shape, kind, opB, herm=None):
    return xz.operands(shape, kind, opB, herm)


@functools.lru_cache(maxsize=256)
def _run(kernel, shape, kind, opB, herm=None):
    """The product [nb, M, N] of one launch (cached: several tests compare the same launches)."""
    from gaunegf_amd.engine import get_engine
    ops = _ops(shape, kind, opB, herm)
    c = ops.call(get_engine(), kernel)
    assert ops.outside_unchanged(c), (kernel, shape, kind, opB)
    return ops.result(c)


def _shape(M, N, K, nb=1, **kw):
    return next(s for s in xz.SHAPES if (s.M, s.N, s.K, s.nb) == (M, N, K, nb)
                and all(getattr(s, k) == v for k, v in kw.items()))


# --------------------------------------------------------------------------- #
# Z1: exact
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("kernel", xz.KERNELS)
def test_z1_is_exact_and_nothing_else_is_written(engine, kernel):
    n = 0
    for s in xz.SHAPES:
        for opB in xz.opbs(s):
            ops = xz.operands(s, "z1", opB)
            c = ops.call(engine, kernel)
            where = (kernel, s, opB)
            assert ops.outside_unchanged(c), where
            got = ops.result(c)
            assert np.all(np.isfinite(got.view(np.float64))), where
            assert np.array_equal(got, xz.truth_c128(s, "z1", bool(opB & 2))), where
            n += 1
    print(f"ACC zgemm kernel {kernel} Z1: {n} launches exact")


@pytest.mark.parametrize("kernel", (0,) + xz.KERNELS)
def test_k0_gives_zeros(engine, kernel):
    s = _shape(16, 16, 0)
    for opB in range(8):
        got = _run(kernel, s, "z1", opB, False)
        assert got.shape == (1, 16, 16) and not np.any(got), (kernel, opB)


# --------------------------------------------------------------------------- #
# Z2 / Z3: the bars
# --------------------------------------------------------------------------- #
def _z2_opbs(kind, herm):
    if herm:
        return (3, 2) if kind == "normal" else (3,)
    return (0, 1, 4, 5) if kind == "normal" else (0, 5)


@pytest.mark.parametrize("kernel", xz.KERNELS)
def test_z2_within_the_bars(engine, kernel):
    worst = {}
    for s, kind, herm in xz.z2_table():
        for opB in (_z2_opbs(kind, herm) if kernel != 3 else ((3,) if herm else (1,))):
            r, g = xz.ratios(_run(kernel, s, kind, opB, herm), s, kind, herm)
            fam = f"{'Z3' if herm else 'Z2'} {kind}"
            worst[fam] = max(worst.get(fam, 0.0), r)
            assert r <= 1.0 and g <= 1.0, (kernel, s, kind, herm, opB, r, g)
    for fam, r in worst.items():
        print(f"ACC zgemm kernel {kernel} {fam}: worst ratio {r:.3g} (C_ZG = {xz.C_ZG:g})")


def test_conventional_bound_on_tiny_imaginary_parts(engine):
    """The four-product kernel meets gamma_{K+1} (|Ar||Pi| + |Ai||Pr|) per element; the 3M kernels cannot (a property
    of the product path, reported here and recorded in DESIGN 4)."""
    worst = {k: 0.0 for k in xz.KERNELS}
    for s in xz.SHAPES:
        if s.K == 0:
            continue
        for k in xz.KERNELS:
            worst[k] = max(worst[k], xz.conventional_ratio(_run(k, s, "tinyim", 1 if k == 3 else 0, False), s, "tinyim"))
    for k in xz.KERNELS:
        print(f"ACC zgemm kernel {k} tinyim against the four-product bound: worst ratio {worst[k]:.3g}")
    assert worst[3] <= 1.0


# --------------------------------------------------------------------------- #
# kernels against each other
# --------------------------------------------------------------------------- #
def test_rule_runs_the_planned_kernel(engine):
    seen = set()
    for s in xz.SHAPES:
        for opB in (1, 3) if s.M == s.N else (1, 4):
            herm = opB == 3
            k = xz.plan(s.M, s.N, s.K, opB, s.nb)["kernel"]
            seen.add(k)
            assert xz.bitwise(_run(0, s, "normal", opB, herm), _run(k, s, "normal", opB, herm)), (s, opB, k)
    assert seen == {1, 2}


def test_mfma_and_flex_agree_bitwise(engine):
    """Each element's three accumulators see the same matrix instructions in the same k order in both kernels.  Under
    the Hermitian promise that holds for the elements both compute directly, i <= j: below the diagonal one kernel's
    diagonal block computes S3(i, j) where the other mirrors S3(j, i), and the 3M imaginary part is not bitwise
    antisymmetric (LAB_NOTES)."""
    for s, kind, herm in xz.z2_table():
        for opB in _z2_opbs(kind, herm):
            a, b = _run(1, s, kind, opB, herm), _run(2, s, kind, opB, herm)
            if herm:
                iu = np.triu_indices(s.M)
                a, b = a[:, iu[0], iu[1]], b[:, iu[0], iu[1]]
            assert xz.bitwise(a, b), (s, kind, opB)


@pytest.mark.parametrize("kernel", (1, 2))
def test_hermitian_blocks(engine, kernel):
    """opB = 3 on B = A against the full product opB = 1 of the same operands."""
    for s in xz.SHAPES:
        if s.M != s.N:
            continue
        H, F = _run(kernel, s, "normal", 3, True), _run(kernel, s, "normal", 1, True)
        blocks = xz.block_ranges(kernel, s.N)
        for by, (r0, rn) in enumerate(blocks):
            for bx, (c0, cn) in enumerate(blocks):
                if by > bx:
                    continue
                rs, cs = slice(16 * r0, 16 * (r0 + rn)), slice(16 * c0, 16 * (c0 + cn))
                assert xz.bitwise(H[:, rs, cs], F[:, rs, cs]), (kernel, s, by, bx)
                if by < bx:
                    assert xz.bitwise(H[:, cs, rs], np.conj(np.swapaxes(H[:, rs, cs], 1, 2))), (kernel, s, by, bx)
    for s in xz.SQUARE[:4]:
        assert xz.bitwise(_run(3, s, "normal", 3, True), _run(3, s, "normal", 1, True)), s


def test_hermitian_bit_is_dropped_as_planned(engine):
    """A promise that cannot be used (M != N, or with bit 2) is dropped: operands that BREAK the promise give the plain
    product, bitwise that of the launch without the bit."""
    rect, sq = _shape(80, 130, 33), _shape(100, 100, 100)
    for k in (1, 2):
        for s, opB in ((rect, 2), (rect, 3), (sq, 6), (sq, 7)):
            assert xz.plan(s.M, s.N, s.K, opB, 1, k)["opB"] == opB & ~2
            assert xz.bitwise(_run(k, s, "normal", opB, False), _run(k, s, "normal", opB & ~2, False)), (k, s, opB)
        assert xz.plan(100, 100, 100, 3, 1, k)["opB"] == 3


# --------------------------------------------------------------------------- #
# batches
# --------------------------------------------------------------------------- #
def _single(s, kind, herm, b):
    """Member b of a batched case as a launch of its own: (Shape with nb = 1, A [1, M, K], P [1, K, N])."""
    A, P = xz.logical(s, kind, herm)
    return s._replace(nb=1, shareA=False, shareB=False), A[b % A.shape[0]][None], P[b % P.shape[0]][None]


@pytest.mark.parametrize("kernel", xz.KERNELS)
def test_batch_members_are_their_single_launches(engine, kernel):
    for s in xz.BATCHED:
        for opB in (1, 3) if s.M == s.N else (0, 5):
            herm = opB == 3
            got = _run(kernel, s, "normal", opB, herm)
            for b in range(s.nb):
                s1, A, P = _single(s, "normal", herm, b)
                ops = xz.Ops(s1, A, P, opB)
                one = ops.result(ops.call(engine, kernel))
                assert xz.bitwise(got[b], one[0]), (kernel, s, opB, b)


@pytest.mark.parametrize("kernel", xz.KERNELS)
def test_shared_operand_is_nb_copies(engine, kernel):
    for s in (x for x in xz.BATCHED if x.shareA or x.shareB):
        for opB in (0, 5):
            A, P = xz.logical(s, "normal", False)
            full = xz.Ops(s, np.broadcast_to(A, (s.nb,) + A.shape[1:]), np.broadcast_to(P, (s.nb,) + P.shape[1:]), opB)
            assert full.strideA > 0 and full.strideB > 0
            shared = _ops(s, "normal", opB, False)
            assert (shared.strideA == 0) == s.shareA and (shared.strideB == 0) == s.shareB
            assert xz.bitwise(_run(kernel, s, "normal", opB, False), full.result(full.call(engine, kernel))), (kernel, s, opB)


@pytest.mark.parametrize("kernel", xz.KERNELS)
def test_nonfinite_entries_stay_in_their_row_column_and_member(engine, kernel):
    s = _shape(100, 100, 20, 9)
    hit, row, col = 4, 71, 11
    A, P = (np.array(x) for x in xz.logical(s, "normal", False))
    A[hit, row, 3] = complex(np.nan, 1.0)
    P[hit, 5, col] = complex(np.inf, 1.0)
    for opB in (0, 1, 4):
        clean = _run(kernel, s, "normal", opB, False)
        ops = xz.Ops(s, A, P, opB)
        c = ops.call(engine, kernel)
        assert ops.outside_unchanged(c)
        got = ops.result(c)
        keep = np.ones(got.shape, dtype=bool)
        keep[hit, row, :] = False
        keep[hit, :, col] = False
        assert xz.bitwise(got[keep], clean[keep]), (kernel, opB)
        bad = ~(np.isfinite(got.real) & np.isfinite(got.imag))
        assert np.all(bad[~keep]), (kernel, opB)


@pytest.mark.parametrize("kernel", (1, 2))
def test_power_of_two_scaling_commutes(engine, kernel):
    for s, kind, opB, herm in ((_shape(80, 130, 33), "normal", 0, False), (_shape(80, 130, 33), "graded", 5, False),
                               (_shape(150, 150, 150), "normal", 1, False), (_shape(130, 130, 130), "graded", 4, False)):
        A, P = xz.logical(s, kind, herm)
        ops = xz.Ops(s, A * 2.0 ** 40, P * 2.0 ** -13, opB)
        got = ops.result(ops.call(engine, kernel))
        assert xz.bitwise(got, _run(kernel, s, kind, opB, herm) * 2.0 ** 27), (kernel, s, kind, opB)


# --------------------------------------------------------------------------- #
# the entry point
# --------------------------------------------------------------------------- #
def test_invalid_arguments_are_refused(engine):
    a = np.zeros(64, dtype=np.complex128)
    p = a.ctypes.data

    def rc(M=4, N=4, K=4, nb=1, A=p, lda=4, sA=16, B=p, ldb=4, sB=16, opB=0, C=p, ldc=4, sC=16, kernel=0):
        return engine._lib.negf_zgemm_batched(engine._ctx, M, N, K, nb, A, lda, sA, B, ldb, sB, opB, C, ldc, sC, kernel)
    assert rc() == _lib.NEGF_OK
    for bad in (dict(M=0), dict(N=0), dict(K=-1), dict(nb=0), dict(A=None), dict(B=None), dict(C=None), dict(lda=3),
                dict(ldb=3), dict(ldc=3), dict(sA=15), dict(sB=15), dict(sC=15), dict(sC=0), dict(opB=8), dict(opB=-1),
                dict(kernel=4), dict(kernel=-1), dict(M=8, opB=4, ldc=4, sC=64)):
        assert rc(**bad) == _lib.NEGF_EINVAL, bad
    assert rc(nb=3, sA=0, sB=0) == _lib.NEGF_OK
