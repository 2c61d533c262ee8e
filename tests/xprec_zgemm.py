"""Exact and extended-precision truth, case table, bars and a restatement with planted defects for the three batched
complex product kernels of k_zgemm.hip (zgemm_mfma_kernel = 1, zgemm_flex_kernel = 2, zgemm_valu_kernel = 3), called
directly through negf_zgemm_batched / Engine.zgemm.  Shared by test_zgemm_accuracy_host.py (CPU) and
test_zgemm_accuracy_gpu.py (MI355X).

Layout.  Every operand lies in a flat array as the kernels see it: leading dimensions beyond the matrix (lda = K + 3,
ldb = columns + 5, ldc = columns + 2), batch strides beyond rows * ld (+ 7), all padding of A and B NaN, C pre-filled
with the pattern C0[i] = (1000 + i) - (2000 + i) i.  An operand with stride 0 is stored once.

Operands.  A [M, K] and P = op(B) [K, N] are drawn; B is stored as P (opB bit 0 clear) or P^H (set), so one truth
A P serves every opB.  Hermitian cases (the promise of opB bit 1 must hold): P = A^H, so C = A A^H.
  Z1 "z1"      integer real and imaginary parts from +-[1, 1024], no zeros, K <= 1024: every partial sum of the 3M form
               stays below 2^33 and is exact in any order.  Truth: the int64 product.  Every kernel must match BITWISE.
  Z2 "normal"  standard normal entries;
     "graded"  the same with the rows of A and the columns of P scaled by 2^e, e in [-20, 20], and the k index of A and
               of P by 2^e, e in [-8, 8] (independently);
     "tinyim"  Im = 1e-9 Re in both operands.
               Truth: the product in np.longdouble real arithmetic on the four real parts.

Bar (Higham, ASNA 23.2.4: the magnitude matrices of the 3M error analysis), per element, u = 2^-53:
    |dRe| <= C_ZG sqrt(K + 4) u (|Ar||Pr| + |Ai||Pi|)
    |dIm| <= C_ZG sqrt(K + 4) u ((|Ar| + |Ai|)(|Pr| + |Pi|) + |Ar||Pr| + |Ai||Pi|)
and, as a ceiling, the same with gamma_{K+4} in place of C_ZG sqrt(K + 4) u (rigorous: K additions of a dot product, two
operand additions of S3, two subtractions of the recombination).  C_ZG = 4 is calibrated, not chosen: the smallest power
of two at least twice the worst ratio over the Z2 table of three float64 host implementations -- the 3M restatement in
k-steps of 4, the same in k-steps of 1, numpy's complex matmul (test_zgemm_accuracy_host.py::test_calibration; measured
worst ratios are in DESIGN 4).  Never measured on the device.
The four-product form also meets the conventional bound |dIm| <= gamma_{K+1} (|Ar||Pi| + |Ai||Pr|); 3M cannot (tinyim:
that magnitude is 2e-9 of 3M's).

Restatement.  model() is the tiled algorithm in numpy on the same flat arrays: blocks of 16 x 16 sub-tiles (4 x 4 per
block for kernel 1, balanced blocks of at most 5 x 5 for kernel 2), sub-tile validity, zero-filled K tail, op(B), the
3M recombination, the conjugate-transposed store, the Hermitian mirror, with the workgroup enumeration taken from
negf_zgemm_plan.  DEFECTS names one switch per planted defect.
"""
import functools
from collections import namedtuple

import numpy as np

from xprec import LD, U, gamma_n, pmap, require_extended

C_ZG = 4.0
KINDS_Z2 = ("normal", "graded", "tinyim")
KERNELS = (1, 2, 3)

Shape = namedtuple("Shape", "M N K nb shareA shareB why")


def _s(M, N, K, nb=1, shareA=False, shareB=False, why=""):
    return Shape(M, N, K, nb, shareA, shareB, why)


RECT = (
    _s(1, 1, 1, why="unit"), _s(16, 16, 4, why="one sub-tile, one k-step"), _s(17, 15, 3, why="around the sub-tile"),
    _s(64, 64, 16, why="one block, one K-tile"), _s(65, 63, 17, why="around the block and the K-tile"),
    _s(16, 16, 0, why="K = 0: exact zeros"),
    _s(80, 130, 33, why="ragged in every dimension"),
    _s(150, 12, 12, why="compact path, first product (stored with bit 2)"),
    _s(150, 150, 12, why="compact path, second product (bit 1)"),
    _s(12, 40, 12, why="channels"), _s(12, 12, 40, why="channels"),
    _s(20, 150, 12, why="channel states"),
)
SQUARE = tuple(_s(n, n, 40 if n == 330 else n, why="square Hermitian") for n in (64, 100, 128, 130, 150, 200, 250, 330))
BATCHED = (
    _s(100, 100, 20, nb=3, why="T = 2: P nb = 3, idle tail"), _s(100, 100, 20, nb=9, why="T = 2: P nb = 9"),
    _s(100, 100, 20, nb=8, why="T = 2: P nb = 8, no idle pair"),
    _s(150, 150, 12, nb=3, why="T = 3, the odd enumeration, batched"),
    _s(250, 250, 16, nb=4, why="T = 4: P nb = 8"), _s(250, 250, 16, nb=3, why="T = 4: P nb = 6"),
    _s(80, 130, 33, nb=3, shareA=True, why="strideA = 0"), _s(80, 130, 33, nb=3, shareB=True, why="strideB = 0"),
    _s(65, 65, 17, nb=9, shareB=True, why="nb = 9, strideB = 0"),
)
SHAPES = RECT + SQUARE + BATCHED


def opbs(shape, square_too=True):
    """opB values a shape runs: the plain, B^H and stored-transposed forms everywhere, the Hermitian promise (2, 3)
    on square shapes with operands that keep it."""
    return (0, 1, 4, 5) + ((2, 3) if square_too and shape.M == shape.N else ())


# --------------------------------------------------------------------------- #
# the plan (negf_zgemm_plan)
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def plan(M, N, K=1, opB=0, nb=1, kernel=0):
    from gaunegf_amd.engine import Engine
    return Engine.zgemm_plan(M, N, K, opB, nb, kernel)


def rule(M, N):
    """The routing rule as launch_zgemm states it: the flexible kernel where the 64 x 64 blocks' area exceeds 1.2 times
    the area of the 16-granular tiles.  Returns (kernel, block rows, block columns)."""
    t = [(d + 15) // 16 for d in (M, N)]
    b = [(d + 63) // 64 for d in (M, N)]
    if 10 * (16 * b[0] * b[1]) > 12 * (t[0] * t[1]):
        return 2, (t[0] + 4) // 5, (t[1] + 4) // 5
    return 1, b[0], b[1]


def block_ranges(kernel, dim):
    """[(first sub-tile, sub-tile count)] of the blocks of one dimension."""
    t16 = (dim + 15) // 16
    if kernel == 1:
        return [(4 * i, min(4, t16 - 4 * i)) for i in range((dim + 63) // 64)]
    nblk = (t16 + 4) // 5
    base, rem = divmod(t16, nblk)
    return [(b * base + min(b, rem), base + (1 if b < rem else 0)) for b in range(nblk)]


# --------------------------------------------------------------------------- #
# operands
# --------------------------------------------------------------------------- #
class Ops:
    """One launch's flat arrays and layout.  A [nbA, M, K], P [nbB, K, N] are the logical operands (P = op(B))."""

    def __init__(self, shape, A, P, opB):
        self.shape, self.opB, self.A, self.P = shape, opB, A, P
        M, N, K, nb = shape.M, shape.N, shape.K, shape.nb
        Bst = np.conj(np.swapaxes(P, 1, 2)) if opB & 1 else P               # as stored
        self.lda, self.ldb = K + 3, Bst.shape[2] + 5
        self.ldc = (M if opB & 4 else N) + 2
        self.c_rows = N if opB & 4 else M
        self.strideA = 0 if A.shape[0] < nb else M * self.lda + 7
        self.strideB = 0 if Bst.shape[0] < nb else Bst.shape[1] * self.ldb + 7
        self.strideC = self.c_rows * self.ldc + 7
        self.a = self._pack(A, self.lda, self.strideA)
        self.b = self._pack(Bst, self.ldb, self.strideB)
        i = np.arange(nb * self.strideC, dtype=np.float64)
        self.c0 = (1000.0 + i) - 1j * (2000.0 + i)

    @staticmethod
    def _pack(X, ld, stride):
        nbx, r, c = X.shape
        per = stride if stride else r * ld
        flat = np.full(max(nbx * per, 1), complex(np.nan, np.nan))
        for b in range(nbx):
            v = flat[b * per: b * per + r * ld].reshape(r, ld)
            v[:, :c] = X[b]
        return flat[:nbx * per] if nbx * per else flat[:0]

    def call(self, engine, kernel):
        s = self.shape
        return engine.zgemm(s.M, s.N, s.K, s.nb, self.a, self.lda, self.strideA, self.b, self.ldb, self.strideB,
                            self.opB, self.c0, self.ldc, self.strideC, kernel)

    def window_index(self):
        """Flat indices [nb, M, N] of the elements of C that hold P[b][i][j] (transposed for bit 2)."""
        s = self.shape
        b = np.arange(s.nb)[:, None, None] * self.strideC
        i, j = np.arange(s.M)[None, :, None], np.arange(s.N)[None, None, :]
        return b + (j * self.ldc + i if self.opB & 4 else i * self.ldc + j)

    def result(self, c):
        """The product [nb, M, N] a flat C holds (conjugated back for bit 2)."""
        v = c[self.window_index()]
        return np.conj(v) if self.opB & 4 else v

    def outside_unchanged(self, c):
        mask = np.ones(c.size, dtype=bool)
        mask[self.window_index().ravel()] = False
        return np.array_equal(c[mask].view(np.float64), self.c0[mask].view(np.float64))

    def expected_flat(self, prod):
        """The flat C that holds exactly `prod` [nb, M, N] in its window and C0 elsewhere."""
        c = self.c0.copy()
        c[self.window_index()] = np.conj(prod) if self.opB & 4 else prod
        return c


def _seed(shape, kind, herm):
    return [SHAPES.index(shape), (("z1",) + KINDS_Z2).index(kind), int(herm), 20261]


@functools.lru_cache(maxsize=None)
def logical(shape, kind, herm=False):
    """(A [nbA, M, K], P [nbB, K, N]) of a shape; herm: P = A^H (shared together)."""
    M, N, K, nb = shape.M, shape.N, shape.K, shape.nb
    rng = np.random.default_rng(_seed(shape, kind, herm))
    nbA = 1 if shape.shareA or (herm and shape.shareB) else nb
    nbB = nbA if herm else (1 if shape.shareB else nb)

    def draw(n, r, c, row_axis):
        if kind == "z1":
            re, im = (rng.integers(1, 1025, (n, r, c)) * rng.choice([-1, 1], (n, r, c)) for _ in range(2))
            return re.astype(np.float64) + 1j * im.astype(np.float64)
        re = rng.standard_normal((n, r, c))
        if kind == "tinyim":
            return re + 1j * (1e-9 * re)
        X = re + 1j * rng.standard_normal((n, r, c))
        if kind == "graded":
            outer = 2.0 ** rng.integers(-20, 21, r if row_axis else c)
            inner = 2.0 ** rng.integers(-8, 9, c if row_axis else r)
            X = X * (outer[:, None] * inner[None, :] if row_axis else inner[:, None] * outer[None, :])
        return X
    A = draw(nbA, M, K, True)
    P = np.conj(np.swapaxes(A, 1, 2)) if herm else draw(nbB, K, N, False)
    A.setflags(write=False); P.setflags(write=False)
    return A, P


def operands(shape, kind, opB, herm=None):
    """The Ops of a launch.  herm defaults to what opB promises after the demotion (bit 1 on a square shape, no bit 2)."""
    if herm is None:
        herm = bool(opB & 2) and shape.M == shape.N and not (opB & 4)
    A, P = logical(shape, kind, herm)
    return Ops(shape, A, P, opB)


def _bc(X, nb):
    return X if X.shape[0] == nb else np.broadcast_to(X, (nb,) + X.shape[1:])


# --------------------------------------------------------------------------- #
# truth and bars
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def truth(shape, kind, herm=False):
    """(Re, Im) [nb, M, N] of A P: int64 for Z1, np.longdouble for Z2; shared operands are multiplied once."""
    A, P = logical(shape, kind, herm)
    if kind == "z1":
        cast = lambda X: np.rint(X).astype(np.int64)
    else:
        require_extended()
        cast = lambda X: X.astype(np.longdouble)
    n = max(A.shape[0], P.shape[0])

    def one(b):
        a, p = A[b % A.shape[0]], P[b % P.shape[0]]
        ar, ai, pr, pi = cast(a.real), cast(a.imag), cast(p.real), cast(p.imag)
        return ar @ pr - ai @ pi, ar @ pi + ai @ pr
    res = pmap(one, range(n))
    re, im = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    return _bc(re, shape.nb), _bc(im, shape.nb)


@functools.lru_cache(maxsize=None)
def magnitudes(shape, kind, herm=False):
    """(mre, mim, mconv) [nb, M, N]: the 3M magnitude matrices of the real and the imaginary part and the
    conventional one of the imaginary part, |Ar||Pi| + |Ai||Pr| (float64; their own rounding is ~K u relative)."""
    A, P = logical(shape, kind, herm)
    n = max(A.shape[0], P.shape[0])
    out = []
    for b in range(n):
        a, p = A[b % A.shape[0]], P[b % P.shape[0]]
        ar, ai, pr, pi = np.abs(a.real), np.abs(a.imag), np.abs(p.real), np.abs(p.imag)
        mre = ar @ pr + ai @ pi
        out.append((mre, (ar + ai) @ (pr + pi) + mre, ar @ pi + ai @ pr))
    return tuple(_bc(np.stack([o[k] for o in out]), shape.nb) for k in range(3))


def _div(err, bound):
    """err / bound with 0 / 0 = 0 (K = 0: no error is allowed and none is made) and x / 0 = inf."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    out = np.full(err.shape, np.inf)
    np.divide(err, bound, out=out, where=bound > 0)
    out[(bound == 0) & (err == 0)] = 0.0
    out[np.isnan(err)] = np.inf
    return out


def errors(got, shape, kind, herm=False):
    """(|dRe|, |dIm|) of a product [nb, M, N] against the truth, float64 (formed in long double)."""
    tr, ti = truth(shape, kind, herm)
    got = np.asarray(got)
    return (np.abs(got.real.astype(np.longdouble) - tr).astype(np.float64),
            np.abs(got.imag.astype(np.longdouble) - ti).astype(np.float64))


def ratios(got, shape, kind, herm=False, c=C_ZG):
    """(worst error / bar, worst error / gamma_{K+4} ceiling) over both parts and all elements."""
    er, ei = errors(got, shape, kind, herm)
    mre, mim, _ = magnitudes(shape, kind, herm)
    f = c * np.sqrt(shape.K + 4.0) * U
    g = gamma_n(shape.K + 4)
    worst = lambda s: max(float(np.max(_div(er, s * mre))), float(np.max(_div(ei, s * mim))))
    return worst(f), worst(g)


def conventional_ratio(got, shape, kind, herm=False):
    """worst |dIm| / (gamma_{K+1} (|Ar||Pi| + |Ai||Pr|)): the four-product form's componentwise bound."""
    _, ei = errors(got, shape, kind, herm)
    return float(np.max(_div(ei, gamma_n(shape.K + 1) * magnitudes(shape, kind, herm)[2])))


def bitwise(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.complex128), np.ascontiguousarray(y, dtype=np.complex128)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def truth_c128(shape, kind="z1", herm=False):
    """The Z1 truth as complex128 (exact: every entry is an integer below 2^32)."""
    tr, ti = truth(shape, kind, herm)
    return tr.astype(np.float64) + 1j * ti.astype(np.float64)


# --------------------------------------------------------------------------- #
# float64 host implementations (calibration)
# --------------------------------------------------------------------------- #
def three_m(a, p, kstep):
    """The 3M form in float64, accumulated over k in steps of `kstep` (the matrix instruction takes 4)."""
    ar, ai, pr, pi = a.real, a.imag, p.real, p.imag
    as_, ps = ar + ai, pr + pi
    s1 = np.zeros((a.shape[0], p.shape[1])); s2 = s1.copy(); s3 = s1.copy()
    for k in range(0, a.shape[1], kstep):
        q = slice(k, k + kstep)
        s1 = s1 + ar[:, q] @ pr[q]; s2 = s2 + ai[:, q] @ pi[q]; s3 = s3 + as_[:, q] @ ps[q]
    return (s1 - s2) + 1j * (s3 - s1 - s2)


HOST_IMPLS = {"3M k-step 4": lambda a, p: three_m(a, p, 4), "3M k-step 1": lambda a, p: three_m(a, p, 1),
              "numpy matmul": lambda a, p: a @ p}


def host_product(shape, kind, impl, herm=False):
    A, P = logical(shape, kind, herm)
    n = max(A.shape[0], P.shape[0])
    return _bc(np.stack([impl(A[b % A.shape[0]], P[b % P.shape[0]]) for b in range(n)]), shape.nb)


def z2_table():
    """[(shape, kind, herm)] of the Z2 checks and of the calibration: every shape with every kind, the square ones
    also in their Hermitian form A A^H (Z3)."""
    out = []
    for s in SHAPES:
        for kind in KINDS_Z2:
            out.append((s, kind, False))
            if s.M == s.N:
                out.append((s, kind, True))
    return out


# --------------------------------------------------------------------------- #
# the restatement with planted defects
# --------------------------------------------------------------------------- #
DEFECTS = ("drop_k_tail", "k_tail_from_padding", "no_conj", "mirror_no_conj", "mirror_no_transpose", "edge_off_by_one",
           "store_t_ld_m", "stride0_full", "s2_sign", "skip_block", "stale_batch")
"""drop_k_tail: the last partial K-tile is dropped.  k_tail_from_padding: the K tail of A is read from the lda padding
instead of zero-filled.  no_conj: B^T for B^H.  mirror_no_conj / mirror_no_transpose: the Hermitian mirror image is
stored without conjugation / not transposed inside its 16 x 16 sub-tile.  edge_off_by_one: a sub-tile counts only when
it lies wholly inside the matrix.  store_t_ld_m: the transposed store uses the leading dimension M.  stride0_full: a
shared operand is stepped through as if every member had its own.  s2_sign: Im = S3 - S1 + S2.  skip_block: the last
block of the Hermitian enumeration is not computed.  stale_batch: the second half of the enumeration's blocks keep the
batch index of the block before them."""


def _take(flat, idx, ok):
    """flat[idx] where ok, 0 elsewhere; an index outside the array reads NaN (the model's 'somebody else's memory')."""
    inside = (idx >= 0) & (idx < flat.size)
    v = np.where(inside, flat[np.clip(idx, 0, max(flat.size - 1, 0))] if flat.size else np.nan, complex(np.nan, np.nan))
    return np.where(ok, v, 0.0)


def model(ops, kernel, defect=None, kstep=4):
    """The flat C after a launch of `kernel` (1, 2: the tiled 3M algorithm; 3: every element, four products), from the
    flat operands, the layout of `ops` and the plan.  `defect`: one of DEFECTS or None."""
    assert defect is None or defect in DEFECTS
    s = ops.shape
    M, N, K, nb = s.M, s.N, s.K, s.nb
    pl = plan(M, N, K, ops.opB, nb, kernel)
    assert pl["kernel"] == kernel
    opB = pl["opB"]
    bh, herm, store_t = bool(opB & 1), bool(opB & 2) and kernel != 3, bool(opB & 4)
    c = ops.c0.copy()
    strideA = M * ops.lda if (defect == "stride0_full" and ops.strideA == 0) else ops.strideA
    strideB = (N if bh else K) * ops.ldb if (defect == "stride0_full" and ops.strideB == 0) else ops.strideB
    ldc_t = M if defect == "store_t_ld_m" else ops.ldc
    if kernel == 3:
        rb, cb = [(0, (M + 15) // 16)], [(0, (N + 15) // 16)]
    else:
        rb, cb = block_ranges(kernel, M), block_ranges(kernel, N)
        assert (len(rb), len(cb)) == tuple(pl["blocks"])
    if herm:
        work = [tuple(int(v) for v in w) for w in pl["decode"] if w[0] >= 0]
        if defect == "skip_block":
            work = work[:-1]
        if defect == "stale_batch":
            h = len(work) // 2
            work = work[:h] + [(w[0], w[1], work[i - 1][2]) for i, w in enumerate(work) if i >= h]
    else:
        work = [(by, bx, b) for b in range(nb) for by in range(len(rb)) for bx in range(len(cb))]
    Kt = 16 * ((K + 15) // 16)
    Kuse = (K // 16) * 16 if defect == "drop_k_tail" else K
    gk = np.arange(Kt)
    for by, bx, b in work:
        (tr0, tm), (tc0, tn) = rb[by], cb[bx]
        gi, gj = 16 * tr0 + np.arange(16 * tm), 16 * tc0 + np.arange(16 * tn)
        okA = (gi[:, None] < M) & (gk[None, :] < (Kt if defect == "k_tail_from_padding" else Kuse))
        a = _take(ops.a, b * strideA + gi[:, None] * ops.lda + gk[None, :], okA)
        okB = (gk[:, None] < Kuse) & (gj[None, :] < N)
        if bh:
            p = _take(ops.b, b * strideB + gj[None, :] * ops.ldb + gk[:, None], okB)
            if defect != "no_conj":
                p = np.conj(p)
        else:
            p = _take(ops.b, b * strideB + gk[:, None] * ops.ldb + gj[None, :], okB)
        if kernel == 3:
            val = a @ p
        else:
            ar, ai, pr, pi = a.real, a.imag, p.real, p.imag
            as_, ps = ar + ai, pr + pi
            s1 = np.zeros((gi.size, gj.size)); s2 = s1.copy(); s3 = s1.copy()
            for k in range(0, Kt, kstep):
                q = slice(k, k + kstep)
                s1 = s1 + ar[:, q] @ pr[q]; s2 = s2 + ai[:, q] @ pi[q]; s3 = s3 + as_[:, q] @ ps[q]
            val = (s1 - s2) + 1j * ((s3 - s1 + s2) if defect == "s2_sign" else (s3 - s1 - s2))
            if defect == "edge_off_by_one":          # sub-tiles not wholly inside do no work: their accumulators stay 0
                val = np.where((gi[:, None] // 16 * 16 + 16 <= M) & (gj[None, :] // 16 * 16 + 16 <= N), val, 0.0)
        inside = (gi[:, None] < M) & (gj[None, :] < N)
        if not store_t:
            idx = b * ops.strideC + gi[:, None] * ops.ldc + gj[None, :]
            c[idx[inside]] = val[inside]
        if store_t or (herm and by < bx):
            img = val if (defect == "mirror_no_conj" and not store_t) else np.conj(val)
            if defect == "mirror_no_transpose" and not store_t:
                img = img.reshape(tm, 16, tn, 16).transpose(2, 1, 0, 3).reshape(16 * tn, 16 * tm)
            else:
                img = img.T
            ld = ldc_t if store_t else ops.ldc
            idx = b * ops.strideC + gj[:, None] * ld + gi[None, :]
            c[idx[inside.T]] = img[inside.T]
    return c
