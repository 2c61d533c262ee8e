// Wide eigenchannel kernels (negf_layered_transmission_channels, negf_eigvalsh_wide_batched): the pivoted Cholesky and
// the Hermitian eigenvalues of k_channels.hip for matrices that do not fit one compute unit's LDS, K <= 512.  One
// workgroup per matrix, the matrix in a workgroup-private slice of global memory (L2-resident: 16 K^2 B <= 4 MB), the
// vectors of a step in LDS.  FP64, no atomics; every sum runs in a fixed order (per thread in index order, then the
// butterfly of wave_sum, then the waves in order), so the results are bitwise the same from run to run and do not
// depend on the batch a matrix is launched in.
//
//   pchol_wide_kernel  left-looking pivoted Cholesky, Gamma = L L^H.  Step k: the argmax of the remaining diagonal
//                      (lowest index on ties; pchol_kernel's cut at 1e-14 max diag and its stop at a non-positive
//                      diagonal), then column k from column p of Gamma and the k columns before it,
//                          l_k = (Gamma[:, p] - sum_{t<k} l_t conj(l_t[p])) / sqrt(d_p),    d -= |l_k|^2,
//                      subtracted in the order t = 0 .. k - 1 with the operation of pchol_kernel's outer-product update:
//                      element for element the same chain of roundings.  Only L^H itself is kept (row k = conj l_k,
//                      rows >= rank zero: pchol_kernel's layout); thread i reads L^H[t][i], coalesced, L^H[t][p] comes
//                      from LDS.  K^3 / 2 complex multiply-adds per matrix.
//   eig_wide_kernel    eigenvalues only.  The matrix is scaled by a power of two to a largest entry in [1/2, 1) (exact,
//                      as jacobi_kernel), stored in full, and reduced to a real tridiagonal (d, |e|) by K - 2 Householder
//                      reflections H = I - g u u^H, u = x + e^{i arg x_0} ||x|| e_0 (no cancellation; H x is a multiple
//                      of e_0 of modulus ||x||, and only |e| enters the eigenvalues, so no phase is kept):
//                          p = g B u,   w = p - (g u^H p / 2) u,   B -= u w^H + w u^H        (B the trailing block)
//                      The product reads B through its columns (p_i = sum_j conj(B[j][i]) u_j: lane i, coalesced) with
//                      the rows j dealt to the waves and the waves' partial sums added in order; the update walks rows.
//                      About 16 K^3 / 3 * 3 bytes of L2 traffic and K^3 complex multiply-adds per matrix.  Then
//                      bisection with Sturm counts on (d, e^2): one eigenvalue per lane, the Gershgorin interval widened
//                      as LAPACK's dstebz does, the pivmin safeguard of dlaebz, halving until the interval is 2^-56 of
//                      the tridiagonal's norm or stops shrinking.  Eigenvalue j of the ascending order comes from lane
//                      j: sorted output, no convergence failure mode (info 2 does not occur).
// Values only: no back-transformation.  info, rank, nout, descending, chk_in, flag_sign: launch_eigvalsh_batched's.
#include "negf_common.h"
#include <cfloat>

namespace {

constexpr int EW_THREADS = 256;
constexpr int EW_WAVES = EW_THREADS / 64;
constexpr int EW_KMAX = 512;

__device__ __forceinline__ double ew_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over the workgroup in a fixed order; every thread gets the result
__device__ __forceinline__ double ew_block_sum(double v, double* red)
{
    v = ew_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < EW_WAVES; ++k) s += red[k];
    __syncthreads();
    return s;
}

// maximum over the workgroup (any sign); every thread gets the result
__device__ __forceinline__ double ew_block_max(double v, double* red)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < EW_WAVES; ++k) s = fmax(s, red[k]);
    __syncthreads();
    return s;
}

// number of eigenvalues of the tridiagonal (d, e2 = e^2) below x
__device__ __forceinline__ int ew_sturm(int n, const double* d, const double* e2, double x, double pivmin)
{
    double q = d[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    int cnt = q < 0.0;
    for (int i = 1; i < n; ++i) {
        q = d[i] - x - e2[i - 1] / q;
        if (fabs(q) < pivmin) q = -pivmin;
        cnt += q < 0.0;
    }
    return cnt;
}

__global__ __launch_bounds__(EW_THREADS) void eig_wide_kernel(int K, const cplx* __restrict__ A, int lda, size_t strideA,
                                                              const int* __restrict__ rank, int rank_stride,
                                                              double* __restrict__ w, int ldw, int nout, int descending,
                                                              int* __restrict__ info, int chk_in, int flag_sign,
                                                              cplx* __restrict__ work, size_t strideW)
{
    __shared__ cplx u[EW_KMAX];
    __shared__ cplx pw[EW_KMAX];
    __shared__ cplx part[EW_WAVES][EW_KMAX];
    __shared__ double dg[EW_KMAX], e2[EW_KMAX];
    __shared__ double red[EW_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double* wb = w + (size_t)b * ldw;
    if (chk_in && info[b] != 0) {
        for (int i = tid; i < nout; i += EW_THREADS) wb[i] = __builtin_nan("");
        return;
    }
    const int n = rank ? min(max(rank[(size_t)b * rank_stride], 0), K) : K;
    const cplx* Ab = A + strideA * b;
    cplx* B = work + strideW * b;                  // n x n, row pitch n
    double amax = 0.0, bad = 0.0;
    for (int idx = tid; idx < n * n; idx += EW_THREADS) {
        const int i = idx / n, j = idx - i * n;
        if (i < j) continue;
        const cplx v = Ab[(size_t)i * lda + j];
        const double y = i == j ? 0.0 : v.y;
        if (!isfinite(v.x) || !isfinite(y)) bad += 1.0;
        else amax = fmax(amax, fmax(fabs(v.x), fabs(y)));
    }
    amax = ew_block_max(amax, red);
    bad = ew_block_sum(bad, red);
    int ex = 0;
    if (amax > 0.0) (void)frexp(amax, &ex);
    double f2 = 0.0;
    for (int idx = tid; idx < n * n; idx += EW_THREADS) {
        const int i = idx / n, j = idx - i * n;
        cplx v = i >= j ? Ab[(size_t)i * lda + j] : cconj(Ab[(size_t)j * lda + i]);
        if (i == j) v.y = 0.0;
        v = cmake(ldexp(v.x, -ex), ldexp(v.y, -ex));
        B[idx] = v;
        f2 += cabs2(v);
    }
    const double fro2 = ew_block_sum(f2, red);     // (its barriers also publish B)
    const int flag = (bad != 0.0 || !isfinite(fro2)) ? 1 : 0;
    if (flag) {
        for (int i = tid; i < nout; i += EW_THREADS) wb[i] = __builtin_nan("");
        if (tid == 0 && info) info[b] = flag_sign * flag;
        return;
    }
    if (amax == 0.0) {                             // the zero matrix (or rank 0): exact zeros, nothing to bisect
        for (int i = tid; i < nout; i += EW_THREADS) wb[i] = 0.0;
        if (tid == 0 && info) info[b] = 0;
        return;
    }
    for (int k = 0; k + 1 < n; ++k) {
        const int m = n - k - 1;
        const cplx* xr = B + (size_t)k * n + (k + 1);              // row k right of the diagonal: conj(x)
        cplx* T = B + (size_t)(k + 1) * n + (k + 1);               // the trailing block, pitch n
        double s = 0.0;
        for (int i = tid; i < m; i += EW_THREADS) s += cabs2(xr[i]);
        const double xn2 = ew_block_sum(s, red);
        if (tid == 0) { dg[k] = B[(size_t)k * n + k].x; e2[k] = xn2; }
        if (!(xn2 > 0.0)) continue;                                // nothing to annihilate (uniform over the workgroup)
        const double xn = sqrt(xn2);
        const cplx alpha = cconj(xr[0]);
        const double aa = sqrt(cabs2(alpha));
        const cplx ph = aa > 0.0 ? cmake(alpha.x / aa, alpha.y / aa) : cmake(1.0, 0.0);
        const double g = 1.0 / (xn * (xn + aa));
        for (int i = tid; i < m; i += EW_THREADS)
            u[i] = i == 0 ? cmake(alpha.x + ph.x * xn, alpha.y + ph.y * xn) : cconj(xr[i]);
        __syncthreads();
        // p = g B u through the columns of B: the rows j = wv, wv + 4, ... of this wave, in order
        for (int i = lane; i < m; i += 64) {
            cplx acc = cmake(0.0, 0.0);
#pragma unroll 4
            for (int j = wv; j < m; j += EW_WAVES) acc = cfma(acc, cconj(T[(size_t)j * n + i]), u[j]);
            part[wv][i] = acc;
        }
        __syncthreads();
        double up = 0.0;
        for (int i = tid; i < m; i += EW_THREADS) {
            cplx p = part[0][i];
#pragma unroll
            for (int q = 1; q < EW_WAVES; ++q) p = cadd(p, part[q][i]);
            p = cscale(p, g);
            pw[i] = p;
            up += u[i].x * p.x + u[i].y * p.y;                     // Re conj(u_i) p_i (u^H B u is real)
        }
        const double kap = 0.5 * g * ew_block_sum(up, red);
        for (int i = tid; i < m; i += EW_THREADS) pw[i] = csub(pw[i], cscale(u[i], kap));
        __syncthreads();
        for (int i = wv; i < m; i += EW_WAVES) {
            const cplx ui = u[i], wi = pw[i];
            cplx* Ti = T + (size_t)i * n;
            for (int j = lane; j < m; j += 64)
                Ti[j] = cfnma(cfnma(Ti[j], ui, cconj(pw[j])), wi, cconj(u[j]));
        }
        __syncthreads();
    }
    if (tid == 0 && n > 0) { dg[n - 1] = B[(size_t)(n - 1) * n + (n - 1)].x; e2[n - 1] = 0.0; }
    __syncthreads();
    // Gershgorin interval, widened
    double lo_l = DBL_MAX, hi_l = -DBL_MAX, em = 0.0;
    for (int i = tid; i < n; i += EW_THREADS) {
        const double el = i > 0 ? sqrt(e2[i - 1]) : 0.0, er = i + 1 < n ? sqrt(e2[i]) : 0.0;
        lo_l = fmin(lo_l, dg[i] - el - er);
        hi_l = fmax(hi_l, dg[i] + el + er);
        em = fmax(em, e2[i]);
    }
    double gl = -ew_block_max(-lo_l, red), gu = ew_block_max(hi_l, red);
    em = ew_block_max(em, red);
    const double pivmin = DBL_MIN * fmax(1.0, em);
    const double tnorm = fmax(fabs(gl), fabs(gu));
    gl -= 2.1 * tnorm * (0.5 * DBL_EPSILON) * n + 4.2 * pivmin;
    gu += 2.1 * tnorm * (0.5 * DBL_EPSILON) * n + 4.2 * pivmin;
    const double atol = ldexp(tnorm, -56);
    for (int j = tid; j < n; j += EW_THREADS) {
        double lo = gl, hi = gu;
        for (int it = 0; it < 2200; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (!(mid > lo && mid < hi)) break;                    // the interval has stopped shrinking
            if (ew_sturm(n, dg, e2, mid, pivmin) <= j) lo = mid; else hi = mid;
            if (hi - lo <= atol) break;
        }
        const int pos = descending ? n - 1 - j : j;
        if (pos < nout) wb[pos] = ldexp(0.5 * (lo + hi), ex);
    }
    for (int i = n + tid; i < nout; i += EW_THREADS) wb[i] = 0.0;
    if (tid == 0 && info) info[b] = 0;
}

__global__ __launch_bounds__(EW_THREADS) void pchol_wide_kernel(int K, const cplx* __restrict__ G, size_t strideG,
                                                                cplx* __restrict__ Lh, size_t strideL, int* __restrict__ rank)
{
    __shared__ double d[EW_KMAX];
    __shared__ cplx prow[EW_KMAX];                 // L^H[t][p], t < k: conj(l_t[p])
    __shared__ unsigned char done[EW_KMAX];
    __shared__ double bv[EW_WAVES];
    __shared__ int bs[EW_WAVES];
    __shared__ int piv_s;
    __shared__ double thr_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const cplx* Gb = G + strideG * b;
    cplx* Lb = Lh + strideL * b;
    for (int i = tid; i < K; i += EW_THREADS) { d[i] = Gb[(size_t)i * K + i].x; done[i] = 0; }
    __syncthreads();
    int k = 0;
    for (; k < K; ++k) {
        // argmax of the remaining diagonal: per thread in index order, across the lanes, then the waves in order
        double best = -1.0; int bi = K;
        for (int i = tid; i < K; i += EW_THREADS)
            if (!done[i] && (d[i] > best || bi == K)) { best = d[i]; bi = i; }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (oi < K && (bi == K || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
        }
        if ((tid & 63) == 0) { bv[tid >> 6] = best; bs[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            best = bv[0]; bi = bs[0];
            for (int q = 1; q < EW_WAVES; ++q) {
                const double ob = bv[q]; const int oi = bs[q];
                if (oi < K && (bi == K || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
            }
            if (k == 0) thr_s = 1e-14 * best;
            // stop: nothing left above the threshold (a zero or non-positive Gamma has rank 0)
            piv_s = (bi < K && best > thr_s && best > 0.0) ? bi : -1;
            if (piv_s >= 0) done[bi] = 1;
        }
        __syncthreads();
        const int p = piv_s;
        if (p < 0) break;
        for (int t = tid; t < k; t += EW_THREADS) prow[t] = Lb[(size_t)t * K + p];
        __syncthreads();
        const double sp = sqrt(d[p]), isp = 1.0 / sp;
        for (int i = tid; i < K; i += EW_THREADS) {
            cplx l = cmake(0.0, 0.0);
            if (i == p) l = cmake(sp, 0.0);
            else if (!done[i]) {
                cplx acc = Gb[(size_t)i * K + p];
#pragma unroll 4
                for (int t = 0; t < k; ++t) acc = cfnma(acc, cconj(Lb[(size_t)t * K + i]), prow[t]);
                l = cscale(acc, isp);
                d[i] -= cabs2(l);
            }
            Lb[(size_t)k * K + i] = cconj(l);
        }
        __syncthreads();                           // row k of L^H and d stand for the next step
    }
    for (size_t idx = (size_t)k * K + tid; idx < (size_t)K * K; idx += EW_THREADS) Lb[idx] = cmake(0.0, 0.0);
    if (tid == 0) rank[b] = k;
}

}  // namespace

int eig_wide_kmax() { return EW_KMAX; }

size_t eig_wide_work_elems(int K) { return (K < 1 || K > EW_KMAX) ? 0 : (size_t)K * K; }

bool launch_eigvalsh_wide(hipStream_t st, int K, int nb, const cplx* A, int lda, size_t strideA, const int* rank,
                          int rank_stride, double* w, int ldw, int nout, bool descending, int* info, bool chk_in, int flag_sign,
                          cplx* work)
{
    if (K < 1 || K > EW_KMAX || nout > ldw || !work) return false;
    if (nb <= 0) return true;
    hipLaunchKernelGGL(eig_wide_kernel, dim3(nb), dim3(EW_THREADS), 0, st, K, A, lda, strideA, rank, rank_stride, w, ldw, nout,
                       descending ? 1 : 0, info, chk_in ? 1 : 0, flag_sign, work, eig_wide_work_elems(K));
    return true;
}

bool launch_pivoted_cholesky_wide(hipStream_t st, int K, int nb, const cplx* G, size_t strideG, cplx* Lh, size_t strideL,
                                  int* rank)
{
    if (K < 1 || K > EW_KMAX) return false;
    if (nb <= 0) return true;
    hipLaunchKernelGGL(pchol_wide_kernel, dim3(nb), dim3(EW_THREADS), 0, st, K, G, strideG, Lh, strideL, rank);
    return true;
}
