// Workgroup-wide complex product and in-place Gauss-Jordan inverse on matrices in global memory: the building blocks of
// the chain kernels for n_c > 64 (k_chain1d.hip: the fixed point, k_chain1d_rd.hip: renormalisation-decimation).
#pragma once
#include "negf_common.h"

static constexpr int CH_THREADS = 256;

// Z (n x n) = X * op(Y), op = identity or conjugate transpose; all row-major ld = n
static __device__ void wg_zgemm(int n, const cplx* __restrict__ X, const cplx* __restrict__ Y, int opY,
                         cplx* __restrict__ Z)
{
    for (int t = threadIdx.x; t < n * n; t += CH_THREADS) {
        const int i = t / n, j = t - i * n;
        cplx acc = cmake(0.0, 0.0);
        if (opY == 0) {
            for (int k = 0; k < n; ++k) acc = cfma(acc, X[i * n + k], Y[k * n + j]);
        } else {
            for (int k = 0; k < n; ++k) acc = cfma(acc, X[i * n + k], cconj(Y[j * n + k]));
        }
        Z[t] = acc;
    }
}

// in-place Gauss-Jordan inverse with partial pivoting (same rule as
// k_inverse_unblocked.hip) on an n x n matrix owned by this workgroup
static __device__ void wg_gj_inverse(int n, cplx* __restrict__ A, cplx* rowk, cplx* colk, int* ipiv,
                              double* red_v, int* red_i, int* piv_row)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = 0; k < n; ++k) {
        double best = -1.0;
        int bi = n;
        for (int r = k + tid; r < n; r += CH_THREADS) {
            const double v = cabs1(A[r * n + k]);
            if (v > best) { best = v; bi = r; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_down(best, off, 64);
            const int oi = __shfl_down(bi, off, 64);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (lane == 0) { red_v[wave] = best; red_i[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            double bv = red_v[0]; int bb = red_i[0];
            for (int w = 1; w < CH_THREADS / 64; ++w)
                if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < bb)) { bv = red_v[w]; bb = red_i[w]; }
            if (bb >= n) bb = k;
            *piv_row = bb;
            ipiv[k] = bb;
        }
        __syncthreads();
        const int p = *piv_row;
        if (p != k) {
            for (int j = tid; j < n; j += CH_THREADS) {
                const cplx a = A[k * n + j], b = A[p * n + j];
                A[k * n + j] = b; A[p * n + j] = a;
            }
        }
        __syncthreads();
        const cplx ip = crecip(A[k * n + k]);
        for (int j = tid; j < n; j += CH_THREADS) {
            rowk[j] = (j == k) ? ip : cmul(A[k * n + j], ip);
            colk[j] = A[j * n + k];
        }
        __syncthreads();
        for (int t = tid; t < n * n; t += CH_THREADS) {
            const int i = t / n, j = t - i * n;
            if (i == k)      A[t] = rowk[j];
            else if (j == k) A[t] = cneg(cmul(colk[i], ip));
            else             A[t] = cfnma(A[t], colk[i], rowk[j]);
        }
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {
        const int p = ipiv[k];
        if (p != k) {
            for (int i = tid; i < n; i += CH_THREADS) {
                const cplx a = A[i * n + k], b = A[i * n + p];
                A[i * n + k] = b; A[i * n + p] = a;
            }
            __syncthreads();
        }
    }
}
