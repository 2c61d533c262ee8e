// Multi-terminal transmission matrix (gfx950): all C^2 entries
//     T[a][b](E) = Re Tr[Gamma_a G Gamma_b G^H] = Re sum_{i in I_a, j in I_b} (Gamma_a G_ab Gamma_b)_ij conj(G_ab,ij),
//     G_ab = G[I_a, I_b],
// of a junction with C terminals -- the provider's contacts followed by the call's probes -- from ONE inverse per
// energy.  Gamma_a = i (Sigma_a - Sigma_a^H) lives on terminal a's orbital list I_a (K_a x K_a), so entry (a, b) costs
// K_a^2 K_b + K_a K_b^2 complex multiply-adds and all of them together K_tot sum_a K_a^2 per energy.
// The reference has no such function.
//   tmat_gamma   : Gamma blocks of a range of terminals from their Sigma blocks (per energy or once per call)
//   tmat_add     : H = F (or F + Sigma_tot) + the probes' Sigma blocks scattered on I_p x I_p, once per call
//   tmat_pair    : one workgroup per (energy, pair) for the pairs whose smaller side is a probe-sized block
//                  (min(K_a, K_b) <= 15) and whose G_ab and Gamma_a G_ab fit in LDS together (K_a K_b <= 1536):
//                  64 threads for K_a K_b <= 128, 256 above.  Pairs of two lead-sized blocks, and blocks too large for
//                  LDS, take the gather / product / trace kernels (k_elementwise.hip, k_zgemm.hip: the FP64 matrix
//                  instructions) from the orchestration code -- one sequence per such pair, of which a junction has few.
//   tmat_nan     : the matrices of singular energies (info != 0) become NaN
// No floating-point atomics.  Every sum has one order, fixed by (K_a, K_b) alone: element t = i K_b + j of the pair is
// owned by thread t mod THREADS, which adds its elements in ascending t; the k sums inside an element run in ascending
// k; the threads' sums meet in a binary tree over the thread index.  THREADS itself follows from K_a K_b.  Results are
// therefore bitwise equal from run to run, independent of the workspace batch and of which other terminals the call
// names: permuting the probes permutes rows and columns of T bit for bit.
#include "negf_common.h"
#include <algorithm>

// ------------------------------------------------------------ Gamma blocks
// terminal t of [t0, t0 + gridDim.x): dst[b * gstride[t] + goff[t] + i K + j] = i (x_ij - conj(x_ji)), x = the K x K block
// at src + b * src_stride + soff[t]
__global__ __launch_bounds__(256) void tmat_gamma_kernel(
    int t0, const int* __restrict__ tK, const int* __restrict__ soff, const int* __restrict__ goff,
    const int* __restrict__ gstride, const cplx* __restrict__ src, size_t src_stride, cplx* __restrict__ dst)
{
    const int t = t0 + blockIdx.x, b = blockIdx.y;
    const int K = tK[t];
    const cplx* x = src + (size_t)b * src_stride + soff[t];
    cplx* o = dst + (size_t)b * gstride[t] + goff[t];
    for (int e = threadIdx.x; e < K * K; e += 256) {
        const int i = e / K, j = e - i * K;
        const cplx u = x[e], v = x[j * K + i];
        o[e] = cmake(-(u.y + v.y), u.x - v.x);
    }
}

void launch_tmat_gamma(hipStream_t st, int t0, int nt, int nb, const int* tK, const int* soff, const int* goff,
                       const int* gstride, const cplx* src, size_t src_stride, cplx* dst)
{
    if (nt <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(tmat_gamma_kernel, dim3(nt, nb), dim3(256), 0, st, t0, tK, soff, goff, gstride, src, src_stride, dst);
}

// ------------------------------------------------------------ probes into H
// One workgroup; the probes one after the other in the order `order` (the host sorts them by content, so that the bits
// of H do not depend on the order in which the caller lists overlapping probes).  Inside a probe the indices are
// distinct: every element of H is touched by one thread.
__global__ __launch_bounds__(256) void tmat_add_probes_kernel(
    int n, int n_probes, const int* __restrict__ order, const int* __restrict__ tK, const int* __restrict__ ioff,
    const int* __restrict__ soff, const int* __restrict__ idx, const cplx* __restrict__ sig, cplx* __restrict__ H)
{
    for (int q = 0; q < n_probes; ++q) {
        const int t = order[q];
        const int K = tK[t];
        const int* I = idx + ioff[t];
        const cplx* s = sig + soff[t];
        for (int e = threadIdx.x; e < K * K; e += 256) {
            const int i = e / K, j = e - i * K;
            const size_t at = (size_t)I[i] * n + I[j];
            H[at] = cadd(H[at], s[e]);
        }
        __syncthreads();
    }
}

void launch_tmat_add_probes(hipStream_t st, int n, int n_probes, const int* order, const int* tK, const int* ioff,
                            const int* soff, const int* idx, const cplx* sig, cplx* H)
{
    if (n_probes <= 0) return;
    hipLaunchKernelGGL(tmat_add_probes_kernel, dim3(1), dim3(256), 0, st, n, n_probes, order, tK, ioff, soff, idx, sig, H);
}

// ------------------------------------------------------------ one pair per workgroup
// LDS: G_ab | X = Gamma_a G_ab (K_a K_b values each) | THREADS doubles of the reduction tree
template <int THREADS>
__global__ __launch_bounds__(THREADS) void tmat_pair_kernel(
    int n, int C, const int* __restrict__ pairs, const int* __restrict__ tK, const int* __restrict__ ioff,
    const int* __restrict__ goff, const int* __restrict__ gstride, const int* __restrict__ idx,
    const cplx* __restrict__ G, const cplx* __restrict__ gam, double* __restrict__ T)
{
    extern __shared__ cplx tmat_lds[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int pr = pairs[blockIdx.x];
    const int ta = pr / C, tb = pr - ta * C;
    const int Ka = tK[ta], Kb = tK[tb], ne = Ka * Kb;
    cplx* sG = tmat_lds;
    cplx* sX = sG + ne;
    double* red = reinterpret_cast<double*>(sX + ne);
    const int* Ia = idx + ioff[ta];
    const int* Ib = idx + ioff[tb];
    const cplx* Gb = G + (size_t)b * n * n;
    const cplx* Ga = gam + (size_t)b * gstride[ta] + goff[ta];
    const cplx* Gm = gam + (size_t)b * gstride[tb] + goff[tb];
    for (int t = tid; t < ne; t += THREADS) {
        const int i = t / Kb, j = t - i * Kb;
        sG[t] = Gb[(size_t)Ia[i] * n + Ib[j]];
    }
    __syncthreads();
    for (int t = tid; t < ne; t += THREADS) {
        const int i = t / Kb, j = t - i * Kb;
        cplx acc = cmake(0.0, 0.0);
        for (int k = 0; k < Ka; ++k) acc = cfma(acc, Ga[i * Ka + k], sG[k * Kb + j]);
        sX[t] = acc;
    }
    __syncthreads();
    double s = 0.0;
    for (int t = tid; t < ne; t += THREADS) {
        const int i = t / Kb, j = t - i * Kb;
        cplx acc = cmake(0.0, 0.0);
        for (int k = 0; k < Kb; ++k) acc = cfma(acc, sX[i * Kb + k], Gm[k * Kb + j]);
        const cplx g = sG[t];
        s += acc.x * g.x + acc.y * g.y;
    }
    red[tid] = s;
    __syncthreads();
#pragma unroll
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) T[((size_t)b * C + ta) * C + tb] = red[0];
}

int tmat_pair_class(int Ka, int Kb)
{
    const long ne = (long)Ka * Kb;
    if (std::min(Ka, Kb) > TMAT_SMALL_K || ne > TMAT_LDS_ELEMS) return 0;
    return ne <= TMAT_TINY_ELEMS ? 1 : 2;
}

void launch_tmat_pairs(hipStream_t st, int cls, int n, int C, int npairs, int max_elems, int nb, const int* pairs,
                       const int* tK, const int* ioff, const int* goff, const int* gstride, const int* idx, const cplx* G,
                       const cplx* gam, double* T)
{
    if (npairs <= 0 || nb <= 0) return;
    if (cls == 1) {
        const size_t lds = (size_t)2 * max_elems * sizeof(cplx) + 64 * sizeof(double);
        hipLaunchKernelGGL(tmat_pair_kernel<64>, dim3(npairs, nb), dim3(64), lds, st, n, C, pairs, tK, ioff, goff, gstride,
                           idx, G, gam, T);
    } else {
        const size_t lds = (size_t)2 * max_elems * sizeof(cplx) + 256 * sizeof(double);
        hipLaunchKernelGGL(tmat_pair_kernel<256>, dim3(npairs, nb), dim3(256), lds, st, n, C, pairs, tK, ioff, goff,
                           gstride, idx, G, gam, T);
    }
}

// ------------------------------------------------------------ singular energies
__global__ __launch_bounds__(256) void tmat_nan_kernel(int C2, const int* __restrict__ info, double* __restrict__ T)
{
    const int b = blockIdx.x;
    if (info[b] == 0) return;                              // (uniform)
    const double qnan = __builtin_nan("");
    for (int t = threadIdx.x; t < C2; t += 256) T[(size_t)b * C2 + t] = qnan;
}

void launch_tmat_nan(hipStream_t st, int C, int nb, const int* info, double* T)
{
    if (nb <= 0) return;
    hipLaunchKernelGGL(tmat_nan_kernel, dim3(nb), dim3(256), 0, st, C * C, info, T);
}
