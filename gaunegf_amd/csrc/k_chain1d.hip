// 1-D chain contact self-energy ("decimation") -- gauNEGF/surfG1D.py:223-295 (g),
// :344-373 (sigma).  One workgroup per (energy, contact): the fixed point is a
// strictly sequential chain of small dense operations, so parallelism comes from
// the energy grid (M x n_contacts independent workgroups) and from the nc x nc
// elements inside one step.
//
//   A = (E + i eta) Sa - a ;  B = (E + i eta) Sb - b ;  B^H = conj(B)^T   (:260-262)
//   g0 = inv(A)                                                          (:287)
//   repeat: g_new = inv(A - B g B^H)                                     (:275)
//           diff  = max |g_new - g| / max(|g_new|, 1e-12)                (:278-279)
//           g     = r g_new + (1-r) g ; count++                          (:282-283)
//   while diff > conv and count < max_iter                               (:269)
//   Sigma_c = t g t^H,  t = E Stau - tau   (no eta)                      (:369-371)
//
// Every workgroup stops on ITS OWN convergence (the reference's vmap runs all
// energies until the slowest lane converges; results are identical because a
// converged lane is frozen there).
#include "negf_common.h"

#include "chain_wg.h"

struct Chain1DArgs {
    const cplx *alpha, *Salpha, *beta, *Sbeta, *tau, *Stau;   // concatenated per contact
    const int* nc;          // [n_contacts]
    const int* blk_off;     // [n_contacts] offset of the contact inside one energy record
    int n_contacts;
    int blk_stride;
    double eta, conv, relFactor;
    int max_iter, force_iters;
};

__global__ __launch_bounds__(CH_THREADS) void chain1d_kernel(
    Chain1DArgs a, const cplx* __restrict__ E, cplx* __restrict__ blk, int* __restrict__ iters,
    int* __restrict__ converged, cplx* __restrict__ scratch, size_t scratch_per_wg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ double red_v[CH_THREADS / 64];
    __shared__ int red_i[CH_THREADS / 64];
    __shared__ int piv_row;
    __shared__ double diff_sh;

    const int c = blockIdx.x, b = blockIdx.y;
    const int n = a.nc[c];
    const int off = a.blk_off[c];
    const int n2 = n * n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    cplx* rowk = reinterpret_cast<cplx*>(smem_raw);
    cplx* colk = rowk + n;
    int* ipiv = reinterpret_cast<int*>(colk + n);

    cplx* ws = scratch + ((size_t)b * a.n_contacts + c) * scratch_per_wg;
    cplx* A = ws;             // A
    cplx* B = A + n2;         // B
    cplx* g = B + n2;         // current (mixed) g
    cplx* T = g + n2;         // B g
    cplx* Mx = T + n2;        // A - T B^H  -> g_new in place

    const cplx e = E[b];
    const cplx z = cmake(e.x, e.y + a.eta);
    for (int t = tid; t < n2; t += CH_THREADS) {
        A[t] = csub(cmul(z, a.Salpha[off + t]), a.alpha[off + t]);
        B[t] = csub(cmul(z, a.Sbeta[off + t]), a.beta[off + t]);
        g[t] = A[t];
    }
    __syncthreads();
    wg_gj_inverse(n, g, rowk, colk, ipiv, red_v, red_i, &piv_row);   // g = inv(A)

    int count = 0;
    double diff = INFINITY;
    while (true) {
        if (a.force_iters >= 0) { if (count >= a.force_iters) break; }
        else if (!(diff > a.conv && count < a.max_iter)) break;
        wg_zgemm(n, B, g, 0, T);
        __syncthreads();
        // Mx = A - T B^H
        for (int t = tid; t < n2; t += CH_THREADS) {
            const int i = t / n, j = t - i * n;
            cplx acc = A[t];
            for (int k = 0; k < n; ++k) acc = cfnma(acc, T[i * n + k], cconj(B[j * n + k]));
            Mx[t] = acc;
        }
        __syncthreads();
        wg_gj_inverse(n, Mx, rowk, colk, ipiv, red_v, red_i, &piv_row);
        // diff and mixing
        double d = 0.0;
        for (int t = tid; t < n2; t += CH_THREADS) {
            const cplx gn = Mx[t], go = g[t];
            const double num = hypot(gn.x - go.x, gn.y - go.y);
            const double den = fmax(hypot(gn.x, gn.y), 1e-12);
            d = fmax(d, num / den);
            g[t] = cmake(gn.x * a.relFactor + go.x * (1.0 - a.relFactor),
                         gn.y * a.relFactor + go.y * (1.0 - a.relFactor));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d = fmax(d, __shfl_down(d, o, 64));
        if (lane == 0) red_v[wave] = d;
        __syncthreads();
        if (tid == 0) {
            double m = red_v[0];
            for (int w = 1; w < CH_THREADS / 64; ++w) m = fmax(m, red_v[w]);
            diff_sh = m;
        }
        __syncthreads();
        diff = diff_sh;
        ++count;
    }
    // Sigma_c = t g t^H, t = E Stau - tau
    for (int t = tid; t < n2; t += CH_THREADS) A[t] = csub(cmul(e, a.Stau[off + t]), a.tau[off + t]);
    __syncthreads();
    wg_zgemm(n, A, g, 0, T);
    __syncthreads();
    wg_zgemm(n, T, A, 1, blk + (size_t)b * a.blk_stride + off);
    if (tid == 0) {
        if (iters) iters[(size_t)b * a.n_contacts + c] = count;
        if (converged) converged[(size_t)b * a.n_contacts + c] = (diff <= a.conv) ? 1 : 0;
    }
}

size_t chain1d_scratch_per_wg(int nc_max) { return (size_t)5 * nc_max * nc_max; }

void launch_chain1d(hipStream_t st, const SigmaProvider& p, const int* d_nc, const int* d_blk_off,
                    int nb, const cplx* E, cplx* blk, int* iters, int* conv, cplx* scratch,
                    size_t scratch_per_wg)
{
    Chain1DArgs a;
    a.alpha = p.d_alpha; a.Salpha = p.d_Salpha; a.beta = p.d_beta; a.Sbeta = p.d_Sbeta;
    a.tau = p.d_tau; a.Stau = p.d_Stau;
    a.nc = d_nc; a.blk_off = d_blk_off;
    a.n_contacts = p.n_contacts; a.blk_stride = p.blk_stride;
    a.eta = p.eta; a.conv = p.conv; a.relFactor = p.relFactor;
    a.max_iter = p.max_iter; a.force_iters = p.force_iters;
    const size_t smem = (size_t)p.nc_max * (2 * sizeof(cplx) + sizeof(int));
    hipLaunchKernelGGL(chain1d_kernel, dim3(p.n_contacts, nb), dim3(CH_THREADS), smem, st, a, E, blk,
                       iters, conv, scratch, scratch_per_wg);
}
