// Floating dephasing probes on a layered device (negf_layered_gless_int_probes, negf_layered_impl.h; gfx950): the two
// passes between the kept column strips and the products A = Y Cfull^H.  Terminals as in k_rgf.hip's strip kernels: n_t end
// terminals followed by the call's probes, J_q the ascending union of the orbitals of the terminals on layer q (|J_q| = nJ[q],
// first column Joff[q] of the K_tot columns of a kept strip).  Every terminal lives in one layer, so the dephased coupling
//     D_s = scatter(Gamma_s) + sum_p R[p][s] scatter(Gamma_p)           (all weights 1 for the total)
// is block diagonal over the layers, D = (+)_q D_q with D_q on J_q, stored per energy as the blocks one after the other
// (D_q at Doff[q], row-major nJ[q] x nJ[q]).
//   rgf_deph_coupling : one workgroup per (layer q, energy).  D_q zeroed, then the terminals of the layer added one after
//                       the other through their positions in J_q (cpos): the selected end terminals in the order they were
//                       made, then the layer's probes in the plan's content order, each scaled by R[p][s] (1 for the total).
//                       Inside a terminal the orbitals are distinct: one thread per element, no atomics.  Element (i, j) and
//                       element (j, i) see the same terminals in the same order, the Gamma blocks are Hermitian element by
//                       element and R is real: D_q is exactly Hermitian (the diagonal product A_ii = Y_i Cfull_i^H relies on it).
//   rgf_blockdiag_mm  : Y_i = Cfull_i blockdiag(D_q) for every layer i, every column block q and every energy of the batch
//                       in ONE launch.  A workgroup owns a 32 x 16 tile of one column block of one layer's Y: the k sum runs
//                       over J_q alone (n |J_q|^2 flops per block, not n K_tot^2), in chunks of 16 through LDS, ascending k
//                       in one chain per element; every element of Y is written once, by one thread.  The bits of Y
//                       depend on the plan alone -- not on the batch or on the grid.  Vector FP64 from LDS: |J_q| is probe
//                       sized (a few to a few tens), one size class.
#include "negf_common.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_TR = 32, RD_TJ = 16, RD_TK = 16;           // rows, columns of a Y tile; the k chunk

__global__ __launch_bounds__(RD_THREADS) void rgf_deph_coupling_kernel(
    int nt, int P, int col, int nsel, const int* __restrict__ sel, const int* __restrict__ tlayer,
    const int* __restrict__ porder, const int* __restrict__ poff, const int* __restrict__ nJ, const int* __restrict__ Doff,
    const int* __restrict__ tK, const int* __restrict__ ioff, const int* __restrict__ goff, const int* __restrict__ gstride,
    const int* __restrict__ cpos, const cplx* __restrict__ gstat, const cplx* __restrict__ gdyn,
    const double* __restrict__ R, cplx* __restrict__ D, size_t strideD)
{
    const int q = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int KJ = nJ[q];
    if (KJ == 0) return;                                                // (uniform) a layer without a terminal
    cplx* Dq = D + (size_t)b * strideD + Doff[q];
    for (int e = tid; e < KJ * KJ; e += RD_THREADS) Dq[e] = cmake(0.0, 0.0);
    __syncthreads();
    const int np = poff[q + 1] - poff[q];
    for (int k = 0; k < nsel + np; ++k) {
        const int t = k < nsel ? sel[k] : porder[poff[q] + (k - nsel)];
        if (tlayer[t] != q) continue;                                   // (uniform) an end terminal of the other end
        const int K = tK[t];
        const int* I = cpos + ioff[t];
        const cplx* g = gstride[t] ? gdyn + (size_t)b * gstride[t] + goff[t] : gstat + goff[t];
        const double wgt = (col < 0 || t < nt) ? 1.0 : R[((size_t)b * P + (t - nt)) * nt + col];
        for (int e = tid; e < K * K; e += RD_THREADS) {
            const int i = e / K, j = e - i * K;
            const size_t at = (size_t)I[i] * KJ + I[j];
            const cplx d = Dq[at], x = g[e];
            Dq[at] = cmake(d.x + wgt * x.x, d.y + wgt * x.y);
        }
        __syncthreads();
    }
}

// blockIdx.x = (layer i * row tiles of the largest layer + row tile) * nct + column tile; ctile [nct][2]: the column tiles
// of all blocks, (q, first column inside J_q).  Cfull / Y of layer i and energy b: + (i * nb_max + b) * cs, n_i x K_tot.
__global__ __launch_bounds__(RD_THREADS) void rgf_blockdiag_mm_kernel(
    int trmax, int nct, int Ktot, int nb_max, size_t cs, const int* __restrict__ nl, const int* __restrict__ nJ,
    const int* __restrict__ Joff, const int* __restrict__ Doff, const int* __restrict__ ctile,
    const cplx* __restrict__ Cfull, const cplx* __restrict__ D, size_t strideD, cplx* __restrict__ Y)
{
    __shared__ cplx sC[RD_TR][RD_TK], sD[RD_TK][RD_TJ];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int ct = blockIdx.x % nct, rest = blockIdx.x / nct;
    const int rt = rest % trmax, i = rest / trmax;
    const int n = nl[i], r0 = rt * RD_TR;
    if (r0 >= n) return;                                                // (uniform) a layer smaller than the largest
    const int q = ctile[2 * ct], j0 = ctile[2 * ct + 1];
    const int KJ = nJ[q], c0 = Joff[q];
    const size_t at = ((size_t)i * nb_max + b) * cs;
    const cplx* Cb = Cfull + at + c0;
    const cplx* Dq = D + (size_t)b * strideD + Doff[q];
    const int tj = tid & (RD_TJ - 1), tr = tid / RD_TJ;                  // rows tr and tr + 16 of the tile, column tj
    cplx acc0 = cmake(0.0, 0.0), acc1 = acc0;
    for (int k0 = 0; k0 < KJ; k0 += RD_TK) {
        const int kc = min(RD_TK, KJ - k0);                             // (uniform)
        for (int e = tid; e < RD_TR * RD_TK; e += RD_THREADS) {
            const int rr = e / RD_TK, kk = e - rr * RD_TK;
            sC[rr][kk] = (r0 + rr < n && kk < kc) ? Cb[(size_t)(r0 + rr) * Ktot + k0 + kk] : cmake(0.0, 0.0);
        }
        {
            const int kk = tid / RD_TJ, jj = tid & (RD_TJ - 1);
            sD[kk][jj] = (kk < kc && j0 + jj < KJ) ? Dq[(size_t)(k0 + kk) * KJ + j0 + jj] : cmake(0.0, 0.0);
        }
        __syncthreads();
        for (int kk = 0; kk < kc; ++kk) {                               // ascending k: one chain per element
            const cplx d = sD[kk][tj];
            acc0 = cfma(acc0, sC[tr][kk], d);
            acc1 = cfma(acc1, sC[tr + 16][kk], d);
        }
        __syncthreads();
    }
    if (j0 + tj >= KJ) return;
    cplx* Yb = Y + at + c0 + j0 + tj;
    if (r0 + tr < n) Yb[(size_t)(r0 + tr) * Ktot] = acc0;
    if (r0 + tr + 16 < n) Yb[(size_t)(r0 + tr + 16) * Ktot] = acc1;
}

}  // namespace

void launch_rgf_deph_coupling(hipStream_t st, int L, int nb, int nt, int P, int col, int nsel, const int* sel,
                              const int* tlayer, const int* porder, const int* poff, const int* nJ, const int* Doff,
                              const int* tK, const int* ioff, const int* goff, const int* gstride, const int* cpos,
                              const cplx* gstat, const cplx* gdyn, const double* R, cplx* D, size_t strideD)
{
    if (L <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(rgf_deph_coupling_kernel, dim3(L, nb), dim3(RD_THREADS), 0, st, nt, P, col, nsel, sel, tlayer, porder,
                       poff, nJ, Doff, tK, ioff, goff, gstride, cpos, gstat, gdyn, R, D, strideD);
}

int rgf_blockdiag_row_tiles(int nmax) { return (nmax + RD_TR - 1) / RD_TR; }

int rgf_blockdiag_col_tiles(int KJ) { return (KJ + RD_TJ - 1) / RD_TJ; }

int rgf_blockdiag_tile_cols() { return RD_TJ; }

void launch_rgf_blockdiag_mm(hipStream_t st, int L, int nmax, int nct, int Ktot, int nb, int nb_max, size_t cs,
                             const int* nl, const int* nJ, const int* Joff, const int* Doff, const int* ctile,
                             const cplx* Cfull, const cplx* D, size_t strideD, cplx* Y)
{
    if (L <= 0 || nct <= 0 || nb <= 0) return;
    const int trmax = rgf_blockdiag_row_tiles(nmax);
    hipLaunchKernelGGL(rgf_blockdiag_mm_kernel, dim3((unsigned)((size_t)L * trmax * nct), nb), dim3(RD_THREADS), 0, st, trmax,
                       nct, Ktot, nb_max, cs, nl, nJ, Joff, Doff, ctile, Cfull, D, strideD, Y);
}
