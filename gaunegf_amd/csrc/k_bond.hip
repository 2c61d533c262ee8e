// Local (bond) transmission: where in the junction the current injected by contact c flows (gfx950).
//     K(E)   = E S - F                              (the assembled matrix WITHOUT the self-energies; never stored)
//     A_c(E) = G Gamma_c G^H                        (what the GrLessInt sequence leaves per energy, Hermitian)
//     flow[i][j](E) = 2 Im[K_ij A_c,ji] = 2 Im[K_ij conj(A_c,ij)]
// so element (i, j) of the result needs element (i, j) of A, S and F: every read is a 16-byte load per lane, consecutive
// lanes on consecutive elements.  A is read ONCE per energy (16 n^2 bytes); S and F are shared by the whole batch and
// the energy is the fastest grid index, so the workgroups that run together read the same rows of S and F (L2).
// The reference has no such function.  No floating-point atomics: every sum below has ONE order, fixed by the
// indices alone -- results are bitwise equal from run to run and do not depend on the workspace batch.
//   bond_orbital : out[b][i][j] = flow                                  (every orbital its own group)
//   bond_group   : out[b][a][g] = sum_{i in a, j in g} flow             (orbital -> group map, sorted once per call)
//   bond_int     : out[i][j]   += sum_b w_b flow_b[i][j]                (chunks of 32 energies of the GRID, in order)
#include "negf_common.h"
#include <algorithm>

static constexpr int BOND_THREADS = 256;

// K = E S - F in assemble_kernel's operation order, then 2 Im[K conj(A)]
__device__ __forceinline__ double bond_flow(const cplx e, const cplx s, const cplx h, const cplx a)
{
    const double kx = e.x * s.x - e.y * s.y - h.x;
    const double ky = e.x * s.y + e.y * s.x - h.y;
    return 2.0 * (ky * a.x - kx * a.y);
}

// ------------------------------------------------------------ per energy, per orbital pair
static constexpr int BOND_EPT = 4;                         // elements per thread and tile
__global__ __launch_bounds__(BOND_THREADS) void bond_orbital_kernel(
    int n2, const cplx* __restrict__ E, const cplx* __restrict__ S, const cplx* __restrict__ F,
    const cplx* __restrict__ A, const int* __restrict__ info, double* __restrict__ out)
{
    const int b = blockIdx.x;
    const cplx e = E[b];
    const cplx* Ab = A + (size_t)b * n2;
    double* o = out + (size_t)b * n2;
    constexpr int TILE = BOND_THREADS * BOND_EPT;
    if (info[b] != 0) {                                    // (uniform) singular energy: a NaN table
        const double qnan = __builtin_nan("");
        for (int t = blockIdx.y * BOND_THREADS + threadIdx.x; t < n2; t += gridDim.y * BOND_THREADS) o[t] = qnan;
        return;
    }
    for (int t0 = blockIdx.y * TILE; t0 < n2; t0 += gridDim.y * TILE) {
        cplx s[BOND_EPT], h[BOND_EPT], a[BOND_EPT];
#pragma unroll
        for (int k = 0; k < BOND_EPT; ++k) {
            const int t = min(t0 + k * BOND_THREADS + (int)threadIdx.x, n2 - 1);   // (clamped: the loads stay in bounds)
            s[k] = S[t]; h[k] = F[t]; a[k] = Ab[t];
        }
#pragma unroll
        for (int k = 0; k < BOND_EPT; ++k) {
            const int t = t0 + k * BOND_THREADS + threadIdx.x;
            if (t < n2) o[t] = bond_flow(e, s[k], h[k], a[k]);
        }
    }
}

// ------------------------------------------------------------ per energy, per group pair
// One workgroup per (energy b, row group a).  perm [n]: the orbitals sorted by group (ascending orbital index inside a
// group), goff [ng + 1]: where each group starts in perm.  Pass 1: thread q owns the column perm[q] and adds the rows of
// group a in perm order -> colsum[q] in LDS.  Pass 2: a wave per column group g: lane l adds colsum[goff[g] + l],
// [.. + l + 64], ... in order, then the 6-step shuffle tree.  The order of every addition depends on the positions
// inside the groups only: relabelling the groups permutes the table bit for bit.
__global__ __launch_bounds__(BOND_THREADS) void bond_group_kernel(
    int n, int ng, const cplx* __restrict__ E, const cplx* __restrict__ S, const cplx* __restrict__ F,
    const cplx* __restrict__ A, const int* __restrict__ info, const int* __restrict__ perm,
    const int* __restrict__ goff, double* __restrict__ out)
{
    extern __shared__ double bond_colsum[];                // [n]
    const int b = blockIdx.x, a = blockIdx.y, tid = threadIdx.x;
    double* o = out + ((size_t)b * ng + a) * ng;
    if (info[b] != 0) {                                    // (uniform)
        const double qnan = __builtin_nan("");
        for (int g = tid; g < ng; g += BOND_THREADS) o[g] = qnan;
        return;
    }
    const cplx e = E[b];
    const cplx* Ab = A + (size_t)b * n * n;
    const int r0 = goff[a], r1 = goff[a + 1];
    for (int q = tid; q < n; q += BOND_THREADS) {
        const int j = perm[q];
        double acc = 0.0;
#pragma unroll 4
        for (int r = r0; r < r1; ++r) {
            const size_t t = (size_t)perm[r] * n + j;
            acc += bond_flow(e, S[t], F[t], Ab[t]);
        }
        bond_colsum[q] = acc;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int g = wave; g < ng; g += BOND_THREADS / 64) {
        double s = 0.0;
        for (int q = goff[g] + lane; q < goff[g + 1]; q += 64) s += bond_colsum[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) o[g] = s;
    }
}

int bond_max_n() { return 8192; }                          // colsum: n doubles of LDS (64 KB)

bool launch_bond_tables(hipStream_t st, int n, int nb, const cplx* E, const cplx* S, const cplx* F, const cplx* A,
                        const int* info, int ng, const int* perm, const int* goff, double* out)
{
    if (nb <= 0) return true;
    if (n > bond_max_n()) return false;
    if (!perm) {
        const int n2 = n * n;
        constexpr int TILE = BOND_THREADS * BOND_EPT;
        const int gy = std::min((n2 + TILE - 1) / TILE, 65535);
        hipLaunchKernelGGL(bond_orbital_kernel, dim3(nb, gy), dim3(BOND_THREADS), 0, st, n2, E, S, F, A, info, out);
        return true;
    }
    hipLaunchKernelGGL(bond_group_kernel, dim3(nb, ng), dim3(BOND_THREADS), (size_t)n * sizeof(double), st, n, ng, E, S,
                       F, A, info, perm, goff, out);
    return true;
}

// ------------------------------------------------------------ energy integral
// out[i] += sum_k w_k flow_k[i] over the batch [m0, m0 + nb) of a grid of m energies, so that the bits do not depend on
// how the grid was cut into batches: chunk c is the energies [32 c, 32 c + 32) OF THE GRID, added in ascending order
// starting from zero, and out receives the chunk sums in ascending chunk order.  A chunk that a batch boundary cuts is
// carried: its running sum waits in `carry` and the next batch continues it.  Store-then-sum: pass 1 writes one record
// per chunk the batch touches (part [chunks][n2]), pass 2 adds the finished ones to out.
static constexpr int BOND_CHUNK = 32;

__global__ __launch_bounds__(BOND_THREADS) void bond_int_partial_kernel(
    int n2, int m0, int nb, int c_first, const cplx* __restrict__ E, const double* __restrict__ w,
    const cplx* __restrict__ S, const cplx* __restrict__ F, const cplx* __restrict__ A,
    const double* __restrict__ carry, double* __restrict__ part)
{
    const int i = blockIdx.x * BOND_THREADS + threadIdx.x;
    const int c = c_first + blockIdx.y;
    if (i >= n2) return;
    // (E, w, A are indexed from the batch's first energy)
    const int b0 = max(c * BOND_CHUNK, m0) - m0, b1 = min((c + 1) * BOND_CHUNK, m0 + nb) - m0;
    const cplx s = S[i], h = F[i];
    double acc = c * BOND_CHUNK < m0 ? carry[i] : 0.0;
    int b = b0;
    for (; b + 4 <= b1; b += 4) {
        const cplx x0 = A[(size_t)(b + 0) * n2 + i], x1 = A[(size_t)(b + 1) * n2 + i];
        const cplx x2 = A[(size_t)(b + 2) * n2 + i], x3 = A[(size_t)(b + 3) * n2 + i];
        acc += w[b + 0] * bond_flow(E[b + 0], s, h, x0); acc += w[b + 1] * bond_flow(E[b + 1], s, h, x1);
        acc += w[b + 2] * bond_flow(E[b + 2], s, h, x2); acc += w[b + 3] * bond_flow(E[b + 3], s, h, x3);
    }
    for (; b < b1; ++b) acc += w[b] * bond_flow(E[b], s, h, A[(size_t)b * n2 + i]);
    part[(size_t)blockIdx.y * n2 + i] = acc;
}

__global__ __launch_bounds__(BOND_THREADS) void bond_int_final_kernel(
    int n2, int nchunks, int last_open, const double* __restrict__ part, double* __restrict__ carry,
    double* __restrict__ out)
{
    const int i = blockIdx.x * BOND_THREADS + threadIdx.x;
    if (i >= n2) return;
    const int closed = nchunks - last_open;
    if (closed > 0) {
        double a = out[i];
        for (int c = 0; c < closed; ++c) a += part[(size_t)c * n2 + i];
        out[i] = a;
    }
    if (last_open) carry[i] = part[(size_t)(nchunks - 1) * n2 + i];
}

size_t bond_int_scratch_doubles(int n2, int nb) { return (size_t)((nb + BOND_CHUNK - 1) / BOND_CHUNK + 1) * n2; }

void launch_bond_int(hipStream_t st, int n2, int m, int m0, int nb, const cplx* E, const double* w, const cplx* S,
                     const cplx* F, const cplx* A, double* carry, double* part, double* out)
{
    if (nb <= 0) return;
    const int c_first = m0 / BOND_CHUNK, c_last = (m0 + nb - 1) / BOND_CHUNK;
    const int nchunks = c_last - c_first + 1;
    // the last chunk stays open when the grid goes on behind this batch inside it
    const int last_open = (m0 + nb < m && (m0 + nb) % BOND_CHUNK != 0) ? 1 : 0;
    const int g = (n2 + BOND_THREADS - 1) / BOND_THREADS;
    hipLaunchKernelGGL(bond_int_partial_kernel, dim3(g, nchunks), dim3(BOND_THREADS), 0, st, n2, m0, nb, c_first, E, w, S,
                       F, A, carry, part);
    hipLaunchKernelGGL(bond_int_final_kernel, dim3(g), dim3(BOND_THREADS), 0, st, n2, nchunks, last_open, part, carry, out);
}
