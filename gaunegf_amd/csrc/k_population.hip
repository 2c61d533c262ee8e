// Overlap / Hamilton populations and projected DOS: where the states sit and which contact fills them (gfx950).
//     retarded form   pop[i][j]   = -(1/pi)  Im[G_ij   conj(X_ij)]      G   = (E S - F - Sigma)^-1
//     contact form    pop_c[i][j] = (1/2 pi) Re[A_c,ij conj(X_ij)]      A_c = G Gamma_c G^H
// X = S (overlap population; its row sums are the Mulliken-projected DOS -Im (G S)_ii / pi) or F (Hamilton population).
// Element (i, j) of the result needs element (i, j) of the matrix M (G or A_c) and of X: every read is a 16-byte load per
// lane, consecutive lanes on consecutive elements.  M is read ONCE per energy; X is shared by the whole batch and the
// energy is the fastest grid index, so the workgroups that run together read the same rows of X (L2).  The reference has
// no such function.  No floating-point atomics: every sum below has ONE order, fixed by the orbital indices and by the
// positions inside the groups alone -- results are bitwise equal from run to run, do not depend on the workspace batch,
// and relabelling the groups permutes tables and rows bit for bit.
//   pop_orbital      : out[b][i][j] = pop                               (table, every orbital its own group)
//   pop_group<.., 0> : out[b][a][g] = sum_{i in a, j in g} pop          (table, orbital -> group map sorted once per call)
//   pop_rows_orbital : out[b][i]    = sum_j pop[i][j]                   (rows, every orbital its own group: a wave per row)
//   pop_group<.., 1> : out[b][a]    = sum_g table[a][g]                 (rows: the table's entries, never stored)
//   pop_transpose_w, pop_coldot : p[b][a] = w_a^H (M w_a) from Y = M W^T (the library's zgemm)
#include "negf_common.h"
#include <algorithm>

// The same element is formed by several kernels (table and row form, with and without a group map) and their results
// are compared bit for bit: no contraction left to the compiler's choice -- the fused operations are written out.
#pragma clang fp contract(off)

static constexpr int POP_THREADS = 256;
static constexpr int POP_EPT = 4;                          // elements per thread and tile

// the element without its factor: Im[m conj(x)] (retarded) or Re[m conj(x)] (contact), and the factor
template <bool RET>
__device__ __forceinline__ double pop_elem(const cplx m, const cplx x)
{
    return RET ? __builtin_fma(m.y, x.x, -(m.x * x.y)) : __builtin_fma(m.x, x.x, m.y * x.y);
}
template <bool RET>
__device__ __forceinline__ double pop_scale()
{
    return RET ? -0.31830988618379067154 : 0.15915494309189533577;      // -1 / pi, 1 / (2 pi)
}

__device__ __forceinline__ double pop_wave_sum(double s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return s;                                              // (lane 0 holds the sum)
}

// ------------------------------------------------------------ table, per orbital pair
template <bool RET>
__global__ __launch_bounds__(POP_THREADS) void pop_orbital_kernel(
    int n2, const cplx* __restrict__ X, const cplx* __restrict__ M, const int* __restrict__ info, double* __restrict__ out)
{
    const int b = blockIdx.x;
    const cplx* Mb = M + (size_t)b * n2;
    double* o = out + (size_t)b * n2;
    constexpr int TILE = POP_THREADS * POP_EPT;
    if (info[b] != 0) {                                    // (uniform) singular energy: a NaN table
        const double qnan = __builtin_nan("");
        for (int t = blockIdx.y * POP_THREADS + threadIdx.x; t < n2; t += gridDim.y * POP_THREADS) o[t] = qnan;
        return;
    }
    for (int t0 = blockIdx.y * TILE; t0 < n2; t0 += gridDim.y * TILE) {
        cplx x[POP_EPT], m[POP_EPT];
#pragma unroll
        for (int k = 0; k < POP_EPT; ++k) {
            const int t = min(t0 + k * POP_THREADS + (int)threadIdx.x, n2 - 1);     // (clamped: the loads stay in bounds)
            x[k] = X[t]; m[k] = Mb[t];
        }
#pragma unroll
        for (int k = 0; k < POP_EPT; ++k) {
            const int t = t0 + k * POP_THREADS + threadIdx.x;
            if (t < n2) o[t] = pop_scale<RET>() * pop_elem<RET>(m[k], x[k]);
        }
    }
}

// ------------------------------------------------------------ rows, every orbital its own group
// A wave per row i: lane l adds scale * pop[i][l], [l + 64], ... in order (four 16-byte loads per matrix in flight),
// then the 6-step shuffle tree -- the order in which pop_group_kernel<.., true> adds the entries of a table row.
template <bool RET>
__global__ __launch_bounds__(POP_THREADS) void pop_rows_orbital_kernel(
    int n, const cplx* __restrict__ X, const cplx* __restrict__ M, const int* __restrict__ info, double* __restrict__ out)
{
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int i = blockIdx.y * (POP_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n) return;                                    // (wave-uniform)
    double* o = out + (size_t)b * n + i;
    if (info[b] != 0) {
        if (lane == 0) *o = __builtin_nan("");
        return;
    }
    const cplx* Mr = M + ((size_t)b * n + i) * n;
    const cplx* Xr = X + (size_t)i * n;
    double s = 0.0;
    for (int j0 = 0; j0 < n; j0 += 64 * POP_EPT) {
        cplx x[POP_EPT], m[POP_EPT];
#pragma unroll
        for (int k = 0; k < POP_EPT; ++k) {
            const int j = min(j0 + k * 64 + lane, n - 1);
            x[k] = Xr[j]; m[k] = Mr[j];
        }
#pragma unroll
        for (int k = 0; k < POP_EPT; ++k)
            if (j0 + k * 64 + lane < n) s += pop_scale<RET>() * pop_elem<RET>(m[k], x[k]);
    }
    s = pop_wave_sum(s);
    if (lane == 0) *o = s;
}

// ------------------------------------------------------------ per group pair / per row group
// One workgroup per (energy b, row group a).  perm [n]: the orbitals sorted by group (ascending orbital index inside a
// group), goff [ng + 1]: where each group starts in perm.  Pass 1: thread q owns the column perm[q] and adds the rows of
// group a in perm order -> colsum[q] in LDS.  Pass 2: a wave per column group g: lane l adds colsum[goff[g] + l],
// [.. + l + 64], ... in order, then the 6-step shuffle tree; times the factor this is table[a][g].
// ROWS: the entry is not stored but parked at val[first orbital of g] (val [n] in LDS, +0.0 elsewhere), and pass 3 adds
// val[l], val[l + 64], ... in order per lane of one wave, then the shuffle tree: the row is the sum of the TABLE's
// entries, in the order of the groups' first orbitals (adding +0.0 changes no sum).  The order of every addition
// depends on the orbital indices and the positions inside the groups only: relabelling the groups permutes table and
// rows bit for bit.
template <bool RET, bool ROWS>
__global__ __launch_bounds__(POP_THREADS) void pop_group_kernel(
    int n, int ng, const cplx* __restrict__ X, const cplx* __restrict__ M, const int* __restrict__ info,
    const int* __restrict__ perm, const int* __restrict__ goff, double* __restrict__ out)
{
    extern __shared__ double pop_lds[];                    // colsum [n] (| val [n])
    double* colsum = pop_lds;
    double* val = pop_lds + n;
    const int b = blockIdx.x, a = blockIdx.y, tid = threadIdx.x;
    double* o = ROWS ? out + (size_t)b * ng + a : out + ((size_t)b * ng + a) * ng;
    if (info[b] != 0) {                                    // (uniform)
        const double qnan = __builtin_nan("");
        for (int g = tid; g < (ROWS ? 1 : ng); g += POP_THREADS) o[g] = qnan;
        return;
    }
    const cplx* Mb = M + (size_t)b * n * n;
    const int r0 = goff[a], r1 = goff[a + 1];
    for (int q = tid; q < n; q += POP_THREADS) {
        const int j = perm[q];
        double acc = 0.0;
#pragma unroll 4
        for (int r = r0; r < r1; ++r) {
            const size_t t = (size_t)perm[r] * n + j;
            acc += pop_elem<RET>(Mb[t], X[t]);
        }
        colsum[q] = acc;
        if (ROWS) val[q] = 0.0;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int g = wave; g < ng; g += POP_THREADS / 64) {
        const int q0 = goff[g], q1 = goff[g + 1];
        double s = 0.0;
        for (int q = q0 + lane; q < q1; q += 64) s += colsum[q];
        s = pop_wave_sum(s);
        if (lane == 0) {
            if (!ROWS) o[g] = pop_scale<RET>() * s;
            else if (q1 > q0) val[perm[q0]] = pop_scale<RET>() * s;
        }
    }
    if (!ROWS) return;
    __syncthreads();
    if (wave == 0) {
        double s = 0.0;
        for (int j = lane; j < n; j += 64) s += val[j];
        s = pop_wave_sum(s);
        if (lane == 0) o[0] = s;
    }
}

template <bool RET>
static bool pop_launch(hipStream_t st, int n, int nb, const cplx* X, const cplx* M, const int* info, int rows_only, int ng,
                       const int* perm, const int* goff, double* out)
{
    if (!perm) {
        if (rows_only) {
            const int per = POP_THREADS / 64;
            hipLaunchKernelGGL(pop_rows_orbital_kernel<RET>, dim3(nb, (n + per - 1) / per), dim3(POP_THREADS), 0, st, n, X, M,
                               info, out);
        } else {
            const int n2 = n * n;
            constexpr int TILE = POP_THREADS * POP_EPT;
            const int gy = std::min((n2 + TILE - 1) / TILE, 65535);
            hipLaunchKernelGGL(pop_orbital_kernel<RET>, dim3(nb, gy), dim3(POP_THREADS), 0, st, n2, X, M, info, out);
        }
        return true;
    }
    if (rows_only) {
        const size_t lds = (size_t)2 * n * sizeof(double);
        // (n > 4096: beyond the default limit of dynamic LDS; the attribute belongs to the current device's copy of the
        //  kernel, so it is set at every such launch -- a host-side call, no flag to go stale on another device or thread)
        if (lds > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(&pop_group_kernel<RET, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        hipLaunchKernelGGL((pop_group_kernel<RET, true>), dim3(nb, ng), dim3(POP_THREADS), lds, st, n, ng, X, M, info, perm,
                           goff, out);
    } else {
        hipLaunchKernelGGL((pop_group_kernel<RET, false>), dim3(nb, ng), dim3(POP_THREADS), (size_t)n * sizeof(double), st, n,
                           ng, X, M, info, perm, goff, out);
    }
    return true;
}

bool launch_population(hipStream_t st, int n, int nb, bool retarded, const cplx* X, const cplx* M, const int* info,
                       int rows_only, int ng, const int* perm, const int* goff, double* out)
{
    if (nb <= 0) return true;
    if (n > bond_max_n()) return false;
    return retarded ? pop_launch<true>(st, n, nb, X, M, info, rows_only, ng, perm, goff, out)
                    : pop_launch<false>(st, n, nb, X, M, info, rows_only, ng, perm, goff, out);
}

// ------------------------------------------------------------ projection on vectors
// Wt[i][a] = W[a][i]: the k vectors as the columns of an n x k matrix, the plain second operand of Y = M Wt
__global__ __launch_bounds__(POP_THREADS) void pop_transpose_w_kernel(int n, int k, const cplx* __restrict__ W,
                                                                      cplx* __restrict__ Wt)
{
    const size_t cnt = (size_t)n * k;
    for (size_t t = (size_t)blockIdx.x * POP_THREADS + threadIdx.x; t < cnt; t += (size_t)gridDim.x * POP_THREADS) {
        const size_t i = t / k, a = t - i * k;
        Wt[t] = W[a * n + i];
    }
}

void launch_pop_transpose_w(hipStream_t st, int n, int k, const cplx* W, cplx* Wt)
{
    const size_t cnt = (size_t)n * k;
    const int g = (int)std::min<size_t>((cnt + POP_THREADS - 1) / POP_THREADS, 2048);
    hipLaunchKernelGGL(pop_transpose_w_kernel, dim3(g), dim3(POP_THREADS), 0, st, n, k, W, Wt);
}

// out[b][a] = factor * Im / Re [sum_i conj(Wt[i][a]) Y[b][i][a]].  Lane l of a workgroup owns vector a = 64 blockIdx.y + l
// (consecutive lanes on consecutive elements of a row of Y and of Wt); wave w adds the rows i = w, w + 4, ... in order, and
// the four partial sums are added as (p0 + p1) + (p2 + p3): the order depends on n alone, so a vector's value does not
// depend on k or on its neighbours.
template <bool RET>
__global__ __launch_bounds__(POP_THREADS) void pop_coldot_kernel(
    int n, int k, const cplx* __restrict__ Wt, const cplx* __restrict__ Y, size_t strideY, const int* __restrict__ info,
    double* __restrict__ out)
{
    __shared__ double part[POP_THREADS / 64][64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a = blockIdx.y * 64 + lane;
    const cplx* Yb = Y + (size_t)b * strideY;
    double acc = 0.0;
    if (a < k && info[b] == 0) {
        for (int i = wave; i < n; i += POP_THREADS / 64) {
            const cplx w = Wt[(size_t)i * k + a], y = Yb[(size_t)i * k + a];
            acc += RET ? __builtin_fma(w.x, y.y, -(w.y * y.x)) : __builtin_fma(w.x, y.x, w.y * y.y);     // Im / Re of conj(w) y
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && a < k) {
        const double s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        out[(size_t)b * k + a] = info[b] != 0 ? __builtin_nan("") : pop_scale<RET>() * s;
    }
}

void launch_pop_coldot(hipStream_t st, int n, int k, int nb, bool retarded, const cplx* Wt, const cplx* Y, size_t strideY,
                       const int* info, double* out)
{
    if (nb <= 0) return;
    const dim3 grid(nb, (k + 63) / 64);
    if (retarded) hipLaunchKernelGGL(pop_coldot_kernel<true>, grid, dim3(POP_THREADS), 0, st, n, k, Wt, Y, strideY, info, out);
    else hipLaunchKernelGGL(pop_coldot_kernel<false>, grid, dim3(POP_THREADS), 0, st, n, k, Wt, Y, strideY, info, out);
}
