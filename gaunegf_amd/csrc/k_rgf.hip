// Layer-wise passes of the recursive Green's function path (negf_layered_*, negf_layered_impl.h; gfx950).
// The layer inverses and products are the dense path's own launchers; what is here is the HBM-bound work around them:
//   rgf_diag      : D_b = E_b S_ii - F_ii - P_b - sum_t scatter(Sigma_t,b)     one pass, terminals and Schur term included
//   rgf_coupling  : C_b = F_ij - E_b S_ij                                       the NEGATED coupling block -A_ij
//   rgf_add       : G_ii = g_i + W                                              the backward sweep's update
//   rgf_gamma     : Gamma = i (Sigma - Sigma^H) on a terminal's K x K block
//   rgf_dos_*     : -Im G_rr / pi, and the rows of -Im (G S) / pi block by block
//   rgf_accumulate: acc += sum_b w_b X_b, b ascending in ONE chain per element (bitwise independent of the batch cut)
//   rgf_gather_cols / rgf_gamma_union / rgf_accumulate_ct / rgf_pop_*: the passes of G Gamma G^H on the pattern of S
//                   (negf_layered_gless_int, negf_layered_contact_dos): the columns G[:, J] of a terminal set, its Gamma
//                   on the union list J, the conjugate-transposed sum of the lower blocks, the contact Mulliken rows
//   rgf_sub_probes / rgf_strip_pair: the transmission matrix with probes on any layer (negf_layered_transmission_matrix):
//                   the probes' Sigma blocks subtracted from an assembled diagonal matrix, and T[a][b] of the terminal pairs
//                   of one layer level from the column strip [G_ii[:, J_i] | G_{i,i+1}[:, J_{i+1}] | ...] of that level
//   rgf_bond_*    : bond currents and local transmission on the pattern of S (negf_layered_local_transmission,
//                   negf_layered_bond_int): flow = 2 Im[(E S - F) conj(A)] of a block of A = G Gamma G^H per energy, its
//                   group table, and its weighted sum over the energies; a transposed form of each for the lower blocks
// Every matrix of a batch is compact row-major (leading dimension = its own column count) at a batch stride the
// caller gives; consecutive lanes touch consecutive 16-byte elements.  No atomics.
#include "negf_common.h"

static constexpr int RGF_THREADS = 256;

static __device__ __forceinline__ double rgf_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

static int rgf_grid(size_t count)
{
    size_t gx = (count + RGF_THREADS - 1) / RGF_THREADS;
    return (int)(gx > 256 ? 256 : (gx < 1 ? 1 : gx));
}

__global__ __launch_bounds__(RGF_THREADS) void rgf_diag_kernel(
    int n, const cplx* __restrict__ E, const cplx* __restrict__ S, const cplx* __restrict__ F,
    const cplx* __restrict__ P, size_t strideP, RgfTermArgs t, cplx* __restrict__ D, size_t strideD)
{
    const int b = blockIdx.y;
    const cplx e = E[b];
    const cplx* Pb = P ? P + (size_t)b * strideP : nullptr;
    cplx* Db = D + (size_t)b * strideD;
    const int n2 = n * n;
    for (int i = blockIdx.x * RGF_THREADS + threadIdx.x; i < n2; i += gridDim.x * RGF_THREADS) {
        const cplx s = S[i];
        const cplx h = F[i];
        cplx a = cmake(e.x * s.x - e.y * s.y - h.x, e.x * s.y + e.y * s.x - h.y);      // E S - F as the dense assemble forms it
        if (Pb) a = csub(a, Pb[i]);
        if (t.count > 0) {
            const int r = i / n, c = i - r * n;
            for (int k = 0; k < t.count; ++k) {                                       // terminal order: a fixed sum
                const int pr = t.pos[k][r], pc = t.pos[k][c];
                if (pr >= 0 && pc >= 0) a = csub(a, t.sig[k][(size_t)b * t.stride[k] + (size_t)pr * t.K[k] + pc]);
            }
        }
        Db[i] = a;
    }
}

void launch_rgf_diag(hipStream_t st, int n, int nb, const cplx* E, const cplx* S, const cplx* F, const cplx* P,
                     size_t strideP, const RgfTermArgs& t, cplx* D, size_t strideD)
{
    hipLaunchKernelGGL(rgf_diag_kernel, dim3(rgf_grid((size_t)n * n), nb), dim3(RGF_THREADS), 0, st, n, E, S, F, P,
                       strideP, t, D, strideD);
}

__global__ __launch_bounds__(RGF_THREADS) void rgf_coupling_kernel(
    int count, const cplx* __restrict__ E, const cplx* __restrict__ S, const cplx* __restrict__ F,
    cplx* __restrict__ C, size_t strideC)
{
    const int b = blockIdx.y;
    const cplx e = E[b];
    cplx* Cb = C + (size_t)b * strideC;
    for (int i = blockIdx.x * RGF_THREADS + threadIdx.x; i < count; i += gridDim.x * RGF_THREADS) {
        const cplx s = S[i];
        const cplx h = F[i];
        Cb[i] = cmake(h.x - (e.x * s.x - e.y * s.y), h.y - (e.x * s.y + e.y * s.x));
    }
}

void launch_rgf_coupling(hipStream_t st, int count, int nb, const cplx* E, const cplx* S, const cplx* F, cplx* C,
                         size_t strideC)
{
    hipLaunchKernelGGL(rgf_coupling_kernel, dim3(rgf_grid((size_t)count), nb), dim3(RGF_THREADS), 0, st, count, E, S, F,
                       C, strideC);
}

__global__ __launch_bounds__(RGF_THREADS) void rgf_add_kernel(
    int count, const cplx* __restrict__ g, size_t strideg, const cplx* __restrict__ W, size_t strideW,
    cplx* __restrict__ G, size_t strideG)
{
    const int b = blockIdx.y;
    const cplx* gb = g + (size_t)b * strideg;
    const cplx* Wb = W + (size_t)b * strideW;
    cplx* Gb = G + (size_t)b * strideG;
    for (int i = blockIdx.x * RGF_THREADS + threadIdx.x; i < count; i += gridDim.x * RGF_THREADS)
        Gb[i] = cadd(gb[i], Wb[i]);
}

void launch_rgf_add(hipStream_t st, int count, int nb, const cplx* g, size_t strideg, const cplx* W, size_t strideW,
                    cplx* G, size_t strideG)
{
    hipLaunchKernelGGL(rgf_add_kernel, dim3(rgf_grid((size_t)count), nb), dim3(RGF_THREADS), 0, st, count, g, strideg, W,
                       strideW, G, strideG);
}

__global__ __launch_bounds__(RGF_THREADS) void rgf_gamma_kernel(
    int K, const cplx* __restrict__ sig, size_t stride_sig, cplx* __restrict__ out, size_t stride_out)
{
    const int b = blockIdx.y;
    const cplx* s = sig + (size_t)b * stride_sig;
    cplx* o = out + (size_t)b * stride_out;
    for (int t = blockIdx.x * RGF_THREADS + threadIdx.x; t < K * K; t += gridDim.x * RGF_THREADS) {
        const int i = t / K, j = t - i * K;
        const cplx a = s[t], c = s[(size_t)j * K + i];
        // i (a - conj(c))
        o[t] = cmake(-(a.y + c.y), a.x - c.x);
    }
}

void launch_rgf_gamma(hipStream_t st, int K, int nb, const cplx* sig, size_t stride_sig, cplx* out, size_t stride_out)
{
    hipLaunchKernelGGL(rgf_gamma_kernel, dim3(rgf_grid((size_t)K * K), nb), dim3(RGF_THREADS), 0, st, K, sig, stride_sig,
                       out, stride_out);
}

__global__ __launch_bounds__(RGF_THREADS) void rgf_dos_diag_kernel(
    int n, const cplx* __restrict__ G, size_t strideG, double* __restrict__ site, size_t site_stride)
{
    const int b = blockIdx.y;
    const cplx* g = G + (size_t)b * strideG;
    const double pi = 3.14159265358979323846;
    for (int i = blockIdx.x * RGF_THREADS + threadIdx.x; i < n; i += gridDim.x * RGF_THREADS)
        site[(size_t)b * site_stride + i] = -g[(size_t)i * n + i].y / pi;
}

void launch_rgf_dos_diag(hipStream_t st, int n, int nb, const cplx* G, size_t strideG, double* site, size_t site_stride)
{
    hipLaunchKernelGGL(rgf_dos_diag_kernel, dim3(rgf_grid((size_t)n), nb), dim3(RGF_THREADS), 0, st, n, G, strideG, site,
                       site_stride);
}

// one wave per (energy, row): site[b][r] (+)= -Im sum_k G_b[r][k] conj(X[r][k]) / pi, where X[r][k] = S block read
// through S_kr = conj(S_rk)
__global__ __launch_bounds__(RGF_THREADS) void rgf_dos_rows_kernel(
    int nr, int nk, const cplx* __restrict__ G, size_t strideG, const cplx* __restrict__ X,
    double* __restrict__ site, size_t site_stride, int accumulate)
{
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (RGF_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= nr) return;                                    // whole waves leave together
    const cplx* g = G + (size_t)b * strideG + (size_t)r * nk;
    const cplx* x = X + (size_t)r * nk;
    double s = 0.0;
    for (int k = lane; k < nk; k += 64) {
        const cplx a = g[k], c = x[k];
        s += a.y * c.x - a.x * c.y;                         // Im[a conj(c)]
    }
    s = rgf_wave_sum(s);
    if (lane == 0) {
        const double pi = 3.14159265358979323846;
        double* o = site + (size_t)b * site_stride + r;
        const double v = -s / pi;
        *o = accumulate ? *o + v : v;
    }
}

void launch_rgf_dos_rows(hipStream_t st, int nr, int nk, int nb, const cplx* G, size_t strideG, const cplx* X,
                         double* site, size_t site_stride, bool accumulate)
{
    const int rows_per = RGF_THREADS / 64;
    hipLaunchKernelGGL(rgf_dos_rows_kernel, dim3((nr + rows_per - 1) / rows_per, nb), dim3(RGF_THREADS), 0, st, nr, nk, G,
                       strideG, X, site, site_stride, accumulate ? 1 : 0);
}

// tot[b] = sum_i site[b][i]: thread t adds its stride of orbitals in order, then a fixed tree
__global__ __launch_bounds__(RGF_THREADS) void rgf_dos_total_kernel(
    int N, const double* __restrict__ site, size_t site_stride, double* __restrict__ tot)
{
    __shared__ double part[RGF_THREADS / 64];
    const int b = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < N; i += RGF_THREADS) s += site[(size_t)b * site_stride + i];
    s = rgf_wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < RGF_THREADS / 64; ++k) t += part[k];
        tot[b] = t;
    }
}

void launch_rgf_dos_total(hipStream_t st, int N, int nb, const double* site, size_t site_stride, double* tot)
{
    hipLaunchKernelGGL(rgf_dos_total_kernel, dim3(nb), dim3(RGF_THREADS), 0, st, N, site, site_stride, tot);
}

__global__ __launch_bounds__(RGF_THREADS) void rgf_accumulate_kernel(
    int count, int nb, const cplx* __restrict__ w, const cplx* __restrict__ X, size_t strideX, cplx* __restrict__ acc)
{
    const int i = blockIdx.x * RGF_THREADS + threadIdx.x;
    if (i >= count) return;
    cplx v = acc[i];
    for (int b = 0; b < nb; ++b) v = cfma(v, w[b], X[(size_t)b * strideX + i]);
    acc[i] = v;
}

void launch_rgf_accumulate(hipStream_t st, int count, int nb, const cplx* w, const cplx* X, size_t strideX, cplx* acc)
{
    if (count <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(rgf_accumulate_kernel, dim3((count + RGF_THREADS - 1) / RGF_THREADS), dim3(RGF_THREADS), 0, st,
                       count, nb, w, X, strideX, acc);
}

// out[b][r][a] = G[b][r][idx[a]]: the K columns `idx` of an n x n matrix, compact n x K
// (ld: the leading dimension of out -- K for a compact set, the strip's width for the head of a column strip)
__global__ __launch_bounds__(RGF_THREADS) void rgf_gather_cols_kernel(
    int n, int K, int ld, const cplx* __restrict__ G, size_t strideG, const int* __restrict__ idx, cplx* __restrict__ out,
    size_t stride_out)
{
    const int b = blockIdx.y;
    const cplx* g = G + (size_t)b * strideG;
    cplx* o = out + (size_t)b * stride_out;
    const int cnt = n * K;
    for (int t = blockIdx.x * RGF_THREADS + threadIdx.x; t < cnt; t += gridDim.x * RGF_THREADS) {
        const int r = t / K, a = t - r * K;
        o[(size_t)r * ld + a] = g[(size_t)r * n + idx[a]];
    }
}

void launch_rgf_gather_cols(hipStream_t st, int n, int K, int nb, const cplx* G, size_t strideG, const int* idx, cplx* out,
                            size_t stride_out)
{
    hipLaunchKernelGGL(rgf_gather_cols_kernel, dim3(rgf_grid((size_t)n * K), nb), dim3(RGF_THREADS), 0, st, n, K, K, G,
                       strideG, idx, out, stride_out);
}

void launch_rgf_strip_head(hipStream_t st, int n, int K, int ld, int nb, const cplx* G, size_t strideG, const int* idx,
                           cplx* out, size_t stride_out)
{
    if (K <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(rgf_gather_cols_kernel, dim3(rgf_grid((size_t)n * K), nb), dim3(RGF_THREADS), 0, st, n, K, ld, G,
                       strideG, idx, out, stride_out);
}

// out[b][p][q] = sum over the terminals k, in their order, of Gamma_k[pos_k[J[p]]][pos_k[J[q]]] where both lie in terminal
// k's list; Gamma_k = i (Sigma_k - Sigma_k^H) element by element as rgf_gamma forms it
__global__ __launch_bounds__(RGF_THREADS) void rgf_gamma_union_kernel(
    int KJ, const int* __restrict__ J, RgfTermArgs t, cplx* __restrict__ out, size_t stride_out)
{
    const int b = blockIdx.y;
    cplx* o = out + (size_t)b * stride_out;
    for (int e = blockIdx.x * RGF_THREADS + threadIdx.x; e < KJ * KJ; e += gridDim.x * RGF_THREADS) {
        const int p = e / KJ, q = e - p * KJ;
        const int jp = J[p], jq = J[q];
        cplx v = cmake(0.0, 0.0);
        for (int k = 0; k < t.count; ++k) {
            const int i = t.pos[k][jp], j = t.pos[k][jq];
            if (i < 0 || j < 0) continue;
            const cplx* s = t.sig[k] + (size_t)b * t.stride[k];
            const cplx a = s[(size_t)i * t.K[k] + j], c = s[(size_t)j * t.K[k] + i];
            v = cadd(v, cmake(-(a.y + c.y), a.x - c.x));
        }
        o[e] = v;
    }
}

void launch_rgf_gamma_union(hipStream_t st, int KJ, int nb, const int* J, const RgfTermArgs& t, cplx* out, size_t stride_out)
{
    hipLaunchKernelGGL(rgf_gamma_union_kernel, dim3(rgf_grid((size_t)KJ * KJ), nb), dim3(RGF_THREADS), 0, st, KJ, J, t, out,
                       stride_out);
}

// acc[c][r] += sum_b w_b conj(X_b[r][c]) (X nr x nc, acc nc x nr), b ascending in one chain per element.  A 16 x 16 tile
// goes through LDS so that the read of X and the write of acc both run along rows; the tile's rows are padded by one
// double against bank conflicts of the transposed read.
static constexpr int RGF_CT_TILE = 16;

__global__ __launch_bounds__(RGF_CT_TILE * RGF_CT_TILE) void rgf_accumulate_ct_kernel(
    int nr, int nc, int nb, const cplx* __restrict__ w, const cplx* __restrict__ X, size_t strideX, cplx* __restrict__ acc)
{
    __shared__ double tre[RGF_CT_TILE][RGF_CT_TILE + 1], tim[RGF_CT_TILE][RGF_CT_TILE + 1];
    const int tx = threadIdx.x & (RGF_CT_TILE - 1), ty = threadIdx.x / RGF_CT_TILE;
    const int r0 = blockIdx.y * RGF_CT_TILE, c0 = blockIdx.x * RGF_CT_TILE;
    const bool in_ok = r0 + ty < nr && c0 + tx < nc;        // X[r0 + ty][c0 + tx]
    const bool out_ok = c0 + ty < nc && r0 + tx < nr;       // acc[c0 + ty][r0 + tx]
    const size_t in_at = (size_t)(r0 + ty) * nc + c0 + tx, out_at = (size_t)(c0 + ty) * nr + r0 + tx;
    cplx v = out_ok ? acc[out_at] : cmake(0.0, 0.0);
    for (int b = 0; b < nb; ++b) {
        if (in_ok) { const cplx x = X[(size_t)b * strideX + in_at]; tre[ty][tx] = x.x; tim[ty][tx] = x.y; }
        __syncthreads();
        if (out_ok) v = cfma(v, w[b], cmake(tre[tx][ty], -tim[tx][ty]));
        __syncthreads();
    }
    if (out_ok) acc[out_at] = v;
}

void launch_rgf_accumulate_ct(hipStream_t st, int nr, int nc, int nb, const cplx* w, const cplx* X, size_t strideX, cplx* acc)
{
    if (nr <= 0 || nc <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(rgf_accumulate_ct_kernel, dim3((nc + RGF_CT_TILE - 1) / RGF_CT_TILE, (nr + RGF_CT_TILE - 1) / RGF_CT_TILE),
                       dim3(RGF_CT_TILE * RGF_CT_TILE), 0, st, nr, nc, nb, w, X, strideX, acc);
}

// contact Mulliken rows of one block A (nr x nk) against its S block X:
//   rows: site[b][r] (+)= sum_k Re[A_b[r][k] conj(X[r][k])] / 2 pi, one wave per (energy, row), rgf_dos_rows's tree
//   cols: site[b][k]  += sum_r Re[A_b[r][k] conj(X[r][k])] / 2 pi, one thread per column, r ascending
__global__ __launch_bounds__(RGF_THREADS) void rgf_pop_rows_kernel(
    int nr, int nk, const cplx* __restrict__ A, size_t strideA, const cplx* __restrict__ X,
    double* __restrict__ site, size_t site_stride, int accumulate)
{
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (RGF_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= nr) return;                                    // whole waves leave together
    const cplx* a = A + (size_t)b * strideA + (size_t)r * nk;
    const cplx* x = X + (size_t)r * nk;
    double s = 0.0;
    for (int k = lane; k < nk; k += 64) {
        const cplx p = a[k], c = x[k];
        s += p.x * c.x + p.y * c.y;                         // Re[p conj(c)]
    }
    s = rgf_wave_sum(s);
    if (lane == 0) {
        const double two_pi = 6.28318530717958647692;
        double* o = site + (size_t)b * site_stride + r;
        const double v = s / two_pi;
        *o = accumulate ? *o + v : v;
    }
}

__global__ __launch_bounds__(RGF_THREADS) void rgf_pop_cols_kernel(
    int nr, int nk, const cplx* __restrict__ A, size_t strideA, const cplx* __restrict__ X,
    double* __restrict__ site, size_t site_stride)
{
    const int b = blockIdx.y;
    const int k = blockIdx.x * RGF_THREADS + threadIdx.x;
    if (k >= nk) return;
    const cplx* a = A + (size_t)b * strideA;
    double s = 0.0;
    for (int r = 0; r < nr; ++r) {
        const cplx p = a[(size_t)r * nk + k], c = X[(size_t)r * nk + k];
        s += p.x * c.x + p.y * c.y;
    }
    const double two_pi = 6.28318530717958647692;
    site[(size_t)b * site_stride + k] += s / two_pi;
}

void launch_rgf_pop_block(hipStream_t st, int nr, int nk, int nb, const cplx* A, size_t strideA, const cplx* X,
                          double* row_site, bool accumulate_rows, double* col_site, size_t site_stride)
{
    if (nr <= 0 || nk <= 0 || nb <= 0) return;
    const int rows_per = RGF_THREADS / 64;
    hipLaunchKernelGGL(rgf_pop_rows_kernel, dim3((nr + rows_per - 1) / rows_per, nb), dim3(RGF_THREADS), 0, st, nr, nk, A,
                       strideA, X, row_site, site_stride, accumulate_rows ? 1 : 0);
    if (col_site)
        hipLaunchKernelGGL(rgf_pop_cols_kernel, dim3((nk + RGF_THREADS - 1) / RGF_THREADS, nb), dim3(RGF_THREADS), 0, st, nr,
                           nk, A, strideA, X, col_site, site_stride);
}

// info[b] = offset + linfo[b] for the first layer that reported a zero pivot
__global__ void rgf_merge_info_kernel(int nb, int offset, const int* __restrict__ linfo, int* __restrict__ info)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nb && info[b] == 0 && linfo[b] != 0) info[b] = offset + linfo[b];
}

void launch_rgf_merge_info(hipStream_t st, int nb, int offset, const int* linfo, int* info)
{
    hipLaunchKernelGGL(rgf_merge_info_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, nb, offset, linfo, info);
}

// ------------------------------------------------------------ probes of a layer into its assembled matrix
// D[b][I_p, I_p] -= Sigma_p for the probes order[0 .. n_probes) (terminal numbers) of ONE layer, one after the other in
// that order (the host sorts them by content: overlapping probes meet in an order the caller's listing does not change).
// One workgroup per energy; inside a probe the indices are distinct, so every element is touched by one thread.
// rows: the probes' orbitals counted inside the layer, at ioff[t]; sig: their blocks, at soff[t], the same for all energies.
__global__ __launch_bounds__(RGF_THREADS) void rgf_sub_probes_kernel(
    int n, int n_probes, const int* __restrict__ order, const int* __restrict__ tK, const int* __restrict__ ioff,
    const int* __restrict__ soff, const int* __restrict__ rows, const cplx* __restrict__ sig, cplx* __restrict__ D,
    size_t strideD)
{
    cplx* Db = D + (size_t)blockIdx.x * strideD;
    for (int q = 0; q < n_probes; ++q) {
        const int t = order[q];
        const int K = tK[t];
        const int* I = rows + ioff[t];
        const cplx* s = sig + soff[t];
        for (int e = threadIdx.x; e < K * K; e += RGF_THREADS) {
            const int i = e / K, j = e - i * K;
            const size_t at = (size_t)I[i] * n + I[j];
            Db[at] = csub(Db[at], s[e]);
        }
        __syncthreads();
    }
}

void launch_rgf_sub_probes(hipStream_t st, int n, int n_probes, int nb, const int* order, const int* tK, const int* ioff,
                           const int* soff, const int* rows, const cplx* sig, cplx* D, size_t strideD)
{
    if (n_probes <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(rgf_sub_probes_kernel, dim3(nb), dim3(RGF_THREADS), 0, st, n, n_probes, order, tK, ioff, soff, rows,
                       sig, D, strideD);
}

// ------------------------------------------------------------ one terminal pair per workgroup, G_ab read from a strip
// T[b][a][b'] = Re sum_ij (Gamma_a G_ab Gamma_b')_ij conj(G_ab,ij) for the pairs (a * C + b') of one layer level and one
// class (tmat_pair_class).  G_ab,ij = strip[b][rows_a[i]][tcol[b'] - col0 + cpos_b'[j]]: a's orbitals are rows of the
// level's layer, b''s orbitals columns of the strip through their position in the union list of b''s layer (cpos) and
// that list's first column (tcol[b'] - col0).  Gamma_t: gstat + goff[t] where gstride[t] = 0, gdyn + b gstride[t] + goff[t]
// otherwise.  LDS and every summation order are tmat_pair_kernel's (k_tmatrix.hip): element t = i K_b + j belongs to thread
// t mod THREADS, which adds its elements in ascending t, the k sums run in ascending k, and the threads' sums meet in a
// binary tree over the thread index.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void rgf_strip_pair_kernel(
    int C, const int* __restrict__ pairs, const int* __restrict__ tK, const int* __restrict__ ioff,
    const int* __restrict__ goff, const int* __restrict__ gstride, const int* __restrict__ tcol, int col0,
    const int* __restrict__ rows, const int* __restrict__ cpos, const cplx* __restrict__ strip, int ld, size_t strideS,
    const cplx* __restrict__ gstat, const cplx* __restrict__ gdyn, double* __restrict__ T)
{
    extern __shared__ cplx rgf_pair_lds[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int pr = pairs[blockIdx.x];
    const int ta = pr / C, tb = pr - ta * C;
    const int Ka = tK[ta], Kb = tK[tb], ne = Ka * Kb;
    cplx* sG = rgf_pair_lds;
    cplx* sX = sG + ne;
    double* red = reinterpret_cast<double*>(sX + ne);
    const int* Ia = rows + ioff[ta];
    const int* Jb = cpos + ioff[tb];
    const cplx* Sb = strip + (size_t)b * strideS + (tcol[tb] - col0);
    const cplx* Ga = gstride[ta] ? gdyn + (size_t)b * gstride[ta] + goff[ta] : gstat + goff[ta];
    const cplx* Gm = gstride[tb] ? gdyn + (size_t)b * gstride[tb] + goff[tb] : gstat + goff[tb];
    for (int t = tid; t < ne; t += THREADS) {
        const int i = t / Kb, j = t - i * Kb;
        sG[t] = Sb[(size_t)Ia[i] * ld + Jb[j]];
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

void launch_rgf_strip_pairs(hipStream_t st, int cls, int C, int npairs, int max_elems, int nb, const int* pairs,
                            const int* tK, const int* ioff, const int* goff, const int* gstride, const int* tcol, int col0,
                            const int* rows, const int* cpos, const cplx* strip, int ld, size_t strideS, const cplx* gstat,
                            const cplx* gdyn, double* T)
{
    if (npairs <= 0 || nb <= 0) return;
    if (cls == 1) {
        const size_t lds = (size_t)2 * max_elems * sizeof(cplx) + 64 * sizeof(double);
        hipLaunchKernelGGL(rgf_strip_pair_kernel<64>, dim3(npairs, nb), dim3(64), lds, st, C, pairs, tK, ioff, goff, gstride,
                           tcol, col0, rows, cpos, strip, ld, strideS, gstat, gdyn, T);
    } else {
        const size_t lds = (size_t)2 * max_elems * sizeof(cplx) + 256 * sizeof(double);
        hipLaunchKernelGGL(rgf_strip_pair_kernel<256>, dim3(npairs, nb), dim3(256), lds, st, C, pairs, tK, ioff, goff,
                           gstride, tcol, col0, rows, cpos, strip, ld, strideS, gstat, gdyn, T);
    }
}

// ------------------------------------------------------------ bond currents and local transmission on the pattern of S
// flow[r][c](E) = 2 Im[K_rc conj(A_rc)], K = E S - F formed in registers in rgf_diag's operation order (k_bond.hip's
// bond_flow on a layered system; negf_layered_local_transmission, negf_layered_bond_int).  The row-major kernels serve a
// diagonal block and an upper block (i, i+1): element (r, c) of the result needs element (r, c) of S, F and A.  The lower
// block (i+1, i) is 2 Im[K_l[r][c] A_u[c][r]] (A_{i+1,i} = A_{i,i+1}^H is never formed): its kernels read the stored lower
// blocks of S and F at the element they write and A_u through rgf_accumulate_ct's padded 16 x 16 LDS tile, so that the read
// of A_u and the write of the result both run along rows.  A singular energy (info != 0) gives a NaN table.  No atomics:
// every sum below has ONE order.  The flow itself is formed without FP contraction, so that every kernel here gives the
// same bits for the same element (one-hot weights of the integral reproduce the per-energy table).
static __device__ __forceinline__ double rgf_bond_flow(const cplx e, const cplx s, const cplx h, const cplx a)
{
#pragma clang fp contract(off)
    const double kx = e.x * s.x - e.y * s.y - h.x;
    const double ky = e.x * s.y + e.y * s.x - h.y;
    return 2.0 * (ky * a.x - kx * a.y);
}

// out[b][i] = flow(E_b, S[i], F[i], A_b[i]) over `count` elements
__global__ __launch_bounds__(RGF_THREADS) void rgf_bond_flow_kernel(
    int count, const cplx* __restrict__ E, const cplx* __restrict__ S, const cplx* __restrict__ F,
    const cplx* __restrict__ A, size_t strideA, const int* __restrict__ info, double* __restrict__ out, size_t stride_out)
{
    const int b = blockIdx.y;
    const cplx e = E[b];
    const cplx* Ab = A + (size_t)b * strideA;
    double* o = out + (size_t)b * stride_out;
    const bool bad = info[b] != 0;                                     // (uniform)
    const double qnan = __builtin_nan("");
    for (int i = blockIdx.x * RGF_THREADS + threadIdx.x; i < count; i += gridDim.x * RGF_THREADS)
        o[i] = bad ? qnan : rgf_bond_flow(e, S[i], F[i], Ab[i]);
}

void launch_rgf_bond_flow(hipStream_t st, int count, int nb, const cplx* E, const cplx* S, const cplx* F, const cplx* A,
                          size_t strideA, const int* info, double* out, size_t stride_out)
{
    if (count <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(rgf_bond_flow_kernel, dim3(rgf_grid((size_t)count), nb), dim3(RGF_THREADS), 0, st, count, E, S, F, A,
                       strideA, info, out, stride_out);
}

// out[b][c][r] = 2 Im[K_l[c][r] A_b[r][c]]   (A nr x nc: the upper block; Sl, Fl, out nc x nr: the lower one)
__global__ __launch_bounds__(RGF_CT_TILE * RGF_CT_TILE) void rgf_bond_flow_t_kernel(
    int nr, int nc, const cplx* __restrict__ E, const cplx* __restrict__ Sl, const cplx* __restrict__ Fl,
    const cplx* __restrict__ A, size_t strideA, const int* __restrict__ info, double* __restrict__ out, size_t stride_out)
{
    __shared__ double tre[RGF_CT_TILE][RGF_CT_TILE + 1], tim[RGF_CT_TILE][RGF_CT_TILE + 1];
    const int b = blockIdx.z;
    const int tx = threadIdx.x & (RGF_CT_TILE - 1), ty = threadIdx.x / RGF_CT_TILE;
    const int r0 = blockIdx.y * RGF_CT_TILE, c0 = blockIdx.x * RGF_CT_TILE;
    const bool in_ok = r0 + ty < nr && c0 + tx < nc;        // A[r0 + ty][c0 + tx]
    const bool out_ok = c0 + ty < nc && r0 + tx < nr;       // out[c0 + ty][r0 + tx]
    const size_t in_at = (size_t)(r0 + ty) * nc + c0 + tx, out_at = (size_t)(c0 + ty) * nr + r0 + tx;
    if (in_ok) { const cplx x = A[(size_t)b * strideA + in_at]; tre[ty][tx] = x.x; tim[ty][tx] = x.y; }
    __syncthreads();
    if (!out_ok) return;
    double* o = out + (size_t)b * stride_out;
    if (info[b] != 0) { o[out_at] = __builtin_nan(""); return; }
    // 2 Im[K a] = 2 Im[K conj(conj(a))]
    o[out_at] = rgf_bond_flow(E[b], Sl[out_at], Fl[out_at], cmake(tre[tx][ty], -tim[tx][ty]));
}

void launch_rgf_bond_flow_t(hipStream_t st, int nr, int nc, int nb, const cplx* E, const cplx* Sl, const cplx* Fl,
                            const cplx* A, size_t strideA, const int* info, double* out, size_t stride_out)
{
    if (nr <= 0 || nc <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(rgf_bond_flow_t_kernel,
                       dim3((nc + RGF_CT_TILE - 1) / RGF_CT_TILE, (nr + RGF_CT_TILE - 1) / RGF_CT_TILE, nb),
                       dim3(RGF_CT_TILE * RGF_CT_TILE), 0, st, nr, nc, E, Sl, Fl, A, strideA, info, out, stride_out);
}

// Group table of one block, bond_group_kernel's scheme with a map per layer: one workgroup per (energy b, row group a).
// rperm / cperm: the orbitals of the block's row / column layer sorted by group (ascending inside a group), rgoff / cgoff
// [groups + 1]: where each group starts.  Pass 1: thread q owns the column cperm[q] and adds the rows of group a in rperm
// order -> colsum[q] in LDS.  Pass 2: a wave per column group g: lane l adds colsum[cgoff[g] + l], [.. + l + 64], ... in
// order, then the 6-step shuffle tree.  The order of every addition depends on the positions inside the groups only:
// relabelling the groups permutes the table bit for bit.
// lower = 0: out[a][g] of the block itself (diagonal, upper).  lower = 1: A is the upper block (i, i+1) and the table is
// the lower block's, out[g][a] = sum_{c in g, r in a} 2 Im[K_l[c][r] A[r][c]]; K_l[c][r] is read as conj of the upper S
// and F at [r][c] -- the stored lower blocks are those conjugates bit for bit (negf_layered_create) -- so that this read
// runs along the rows of A as well.
template <int LOWER>
__global__ __launch_bounds__(RGF_THREADS) void rgf_bond_group_kernel(
    int nc, int ngr, int ngc, const cplx* __restrict__ E, const cplx* __restrict__ S, const cplx* __restrict__ F,
    const cplx* __restrict__ A, size_t strideA, const int* __restrict__ info, const int* __restrict__ rperm,
    const int* __restrict__ rgoff, const int* __restrict__ cperm, const int* __restrict__ cgoff,
    double* __restrict__ out, size_t stride_out)
{
    extern __shared__ double rgf_bond_colsum[];             // [nc]
    const int b = blockIdx.x, a = blockIdx.y, tid = threadIdx.x;
    double* o = out + (size_t)b * stride_out;
    const size_t o_at = LOWER ? (size_t)a : (size_t)a * ngc, o_step = LOWER ? (size_t)ngr : 1;
    if (info[b] != 0) {                                     // (uniform)
        const double qnan = __builtin_nan("");
        for (int g = tid; g < ngc; g += RGF_THREADS) o[o_at + g * o_step] = qnan;
        return;
    }
    const cplx e = E[b];
    const cplx* Ab = A + (size_t)b * strideA;
    const int r0 = rgoff[a], r1 = rgoff[a + 1];
    for (int q = tid; q < nc; q += RGF_THREADS) {
        const int j = cperm[q];
        double acc = 0.0;
#pragma unroll 4
        for (int r = r0; r < r1; ++r) {
            const size_t t = (size_t)rperm[r] * nc + j;
            const cplx s = S[t], h = F[t], x = Ab[t];
            acc += LOWER ? rgf_bond_flow(e, cmake(s.x, -s.y), cmake(h.x, -h.y), cmake(x.x, -x.y)) : rgf_bond_flow(e, s, h, x);
        }
        rgf_bond_colsum[q] = acc;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int g = wave; g < ngc; g += RGF_THREADS / 64) {
        double s = 0.0;
        for (int q = cgoff[g] + lane; q < cgoff[g + 1]; q += 64) s += rgf_bond_colsum[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) o[o_at + g * o_step] = s;
    }
}

void launch_rgf_bond_group(hipStream_t st, int nc, int ngr, int ngc, int nb, bool lower, const cplx* E, const cplx* S,
                           const cplx* F, const cplx* A, size_t strideA, const int* info, const int* rperm, const int* rgoff,
                           const int* cperm, const int* cgoff, double* out, size_t stride_out)
{
    if (nc <= 0 || ngr <= 0 || ngc <= 0 || nb <= 0) return;
    const size_t lds = (size_t)nc * sizeof(double);         // a layer holds at most 8192 orbitals: 64 KB
    if (lower)
        hipLaunchKernelGGL(rgf_bond_group_kernel<1>, dim3(nb, ngr), dim3(RGF_THREADS), lds, st, nc, ngr, ngc, E, S, F, A,
                           strideA, info, rperm, rgoff, cperm, cgoff, out, stride_out);
    else
        hipLaunchKernelGGL(rgf_bond_group_kernel<0>, dim3(nb, ngr), dim3(RGF_THREADS), lds, st, nc, ngr, ngc, E, S, F, A,
                           strideA, info, rperm, rgoff, cperm, cgoff, out, stride_out);
}

// acc[i] += sum_b w_b flow(E_b, S[i], F[i], A_b[i]) with real w: rgf_accumulate's rule, one chain per element with b
// ascending, carried through acc from batch to batch -- bitwise independent of the batch cut
__global__ __launch_bounds__(RGF_THREADS) void rgf_bond_accumulate_kernel(
    int count, int nb, const cplx* __restrict__ E, const double* __restrict__ w, const cplx* __restrict__ S,
    const cplx* __restrict__ F, const cplx* __restrict__ A, size_t strideA, double* __restrict__ acc)
{
    const int i = blockIdx.x * RGF_THREADS + threadIdx.x;
    if (i >= count) return;
    const cplx s = S[i], h = F[i];
    double v = acc[i];
    for (int b = 0; b < nb; ++b) v += w[b] * rgf_bond_flow(E[b], s, h, A[(size_t)b * strideA + i]);
    acc[i] = v;
}

void launch_rgf_bond_accumulate(hipStream_t st, int count, int nb, const cplx* E, const double* w, const cplx* S,
                                const cplx* F, const cplx* A, size_t strideA, double* acc)
{
    if (count <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(rgf_bond_accumulate_kernel, dim3((count + RGF_THREADS - 1) / RGF_THREADS), dim3(RGF_THREADS), 0, st,
                       count, nb, E, w, S, F, A, strideA, acc);
}

// acc[c][r] += sum_b w_b 2 Im[K_l[c][r](E_b) A_b[r][c]]   (A nr x nc, Sl, Fl, acc nc x nr): the lower block's chain
__global__ __launch_bounds__(RGF_CT_TILE * RGF_CT_TILE) void rgf_bond_accumulate_t_kernel(
    int nr, int nc, int nb, const cplx* __restrict__ E, const double* __restrict__ w, const cplx* __restrict__ Sl,
    const cplx* __restrict__ Fl, const cplx* __restrict__ A, size_t strideA, double* __restrict__ acc)
{
    __shared__ double tre[RGF_CT_TILE][RGF_CT_TILE + 1], tim[RGF_CT_TILE][RGF_CT_TILE + 1];
    const int tx = threadIdx.x & (RGF_CT_TILE - 1), ty = threadIdx.x / RGF_CT_TILE;
    const int r0 = blockIdx.y * RGF_CT_TILE, c0 = blockIdx.x * RGF_CT_TILE;
    const bool in_ok = r0 + ty < nr && c0 + tx < nc;        // A[r0 + ty][c0 + tx]
    const bool out_ok = c0 + ty < nc && r0 + tx < nr;       // acc[c0 + ty][r0 + tx]
    const size_t in_at = (size_t)(r0 + ty) * nc + c0 + tx, out_at = (size_t)(c0 + ty) * nr + r0 + tx;
    cplx s = cmake(0.0, 0.0), h = s;
    double v = 0.0;
    if (out_ok) { s = Sl[out_at]; h = Fl[out_at]; v = acc[out_at]; }
    for (int b = 0; b < nb; ++b) {
        if (in_ok) { const cplx x = A[(size_t)b * strideA + in_at]; tre[ty][tx] = x.x; tim[ty][tx] = x.y; }
        __syncthreads();
        if (out_ok) v += w[b] * rgf_bond_flow(E[b], s, h, cmake(tre[tx][ty], -tim[tx][ty]));
        __syncthreads();
    }
    if (out_ok) acc[out_at] = v;
}

void launch_rgf_bond_accumulate_t(hipStream_t st, int nr, int nc, int nb, const cplx* E, const double* w, const cplx* Sl,
                                  const cplx* Fl, const cplx* A, size_t strideA, double* acc)
{
    if (nr <= 0 || nc <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(rgf_bond_accumulate_t_kernel,
                       dim3((nc + RGF_CT_TILE - 1) / RGF_CT_TILE, (nr + RGF_CT_TILE - 1) / RGF_CT_TILE),
                       dim3(RGF_CT_TILE * RGF_CT_TILE), 0, st, nr, nc, nb, E, w, Sl, Fl, A, strideA, acc);
}

// A[b] = (A[b] + A[b]^H) / 2 in place (n x n): the Hermitian part of a diagonal block A_ii = (W Gamma) W^H, which is
// Hermitian only to the rounding of its products.  One workgroup per pair of mirrored 16 x 16 tiles (bx >= by; the others
// leave at once), both tiles through the padded LDS tile so that every read and write runs along rows.  Element (r, c)
// and element (c, r) are formed from the same two numbers by commutative sums: exact conjugates of each other.
__global__ __launch_bounds__(RGF_CT_TILE * RGF_CT_TILE) void rgf_bond_hermitize_kernel(int n, cplx* __restrict__ A, size_t strideA)
{
    __shared__ double ure[RGF_CT_TILE][RGF_CT_TILE + 1], uim[RGF_CT_TILE][RGF_CT_TILE + 1];   // the tile (by, bx)
    __shared__ double lre[RGF_CT_TILE][RGF_CT_TILE + 1], lim[RGF_CT_TILE][RGF_CT_TILE + 1];   // the tile (bx, by)
    if (blockIdx.x < blockIdx.y) return;                   // (uniform)
    const int tx = threadIdx.x & (RGF_CT_TILE - 1), ty = threadIdx.x / RGF_CT_TILE;
    const int r0 = blockIdx.y * RGF_CT_TILE, c0 = blockIdx.x * RGF_CT_TILE;
    cplx* Ab = A + (size_t)blockIdx.z * strideA;
    const bool u_ok = r0 + ty < n && c0 + tx < n;          // A[r0 + ty][c0 + tx]
    const bool l_ok = c0 + ty < n && r0 + tx < n;          // A[c0 + ty][r0 + tx]
    const size_t u_at = (size_t)(r0 + ty) * n + c0 + tx, l_at = (size_t)(c0 + ty) * n + r0 + tx;
    if (u_ok) { const cplx x = Ab[u_at]; ure[ty][tx] = x.x; uim[ty][tx] = x.y; }
    if (l_ok) { const cplx x = Ab[l_at]; lre[ty][tx] = x.x; lim[ty][tx] = x.y; }
    __syncthreads();
    // (on a diagonal tile pair both stores write the same tile with the same values)
    if (u_ok) Ab[u_at] = cmake(0.5 * (ure[ty][tx] + lre[tx][ty]), 0.5 * (uim[ty][tx] - lim[tx][ty]));
    if (l_ok) Ab[l_at] = cmake(0.5 * (lre[ty][tx] + ure[tx][ty]), 0.5 * (lim[ty][tx] - uim[tx][ty]));
}

void launch_rgf_bond_hermitize(hipStream_t st, int n, int nb, cplx* A, size_t strideA)
{
    if (n <= 0 || nb <= 0) return;
    const int t = (n + RGF_CT_TILE - 1) / RGF_CT_TILE;
    hipLaunchKernelGGL(rgf_bond_hermitize_kernel, dim3(t, t, nb), dim3(RGF_CT_TILE * RGF_CT_TILE), 0, st, n, A, strideA);
}
