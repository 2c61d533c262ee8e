// 1-D chain contact self-energy by renormalisation-decimation ("doubling", Lopez Sancho - Rubio).  gfx950.
// The opt-in second solver for the surface Green's function that gauNEGF/surfG1D.py:223-295 finds with the relaxed
// fixed-point loop (k_chain1d_rs.hip / k_chain1d.hip: the default).
//
//   A = (E + i eta) Sa - a ;  B = (E + i eta) Sb - b                 (z = E + i eta formed in float64)
//   es = e = A,  a = B,  b = B^H  (b as a MATRIX: it conjugates the complex energy, as surfG1D.py:262 does)
//   step:  G = inv(e);  P = a G;  Q = b G;  D = P b
//          es <- es - D;   e <- (e - D) - Q a;   a <- P a;   b <- Q b;   steps += 1
//   stop after the step in which  max |D_ij| <= tol * max |es_ij|  (es already updated), or at max_steps;
//          |x| = |re| + |im| (the izamax metric of the pivot search): a relative test, exact under power-of-two scaling
//   g = inv(es);   Sigma = t g t^H,  t = E Stau - tau  (no eta)
//
// Step k of the recursion is iterate 2^k - 1 of the UNRELAXED loop g <- inv(A - B g B^H) started from inv(A): the
// same semi-infinite chain, built by doubling its length instead of adding one cell.  force_steps >= 0 runs exactly that
// many steps (0: g = inv(A)).  A unit that reaches max_steps reports converged = 0 and returns what it has; non-finite
// input or a zero pivot propagates as NaN and reports converged = 0 (the maxima of the stop rule keep a NaN).
//
// One UNIT is one (energy, contact); one workgroup (256 threads) runs a unit from A, B to Sigma without going back to the
// host, and every unit stops on its own step count.
//
// n_c <= 64 (chain1d_rd_kernel): the matrix being inverted sits in LDS and is inverted by the blocked Gauss-Jordan of the
// fixed-point kernel (chain_rs_inverse.h: partial pivoting, izamax metric, pivot rows replaced, not updated).  The state --
// es, e, a, b (a, b double-buffered), G, P, Q: nine matrices of pitch NP = 16 ceil(n/16), padding zero -- lives in a
// workspace in global memory that belongs to the RESIDENT SLOT, not to the unit: the launch is one persistent workgroup
// per slot, which takes units slot, slot + slots, ... (units differ by at most a factor two in length: no queue).  The six
// products of a step run on v_mfma_f64_16x16x4_f64 in the 3-real-product form (mfma3); wave w owns row tile w of every
// product, and every element of es / e is owned by one lane, which updates it in place.  Two workgroups share a CU:
// the LDS matrix is at most 66.8 KB (pitch 65), and __launch_bounds__(256, 2) leaves each wave 256 VGPRs (a product
// holds 3 x T16 accumulator tiles = 96 VGPRs at T16 = 4, plus the operand fragments of a k-step).
//
// n_c > 64 (chain1d_rd_global_kernel): the same recursion from the workgroup routines of the global fixed-point kernel
// (chain_wg.h), state in global memory, one workgroup per unit.  Correct, not tuned.
#include "negf_common.h"
#include "chain_rs_inverse.h"
#include "chain_wg.h"
#include <algorithm>

namespace {

struct ChainRdArgs {
    const cplx *alpha, *Salpha, *beta, *Sbeta, *tau, *Stau;   // concatenated per contact
    const int* nc;
    const int* blk_off;
    int n_contacts, blk_stride;
    double eta, tol;
    int max_steps, force_steps;
    int units;                       // energies * contacts
    cplx* ws;                        // workspace: [slots][ws_per_slot] (LDS kernel), [units][ws_per_slot] (global kernel)
    size_t ws_per_slot;
    cplx* gcache;                    // g(E) cache, as in the fixed-point kernel: gc_mode 1 = store the final g, 2 = load it and
    int gc_mode;                     //   only form Sigma (the same instructions on the same operands as the last pass of a miss)
};

// maximum that keeps a NaN: the stop rule must not pass because fmax dropped one
__device__ __forceinline__ double rd_nanmax(double x, double y) { return (y > x || y != y) ? y : x; }

// both maxima over the workgroup; red: [2 * RS_WAVES] LDS.  Ends with the values in every thread.
__device__ __forceinline__ void rd_reduce2(double& u, double& v, double* red, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        u = rd_nanmax(u, __shfl_xor(u, o, 64));
        v = rd_nanmax(v, __shfl_xor(v, o, 64));
    }
    __syncthreads();                                     // (red is free: every thread has read the previous result)
    if (lane == 0) { red[wave] = u; red[RS_WAVES + wave] = v; }
    __syncthreads();
    u = red[0]; v = red[RS_WAVES];
#pragma unroll
    for (int w = 1; w < RS_WAVES; ++w) { u = rd_nanmax(u, red[w]); v = rd_nanmax(v, red[RS_WAVES + w]); }
}

// row tile `wave` of X Y on the matrix cores, 3M form: a = sum xr yr, b = sum xi yi, c = sum (xr + xi)(yr + yi).
// X, Y: global, pitch NP, zero outside n x n; ksteps = ceil(n / 4) <= NP / 4.
template <int T16, int NP>
__device__ __forceinline__ void rd_gemm_rowtile(const cplx* X, const cplx* Y, int ksteps, int wave, int lane,
                                                d4 (&ar)[T16], d4 (&ai)[T16], d4 (&ac)[T16])
{
    const int fi = lane & 15, fk = lane >> 4;
    const cplx* xa = X + (wave * 16 + fi) * NP + fk;
    const cplx* yb = Y + fk * NP + fi;
#pragma unroll
    for (int tj = 0; tj < T16; ++tj) { ar[tj] = (d4){0, 0, 0, 0}; ai[tj] = (d4){0, 0, 0, 0}; ac[tj] = (d4){0, 0, 0, 0}; }
#pragma unroll 1
    for (int ks = 0; ks < ksteps; ++ks) {
        const cplx pa = xa[ks * 4];
        cplx qb[T16];
#pragma unroll
        for (int tj = 0; tj < T16; ++tj) qb[tj] = yb[ks * 4 * NP + tj * 16];
        const double ps = pa.x + pa.y;
#pragma unroll
        for (int tj = 0; tj < T16; ++tj) mfma3(ar[tj], ai[tj], ac[tj], pa.x, pa.y, ps, qb[tj].x, qb[tj].y, qb[tj].x + qb[tj].y);
    }
}

// f(i, j, re, im) for every element of row tile `wave` this lane holds (C layout: rows fk + 4r, column fi of tile tj)
template <int T16, class F>
__device__ __forceinline__ void rd_for_rowtile(int n, int wave, int lane, const d4 (&ar)[T16], const d4 (&ai)[T16],
                                               const d4 (&ac)[T16], F f)
{
    const int fi = lane & 15, fk = lane >> 4;
#pragma unroll
    for (int tj = 0; tj < T16; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = wave * 16 + fk + 4 * r, j = tj * 16 + fi;
            if (i < n && j < n) f(i, j, ar[tj][r] - ai[tj][r], ac[tj][r] - ar[tj][r] - ai[tj][r]);
        }
}

template <int P>
__global__ __launch_bounds__(RS_THREADS, 2) void chain1d_rd_kernel(
    ChainRdArgs a, const cplx* __restrict__ E, cplx* __restrict__ blk, int* __restrict__ iters,
    int* __restrict__ converged)
{
    constexpr int T16 = (P - 1 + 15) / 16;
    constexpr int NP = 16 * T16;                         // pitch of the state matrices in global memory
    constexpr int NP2 = NP * NP;
    constexpr int WELEMS = 16 * T16 * P + 16;            // the LDS matrix of rs_inverse (pitch P, a few elements of slack)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ int pivrow[64], colof[64];
    __shared__ cplx rowline[RS_NB];
    __shared__ double red[2 * RS_WAVES];
    cplx* Ws = reinterpret_cast<cplx*>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    cplx* base = a.ws + (size_t)blockIdx.x * a.ws_per_slot;
    cplx* ES = base;
    cplx* EP = ES + NP2;
    cplx* Gm = EP + NP2;
    cplx* PM = Gm + NP2;
    cplx* QM = PM + NP2;
    cplx* ab[2] = {QM + NP2, QM + 2 * NP2};
    cplx* bb[2] = {QM + 3 * NP2, QM + 4 * NP2};

    // W (LDS) <- src; W <- reduced form; Gm <- inv(src).  colof is -1 on entry and on return.
    auto invert = [&](int n, const cplx* src) __attribute__((always_inline)) {
        for (int t = tid; t < n * n; t += RS_THREADS) { const int i = t / n, j = t - i * n; Ws[i * P + j] = src[i * NP + j]; }
        __syncthreads();
        rs_inverse<T16, P, -1>(n, Ws, pivrow, colof, rowline, tid, wave, false);
        for (int t = tid; t < n * n; t += RS_THREADS) { const int i = t / n, j = t - i * n; Gm[i * NP + j] = Ws[pivrow[i] * P + colof[j]]; }
        __syncthreads();
        if (tid < 64) colof[tid] = -1;
        __syncthreads();
    };
    // Z <- X Y (guarded stores: the padding of Z stays zero)
    auto product = [&](int n, int ksteps, const cplx* X, const cplx* Y, cplx* Z) __attribute__((always_inline)) {
        if (wave < T16 && wave * 16 < n) {
            d4 ar[T16], ai[T16], ac[T16];
            rd_gemm_rowtile<T16, NP>(X, Y, ksteps, wave, lane, ar, ai, ac);
            rd_for_rowtile<T16>(n, wave, lane, ar, ai, ac, [&](int i, int j, double re, double im) { Z[i * NP + j] = cmake(re, im); });
        }
    };

    int n_prev = -1;
    for (int unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        const int c = unit % a.n_contacts, b = unit / a.n_contacts;
        const int n = a.nc[c], off = a.blk_off[c], ksteps = (n + 3) >> 2;
        if (n != n_prev) {
            // the padding of every matrix is zero and is never written: set once per slot (again when the contact size changes)
            __syncthreads();
            for (int t = tid; t < 9 * NP2; t += RS_THREADS) base[t] = cmake(0.0, 0.0);
            for (int t = tid; t < WELEMS; t += RS_THREADS) Ws[t] = cmake(0.0, 0.0);
            if (tid < 64) { colof[tid] = -1; pivrow[tid] = 0; }
            n_prev = n;
        }
        __syncthreads();
        const cplx e = E[b];
        const cplx z = cmake(e.x, e.y + a.eta);
        const bool hit = a.gc_mode == 2;
        int cur = 0, steps = 0;
        bool conv = false;
        if (!hit) {
            for (int t = tid; t < n * n; t += RS_THREADS) {
                const int i = t / n, j = t - i * n;
                const cplx Av = csub(cmul(z, a.Salpha[off + t]), a.alpha[off + t]);
                const cplx Bv = csub(cmul(z, a.Sbeta[off + t]), a.beta[off + t]);
                ES[i * NP + j] = Av; EP[i * NP + j] = Av;
                ab[0][i * NP + j] = Bv; bb[0][j * NP + i] = cconj(Bv);
            }
            __syncthreads();
            while (a.force_steps >= 0 ? steps < a.force_steps : (!conv && steps < a.max_steps)) {
                const cplx *av = ab[cur], *bv = bb[cur];
                invert(n, EP);                               // G = inv(e)
                product(n, ksteps, av, Gm, PM);              // P = a G
                product(n, ksteps, bv, Gm, QM);              // Q = b G
                __syncthreads();
                double dmax = 0.0, emax = 0.0;
                if (wave < T16 && wave * 16 < n) {
                    d4 ar[T16], ai[T16], ac[T16];
                    rd_gemm_rowtile<T16, NP>(PM, bv, ksteps, wave, lane, ar, ai, ac);        // D = P b
                    rd_for_rowtile<T16>(n, wave, lane, ar, ai, ac, [&](int i, int j, double re, double im) {
                        const cplx s = ES[i * NP + j], p = EP[i * NP + j];
                        const cplx sn = cmake(s.x - re, s.y - im);
                        ES[i * NP + j] = sn; EP[i * NP + j] = cmake(p.x - re, p.y - im);
                        dmax = rd_nanmax(dmax, fabs(re) + fabs(im));
                        emax = rd_nanmax(emax, cabs1(sn));
                    });
                    rd_gemm_rowtile<T16, NP>(QM, av, ksteps, wave, lane, ar, ai, ac);        // Q a
                    rd_for_rowtile<T16>(n, wave, lane, ar, ai, ac, [&](int i, int j, double re, double im) {
                        const cplx p = EP[i * NP + j];
                        EP[i * NP + j] = cmake(p.x - re, p.y - im);
                    });
                }
                product(n, ksteps, PM, av, ab[cur ^ 1]);     // a <- P a
                product(n, ksteps, QM, bv, bb[cur ^ 1]);     // b <- Q b
                rd_reduce2(dmax, emax, red, tid);
                cur ^= 1;
                ++steps;
                conv = dmax <= a.tol * emax && emax < INFINITY;
                __syncthreads();
            }
            invert(n, ES);                                   // g = inv(es)
            if (a.gc_mode == 1) {
                cplx* gcj = a.gcache + (size_t)b * a.blk_stride + off;
                for (int t = tid; t < n * n; t += RS_THREADS) { const int i = t / n; gcj[t] = Gm[i * NP + (t - i * n)]; }
            }
        } else {
            const cplx* gcj = a.gcache + (size_t)b * a.blk_stride + off;
            for (int t = tid; t < n * n; t += RS_THREADS) { const int i = t / n; Gm[i * NP + (t - i * n)] = gcj[t]; }
        }
        // Sigma = t g t^H, t = E Stau - tau: t and t^H take the places of a and b
        for (int t = tid; t < n * n; t += RS_THREADS) {
            const int i = t / n, j = t - i * n;
            const cplx tv = csub(cmul(e, a.Stau[off + t]), a.tau[off + t]);
            ab[cur][i * NP + j] = tv; bb[cur][j * NP + i] = cconj(tv);
        }
        __syncthreads();
        product(n, ksteps, ab[cur], Gm, PM);
        __syncthreads();
        if (wave < T16 && wave * 16 < n) {
            d4 ar[T16], ai[T16], ac[T16];
            rd_gemm_rowtile<T16, NP>(PM, bb[cur], ksteps, wave, lane, ar, ai, ac);
            cplx* out = blk + (size_t)b * a.blk_stride + off;
            rd_for_rowtile<T16>(n, wave, lane, ar, ai, ac, [&](int i, int j, double re, double im) { out[i * n + j] = cmake(re, im); });
        }
        if (tid == 0 && !hit) {                              // (a hit's counts and flags are copied from the cache by the caller)
            if (iters) iters[unit] = steps;
            if (converged) converged[unit] = conv ? 1 : 0;
        }
        __syncthreads();                                     // the slot's workspace is free for the next unit
    }
}

// ---- n_c > 64: state in global memory, one workgroup per unit (the routines of chain_wg.h)
__global__ __launch_bounds__(CH_THREADS) void chain1d_rd_global_kernel(
    ChainRdArgs a, const cplx* __restrict__ E, cplx* __restrict__ blk, int* __restrict__ iters,
    int* __restrict__ converged)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ double red_v[CH_THREADS / 64];
    __shared__ int red_i[CH_THREADS / 64];
    __shared__ int piv_row;
    __shared__ double red[2 * RS_WAVES];

    const int c = blockIdx.x, b = blockIdx.y;
    const int unit = b * a.n_contacts + c;
    const int n = a.nc[c], off = a.blk_off[c], n2 = n * n;
    const int tid = threadIdx.x;
    cplx* rowk = reinterpret_cast<cplx*>(smem_raw);
    cplx* colk = rowk + n;
    int* ipiv = reinterpret_cast<int*>(colk + n);

    cplx* ES = a.ws + (size_t)unit * a.ws_per_slot;
    cplx* EP = ES + n2;
    cplx* Am = EP + n2;
    cplx* Bm = Am + n2;
    cplx* Gm = Bm + n2;
    cplx* PM = Gm + n2;
    cplx* QM = PM + n2;
    cplx* T1 = QM + n2;
    cplx* T2 = T1 + n2;

    const cplx e = E[b];
    const cplx z = cmake(e.x, e.y + a.eta);
    for (int t = tid; t < n2; t += CH_THREADS) {
        const int i = t / n, j = t - i * n;
        const cplx Av = csub(cmul(z, a.Salpha[off + t]), a.alpha[off + t]);
        const cplx Bv = csub(cmul(z, a.Sbeta[off + t]), a.beta[off + t]);
        ES[t] = Av; EP[t] = Av; Am[t] = Bv; Bm[j * n + i] = cconj(Bv);
    }
    __syncthreads();
    int steps = 0;
    bool conv = false;
    while (a.force_steps >= 0 ? steps < a.force_steps : (!conv && steps < a.max_steps)) {
        for (int t = tid; t < n2; t += CH_THREADS) Gm[t] = EP[t];
        __syncthreads();
        wg_gj_inverse(n, Gm, rowk, colk, ipiv, red_v, red_i, &piv_row);
        __syncthreads();
        wg_zgemm(n, Am, Gm, 0, PM);
        wg_zgemm(n, Bm, Gm, 0, QM);
        __syncthreads();
        wg_zgemm(n, PM, Bm, 0, T1);                      // D
        wg_zgemm(n, QM, Am, 0, T2);                      // Q a
        __syncthreads();
        double dmax = 0.0, emax = 0.0;
        for (int t = tid; t < n2; t += CH_THREADS) {
            const cplx d = T1[t], q = T2[t], s = ES[t], p = EP[t];
            const cplx sn = cmake(s.x - d.x, s.y - d.y);
            ES[t] = sn;
            EP[t] = cmake((p.x - d.x) - q.x, (p.y - d.y) - q.y);
            dmax = rd_nanmax(dmax, cabs1(d));
            emax = rd_nanmax(emax, cabs1(sn));
        }
        rd_reduce2(dmax, emax, red, tid);
        wg_zgemm(n, PM, Am, 0, T1);
        wg_zgemm(n, QM, Bm, 0, T2);
        __syncthreads();
        for (int t = tid; t < n2; t += CH_THREADS) { Am[t] = T1[t]; Bm[t] = T2[t]; }
        __syncthreads();
        ++steps;
        conv = dmax <= a.tol * emax && emax < INFINITY;
    }
    for (int t = tid; t < n2; t += CH_THREADS) Gm[t] = ES[t];
    __syncthreads();
    wg_gj_inverse(n, Gm, rowk, colk, ipiv, red_v, red_i, &piv_row);
    for (int t = tid; t < n2; t += CH_THREADS) Am[t] = csub(cmul(e, a.Stau[off + t]), a.tau[off + t]);
    __syncthreads();
    wg_zgemm(n, Am, Gm, 0, T1);
    __syncthreads();
    wg_zgemm(n, T1, Am, 1, blk + (size_t)b * a.blk_stride + off);
    if (tid == 0) {
        if (iters) iters[unit] = steps;
        if (converged) converged[unit] = conv ? 1 : 0;
    }
}

int rd_slots()
{
    static int n_cus = 0;
    if (!n_cus) {
        int dev = 0; hipDeviceProp_t prop;
        n_cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 256;
    }
    return 2 * n_cus;                                        // two workgroups per CU (see the head of this file)
}
int rd_np(int nc_max) { return 16 * ((nc_max + 15) / 16); }

template <int P>
void chain1d_rd_launch(hipStream_t st, const ChainRdArgs& a, int grid, const cplx* E, cplx* blk, int* iters, int* conv)
{
    constexpr int T16 = (P - 1 + 15) / 16;
    const size_t smem = (size_t)(16 * T16 * P + 16) * sizeof(cplx);
    auto k = chain1d_rd_kernel<P>;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024) != hipSuccess)
        (void)hipGetLastError();
    hipLaunchKernelGGL(k, dim3(grid), dim3(RS_THREADS), smem, st, a, E, blk, iters, conv);
}

}  // namespace

// complex values of workspace a launch of nb energies needs (LDS kernel: per resident slot; global kernel: per unit)
size_t chain1d_rd_scratch_elems(int nc_max, int n_contacts, int nb)
{
    const size_t units = (size_t)n_contacts * nb;
    if (nc_max <= 64) return std::min(units, (size_t)rd_slots()) * 9 * rd_np(nc_max) * rd_np(nc_max);
    return units * 9 * nc_max * nc_max;
}

void launch_chain1d_rd(hipStream_t st, const SigmaProvider& p, const int* d_nc, const int* d_blk_off, int nb,
                       const cplx* E, cplx* blk, int* iters, int* conv, cplx* scratch, cplx* gcache, int gc_mode)
{
    ChainRdArgs a;
    a.alpha = p.d_alpha; a.Salpha = p.d_Salpha; a.beta = p.d_beta; a.Sbeta = p.d_Sbeta;
    a.tau = p.d_tau; a.Stau = p.d_Stau;
    a.nc = d_nc; a.blk_off = d_blk_off;
    a.n_contacts = p.n_contacts; a.blk_stride = p.blk_stride;
    a.eta = p.eta; a.tol = p.conv; a.max_steps = p.max_iter; a.force_steps = p.force_iters;
    a.units = p.n_contacts * nb;
    a.ws = scratch;
    a.gcache = gcache; a.gc_mode = gcache ? gc_mode : 0;
    const int n = p.nc_max;
    if (n > 64) {
        a.ws_per_slot = (size_t)9 * n * n;
        a.gcache = nullptr; a.gc_mode = 0;
        const size_t smem = (size_t)n * (2 * sizeof(cplx) + sizeof(int));
        hipLaunchKernelGGL(chain1d_rd_global_kernel, dim3(p.n_contacts, nb), dim3(CH_THREADS), smem, st, a, E, blk, iters, conv);
        return;
    }
    a.ws_per_slot = (size_t)9 * rd_np(n) * rd_np(n);
    const int grid = std::min(a.units, rd_slots());
    if (n <= 16) chain1d_rd_launch<17>(st, a, grid, E, blk, iters, conv);
    else if (n <= 32) chain1d_rd_launch<33>(st, a, grid, E, blk, iters, conv);
    else if (n <= 48) chain1d_rd_launch<49>(st, a, grid, E, blk, iters, conv);
    else chain1d_rd_launch<65>(st, a, grid, E, blk, iters, conv);
}
