// Transmission eigenchannels (negf_transmission_channels, negf_eigvalsh_batched): two one-workgroup-per-matrix kernels
// with the matrix held in LDS.
//
//   pchol_kernel   pivoted Cholesky of a PSD block, Gamma = L L^H, truncated where the largest remaining diagonal is
//                  <= 1e-14 max diag Gamma; writes L^H (rows >= rank zero) and the rank.
//   jacobi_kernel  eigenvalues of a Hermitian K x K matrix, K <= 96: cyclic two-sided complex Jacobi in round-robin
//                  ordering.  A step applies K/2 disjoint rotations at once: one lane per pair forms its rotation
//                  (the phase of a_pq is removed, then a real rotation zeroes it), then every 2 x 2 block (P, Q) of
//                  pairs, P <= Q, is replaced by J_P^H A_PQ J_Q and its mirror -- the matrix stays exactly Hermitian.
//                  Stops when off(A)^2 <= (eps ||A||_F)^2 (eps = DBL_EPSILON, off summed directly: the difference
//                  ||A||^2 - ||diag||^2 cancels to sqrt(eps)) or after JAC_MAX_SWEEPS sweeps (flagged in info).
//                  The matrix is first scaled by a power of two (exact) to a largest entry in [1/2, 1).
//
// LDS: the matrix at row pitch Kpad + 1 (Kpad = K rounded up to even): an odd pitch in 16-byte elements puts the 16
// lanes of a ds_read_b128 group that read one column on 16 different bank slots.  96 x 97 x 16 B = 145.5 KB fits the
// 160 KB of a CU; with the ~5.5 KB of static LDS, K <= 54 fits three workgroups per CU, K <= 64 two (LDS is the
// limiter: 88 VGPRs would allow five workgroups of four waves).
#include "negf_common.h"
#include <atomic>
#include <cfloat>

namespace {

constexpr int CH_THREADS = 256;
constexpr int JAC_MAX_SWEEPS = 30;
constexpr int CH_KMAX = 96;
constexpr int CH_PMAX = CH_KMAX / 2;

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over the workgroup; every thread gets the result (red: CH_THREADS / 64 doubles of LDS)
__device__ __forceinline__ double block_sum(double v, double* red)
{
    v = wave_sum(v);
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wid] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < CH_THREADS / 64; ++k) s += red[k];
    __syncthreads();
    return s;
}

// maximum over the workgroup (non-negative values); every thread gets the result
__device__ __forceinline__ double block_max(double v, double* red)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wid] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < CH_THREADS / 64; ++k) s = fmax(s, red[k]);
    __syncthreads();
    return s;
}

// round-robin (circle) schedule on N players, N even: in step st player N-1 meets st, and (st + P) meets (st - P)
__device__ __forceinline__ void rr_pair(int st, int P, int N, int* p, int* q)
{
    const int M = N - 1;
    if (P == 0) { *p = M; *q = st; return; }
    *p = (st + P) % M;
    *q = (st - P + M) % M;
}

struct JacPair { int p, q; double c, s, tb; cplx w; };

// w[b * ldw + 0 .. nout): eigenvalues of the Hermitian matrix in the lower triangle of A[b] (the leading r x r block,
// r = rank ? rank[b * rank_stride] : K), ascending (descending = 0) or descending; positions r .. nout are exact zeros.
// info: chk_in -> an energy whose info is already nonzero gets a NaN row and keeps its info; otherwise info[b] =
// flag_sign * (1: non-finite input, NaN row; 2: not converged), 0 when converged.
__global__ __launch_bounds__(CH_THREADS) void jacobi_kernel(int K, int pitch, const cplx* __restrict__ A, int lda,
                                                            size_t strideA, const int* __restrict__ rank, int rank_stride,
                                                            double* __restrict__ w,
                                                            int ldw, int nout, int descending, int* __restrict__ info,
                                                            int chk_in, int flag_sign)
{
    extern __shared__ cplx M[];                    // [N][pitch]
    __shared__ JacPair pr[CH_PMAX];
    __shared__ unsigned short tab[CH_PMAX * (CH_PMAX + 1) / 2];
    __shared__ double red[CH_THREADS / 64];
    __shared__ double dg[CH_KMAX];
    __shared__ int flag_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    double* wb = w + (size_t)b * ldw;
    if (chk_in && info[b] != 0) {
        for (int i = tid; i < nout; i += CH_THREADS) wb[i] = __builtin_nan("");
        return;
    }
    const int r = rank ? min(max(rank[(size_t)b * rank_stride], 0), K) : K;
    const int N = r + (r & 1), Np = N / 2;
    const cplx* Ab = A + strideA * b;
    // scale by a power of two (exact) so that the largest |re|, |im| of the lower triangle lies in [1/2, 1): the norms
    // below neither overflow (entries ~1e154 and above) nor underflow to zero (~1e-160 and below) at any input scale
    double amax = 0.0, bad = 0.0;
    for (int idx = tid; idx < r * r; idx += CH_THREADS) {
        const int i = idx / r, j = idx - i * r;
        if (i < j) continue;
        const cplx v = Ab[(size_t)i * lda + j];
        const double y = i == j ? 0.0 : v.y;
        if (!isfinite(v.x) || !isfinite(y)) bad += 1.0;
        else amax = fmax(amax, fmax(fabs(v.x), fabs(y)));
    }
    amax = block_max(amax, red);
    bad = block_sum(bad, red);
    int ex = 0;
    if (amax > 0.0) (void)frexp(amax, &ex);
    double f2 = 0.0;
    for (int idx = tid; idx < N * N; idx += CH_THREADS) {
        const int i = idx / N, j = idx - i * N;
        cplx v = cmake(0.0, 0.0);
        if (i < r && j < r) {
            v = i >= j ? Ab[(size_t)i * lda + j] : cconj(Ab[(size_t)j * lda + i]);
            if (i == j) v.y = 0.0;
            v = cmake(ldexp(v.x, -ex), ldexp(v.y, -ex));
        }
        M[i * pitch + j] = v;
        f2 += cabs2(v);
    }
    const int ntab = Np * (Np + 1) / 2;
    for (int t = tid; t < ntab; t += CH_THREADS) {
        int P = 0, rem = t;                        // t -> (P, Q), P <= Q, row-major over the upper triangle
        while (rem >= Np - P) { rem -= Np - P; ++P; }
        tab[t] = (unsigned short)(P * 64 + P + rem);
    }
    const double fro2 = block_sum(f2, red);        // (its barriers also publish M and tab)
    int flag = 0;
    if (bad != 0.0 || !isfinite(fro2)) flag = 1;
    else {
        const double tol2 = DBL_EPSILON * DBL_EPSILON * fro2;
        const double skip = DBL_EPSILON * sqrt(fro2) / (4.0 * (N > 0 ? N : 1));
        for (int sweep = 0;; ++sweep) {
            double o2 = 0.0;
            for (int idx = tid; idx < N * N; idx += CH_THREADS) {
                const int i = idx / N, j = idx - i * N;
                if (i != j) o2 += cabs2(M[i * pitch + j]);
            }
            o2 = block_sum(o2, red);
            if (o2 <= tol2) break;
            if (sweep == JAC_MAX_SWEEPS) { flag = 2; break; }
            for (int st = 0; st < N - 1; ++st) {
                if (tid < Np) {
                    JacPair J;
                    rr_pair(st, tid, N, &J.p, &J.q);
                    const double a = M[J.p * pitch + J.p].x, d = M[J.q * pitch + J.q].x;
                    const cplx bpq = M[J.p * pitch + J.q];
                    const double ab = sqrt(cabs2(bpq));
                    if (!(ab > skip)) { J.c = 1.0; J.s = 0.0; J.tb = 0.0; J.w = cmake(1.0, 0.0); }
                    else {
                        const double z = (d - a) / (2.0 * ab);
                        const double t = (z >= 0.0 ? 1.0 : -1.0) / (fabs(z) + sqrt(z * z + 1.0));
                        J.c = 1.0 / sqrt(t * t + 1.0); J.s = t * J.c; J.tb = t * ab;
                        J.w = cmake(bpq.x / ab, bpq.y / ab);
                    }
                    pr[tid] = J;
                }
                __syncthreads();
                for (int k = tid; k < ntab; k += CH_THREADS) {
                    const int P = tab[k] >> 6, Q = tab[k] & 63;
                    const JacPair JP = pr[P];
                    cplx* r0 = M + JP.p * pitch;
                    cplx* r1 = M + JP.q * pitch;
                    if (P == Q) {
                        // closed form of the diagonal block: diag(a - t|b|, d + t|b|), zero coupling
                        r0[JP.p] = cmake(r0[JP.p].x - JP.tb, 0.0);
                        r1[JP.q] = cmake(r1[JP.q].x + JP.tb, 0.0);
                        r0[JP.q] = cmake(0.0, 0.0);
                        r1[JP.p] = cmake(0.0, 0.0);
                        continue;
                    }
                    const JacPair JQ = pr[Q];
                    // J = [[c, s w], [-s conj(w), c]];  Y = J_P^H X J_Q
                    const cplx x00 = r0[JQ.p], x01 = r0[JQ.q], x10 = r1[JQ.p], x11 = r1[JQ.q];
                    // U = J_P^H X:  J^H = [[c, -s w], [s conj(w), c]]
                    const cplx swP = cscale(JP.w, JP.s), swPc = cconj(swP);
                    const cplx u00 = csub(cscale(x00, JP.c), cmul(swP, x10));
                    const cplx u01 = csub(cscale(x01, JP.c), cmul(swP, x11));
                    const cplx u10 = cadd(cmul(swPc, x00), cscale(x10, JP.c));
                    const cplx u11 = cadd(cmul(swPc, x01), cscale(x11, JP.c));
                    // Y = U J_Q
                    const cplx swQ = cscale(JQ.w, JQ.s), swQc = cconj(swQ);
                    const cplx y00 = csub(cscale(u00, JQ.c), cmul(u01, swQc));
                    const cplx y01 = cadd(cmul(u00, swQ), cscale(u01, JQ.c));
                    const cplx y10 = csub(cscale(u10, JQ.c), cmul(u11, swQc));
                    const cplx y11 = cadd(cmul(u10, swQ), cscale(u11, JQ.c));
                    r0[JQ.p] = y00; r0[JQ.q] = y01; r1[JQ.p] = y10; r1[JQ.q] = y11;
                    M[JQ.p * pitch + JP.p] = cconj(y00); M[JQ.q * pitch + JP.p] = cconj(y01);
                    M[JQ.p * pitch + JP.q] = cconj(y10); M[JQ.q * pitch + JP.q] = cconj(y11);
                }
                __syncthreads();
            }
        }
    }
    if (tid == 0) flag_s = flag;
    for (int i = tid; i < r; i += CH_THREADS) dg[i] = ldexp(M[i * pitch + i].x, ex);
    __syncthreads();
    flag = flag_s;
    if (flag == 1) {
        for (int i = tid; i < nout; i += CH_THREADS) wb[i] = __builtin_nan("");
    } else {
        // rank sort: position of value i = number of values before it in the requested order (ties by index)
        for (int i = tid; i < r; i += CH_THREADS) {
            const double v = dg[i];
            int pos = 0;
            for (int j = 0; j < r; ++j) {
                const double u = dg[j];
                pos += (descending ? u > v : u < v) || (u == v && j < i);
            }
            if (pos < nout) wb[pos] = v;
        }
        for (int i = r + tid; i < nout; i += CH_THREADS) wb[i] = 0.0;
    }
    if (tid == 0 && info) info[b] = flag_sign * flag;
}

// Pivoted Cholesky (outer-product form, pivots by the largest remaining diagonal, lowest index on ties) of the
// Hermitian PSD matrix G[b] (K x K, read in full).  Lh[b] (K x K, row k = conj of column k of L in the original
// orbital order) and rank[b]; rows >= rank are zero.
__global__ __launch_bounds__(CH_THREADS) void pchol_kernel(int K, int pitch, const cplx* __restrict__ G, size_t strideG,
                                                           cplx* __restrict__ Lh, size_t strideL, int* __restrict__ rank)
{
    extern __shared__ cplx M[];                    // [K][pitch]
    __shared__ cplx lcol[CH_KMAX];
    __shared__ double d[CH_KMAX];
    __shared__ unsigned char done[CH_KMAX];
    __shared__ int piv_s;
    __shared__ double thr_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const cplx* Gb = G + strideG * b;
    cplx* Lb = Lh + strideL * b;
    for (int idx = tid; idx < K * K; idx += CH_THREADS) {
        const int i = idx / K, j = idx - i * K;
        M[i * pitch + j] = Gb[idx];
    }
    for (int i = tid; i < K; i += CH_THREADS) { d[i] = Gb[(size_t)i * K + i].x; done[i] = 0; }
    __syncthreads();
    int k = 0;
    for (; k < K; ++k) {
        if (tid < 64) {
            // wave 0: argmax of the remaining diagonal (K <= 96: two candidates per lane)
            double best = -1.0; int bi = K;
            for (int i = tid; i < K; i += 64)
                if (!done[i] && (d[i] > best || bi == K)) { best = d[i]; bi = i; }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const double ob = __shfl_xor(best, o);
                const int oi = __shfl_xor(bi, o);
                if (oi < K && (bi == K || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
            }
            if (tid == 0) {
                if (k == 0) thr_s = 1e-14 * best;
                // stop: nothing left above the threshold (a zero or non-positive Gamma has rank 0)
                piv_s = (bi < K && best > thr_s && best > 0.0) ? bi : -1;
                if (piv_s >= 0) done[bi] = 1;
            }
        }
        __syncthreads();
        const int p = piv_s;
        if (p < 0) break;
        const double sp = sqrt(d[p]), isp = 1.0 / sp;
        for (int i = tid; i < K; i += CH_THREADS) {
            cplx l = cmake(0.0, 0.0);
            if (i == p) l = cmake(sp, 0.0);
            else if (!done[i]) l = cscale(M[i * pitch + p], isp);
            lcol[i] = l;
            Lb[(size_t)k * K + i] = cconj(l);
        }
        __syncthreads();
        for (int idx = tid; idx < K * K; idx += CH_THREADS) {
            const int i = idx / K, j = idx - i * K;
            if (done[i] || done[j]) continue;
            M[i * pitch + j] = cfnma(M[i * pitch + j], lcol[i], cconj(lcol[j]));
        }
        for (int i = tid; i < K; i += CH_THREADS)
            if (!done[i]) d[i] -= cabs2(lcol[i]);
        __syncthreads();
    }
    for (int idx = k * K + tid; idx < K * K; idx += CH_THREADS) Lb[idx] = cmake(0.0, 0.0);
    if (tid == 0) rank[b] = k;
}

int ch_pitch(int K) { return (K + (K & 1)) + 1; }
size_t ch_lds_bytes(int K) { return (size_t)(K + (K & 1)) * ch_pitch(K) * sizeof(cplx); }

// raise the kernel's dynamic LDS limit to what K = CH_KMAX needs, once per kernel and device (not on every launch)
template <typename Kern>
void ch_set_lds(Kern k, std::atomic<unsigned long long>& done, size_t max_bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_relaxed) & bit) return;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_bytes) != hipSuccess)
        (void)hipGetLastError();
    done.fetch_or(bit, std::memory_order_relaxed);
}
std::atomic<unsigned long long> g_jacobi_lds_set{0}, g_pchol_lds_set{0};

}  // namespace

int channels_kmax() { return CH_KMAX; }

bool launch_eigvalsh_batched(hipStream_t st, int K, int nb, const cplx* A, int lda, size_t strideA, const int* rank,
                             int rank_stride, double* w, int ldw, int nout, bool descending, int* info, bool chk_in, int flag_sign)
{
    if (K < 1 || K > CH_KMAX || nout > ldw) return false;
    if (nb <= 0) return true;
    const size_t lds = ch_lds_bytes(K);
    ch_set_lds(jacobi_kernel, g_jacobi_lds_set, ch_lds_bytes(CH_KMAX));
    hipLaunchKernelGGL(jacobi_kernel, dim3(nb), dim3(CH_THREADS), lds, st, K, ch_pitch(K), A, lda, strideA, rank, rank_stride, w, ldw,
                       nout, descending ? 1 : 0, info, chk_in ? 1 : 0, flag_sign);
    return true;
}

bool launch_pivoted_cholesky(hipStream_t st, int K, int nb, const cplx* G, size_t strideG, cplx* Lh, size_t strideL,
                             int* rank)
{
    if (K < 1 || K > CH_KMAX) return false;
    if (nb <= 0) return true;
    const size_t lds = (size_t)K * ch_pitch(K) * sizeof(cplx);
    ch_set_lds(pchol_kernel, g_pchol_lds_set, (size_t)CH_KMAX * ch_pitch(CH_KMAX) * sizeof(cplx));
    hipLaunchKernelGGL(pchol_kernel, dim3(nb), dim3(CH_THREADS), lds, st, K, ch_pitch(K), G, strideG, Lh, strideL, rank);
    return true;
}
