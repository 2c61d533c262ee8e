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
//
// Eigenvectors (negf_eigh_batched, negf_channel_states): jacobi_kernel<true> is the same kernel -- same schedule, skip
// threshold, closed-form diagonal update, scaling and stop rule, hence bitwise the same eigenvalues -- that also
// accumulates X <- X J for the K/2 rotations of every step, from a caller-given X0 (rows x r; the identity gives the
// eigenvectors V, the Cholesky factor L gives L V in one go).  X is held column-major, X[col * rows + i], and a step's
// work items are (row i, pair P) with i the fast index: the lanes of a wave touch consecutive 16-byte slots of two
// columns, conflict-free in LDS at any pitch and coalesced in global memory.  No rotation is formed for X: the pairs'
// (c, s, w) of the matrix update are reused between the same two barriers.
// Where X lives follows from the LDS budget: matrix + X = 16 N (N + 1 + K) bytes (N = K rounded up to even) next to
// the static LDS, for which CH_STATIC_LDS = 6 KB are set aside (5.5 KB used, checked at compile time), must fit 160 KB:
// N (N + 1 + K) <= 9856, which holds up to K = 69 (70 x 140 = 9800) and fails from K = 70 (70 x 141 = 9870).  So
// K <= 69 keeps X in LDS (K <= 38: three workgroups per CU, K <= 48: two, else one); K = 70 .. 96 rotates X in a
// workgroup-private slice of global memory (N K x 16 B <= 147 KB, L2-resident, each element read and written by one
// lane per step, ordered by the step's barriers; no atomics), with the matrix alone in LDS: one workgroup per CU (its
// 70 x 71 x 16 B and up exceed half of the LDS).  The values-only instantiation jacobi_kernel<false> compiles to the
// code it was before the flag existed.
//
//   gauge_kernel   last pass of the channel states: one workgroup per (energy, channel) takes conj(psi) as the product
//                  left it, fixes the phase (largest |psi_i|^2 real positive, lowest index on ties), writes zeros for
//                  channels at or beyond the rank and NaN for a flagged energy.
#include "negf_common.h"
#include <atomic>
#include <cfloat>
#include <type_traits>

namespace {

constexpr int CH_THREADS = 256;
constexpr int JAC_MAX_SWEEPS = 30;
constexpr int CH_KMAX = 96;
constexpr int CH_PMAX = CH_KMAX / 2;
constexpr size_t CH_LDS_CU = 160 * 1024;       // LDS of a compute unit = the most one workgroup can have
constexpr size_t CH_STATIC_LDS = 6 * 1024;     // set aside for the kernels' static LDS when X is placed

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

// (JacVec, what jacobi_kernel<true> accumulates from and writes to: negf_common.h)
struct JacNoVec {};

// X <- X diag(J_P) for the step's pairs: item (i, P) rotates row i of the columns (p, q) of pair P
template <typename XPtr>
__device__ __forceinline__ void jac_rotate_x(XPtr X, int rows, int Np, const JacPair* pr, int tid)
{
    for (int idx = tid; idx < rows * Np; idx += CH_THREADS) {
        const int P = idx / rows, i = idx - P * rows;
        const JacPair J = pr[P];
        if (J.s == 0.0) continue;                  // a skipped pair: the identity
        const cplx xp = X[J.p * rows + i], xq = X[J.q * rows + i];
        const cplx sw = cscale(J.w, J.s), swc = cconj(sw);
        // J = [[c, s w], [-s conj(w), c]]
        X[J.p * rows + i] = csub(cscale(xp, J.c), cmul(xq, swc));
        X[J.q * rows + i] = cadd(cmul(xp, sw), cscale(xq, J.c));
    }
}

template <typename XPtr>
__device__ __forceinline__ void jac_write_x(XPtr X, const JacVec& v, cplx* ob, int r, const unsigned short* pos, int tid)
{
    for (int idx = tid; idx < v.rows * r; idx += CH_THREADS) {
        const int j = idx / v.rows, i = idx - j * v.rows;
        const int ps = pos[j];
        if (ps >= v.ncol) continue;
        const cplx x = X[j * v.rows + i];
        ob[(size_t)i * v.out_ri + (size_t)ps * v.out_cj] = v.out_conj ? cconj(x) : x;
    }
}

// w[b * ldw + 0 .. nout): eigenvalues of the Hermitian matrix in the lower triangle of A[b] (the leading r x r block,
// r = rank ? rank[b * rank_stride] : K), ascending (descending = 0) or descending; positions r .. nout are exact zeros.
// info: chk_in -> an energy whose info is already nonzero gets a NaN row and keeps its info; otherwise info[b] =
// flag_sign * (1: non-finite input, NaN row; 2: not converged), 0 when converged.
// VEC: also the accumulated rotations (JacVec above); the values-only form takes an empty JacNoVec.
template <bool VEC>
__global__ __launch_bounds__(CH_THREADS) void jacobi_kernel(int K, int pitch, const cplx* __restrict__ A, int lda,
                                                            size_t strideA, const int* __restrict__ rank, int rank_stride,
                                                            double* __restrict__ w,
                                                            int ldw, int nout, int descending, int* __restrict__ info,
                                                            int chk_in, int flag_sign,
                                                            typename std::conditional<VEC, JacVec, JacNoVec>::type vec)
{
    extern __shared__ cplx M[];                    // [N][pitch]
    __shared__ JacPair pr[CH_PMAX];
    __shared__ unsigned short tab[CH_PMAX * (CH_PMAX + 1) / 2];
    __shared__ double red[CH_THREADS / 64];
    __shared__ double dg[CH_KMAX];
    __shared__ int flag_s;
    static_assert(sizeof(pr) + sizeof(tab) + sizeof(red) + sizeof(dg) + 64 <= CH_STATIC_LDS, "static LDS exceeds what X's placement sets aside");
    const int b = blockIdx.x, tid = threadIdx.x;
    double* wb = w + (size_t)b * ldw;
    if (chk_in && info[b] != 0) {
        for (int i = tid; i < nout; i += CH_THREADS) wb[i] = __builtin_nan("");
        if constexpr (VEC) {
            cplx* ob = vec.out + vec.out_stride * b;
            for (int idx = tid; idx < vec.rows * vec.ncol; idx += CH_THREADS) {
                const int j = idx / vec.rows, i = idx - j * vec.rows;
                ob[(size_t)i * vec.out_ri + (size_t)j * vec.out_cj] = cmake(__builtin_nan(""), __builtin_nan(""));
            }
        }
        return;
    }
    const int r = rank ? min(max(rank[(size_t)b * rank_stride], 0), K) : K;
    const int N = r + (r & 1), Np = N / 2;
    [[maybe_unused]] cplx* Xl = nullptr;           // X in LDS, behind the matrix as the launch laid it out (K's pitch)
    [[maybe_unused]] cplx* Xg = nullptr;
    if constexpr (VEC) {
        Xl = M + (K + (K & 1)) * pitch;
        Xg = vec.xg ? vec.xg + vec.xg_stride * b : nullptr;
        // X0: rows x r, and a zero column where r is odd (its pair never rotates)
        for (int idx = tid; idx < vec.rows * N; idx += CH_THREADS) {
            const int j = idx / vec.rows, i = idx - j * vec.rows;
            cplx x = cmake(0.0, 0.0);
            if (j < r) {
                if (!vec.x0) x = cmake(i == j ? 1.0 : 0.0, 0.0);
                else {
                    x = vec.x0[vec.x0_stride * b + (size_t)i * vec.x0_ri + (size_t)j * vec.x0_cj];
                    if (vec.x0_conj) x = cconj(x);
                }
            }
            if (Xg) Xg[idx] = x; else Xl[idx] = x;
        }
    }
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
                if constexpr (VEC) {
                    if (Xg) jac_rotate_x(Xg, vec.rows, Np, pr, tid);
                    else jac_rotate_x(Xl, vec.rows, Np, pr, tid);
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
        if constexpr (VEC) {
            cplx* ob = vec.out + vec.out_stride * b;
            for (int idx = tid; idx < vec.rows * vec.ncol; idx += CH_THREADS) {
                const int j = idx / vec.rows, i = idx - j * vec.rows;
                ob[(size_t)i * vec.out_ri + (size_t)j * vec.out_cj] = cmake(__builtin_nan(""), __builtin_nan(""));
            }
        }
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
            if constexpr (VEC) tab[i] = (unsigned short)pos;      // (the pair table has served)
        }
        for (int i = r + tid; i < nout; i += CH_THREADS) wb[i] = 0.0;
        if constexpr (VEC) {
            __syncthreads();
            cplx* ob = vec.out + vec.out_stride * b;
            if (Xg) jac_write_x(Xg, vec, ob, r, tab, tid);
            else jac_write_x(Xl, vec, ob, r, tab, tid);
            for (int idx = tid; idx < vec.rows * (vec.ncol - r); idx += CH_THREADS) {
                const int j = r + idx / vec.rows, i = idx % vec.rows;
                ob[(size_t)i * vec.out_ri + (size_t)j * vec.out_cj] = cmake(0.0, 0.0);
            }
        }
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

// psi[b][c][0..n) from Pc[b * strideP + c * n + i] = conj(psi_c[i]), c < nce (the channels computed); channels
// >= min(rank, nce) are zeros; info[b] other than 0 and -2 (not converged: the values stand) gives NaN.
__global__ __launch_bounds__(CH_THREADS) void gauge_kernel(int n, int nce, int nchan, const cplx* __restrict__ Pc, size_t strideP,
                                                           const int* __restrict__ rank, int rank_stride,
                                                           const int* __restrict__ info, cplx* __restrict__ psi)
{
    __shared__ double bv[CH_THREADS / 64];
    __shared__ int bi[CH_THREADS / 64];
    const int ch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    cplx* out = psi + ((size_t)b * nchan + ch) * n;
    const int fl = info[b];
    if (fl != 0 && fl != -2) {
        for (int i = tid; i < n; i += CH_THREADS) out[i] = cmake(__builtin_nan(""), __builtin_nan(""));
        return;
    }
    const int r = min(max(rank[(size_t)b * rank_stride], 0), nce);
    if (ch >= r) {
        for (int i = tid; i < n; i += CH_THREADS) out[i] = cmake(0.0, 0.0);
        return;
    }
    const cplx* in = Pc + strideP * b + (size_t)ch * n;
    // argmax of |psi_i|^2, lowest index on ties: per lane in index order, then across lanes and waves
    double best = -1.0; int at = n;
    for (int i = tid; i < n; i += CH_THREADS) {
        const double v = cabs2(in[i]);
        if (v > best) { best = v; at = i; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(at, o);
        if (ob > best || (ob == best && oi < at)) { best = ob; at = oi; }
    }
    if ((tid & 63) == 0) { bv[tid >> 6] = best; bi[tid >> 6] = at; }
    __syncthreads();
    best = bv[0]; at = bi[0];
#pragma unroll
    for (int k = 1; k < CH_THREADS / 64; ++k)
        if (bv[k] > best || (bv[k] == best && bi[k] < at)) { best = bv[k]; at = bi[k]; }
    if (!(best > 0.0) || at >= n) {                // a zero state has no phase to fix (NaN components stay NaN)
        for (int i = tid; i < n; i += CH_THREADS) out[i] = cconj(in[i]);
        return;
    }
    const double mag = sqrt(best);
    const cplx pm = in[at];                        // conj(psi*) : psi_i conj(psi*) / |psi*|
    const cplx ph = cmake(pm.x / mag, pm.y / mag);
    for (int i = tid; i < n; i += CH_THREADS)
        out[i] = i == at ? cmake(mag, 0.0) : cmul(cconj(in[i]), ph);
}

int ch_pitch(int K) { return (K + (K & 1)) + 1; }
size_t ch_lds_bytes(int K) { return (size_t)(K + (K & 1)) * ch_pitch(K) * sizeof(cplx); }
// X (N x K, column-major) of the vector form: its bytes, and whether it fits in LDS behind the matrix
size_t ch_x_bytes(int K) { return (size_t)(K + (K & 1)) * K * sizeof(cplx); }
bool ch_x_in_lds(int K) { return ch_lds_bytes(K) + ch_x_bytes(K) + CH_STATIC_LDS <= CH_LDS_CU; }

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
std::atomic<unsigned long long> g_jacobi_lds_set{0}, g_jacobi_vec_lds_set{0}, g_pchol_lds_set{0};

}  // namespace

int channels_kmax() { return CH_KMAX; }

bool launch_eigvalsh_batched(hipStream_t st, int K, int nb, const cplx* A, int lda, size_t strideA, const int* rank,
                             int rank_stride, double* w, int ldw, int nout, bool descending, int* info, bool chk_in, int flag_sign)
{
    if (K < 1 || K > CH_KMAX || nout > ldw) return false;
    if (nb <= 0) return true;
    const size_t lds = ch_lds_bytes(K);
    ch_set_lds(jacobi_kernel<false>, g_jacobi_lds_set, ch_lds_bytes(CH_KMAX));
    hipLaunchKernelGGL(jacobi_kernel<false>, dim3(nb), dim3(CH_THREADS), lds, st, K, ch_pitch(K), A, lda, strideA, rank, rank_stride, w, ldw,
                       nout, descending ? 1 : 0, info, chk_in ? 1 : 0, flag_sign, JacNoVec{});
    return true;
}

size_t eigh_scratch_elems(int K) { return (K < 1 || K > CH_KMAX || ch_x_in_lds(K)) ? 0 : ch_x_bytes(K) / sizeof(cplx); }

bool launch_eigh_batched(hipStream_t st, int K, int nb, const cplx* A, int lda, size_t strideA, const int* rank,
                         int rank_stride, double* w, int ldw, int nout, bool descending, int* info, bool chk_in, int flag_sign,
                         JacVec vec)
{
    if (K < 1 || K > CH_KMAX || nout > ldw || !vec.out || vec.ncol < 0) return false;
    const bool in_lds = ch_x_in_lds(K);
    if (!in_lds && !vec.xg) return false;
    if (nb <= 0) return true;
    vec.rows = K;
    if (in_lds) vec.xg = nullptr;
    vec.xg_stride = eigh_scratch_elems(K);
    // the largest LDS image is the last K that keeps X beside the matrix (above it the matrix is alone, as in the values form)
    size_t lds_max = ch_lds_bytes(CH_KMAX);
    for (int k = 1; k <= CH_KMAX; ++k)
        if (ch_x_in_lds(k)) lds_max = std::max(lds_max, ch_lds_bytes(k) + ch_x_bytes(k));
    const size_t lds = ch_lds_bytes(K) + (in_lds ? ch_x_bytes(K) : 0);
    ch_set_lds(jacobi_kernel<true>, g_jacobi_vec_lds_set, lds_max);
    hipLaunchKernelGGL(jacobi_kernel<true>, dim3(nb), dim3(CH_THREADS), lds, st, K, ch_pitch(K), A, lda, strideA, rank, rank_stride, w, ldw,
                       nout, descending ? 1 : 0, info, chk_in ? 1 : 0, flag_sign, vec);
    return true;
}

void launch_channel_gauge(hipStream_t st, int n, int nce, int nchan, int nb, const cplx* Pc, size_t strideP, const int* rank,
                          int rank_stride, const int* info, cplx* psi)
{
    if (nb <= 0 || nchan <= 0 || n <= 0) return;
    hipLaunchKernelGGL(gauge_kernel, dim3(nchan, nb), dim3(CH_THREADS), 0, st, n, nce, nchan, Pc, strideP, rank, rank_stride, info, psi);
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
