// Floating dephasing probes (gfx950): the probes' response to the real contacts and the dephased coupling matrix of
// the lesser Green's function, behind the transmission-matrix pass of k_tmatrix.hip.  Terminals as there: n_c contacts
// followed by P probes, C = n_c + P.  Per energy, with To = T with zero diagonal,
//     W_pp = sum_{c != p} To[p][c] (c over ALL terminals),   W_pq = -To[p][q],   P' = probes with W_pp > 0,
//     R[P', :] = W^-1 To[P', 0:n_c]              (rows of probes outside P' are exact zeros)
//     D_s = scatter(Gamma_s on I_s) + sum_p R[p][s] scatter(Gamma_p on I_p)         (ind = None: all weights 1)
// The floating condition is a real-axis notion; for complex energies the formulas are applied literally.
// The reference has no such function.
//   deph_response : one workgroup per energy.  The augmented matrix [W | To[P, 0:n_c]] (P x (P + n_c) doubles) lives in
//                   LDS for P <= DEPH_LDS_MAX_P and n_c <= DEPH_LDS_MAX_RHS, otherwise in a per-energy global work area.
//                   LU WITHOUT pivoting: W is an M-matrix, weakly diagonally dominant by rows (T >= 0), for which
//                   elimination without pivoting is backward stable and under which dominance is preserved; then a
//                   column-oriented back substitution.  A probe outside P' keeps a unit row and column and a zero
//                   right-hand side, which the elimination passes through untouched (its multipliers are exact zeros).
//                   A pivot that is not positive -- probes that reach no contact, whose W is singular -- gives a NaN R
//                   for that energy, as a non-finite T does.
//   deph_coupling : one workgroup per energy; D on the sorted union U of the orbitals involved (K_U x K_U), the terminals
//                   added one after the other through an index map.
// No floating-point atomics.  Every element of the matrix is owned by one thread in every step and the steps run in one
// order: rows and columns of W are the probes in the CONTENT order the transmission-matrix plan derives, the row sums
// run over the contacts 0 .. n_c - 1 and then over the probes in that order.  The bits of R therefore depend on P, n_c
// and the probes' content alone -- not on the order in which the caller lists them (permuting the probes permutes the
// rows of R bit for bit), nor on the thread count, the size class' memory or the workspace batch.
#include "negf_common.h"
#include <algorithm>

namespace {

constexpr int DEPH_THREADS = 256;                          // the coupling kernel, and the response kernel's LDS class
constexpr int DEPH_THREADS_GLOBAL = 1024;                  // the response kernel's global class

// a[r][0 .. L): r-th row of the augmented matrix.  false: a pivot that is not positive (zero, negative or NaN) -- W is
// singular, which is what probes without a path to any contact give (a cluster that sees only itself has rows that sum to
// zero); every thread reads the same pivot after a barrier, so the exit is uniform.
template <int THREADS>
__device__ __forceinline__ bool deph_solve(double* __restrict__ a, int P, int L, int tid)
{
    // forward elimination: multipliers of column k, then the trailing update; one owner per element and step
    for (int k = 0; k < P - 1; ++k) {
        const double piv = a[(size_t)k * L + k];
        if (!(piv > 0.0)) return false;
        for (int i = k + 1 + tid; i < P; i += THREADS) a[(size_t)i * L + k] /= piv;
        __syncthreads();
        const int w = L - k - 1, cnt = (P - k - 1) * w;
        for (int e = tid; e < cnt; e += THREADS) {
            const int i = k + 1 + e / w, j = k + 1 + e % w;
            a[(size_t)i * L + j] -= a[(size_t)i * L + k] * a[(size_t)k * L + j];
        }
        __syncthreads();
    }
    if (!(a[(size_t)(P - 1) * L + P - 1] > 0.0)) return false;
    // back substitution, column oriented: x_k = b_k / u_kk, then b_i -= u_ik x_k for i < k
    const int nr = L - P;
    for (int k = P - 1; k >= 0; --k) {
        const double piv = a[(size_t)k * L + k];
        __syncthreads();
        for (int r = tid; r < nr; r += THREADS) a[(size_t)k * L + P + r] /= piv;
        __syncthreads();
        for (int e = tid; e < k * nr; e += THREADS) {
            const int i = e / nr, r = e - i * nr;
            a[(size_t)i * L + P + r] -= a[(size_t)i * L + k] * a[(size_t)k * L + P + r];
        }
    }
    __syncthreads();
    return true;
}

// T [C][C] of energy blockIdx.x -> R [P][nc]; order[r] = terminal index (nc + probe) of row r
template <int THREADS, bool LDS>
__global__ __launch_bounds__(THREADS) void deph_response_kernel(
    int C, int nc, const int* __restrict__ order, const double* __restrict__ T, double* __restrict__ work,
    double* __restrict__ R)
{
    extern __shared__ double deph_lds[];
    __shared__ int s_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int P = C - nc, L = P + nc;
    const double* Tb = T + (size_t)b * C * C;
    double* Rb = R + (size_t)b * P * nc;
    double* a = LDS ? deph_lds : work + (size_t)b * P * L;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int bad = 0;
    for (int e = tid; e < C * C; e += THREADS) bad |= !(fabs(Tb[e]) <= 1.79769313486231570815e308);
    if (bad) s_bad = 1;                                            // (every writer stores the same value)
    __syncthreads();
    if (s_bad) {                                                   // (uniform) singular energy or a non-finite T
        const double qnan = __builtin_nan("");
        for (int e = tid; e < P * nc; e += THREADS) Rb[e] = qnan;
        return;
    }
    // row sums W_pp: contacts 0 .. nc - 1, then the probes in content order, the probe itself left out
    for (int r = tid; r < P; r += THREADS) {
        const int p = order[r];
        const double* row = Tb + (size_t)p * C;
        double s = 0.0;
        for (int c = 0; c < nc; ++c) s += row[c];
        for (int q = 0; q < P; ++q) { const int t = order[q]; if (t != p) s += row[t]; }
        a[(size_t)r * L + r] = s;
    }
    __syncthreads();
    auto wpp = [&](int r) { return a[(size_t)r * L + r]; };
    // off-diagonal entries and the right-hand sides; probes outside P' keep a unit row / column and a zero right-hand side
    for (int e = tid; e < P * L; e += THREADS) {
        const int r = e / L, j = e - r * L;
        if (j == r) continue;
        const bool on = wpp(r) > 0.0 && (j >= P || wpp(j) > 0.0);
        const int p = order[r];
        double v = 0.0;
        if (on) v = j < P ? -Tb[(size_t)p * C + order[j]] : Tb[(size_t)p * C + (j - P)];
        a[(size_t)r * L + j] = v;
    }
    __syncthreads();
    for (int r = tid; r < P; r += THREADS) {
        const double s = wpp(r);
        a[(size_t)r * L + r] = s > 0.0 ? s : 1.0;
    }
    __syncthreads();
    if (!deph_solve<THREADS>(a, P, L, tid)) {                      // (uniform) singular W: no defined occupations
        const double qnan = __builtin_nan("");
        for (int e = tid; e < P * nc; e += THREADS) Rb[e] = qnan;
        return;
    }
    for (int e = tid; e < P * nc; e += THREADS) {
        const int r = e / nc, c = e - r * nc;
        double v = a[(size_t)r * L + P + c];
        if (v == 0.0) v = 0.0;                                     // (a probe outside P' solves to a zero of either sign)
        Rb[(size_t)(order[r] - nc) * nc + c] = v;
    }
}

// D [K_U][K_U] of energy blockIdx.x: zero, then the terminals list[0 .. nlist) one after the other.  weight: contact s
// (col >= 0) -> terminal t < nc enters with 1, probe t with R[b][t - nc][col]; col < 0 -> every terminal with 1.
__global__ __launch_bounds__(DEPH_THREADS) void deph_coupling_kernel(
    int KU, int nc, int P, int col, int nlist, const int* __restrict__ list, const int* __restrict__ tK,
    const int* __restrict__ ioff, const int* __restrict__ goff, const int* __restrict__ gstride,
    const int* __restrict__ pos, const cplx* __restrict__ gam, const double* __restrict__ R, cplx* __restrict__ D,
    size_t strideD)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    cplx* Db = D + (size_t)b * strideD;
    const size_t cnt = (size_t)KU * KU;
    for (size_t e = tid; e < cnt; e += DEPH_THREADS) Db[e] = cmake(0.0, 0.0);
    __syncthreads();
    for (int q = 0; q < nlist; ++q) {
        const int t = list[q];
        const int K = tK[t];
        const int* I = pos + ioff[t];
        const cplx* g = gam + (size_t)b * gstride[t] + goff[t];
        const double wgt = (col < 0 || t < nc) ? 1.0 : R[((size_t)b * P + (t - nc)) * nc + col];
        for (int e = tid; e < K * K; e += DEPH_THREADS) {
            const int i = e / K, j = e - i * K;
            const size_t at = (size_t)I[i] * KU + I[j];
            const cplx d = Db[at], x = g[e];
            Db[at] = cmake(d.x + wgt * x.x, d.y + wgt * x.y);
        }
        __syncthreads();
    }
}

}  // namespace

bool deph_response_in_lds(int P, int nc) { return P <= DEPH_LDS_MAX_P && nc <= DEPH_LDS_MAX_RHS; }

size_t deph_response_work_doubles(int P, int nc) { return deph_response_in_lds(P, nc) ? 0 : (size_t)P * (P + nc); }

void launch_deph_response(hipStream_t st, int C, int nc, int nb, const int* order, const double* T, double* work, double* R)
{
    const int P = C - nc;
    if (nb <= 0 || P <= 0 || nc <= 0) return;
    if (deph_response_in_lds(P, nc)) {
        const size_t lds = (size_t)P * (P + nc) * sizeof(double);
        hipLaunchKernelGGL((deph_response_kernel<DEPH_THREADS, true>), dim3(nb), dim3(DEPH_THREADS), lds, st, C, nc, order, T,
                           work, R);
    } else {
        hipLaunchKernelGGL((deph_response_kernel<DEPH_THREADS_GLOBAL, false>), dim3(nb), dim3(DEPH_THREADS_GLOBAL), 0, st, C, nc,
                           order, T, work, R);
    }
}

void launch_deph_coupling(hipStream_t st, int KU, int nc, int P, int col, int nlist, int nb, const int* list, const int* tK,
                          const int* ioff, const int* goff, const int* gstride, const int* pos, const cplx* gam,
                          const double* R, cplx* D, size_t strideD)
{
    if (nb <= 0 || KU <= 0) return;
    hipLaunchKernelGGL(deph_coupling_kernel, dim3(nb), dim3(DEPH_THREADS), 0, st, KU, nc, P, col, nlist, list, tK, ioff, goff,
                       gstride, pos, gam, R, D, strideD);
}
