// The small in-place inverse of the 1-D chain kernels (n <= 64): blocked Gauss-Jordan with implicit partial pivoting on
// ONE n x n matrix in LDS, four waves, products and updates on the FP64 matrix cores in 3M form.  Shared by the
// fixed-point kernel (k_chain1d_rs.hip) and the renormalisation-decimation kernel (k_chain1d_rd.hip); both include it
// inside their own translation unit (everything here has internal linkage).
#pragma once
#include "negf_common.h"
#include "wave_utils.h"
#include "chain_rs_sched.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = 4;
constexpr int RS_NB = 8;                  // panel width of the small inverse: half a column tile
// The pivot rows of a panel are replaced, not updated: W[pivot row][col] = 0 + P[pivot row][:] Q[:][col].  The trailing
// update needs no per-tile mask for that: the owner of a column tile has the panel's pivot rows of its columns (the Q
// fragment) in registers before it writes, so it zeroes them in LDS first and every tile is then a pure accumulation
// W += P Q (rs_update_col).  Only the look-ahead tile, whose Q fragment every wave reads, masks its seed
// (rs_update_tile<.., true>).  Storing P - E instead (a one short at every (pivot row, its column), added back where
// the inverse is read) saves the zeroing but forms the pivot row as q + (1/p - 1) q: 1/p - 1 is rounded to an
// absolute u, so the row loses log2 |p| bits, all of them for |p| >= 2^53, and the read-back (x - 1) + 1 loses u / |x|.
#ifndef RS_ABLATE
#define RS_ABLATE 0                   // diagnostic builds only (wrong results; timing with force_iters): 1 = no panel factoring (the chain
#endif                                //    wave's pivot steps), 2 = no trailing / look-ahead updates, 4 = no products, 8 = no mixing phase
#ifndef RS_STAMPS
#define RS_STAMPS 0                   // 1: diagnostic build -- the phase / cycle stamps of NEGF_CHAIN_STAMPS=1 are compiled in
#endif                                //    (NEGF_EXTRA_HIPCC_FLAGS=-DRS_STAMPS=1 python -m gaunegf_amd.build --force); the production
                                      //    kernel carries none of their branches

// maximum of a 32-bit key over the wave (all lanes active), wave-uniform result.  Four DPP steps inside the rows
// of 16 lanes leave the row maximum in every lane of a row; row_bcast:15 / row_bcast:31 (the GFX9 wave-reduction
// steps) then carry it across the rows into lane 63: seven vector instructions and one v_readlane.  With
// bound_ctrl and a zero "old" value the compiler folds each lane move into its v_max_u32 (v_max_u32_dpp);
// zero is the identity of the maximum, and the row steps read no invalid lane.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ unsigned rs_dpp_max_u32(unsigned k)
{
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)k, CTRL, ROW_MASK, 0xF, true);
    return o > k ? o : k;
}

__device__ __forceinline__ unsigned rs_wave_max_u32(unsigned k)
{
    k = rs_dpp_max_u32<0xB1>(k);            // quad_perm [1,0,3,2]
    k = rs_dpp_max_u32<0x4E>(k);            // quad_perm [2,3,0,1]
    k = rs_dpp_max_u32<0x141>(k);           // row_half_mirror
    k = rs_dpp_max_u32<0x140>(k);           // row_mirror: every lane of a row holds the row maximum
    k = rs_dpp_max_u32<0x142, 0xA>(k);      // row_bcast:15 into rows 1 and 3
    k = rs_dpp_max_u32<0x143, 0xC>(k);      // row_bcast:31 into rows 2 and 3: lane 63 holds the maximum
    return (unsigned)__builtin_amdgcn_readlane((int)k, 63);
}

// ---- remainder tiles.  n_c = 50 is three tiles of 16 and two more rows / columns; a fourth 16 x 16 tile for
// them costs as much as a full one.  v_mfma_f64_4x4x4_4b_f64 has the operand maps of the 16x16x4 instruction
// (A: lane l holds A[l&15][l>>4], B: B[l>>4][l&15]) and computes the four DIAGONAL 4 x 4 blocks of the
// 16 x 16 product, D_b[i][j] at lane 16 i + 4 b + j, in a quarter of the time (probed on MI355X,
// scripts/probe/mfma4x4_probe.hip).  Used in two ways when the last tile holds <= 4 rows / columns:
//   row strip  (last ROW tile):    every 4-row block of the A operand is loaded with the SAME rows
//              (row R0 + (l&3)); the B operand is the normal 16-column fragment.  D lane l holds element
//              (R0 + (l>>4), C0 + (l&15)) -- exactly component r = 0 of the 16 x 16 C layout.
//   column strip (last COLUMN tile): every 4-column block of the B operand holds the SAME columns
//              (column C0 + (l&3)); the A operand is the normal 16-row fragment.  D lane l holds element
//              (R0 + 4 ((l>>2)&3) + (l>>4), C0 + (l&3)).
// Both leave their result in component 0 of the tile's accumulator.
__device__ __forceinline__ void zmfma4(double& ar, double& ai, cplx pa, cplx qb)
{
    ar = __builtin_amdgcn_mfma_f64_4x4x4f64(pa.x, qb.x, ar, 0, 0, 0);
    ar = __builtin_amdgcn_mfma_f64_4x4x4f64(pa.y, -qb.y, ar, 0, 0, 0);
    ai = __builtin_amdgcn_mfma_f64_4x4x4f64(pa.x, qb.y, ai, 0, 0, 0);
    ai = __builtin_amdgcn_mfma_f64_4x4x4f64(pa.y, qb.x, ai, 0, 0, 0);
}
// pa * conj(b)
__device__ __forceinline__ void zmfma4_conjb(double& ar, double& ai, cplx pa, cplx b)
{
    ar = __builtin_amdgcn_mfma_f64_4x4x4f64(pa.x, b.x, ar, 0, 0, 0);
    ar = __builtin_amdgcn_mfma_f64_4x4x4f64(pa.y, b.y, ar, 0, 0, 0);
    ai = __builtin_amdgcn_mfma_f64_4x4x4f64(pa.y, b.x, ai, 0, 0, 0);
    ai = __builtin_amdgcn_mfma_f64_4x4x4f64(-pa.x, b.y, ai, 0, 0, 0);
}
#define RS_M3S(A, B, C, PR, PI, PS, QR, QI, QS) do { double a_ = (A)[0], b_ = (B)[0], c_ = (C)[0]; mfma3s(a_, b_, c_, PR, PI, PS, QR, QI, QS); (A)[0] = a_; (B)[0] = b_; (C)[0] = c_; } while (0)
#define RS_ZMFMA4(ACCR, ACCI, PA, QB) do { double r_ = (ACCR)[0], i_ = (ACCI)[0]; zmfma4(r_, i_, PA, QB); (ACCR)[0] = r_; (ACCI)[0] = i_; } while (0)
#define RS_ZMFMA4C(ACCR, ACCI, PA, QB) do { double r_ = (ACCR)[0], i_ = (ACCI)[0]; zmfma4_conjb(r_, i_, PA, QB); (ACCR)[0] = r_; (ACCI)[0] = i_; } while (0)

// ---- complex products by three real ones ("3M"): with p = pr + i pi, q = qr + i qi
//        a = sum pr qr,   b = sum pi qi,   c = sum (pr + pi)(qr + qi)     =>  p q       = (a - b) + i (c - a - b)
//        a, b as above,                    c = sum (pr + pi)(qr - qi)     =>  p conj(q) = (a + b) + i (c - a + b)
// i.e. 3 matrix instructions per tile and k-step instead of 4: a quarter of the matrix-pipe time of every product
// and update, for one or two additions per operand fragment.  The FP64 matrix instruction holds its SIMD's vector
// issue for most of its 64 cycles (rs_wave_role below), so matrix-pipe time is what the sweep is made of.
__device__ __forceinline__ void mfma3(d4& a, d4& b, d4& c, double pr, double pi, double ps, double qr, double qi, double qs)
{
    a = __builtin_amdgcn_mfma_f64_16x16x4f64(pr, qr, a, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f64_16x16x4f64(pi, qi, b, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(ps, qs, c, 0, 0, 0);
}
// the trailing / look-ahead updates (K = 8) run in 3M form in the 168-VGPR kernels: operand sums and a 12-instruction
// recombination per tile; below that pitch four products per tile and k-step, no vector work per tile at all
constexpr bool rs_upd_3m(int P) { return P > 35; }
// the same on the 4x4x4 instruction (remainder strips, one value per lane)
__device__ __forceinline__ void mfma3s(double& a, double& b, double& c, double pr, double pi, double ps, double qr, double qi, double qs)
{
    a = __builtin_amdgcn_mfma_f64_4x4x4f64(pr, qr, a, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f64_4x4x4f64(pi, qi, b, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f64_4x4x4f64(ps, qs, c, 0, 0, 0);
}

// Hide a loop-invariant value from the optimiser: without this LLVM hoists every (tile, k-step)
// LDS address of the sweep out of the fixed-point loop -- hundreds of live address registers that
// are then spilled to scratch and reloaded inside the MFMA loops.
template <class T>
__device__ __forceinline__ T rs_opaque(T v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// ---- pinned arithmetic.  The compiler contracts a * b + c * d into one product and one fused multiply-add, and WHICH
// product is fused is its choice per basic block: code that moves such an expression into another block (a branch
// around it, a loop split in two, an instantiation without the column tests) may change the last bit of every result.
// Where the chain kernel restructures such code the expressions are therefore written out -- the fused operation as
// __builtin_fma, the rounded product as a product -- in the form the compiler chose for the generic code (read from its
// ISA; scripts/isa_fp64_compare.py holds a build to it), inside functions with contraction switched off, so that
// nothing is fused or unfused behind them.
// the stopping test of one element: |g_new - g|^2 > conv^2 max(|g_new|^2, 1e-24) (over) / <= (ok); an element that does
// not exist (!v) is neither over nor not ok, a NaN element is neither over nor ok
__device__ __forceinline__ void rs_stop_test(cplx gn, cplx go, double conv2, bool v, bool& over, bool& ok)
{
#pragma clang fp contract(off)
    const double dx = gn.x - go.x, dy = gn.y - go.y;
    const double num2 = __builtin_fma(dx, dx, dy * dy);
    const double den2 = fmax(__builtin_fma(gn.x, gn.x, gn.y * gn.y), 1e-24);
    const double thr = conv2 * den2;
    over |= v && num2 > thr;
    ok &= !v || num2 <= thr;
}
// the mixing of one element: r g_new + (1 - r) g
__device__ __forceinline__ cplx rs_mix(cplx gn, cplx go, double rf, double rf1)
{
#pragma clang fp contract(off)
    return cmake(__builtin_fma(go.x, rf1, gn.x * rf), __builtin_fma(go.y, rf1, gn.y * rf));
}

// ---- panel [p0, p0+pw) factored by ONE wave: lane = row, 16 complex per lane, no barrier inside.  A wave
// alone issues one instruction per ~4 cycles whatever its kind, and the vector ALU of its SIMD is what
// the co-resident workgroups compete for, so the column step is written for instruction count:
//   * pivot search: |re|+|im| (izamax metric) compared on the HIGH WORD of the double -- sign 0, exponent,
//     20 mantissa bits -- with one v_max_u32 per DPP step; the pivot is the lowest row whose high word
//     equals the maximum (ballot + find-first): the LAPACK choice up to ties within 2^-20 relative, which
//     go to the lower row as LAPACK's exact ties do;
//   * the pivot row reaches the other lanes through a 256-byte LDS line (the pivot lane writes its 16
//     values, every lane reads them back: 32 LDS instructions instead of 68 v_readlane, and off the VALU);
//   * 1/|pivot|^2 by v_rcp_f64 and two Newton steps (the pivots of these matrices are far from the
//     overflow / denormal range the IEEE division sequence guards).
// A pivot row is not scaled at its column step (multiplier 0, a one in the pivot column) but once at
// the end of the panel: the later steps act linearly on it, and every lane runs the same select-free update.
//
// ---- pinned factoring.  The stage schedule (rs_inverse_sched) factors its narrow last panel in an instantiation of NBW = 4
// columns instead of 8, with the arithmetic pinned to what the compiler makes of the 8-column instantiation in the generic
// loop of the same class (read from the ISA of chain1d_rs_kernel<35 | 51, ...>, every column step, the plain and the
// round-robin instantiations):
//     a b          = ( fma(ax, bx, -(ay by)),  fma(ay, bx, ax by) )                       pivot-row scaling, a[j] ip
//     a + coef rb  = ( fma(-rby, cy, fma(rbx, cx, ax)),  fma(rbx, cy, fma(rby, cx, ay)) )
//     |pv|^2       = fma(pvy, pvy, pvx pvx) -- but fma(pvx, pvx, pvy pvy) in the LAST of the eight column steps, the one
//                    place where the compiler's choice differs from step to step (in every instantiation the same way);
//     Newton: sc = fma(sc, fma(-d, sc, 1), sc);   ip = (pvx sc, -pvy sc)
__device__ __forceinline__ cplx rs_cmul_pinned(cplx a, cplx b)
{
#pragma clang fp contract(off)
    return cmake(__builtin_fma(a.x, b.x, -(a.y * b.y)), __builtin_fma(a.y, b.x, a.x * b.y));
}
// a b of the deferred pivot-row scaling.  The same value as rs_cmul_pinned; the rounded product of the real part passes through
// an empty asm so that its sign stays on the addend of the fused operation (v_fma r r -r, the instruction the generic code
// holds there and scripts/isa_fp64_compare.py counts) instead of moving into a factor of the product
__device__ __forceinline__ cplx rs_scale_pinned(cplx a, cplx b)
{
#pragma clang fp contract(off)
    double t = a.y * b.y;
    asm("" : "+v"(t));
    return cmake(__builtin_fma(a.x, b.x, -t), __builtin_fma(a.y, b.x, a.x * b.y));
}
__device__ __forceinline__ cplx rs_cfma_pinned(cplx a, cplx coef, cplx rb)
{
#pragma clang fp contract(off)
    return cmake(__builtin_fma(-rb.y, coef.y, __builtin_fma(rb.x, coef.x, a.x)), __builtin_fma(rb.x, coef.y, __builtin_fma(rb.y, coef.x, a.y)));
}
__device__ __forceinline__ cplx rs_pivot_recip_pinned(cplx pv, bool last /* column step 7 of rs_factor's eight */)
{
#pragma clang fp contract(off)
    const double d = last ? __builtin_fma(pv.x, pv.x, pv.y * pv.y) : __builtin_fma(pv.y, pv.y, pv.x * pv.x);
    double sc = __builtin_amdgcn_rcp(d);
    sc = __builtin_fma(sc, __builtin_fma(-d, sc, 1.0), sc);
    sc = __builtin_fma(sc, __builtin_fma(-d, sc, 1.0), sc);
    return cmake(pv.x * sc, -pv.y * sc);
}
// the three arithmetic sites of rs_factor: the compiler's contraction (the generic loop) or the pinned form
template <bool PINNED>
__device__ __forceinline__ cplx rs_factor_recip(cplx pv, bool last)
{
    if constexpr (PINNED) return rs_pivot_recip_pinned(pv, last);
    else {
        const double d = pv.x * pv.x + pv.y * pv.y;
        double sc = __builtin_amdgcn_rcp(d);
        sc = fma(sc, fma(-d, sc, 1.0), sc);
        sc = fma(sc, fma(-d, sc, 1.0), sc);
        return cmake(pv.x * sc, -pv.y * sc);
    }
}
template <bool PINNED>
__device__ __forceinline__ cplx rs_factor_cmul(cplx a, cplx b)
{
    if constexpr (PINNED) return rs_cmul_pinned(a, b); else return cmul(a, b);
}
template <bool PINNED>
__device__ __forceinline__ cplx rs_factor_cfma(cplx a, cplx coef, cplx rb)
{
    if constexpr (PINNED) return rs_cfma_pinned(a, coef, rb); else return cfma(a, coef, rb);
}

// NBW: columns the code is written for (pw <= NBW).  PINNED: the arithmetic in the written-out form above (rs_*_pinned).
// avail: the rows that may still become pivots, one bit per lane in a scalar register pair: the column steps combine it
// with their compare masks by scalar and / and-not, and no lane carries a flag of its own through selects.  The mask belongs
// to the CALLER.  The stage schedule starts every inverse with rs_rows_mask(n) and hands the same mask to every panel
// (reread = false): only the factoring wave writes colof during an inverse, so the mask IS colof[r] < 0, without the LDS
// round trip behind the look-ahead barrier.  The generic loop has it read from colof at every panel (reread = true).
// ROWS: rows of the work matrix (16 T16).  The panel is loaded WITHOUT a test on r < n: the lanes n <= r < 64 read row
// min(r, ROWS - 1) -- inside W in every class -- and carry whatever lies there through the column steps (zero padding, or,
// when three workgroups share a CU, the old iterate's slots, Inf / NaN when the iterate is).  Nothing of it is used: such a
// lane is never in avail, so its key is 0 (usable = finite & avail) and it is never a candidate, never is_piv, never writes
// the LDS line or a table entry, and its write-back is under r < n.
__device__ __forceinline__ unsigned long long rs_rows_mask(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }   // ballot(lane < n), scalar

template <int P, int ROWS, int NBW = RS_NB, bool PINNED = false>
__device__ __forceinline__ void rs_factor(int n, cplx* W, int* pivrow, int* colof, cplx* rowline /*[16] LDS*/,
                                          int p0, int pw, int lane, unsigned long long& avail, bool reread,
                                          unsigned long long* fst = nullptr /* diagnostic: cycle stamps of column step 4 */,
                                          int* pivoff = nullptr /* the stage schedule: the pivot rows as byte offsets, see rs_at */)
{
    const int r = rs_opaque(lane);                      // (see rs_opaque: nothing derived from the lane index is
    cplx a[NBW];                                        //  hoisted out of the fixed-point loop and kept alive)
    if (reread) {
        int cr = 0;
        if (r < n) cr = colof[r];
        avail = __builtin_amdgcn_ballot_w64(cr < 0);
    }
    cplx myip = cmake(1.0, 0.0);
    cplx* wrow = W + min(r, ROWS - 1) * P + p0;         // (the row itself wherever it is written back: r < n)
#pragma unroll
    for (int s = 0; s < NBW; ++s) {
        const cplx v = wrow[s];
        const bool ok = s < pw;                         // (folds where pw is a constant: the full panels of the stage schedule)
        a[s] = cmake(ok ? v.x : 0.0, ok ? v.y : 0.0);
    }
    // the pivot tables of the panel, stored once behind the last column step (nobody reads them before the barrier that closes
    // the stage): lane j holds pivrow[p0 + j], the pivot lane of a step the column it took.  -1: nothing to store -- the
    // lanes j >= pw, the rows that were no pivot here, and a step that found no row available (it leaves both tables alone)
    int prow = -1, mycol = -1;
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        if (j < pw) {
            const bool stamp_here = fst && j == 4;
            unsigned long long tq0 = 0, tq1 = 0, tq2 = 0, tq3 = 0, tq4 = 0;
            if (stamp_here) tq0 = __builtin_amdgcn_s_memtime();
            const double v = cabs1(a[j]);
            const bool usable = __builtin_amdgcn_inverse_ballot_w64(__builtin_amdgcn_ballot_w64(v == v) & avail);
            const unsigned hi = usable ? (unsigned)__double2hiint(v) : 0u;
            const unsigned m = rs_wave_max_u32(hi);
            // the lowest available row whose key equals the maximum.  With no usable candidate (m == 0: a zero / NaN column)
            // every available row has the key 0, and that is the lowest available row; with none available no lane
            // equals -1 and the step has no pivot lane.  One straight line, no branch on m.
            const unsigned long long cand = __builtin_amdgcn_ballot_w64(hi == m) & avail;
            const int pphys = cand ? __builtin_ctzll(cand) : -1;
            if (stamp_here) tq1 = __builtin_amdgcn_s_memtime();
            const bool is_piv = r == pphys;
            avail &= ~__builtin_amdgcn_ballot_w64(is_piv);
            cplx rb[NBW];
            // through a 256-byte LDS line: one lane writes its 16 values, all lanes read them back.  The wave-level
            // barriers keep the compiler from ordering the two sides of the divergent branch the other way round
            // (it does, without them), the LDS then executes the wave's instructions in order
            __builtin_amdgcn_wave_barrier();            // the reads of the previous column step are issued
            asm("v_writelane_b32 %0, %1, %2" : "+v"(prow) : "s"(pphys), "n"(j));
            if (is_piv) {
#pragma unroll
                for (int s = 0; s < NBW; ++s) rowline[s] = a[s];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int s = 0; s < NBW; ++s) rb[s] = rowline[s];
            if (stamp_here) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); tq2 = __builtin_amdgcn_s_memtime(); }
            const cplx ip = rs_factor_recip<PINNED>(rb[j], j == RS_NB - 1);
            const cplx mf = cneg(rs_factor_cmul<PINNED>(a[j], ip));
            // the pivot lane's own values -- multiplier 0, a one in the pivot column, its reciprocal -- are moves under an exec
            // mask that holds that lane alone, not selects in every lane (the empty asm keeps the branch from becoming
            // selects again).  The lane stays in the update below: a + 0 rb, NaN where its row is not finite.  The imaginary
            // part of the new a[j] is that of the multiplier in every lane.
            cplx coef = mf;
            cplx aj = mf;
            if (is_piv) {
                coef = cmake(0.0, 0.0); aj = cmake(1.0, 0.0); myip = ip;
                mycol = p0 + j;
                asm("" : "+v"(aj.x));
            }
            if (stamp_here) { asm volatile("" :: "v"(coef.x), "v"(coef.y)); tq3 = __builtin_amdgcn_s_memtime(); }
#pragma unroll
            for (int s = 0; s < NBW; ++s) a[s] = rs_factor_cfma<PINNED>(a[s], coef, rb[s]);
            if (stamp_here) {
#pragma unroll
                for (int s = 0; s < NBW; ++s) asm volatile("" :: "v"(a[s].x), "v"(a[s].y));
                tq4 = __builtin_amdgcn_s_memtime();
                if (lane == 0) { fst[0] = tq0; fst[1] = tq1; fst[2] = tq2; fst[3] = tq3; fst[4] = tq4; }
            }
            a[j] = aj;
        }
    }
    // the deferred pivot-row scaling, pinned in every instantiation: where no test lies between them (the full panels of the
    // stage schedule) it shares a basic block with the last column step's update, and the compiler's choice of the fused
    // product in its imaginary part then follows whatever else that block holds
    if (r < n) {
#pragma unroll
        for (int s = 0; s < NBW; ++s)
            if (s < pw) wrow[s] = PINNED ? rs_cmul_pinned(a[s], myip) : rs_scale_pinned(a[s], myip);
    }
    if (prow >= 0) {
        pivrow[p0 + r] = prow;
        if (pivoff) pivoff[p0 + r] = prow * (P * (int)sizeof(cplx));
    }
    if (mycol >= 0) colof[r] = mycol;
}

// ---- trailing update with panel [p0, p0+pw), in place:
//        W[i][col] = (i pivot row of the panel ? 0 : W[i][col]) + P[i][:] Q[:][col]
// (the 0 by a mask of the seed, MASK, or because the pivot rows were zeroed after Q was read: rs_zero_pivot_rows)
// A Q fragment holds the panel's pivot rows in the columns of one column tile (B operand); for the
// column-strip tile TR every 4-column block holds the same columns TR*16 + (l&3) (see mfma3s).
template <int P, int NKS, int TR /* last tile when it is a remainder strip, else -1 */, bool FULL = false /* pw == 4 NKS is known */>
__device__ __forceinline__ void rs_load_qf(const cplx* W, const int* pivrow, int tj, int p0, int pw, int fi, int fk,
                                           cplx (&qf)[NKS])
{
    const int col = (TR >= 0 && tj == TR) ? TR * 16 + (fi & 3) : tj * 16 + fi;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int k = ks * 4 + fk;
        const cplx v = W[pivrow[p0 + k] * P + col];          // k >= pw: some valid row, zeroed below
        const bool ok = FULL || k < pw;
        qf[ks] = cmake(ok ? v.x : 0.0, ok ? v.y : 0.0);
    }
}

// the panel's pivot rows in the columns of this lane's Q fragment (rs_load_qf) that are to be updated, [clo, chi) inside
// the matrix, are set to zero: the owner of those columns calls it after its Q fragment is loaded (a wave's LDS
// operations execute in order, and the stores may alias the loads, so neither the compiler nor the LDS reorders them)
template <int P, int NKS, int TR>
__device__ __forceinline__ void rs_zero_pivot_rows(int n, cplx* W, const int* pivrow, int tj, int p0, int pw, int fi, int fk,
                                                   int clo, int chi)
{
    const int col = (TR >= 0 && tj == TR) ? TR * 16 + (fi & 3) : tj * 16 + fi;
    if (col >= clo && col < chi && col < n) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int k = ks * 4 + fk;
            if (k < pw) W[pivrow[p0 + k] * P + col] = cmake(0.0, 0.0);
        }
    }
}

// one tile (ti, tj): a full 16 x 16 tile, or a row / column strip (one value per lane, corner: one block)
template <int P, int NKS, int TR, bool MASK /* seed the pivot rows of the panel with 0 (else they already are 0) */>
__device__ __forceinline__ void rs_update_tile(int n, cplx* W, const int* colof, int ti, int tj, int p0, int pw,
                                               int fi, int fk, const cplx (&qf)[NKS], int clo, int chi /* columns [clo, chi) are stored */)
{
    const bool rowstrip = TR >= 0 && ti == TR, colstrip = TR >= 0 && tj == TR;
    if (!rowstrip && !colstrip) {
        cplx* cbase = W + (ti * 16 + fk) * P + tj * 16 + fi;
        const cplx* pbase = W + (ti * 16 + fi) * P + p0 + fk;
        cplx cv[4], pa[NKS];
        int cf[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { if (MASK) cf[r] = colof[ti * 16 + fk + 4 * r]; cv[r] = cbase[4 * r * P]; }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) pa[ks] = pbase[ks * 4];
        constexpr bool M3 = rs_upd_3m(P);
        d4 ua, ub = {0, 0, 0, 0}, uc;                       // accumulators, seeded with the old tile
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool keep = !MASK || !(cf[r] >= p0 && cf[r] < p0 + pw);
            ua[r] = keep ? cv[r].x : 0.0; uc[r] = keep ? (M3 ? cv[r].x + cv[r].y : cv[r].y) : 0.0;
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            if (M3) mfma3(ua, ub, uc, pa[ks].x, pa[ks].y, pa[ks].x + pa[ks].y, qf[ks].x, qf[ks].y, qf[ks].x + qf[ks].y);
            else zmfma(ua, uc, pa[ks], qf[ks]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ti * 16 + fk + 4 * r;
            const int cj = tj * 16 + fi;
            if (i < n && cj < n && cj >= clo && cj < chi) cbase[4 * r * P] = M3 ? cmake(ua[r] - ub[r], uc[r] - ua[r] - ub[r]) : cmake(ua[r], uc[r]);
        }
    } else {
        const int row = rowstrip ? TR * 16 + fk : ti * 16 + 4 * (fi >> 2) + fk;
        const int col = colstrip ? TR * 16 + (fi & 3) : tj * 16 + fi;
        const bool mine = !(rowstrip && colstrip) || (fi >> 2) == 0;      // the corner block exists four times
        const cplx* prow = W + (rowstrip ? TR * 16 + (fi & 3) : ti * 16 + fi) * P + p0 + fk;
        cplx* cptr = W + row * P + col;
        const int cf = MASK ? colof[row] : -1;
        const cplx cv = *cptr;
        cplx pa[NKS];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) pa[ks] = prow[ks * 4];
        const bool keep = !MASK || !(cf >= p0 && cf < p0 + pw);
        double ua = keep ? cv.x : 0.0, ub = 0.0, uc = keep ? cv.x + cv.y : 0.0;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
            mfma3s(ua, ub, uc, pa[ks].x, pa[ks].y, pa[ks].x + pa[ks].y, qf[ks].x, qf[ks].y, qf[ks].x + qf[ks].y);
        if (mine && row < n && col < n && col >= clo && col < chi) *cptr = cmake(ua - ub, uc - ua - ub);
    }
}

// ---- half tiles.  With panels of 8 many updates may write only 8 columns [c0, c0 + 8) of a full column tile: the
// look-ahead, the other half of the panel's own tile, the other half of the next tile.  Such a 16 x 8 block is two
// column strips at base columns c0 and c0 + 4 (see the remainder tiles above): one P fragment, one Q fragment per strip
// (every 4-column block of the B operand holds the strip's columns c0 + 4 s + (l&3)), 2 x NKS x 3 4x4x4 instructions
// -- half the matrix-pipe time of the whole tile -- and TWO values per lane, elements
// (ti*16 + 4 (fi>>2) + fk, c0 + 4 s + (fi&3)): half the C loads, seeds, recombinations and stores as well.
constexpr bool rs_half_strips(int nks) { return nks == RS_NB / 4; }

template <int P, int NKS, bool FULL = false>
__device__ __forceinline__ void rs_load_qh(const cplx* W, const int* pivrow, int c0, int p0, int pw, int fi, int fk,
                                           cplx (&qh)[2][NKS])
{
    const int col = c0 + (fi & 3);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int k = ks * 4 + fk;
        const cplx* q = W + pivrow[p0 + k] * P + col;        // k >= pw: some valid row, zeroed below
        const cplx v0 = q[0], v1 = q[4];
        const bool ok = FULL || k < pw;
        qh[0][ks] = cmake(ok ? v0.x : 0.0, ok ? v0.y : 0.0);
        qh[1][ks] = cmake(ok ? v1.x : 0.0, ok ? v1.y : 0.0);
    }
}

// the two strips of one row tile: cv (+)= pa qh, cv = this lane's two C elements (seeds, then results)
template <int P, int NKS>
__device__ __forceinline__ void rs_half_mma(cplx (&cv)[2], const cplx (&pa)[NKS], const cplx (&qh)[2][NKS], const double (&qs)[2][NKS])
{
    constexpr bool M3 = rs_upd_3m(P);
    if (M3) {
        double ua[2], ub[2] = {0.0, 0.0}, uc[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) { ua[s] = cv[s].x; uc[s] = cv[s].x + cv[s].y; }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const double ps = pa[ks].x + pa[ks].y;
#pragma unroll
            for (int s = 0; s < 2; ++s) mfma3s(ua[s], ub[s], uc[s], pa[ks].x, pa[ks].y, ps, qh[s][ks].x, qh[s][ks].y, qs[s][ks]);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) cv[s] = cmake(ua[s] - ub[s], uc[s] - ua[s] - ub[s]);
    } else {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int s = 0; s < 2; ++s) zmfma4(cv[s].x, cv[s].y, pa[ks], qh[s][ks]);
    }
}

// one half tile (row tile ti, columns [c0, c0 + 8) inside the matrix) with its own operand loads: the look-ahead
template <int P, int NKS, bool FULLROWS /* all 16 rows of the tile lie inside the matrix */, bool MASK>
__device__ __forceinline__ void rs_update_half(int n, cplx* W, const int* colof, int ti, int p0, int pw, int fi, int fk,
                                               const cplx (&qh)[2][NKS], int c0)
{
    const int row = ti * 16 + 4 * (fi >> 2) + fk;
    cplx* cptr = W + row * P + c0 + (fi & 3);
    const cplx* pbase = W + (ti * 16 + fi) * P + p0 + fk;
    const int cf = MASK ? colof[row] : -1;
    cplx cv[2] = {cptr[0], cptr[4]}, pa[NKS];
    double qs[2][NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) { pa[ks] = pbase[ks * 4]; qs[0][ks] = qh[0][ks].x + qh[0][ks].y; qs[1][ks] = qh[1][ks].x + qh[1][ks].y; }
    if (MASK && cf >= p0 && cf < p0 + pw) { cv[0] = cmake(0.0, 0.0); cv[1] = cmake(0.0, 0.0); }   // a pivot row of the panel (both values: one row)
    rs_half_mma<P, NKS>(cv, pa, qh, qs);
    if (FULLROWS || row < n) { cptr[0] = cv[0]; cptr[4] = cv[1]; }
}

// column tile tj, all row tiles, by the wave that owns the column tile in this stage.  The Q fragment is read
// into registers before the first store, so the owner needs no snapshot of the pivot rows; it then zeroes them, so
// that every tile of the column is a pure accumulation.
template <int T16, int P, int NKS, int TR>
__device__ __forceinline__ void rs_update_col(int n, cplx* W, const int* pivrow, const int* colof,
                                              int tj, int p0, int pw, int lane, int clo, int chi)
{
    constexpr int FT = TR >= 0 ? TR : T16;                   // full row tiles
    const int fi = rs_opaque(lane & 15), fk = rs_opaque(lane >> 4);
    cplx qf[NKS];
    if (rs_half_strips(NKS) && chi - clo == 8 && chi <= n && !(TR >= 0 && tj == TR)) {
        // a half tile: two column strips per row tile (rs_half_mma), row tile ti+1 requested before tile ti is stored
        cplx qh[2][NKS];
        double qs[2][NKS];
        if (TR >= 0) rs_load_qf<P, NKS, TR>(W, pivrow, tj, p0, pw, fi, fk, qf);       // the row strip's 16-column fragment
        rs_load_qh<P, NKS>(W, pivrow, clo, p0, pw, fi, fk, qh);
        rs_zero_pivot_rows<P, NKS, TR>(n, W, pivrow, tj, p0, pw, fi, fk, clo, chi);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) { qs[0][ks] = qh[0][ks].x + qh[0][ks].y; qs[1][ks] = qh[1][ks].x + qh[1][ks].y; }
        const int row = 4 * (fi >> 2) + fk;
        cplx* cbase = W + row * P + clo + (fi & 3);          // C elements (ti*16 + row, clo + 4 s + (fi&3))
        const cplx* pbase = W + fi * P + p0 + fk;
        cplx cv[2][2], pa[2][NKS];
        auto fetch = [&](int ti, int s) __attribute__((always_inline)) {
            cv[s][0] = cbase[ti * 16 * P]; cv[s][1] = cbase[ti * 16 * P + 4];
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) pa[s][ks] = pbase[ti * 16 * P + ks * 4];
        };
        fetch(0, 0);
#pragma unroll
        for (int ti = 0; ti < FT; ++ti) {
            const int s = ti & 1;
            if (ti + 1 < FT) fetch(ti + 1, s ^ 1);
            rs_half_mma<P, NKS>(cv[s], pa[s], qh, qs);
            if (TR >= 0 || ti * 16 + row < n) { cbase[ti * 16 * P] = cv[s][0]; cbase[ti * 16 * P + 4] = cv[s][1]; }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (TR >= 0) rs_update_tile<P, NKS, TR, false>(n, W, colof, TR, tj, p0, pw, fi, fk, qf, clo, chi);    // the row strip
        return;
    }
    rs_load_qf<P, NKS, TR>(W, pivrow, tj, p0, pw, fi, fk, qf);
    rs_zero_pivot_rows<P, NKS, TR>(n, W, pivrow, tj, p0, pw, fi, fk, clo, chi);
    if (TR >= 0 && tj == TR) {                               // the column strip: every tile on the 4x4x4 instruction
#pragma unroll
        for (int ti = 0; ti < T16; ++ti) {
            rs_update_tile<P, NKS, TR, false>(n, W, colof, ti, tj, p0, pw, fi, fk, qf, clo, chi);
            __builtin_amdgcn_sched_barrier(0);
        }
        return;
    }
    const int col = tj * 16 + fi;
    const bool colin = col >= clo && col < chi;             // this lane's column is one of those to be updated
    constexpr bool M3 = rs_upd_3m(P);
    double qs[NKS];                                          // 3M: re + im of the Q fragment, once per column tile
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qs[ks] = qf[ks].x + qf[ks].y;
    cplx* cbase = W + fk * P + col;                          // C tile element (ti*16 + fk + 4r, col)
    const cplx* pbase = W + fi * P + p0 + fk;                // P operand element (ti*16 + fi, p0 + ks*4 + fk)
    // the operands of row tile ti+1 are requested before tile ti is stored (LDS operations of a wave
    // execute in order, and tile ti+1 shares no element with tile ti), so that the loads overlap the MFMAs
    cplx cv[2][4], pa[2][NKS];
    auto fetch = [&](int ti, int s) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) cv[s][r] = cbase[(ti * 16 + 4 * r) * P];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) pa[s][ks] = pbase[ti * 16 * P + ks * 4];   // k >= pw pairs with qf == 0 (finite element)
    };
    fetch(0, 0);
#pragma unroll
    for (int ti = 0; ti < FT; ++ti) {
        const int s = ti & 1;
        if (ti + 1 < FT) fetch(ti + 1, s ^ 1);
        d4 ua, ub = {0, 0, 0, 0}, uc;
#pragma unroll
        for (int r = 0; r < 4; ++r) { ua[r] = cv[s][r].x; uc[r] = M3 ? cv[s][r].x + cv[s][r].y : cv[s][r].y; }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            if (M3) mfma3(ua, ub, uc, pa[s][ks].x, pa[s][ks].y, pa[s][ks].x + pa[s][ks].y, qf[ks].x, qf[ks].y, qs[ks]);
            else zmfma(ua, uc, pa[s][ks], qf[ks]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ti * 16 + fk + 4 * r;
            // with a remainder strip (TR >= 0) the full tiles lie inside the matrix: rows, columns < 16 TR < n
            if (colin && (TR >= 0 || (i < n && col < n))) cbase[(ti * 16 + 4 * r) * P] = M3 ? cmake(ua[r] - ub[r], uc[r] - ua[r] - ub[r]) : cmake(ua[r], uc[r]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (TR >= 0) rs_update_tile<P, NKS, TR, false>(n, W, colof, TR, tj, p0, pw, fi, fk, qf, clo, chi);    // the row strip
}

// In-place blocked Gauss-Jordan reduction of the n x n matrix W (LDS, pitch P) with implicit
// pivoting.  On return  inv[i][j] = W[pivrow[i]][colof[j]].  All 256 threads call it; colof[] must be
// -1 and visible (a barrier since it was reset).  Stage s: all waves apply panel s to the column tile of
// panel s+1 (one row tile each, two barriers), then one wave factors panel s+1 while the other waves apply
// panel s to the remaining column tiles (one owner per column tile, no barrier), one barrier at the end.
template <int T16, int P, int TR>
__device__ __forceinline__ void rs_inverse(int n, cplx* W, int* pivrow, int* colof, cplx* rowline, int tid,
                                           int wave /* role number of this wave, see rs_wave_role */, bool fixed_fw,
                                           unsigned long long* st = nullptr)
{
    const int lane = tid & 63;
    int sti = 0;
    auto stamp = [&]() __attribute__((always_inline)) { if (st && tid == 0) st[sti] = __builtin_amdgcn_s_memrealtime(); ++sti; };
    const int npanels = (n + RS_NB - 1) / RS_NB;
    const int ntiles = (n + 15) >> 4;
    for (int sgi = -1; sgi < npanels; ++sgi) {
        const bool has_cur = sgi >= 0, has_next = sgi + 1 < npanels;
        const int p0 = has_cur ? sgi * RS_NB : 0, pw = has_cur ? min(RS_NB, n - p0) : 0;
        const int n0 = (sgi + 1) * RS_NB, nw = has_next ? min(RS_NB, n - n0) : 0;
        const int tp = p0 >> 4, tl = n0 >> 4;                   // column tiles of the panel and of the next one
        // the wave that factors panel sgi+1: the chain wave (role RS_WAVES-1), or -- roles by wave number -- each in turn
        const int fw = fixed_fw ? RS_WAVES - 1 : (sgi + 1) & (RS_WAVES - 1);
        if (has_cur && has_next) {
            // look-ahead: the columns of panel sgi+1 (a whole column tile, or one half of one), one row tile per wave
            // (T16 <= 4 = number of waves)
            const int fi = rs_opaque(lane & 15), fk = rs_opaque(lane >> 4);
            // the next panel is half of a full column tile: this wave's row tile is a half tile, two column strips with a Q
            // fragment each (the row strip keeps its own form: one 4x4x4 instruction per k-step covers 16 columns already)
            const bool half = n0 + RS_NB <= n && !(TR >= 0 && (tl == TR || wave == TR));
            cplx qh[2][RS_NB / 4];
            cplx (&qf)[RS_NB / 4] = qh[0];                      // (one or the other)
            if (half) rs_load_qh<P, RS_NB / 4>(W, pivrow, n0, p0, pw, fi, fk, qh);
            else rs_load_qf<P, RS_NB / 4, TR>(W, pivrow, tl, p0, pw, fi, fk, qf);
            __syncthreads();
            if (!(RS_ABLATE & 2) && wave < T16 && wave * 16 < n) {
                if (half) rs_update_half<P, RS_NB / 4, TR >= 0, true>(n, W, colof, wave, p0, pw, fi, fk, qh, n0);
                else rs_update_tile<P, RS_NB / 4, TR, true>(n, W, colof, wave, tl, p0, pw, fi, fk, qf, n0, n0 + RS_NB);
            }
            __syncthreads();
        }
        if (has_cur) {
            // the other columns, tile by tile, one owner per tile (the owner reads its Q fragment before it writes):
            // dealt to the three waves that do not factor, to all four after the last panel.  A tile's columns minus
            // the panel's own and minus the look-ahead columns (panels of 8: one half of the panel's tile remains when
            // the panel is its upper half, one half of the next tile when the look-ahead took its lower half).
            const int team = has_next ? RS_WAVES - 1 : RS_WAVES;
            const int me = has_next ? ((wave - fw - 1) & (RS_WAVES - 1)) : wave;
            int cnt = 0;
#pragma unroll 1
            for (int tj = 0; tj < ntiles; ++tj) {
                int clo = tj * 16, chi = tj * 16 + 16;
                if (tj == tp) { if (p0 & 8) chi = p0; else clo = p0 + RS_NB; }
                if (has_next && tj == tl) { if (n0 & 8) chi = min(chi, n0); else clo = max(clo, n0 + RS_NB); }
                if (clo >= chi || clo >= n) continue;
                const bool mine = (!has_next || wave != fw) && (cnt % team == me);
                ++cnt;
                if (mine && !(RS_ABLATE & 2)) {
                    // a narrow last panel (<= 4 columns) runs one k-step
                    if (pw <= 4) rs_update_col<T16, P, 1, TR>(n, W, pivrow, colof, tj, p0, pw, lane, clo, chi);
                    else rs_update_col<T16, P, RS_NB / 4, TR>(n, W, pivrow, colof, tj, p0, pw, lane, clo, chi);
                }
            }
        }
        if (has_next && wave == fw) {
            if (st && lane == 0) st[16 + 2 * (sgi + 1)] = __builtin_amdgcn_s_memrealtime();
            // the factoring wave is its workgroup's critical path (the others wait for it at the barrier):
            // it goes first when it shares its SIMD's issue slots with waves of the other workgroups
            __builtin_amdgcn_s_setprio(3);
            // (the generic loop reads the available rows from colof at every panel: the factoring wave changes with the panel
            // when the roles go by wave number, and a mask carried through this loop costs classes 57 / 65 scratch)
            unsigned long long avail = 0;
            if (!(RS_ABLATE & 1)) rs_factor<P, 16 * T16>(n, W, pivrow, colof, rowline, n0, nw, lane, avail, true, (st && sgi + 1 == 1) ? st + 40 : nullptr);
            else if (lane < nw) { pivrow[n0 + lane] = n0 + lane; colof[n0 + lane] = n0 + lane; }
            __builtin_amdgcn_s_setprio(0);
            if (st && lane == 0) st[17 + 2 * (sgi + 1)] = __builtin_amdgcn_s_memrealtime();
        }
        stamp();
        __syncthreads();                 // panel sgi+1 (columns of W, pivrow/colof) and the update complete
    }
}

// ---- the compile-time stage schedule of the remainder-strip classes (chain_rs_sched.h).  In such a class
// (TR full tiles and a strip, every contact of the launch with 16 TR < n <= 16 TR + 4) with the roles by SIMD the generic
// loop above derives, in every stage of every sweep, what never changes: 2 TR panels that are exactly 8 wide and lie inside
// full tiles, then one narrow panel; role 3 factors; the column-tile jobs of a stage and their owners.  rs_inverse_sched
// runs the same operations on the same operands in the same order with all of that fixed: the jobs of a role come out of one
// 64-bit constant, the kind of a job selects one of three bodies (whole tile, half tile, column strip) that take the tile
// index and the panel's first column as scalars -- one copy of each in the instruction stream --, a full panel's Q
// fragments carry no selects, and full tiles are stored without tests (the factoring wave: rs_factor, pinned factoring).
// (TR = 1, class 19, keeps the generic loop: with the schedule its kernels need 128 VGPRs and 20 - 48 bytes of scratch
//  instead of 110 and none, and the two-per-CU ones fall from four waves per SIMD to three)
constexpr bool rs_stage_sched(int TR) { return TR >= 2 && TR <= 3 && !RS_ABLATE; }     // (an ablation build runs the generic loop, which carries the ablations)

// ---- what a lane of a matrix wave addresses with, made ONCE per inverse (rs_lane at the top of rs_inverse_sched) and handed to
// every update body of its stages.  Every body used to derive its own copies behind rs_opaque -- a quarter-rate v_mul_lo_u32
// and two or three adds per base and body, on SIMDs where another workgroup's matrix instruction holds vector issue.  The
// values pass through rs_opaque here as well, inside the sweep loop: they live from the top of an inverse to its end, while
// the products' accumulators are dead, and are no invariants of the fixed-point loop (see rs_opaque).
//   fi, fk: the lane's place in an operand fragment (l & 15, l >> 4);
//   pb = fi P + fk: the P fragment, element (16 ti + fi, p0 + 4 ks + fk) at W + pb + 16 ti P + p0 + 4 ks;
//   cb = fk P + fi: the C tile, element (16 ti + fk + 4 r, 16 tj + fi) at W + cb + (16 ti + 4 r) P + 16 tj;
//   sb = (4 (fi >> 2) + fk) P + (fi & 3): a column strip's C element (16 ti + 4 (fi >> 2) + fk, c0 + (fi & 3)) at W + sb + 16 ti P + c0;
//   sp = (fi & 3) P + fk: the row strip's P fragment, element (16 TR + (fi & 3), p0 + 4 ks + fk) at W + sp + 16 TR P + p0 + 4 ks.
struct RsLane { int fi, fk, pb, cb, sb, sp; };
template <int P>
__device__ __forceinline__ RsLane rs_lane(int lane)
{
    const int l = rs_opaque(lane);
    RsLane L;
    L.fi = l & 15; L.fk = l >> 4;
    L.pb = rs_opaque(L.fi * P + L.fk);
    L.cb = rs_opaque(L.fk * P + L.fi);
    L.sb = rs_opaque((4 * (L.fi >> 2) + L.fk) * P + (L.fi & 3));
    L.sp = rs_opaque((L.fi & 3) * P + L.fk);
    L.fi = rs_opaque(L.fi); L.fk = rs_opaque(L.fk);
    return L;
}

// ---- the pivot table as offsets.  The factoring wave stores pivoff[k] = pivrow[k] P sizeof(cplx), the pivot row's offset in
// bytes, beside pivrow[k] (rs_factor, once per panel), so the Q fragments and the zeroing of the pivot rows address
// rs_at(W, pivoff[p0 + k], col) without a multiply or a shift per entry and body.  poff = pivoff + p0.  The stage schedule
// only: the generic loop and its kernels keep the row table alone.
__device__ __forceinline__ const cplx* rs_at(const cplx* W, int bytes, int elem) { return reinterpret_cast<const cplx*>(reinterpret_cast<const char*>(W) + bytes) + elem; }
__device__ __forceinline__ cplx* rs_at(cplx* W, int bytes, int elem) { return reinterpret_cast<cplx*>(reinterpret_cast<char*>(W) + bytes) + elem; }
// Q fragment of a full panel (FULL) or of the narrow last one (NKS = 1; k >= pw: entry 0 of the panel, the value zeroed)
template <int NKS, bool FULL>
__device__ __forceinline__ void rs_load_qf_off(const cplx* W, const int* poff, int pw, int fk, int col, cplx (&qf)[NKS])
{
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int k = ks * 4 + fk;
        const bool ok = FULL || k < pw;
        const cplx v = *rs_at(W, poff[ok ? k : 0], col);
        qf[ks] = cmake(ok ? v.x : 0.0, ok ? v.y : 0.0);
    }
}
// the two Q fragments of a half tile (columns col and col + second) under a full panel
template <int NKS>
__device__ __forceinline__ void rs_load_qh_off(const cplx* W, const int* poff, int fk, int col, int second, cplx (&qh)[2][NKS])
{
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const cplx* q = rs_at(W, poff[ks * 4 + fk], col);
        qh[0][ks] = q[0]; qh[1][ks] = q[second];
    }
}

// row strip of column tile tj < TR (rs_update_tile's strip form with the tile inside the matrix): rows 16 TR + fk < n are
// stored; RANGE: only the columns [clo, clo + 8) of the tile; MASK: the panel's pivot rows are seeded with 0
template <int P, int NKS, int TR, bool MASK, bool RANGE>
__device__ __forceinline__ void rs_rowstrip_tile(int n, cplx* W, const int* colof, const RsLane& L, int tj, int p0,
                                                 const cplx (&qf)[NKS], int clo)
{
    const int row = TR * 16 + L.fk, col = tj * 16 + L.fi;
    const cplx* prow = W + L.sp + TR * 16 * P + p0;
    cplx* cptr = W + L.cb + TR * 16 * P + tj * 16;
    const int cf = MASK ? colof[row] : -1;
    const cplx cv = *cptr;
    cplx pa[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) pa[ks] = prow[ks * 4];
    const bool keep = !MASK || !(cf >= p0 && cf < p0 + 4 * NKS);
    double ua = keep ? cv.x : 0.0, ub = 0.0, uc = keep ? cv.x + cv.y : 0.0;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
        mfma3s(ua, ub, uc, pa[ks].x, pa[ks].y, pa[ks].x + pa[ks].y, qf[ks].x, qf[ks].y, qf[ks].x + qf[ks].y);
    if (row < n && (!RANGE || (unsigned)(col - clo) < 8u)) *cptr = cmake(ua - ub, uc - ua - ub);
}

// the pivot rows of a full panel in this lane's column
template <int NKS>
__device__ __forceinline__ void rs_zero_pivot_rows_full(cplx* W, const int* poff, int fk, int col)
{
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) *rs_at(W, poff[ks * 4 + fk], col) = cmake(0.0, 0.0);
}
// ... and of the narrow last panel (one k-step, once a sweep).  Its zero is made here: the 16-byte zero of the full panels
// stays in registers across the sweep only as long as every store that uses it sits on the hot path
__device__ __forceinline__ void rs_zero_pivot_rows_narrow(cplx* W, const int* poff, int pw, int fk, int col)
{
    double z = 0.0;
    asm volatile("" : "+v"(z));
    if (fk < pw) *rs_at(W, poff[fk], col) = cmake(z, z);
}

// job kind WHOLE: full column tile tj under a full panel (FULL, NKS = 2) or under the narrow last one (pw <= 4, NKS = 1) --
// rs_update_col's whole-tile form without a test on the stores
template <int P, int TR, int NKS, bool FULL>
__device__ __forceinline__ void rs_job_whole(int n, cplx* W, const int* pivoff, const int* colof, const RsLane& L, int tj, int p0, int pw)
{
    const int col = tj * 16 + L.fi;
    cplx qf[NKS];
    rs_load_qf_off<NKS, FULL>(W, pivoff + p0, pw, L.fk, col, qf);
    if (FULL) rs_zero_pivot_rows_full<NKS>(W, pivoff + p0, L.fk, col);
    else rs_zero_pivot_rows_narrow(W, pivoff + p0, pw, L.fk, col);
    constexpr bool M3 = rs_upd_3m(P);
    double qs[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qs[ks] = qf[ks].x + qf[ks].y;
    cplx* cbase = W + L.cb + tj * 16;
    const cplx* pbase = W + L.pb + p0;
    cplx cv[2][4], pa[2][NKS];
    auto fetch = [&](int ti, int s) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) cv[s][r] = cbase[(ti * 16 + 4 * r) * P];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) pa[s][ks] = pbase[ti * 16 * P + ks * 4];
    };
    fetch(0, 0);
#pragma unroll
    for (int ti = 0; ti < TR; ++ti) {
        const int s = ti & 1;
        if (ti + 1 < TR) fetch(ti + 1, s ^ 1);
        d4 ua, ub = {0, 0, 0, 0}, uc;
#pragma unroll
        for (int r = 0; r < 4; ++r) { ua[r] = cv[s][r].x; uc[r] = M3 ? cv[s][r].x + cv[s][r].y : cv[s][r].y; }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            if (M3) mfma3(ua, ub, uc, pa[s][ks].x, pa[s][ks].y, pa[s][ks].x + pa[s][ks].y, qf[ks].x, qf[ks].y, qs[ks]);
            else zmfma(ua, uc, pa[s][ks], qf[ks]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) cbase[(ti * 16 + 4 * r) * P] = M3 ? cmake(ua[r] - ub[r], uc[r] - ua[r] - ub[r]) : cmake(ua[r], uc[r]);
        __builtin_amdgcn_sched_barrier(0);
    }
    rs_rowstrip_tile<P, NKS, TR, false, false>(n, W, colof, L, tj, p0, qf, 0);
}

// job kind HALF: columns [clo, clo + 8) of full tile tj under a full panel -- rs_update_col's half-tile form
template <int P, int TR>
__device__ __forceinline__ void rs_job_half(int n, cplx* W, const int* pivoff, const int* colof, const RsLane& L, int tj, int clo, int p0)
{
    constexpr int NKS = RS_NB / 4;
    cplx qf[NKS], qh[2][NKS];
    double qs[2][NKS];
    rs_load_qf_off<NKS, true>(W, pivoff + p0, RS_NB, L.fk, tj * 16 + L.fi, qf);   // the row strip's 16-column fragment
    rs_load_qh_off<NKS>(W, pivoff + p0, L.fk, clo + (L.fi & 3), 4, qh);
    if ((unsigned)(tj * 16 + L.fi - clo) < 8u) rs_zero_pivot_rows_full<NKS>(W, pivoff + p0, L.fk, tj * 16 + L.fi);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) { qs[0][ks] = qh[0][ks].x + qh[0][ks].y; qs[1][ks] = qh[1][ks].x + qh[1][ks].y; }
    cplx* cbase = W + L.sb + clo;
    const cplx* pbase = W + L.pb + p0;
    cplx cv[2][2], pa[2][NKS];
    auto fetch = [&](int ti, int s) __attribute__((always_inline)) {
        cv[s][0] = cbase[ti * 16 * P]; cv[s][1] = cbase[ti * 16 * P + 4];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) pa[s][ks] = pbase[ti * 16 * P + ks * 4];
    };
    fetch(0, 0);
#pragma unroll
    for (int ti = 0; ti < TR; ++ti) {
        const int s = ti & 1;
        if (ti + 1 < TR) fetch(ti + 1, s ^ 1);
        rs_half_mma<P, NKS>(cv[s], pa[s], qh, qs);
        cbase[ti * 16 * P] = cv[s][0]; cbase[ti * 16 * P + 4] = cv[s][1];
        __builtin_amdgcn_sched_barrier(0);
    }
    rs_rowstrip_tile<P, NKS, TR, false, true>(n, W, colof, L, tj, p0, qf, clo);
}

// full row tile ti < TR of the column strip (rs_update_tile's strip form with the rows inside the matrix and nothing masked):
// columns 16 TR + (fi & 3) < n are stored
template <int P, int NKS, int TR>
__device__ __forceinline__ void rs_colstrip_tile(int n, cplx* W, const RsLane& L, int ti, int p0, const cplx (&qf)[NKS])
{
    cplx* cptr = W + L.sb + ti * 16 * P + TR * 16;
    const cplx* prow = W + L.pb + ti * 16 * P + p0;
    const cplx cv = *cptr;
    cplx pa[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) pa[ks] = prow[ks * 4];
    double ua = cv.x, ub = 0.0, uc = cv.x + cv.y;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
        mfma3s(ua, ub, uc, pa[ks].x, pa[ks].y, pa[ks].x + pa[ks].y, qf[ks].x, qf[ks].y, qf[ks].x + qf[ks].y);
    if (TR * 16 + (L.fi & 3) < n) *cptr = cmake(ua - ub, uc - ua - ub);
}

// job kind STRIP: the column strip (tile TR) under a full panel, every row tile on the 4x4x4 instruction
template <int T16, int P, int TR>
__device__ __forceinline__ void rs_job_strip(int n, cplx* W, const int* pivoff, const int* colof, const RsLane& L, int p0)
{
    constexpr int NKS = RS_NB / 4;
    const int col = TR * 16 + (L.fi & 3);
    cplx qf[NKS];
    rs_load_qf_off<NKS, true>(W, pivoff + p0, RS_NB, L.fk, col, qf);
    if (col < n) rs_zero_pivot_rows_full<NKS>(W, pivoff + p0, L.fk, col);
#pragma unroll
    for (int ti = 0; ti < TR; ++ti) {
        rs_colstrip_tile<P, NKS, TR>(n, W, L, ti, p0, qf);
        __builtin_amdgcn_sched_barrier(0);
    }
    // the corner block, once a job, in the generic form: its own index arithmetic behind rs_opaque stays inside it and is not
    // carried through the stages
    rs_update_tile<P, NKS, TR, false>(n, W, colof, TR, TR, p0, RS_NB, rs_opaque(L.fi), rs_opaque(L.fk), qf, TR * 16, TR * 16 + 16);
    __builtin_amdgcn_sched_barrier(0);
}

// the look-ahead on full row tile ti under a full panel: columns [c0, c0 + 8) inside the matrix, the panel's pivot rows seeded
// with 0 -- rs_update_half<P, NKS, true, true> on the lane bases
template <int P, int NKS>
__device__ __forceinline__ void rs_lookahead_half(cplx* W, const int* colof, const RsLane& L, int ti, int p0,
                                                  const cplx (&qh)[2][NKS], int c0)
{
    cplx* cptr = W + L.sb + ti * 16 * P + c0;
    const cplx* pbase = W + L.pb + ti * 16 * P + p0;
    const int cf = colof[ti * 16 + 4 * (L.fi >> 2) + L.fk];
    cplx cv[2] = {cptr[0], cptr[4]}, pa[NKS];
    double qs[2][NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) { pa[ks] = pbase[ks * 4]; qs[0][ks] = qh[0][ks].x + qh[0][ks].y; qs[1][ks] = qh[1][ks].x + qh[1][ks].y; }
    if (cf >= p0 && cf < p0 + 4 * NKS) { cv[0] = cmake(0.0, 0.0); cv[1] = cmake(0.0, 0.0); }   // a pivot row of the panel (both values: one row)
    rs_half_mma<P, NKS>(cv, pa, qh, qs);
    cptr[0] = cv[0]; cptr[4] = cv[1];
}

// rs_inverse for a remainder-strip class with the roles by SIMD (wave = role; role 3 factors every panel).  pivoff: a second
// table of 64 entries beside pivrow, the pivot rows as byte offsets (rs_at); written and read here alone
template <int T16, int P, int TR>
__device__ __forceinline__ void rs_inverse_sched(int n, cplx* W, int* pivrow, int* pivoff, int* colof, cplx* rowline, int tid, int wave,
                                                 unsigned long long* st = nullptr)
{
    static_assert(TR == T16 - 1 && rs_sched_fits(TR), "a remainder-strip class");
    constexpr int NKS = RS_NB / 4;
    const int lane = tid & 63;
    int sti = 0;
    auto stamp = [&]() __attribute__((always_inline)) { if (st && tid == 0) st[sti] = __builtin_amdgcn_s_memrealtime(); ++sti; };
    // this role's jobs of the full stages (roles 0 .. 2; role 3 factors)
    wave = __builtin_amdgcn_readfirstlane(wave);                // (the same in every lane: the table stays in scalar registers)
    unsigned long long avail = rs_rows_mask(n);                 // the rows still to become pivots, carried through the panels (rs_factor)
    const unsigned long long jobs = wave == 0 ? rs_sched_word(TR, 0) : wave == 1 ? rs_sched_word(TR, 1) : wave == 2 ? rs_sched_word(TR, 2) : 0ull;
    const RsLane L = rs_lane<P>(lane);                          // the lane bases of every update body of this inverse
#pragma unroll 1
    for (int sgi = -1; sgi < 2 * TR; ++sgi) {
        // stage sgi: the full panel [p0, p0 + 8) is applied, panel [n0, n0 + 8) -- the narrow last one after stage 2 TR - 1 -- factored
        const int p0 = sgi * RS_NB, n0 = p0 + RS_NB;
        const bool full_next = sgi + 1 < 2 * TR;
        if (sgi >= 0) {
            // look-ahead: the next panel's columns, one row tile per wave.  A full next panel is half of a full tile (two column
            // strips per row tile, the row strip in its own form), the last one the column strip
            const int tl = n0 >> 4;
            // The Q fragments are loaded in ONE straight line whatever the role -- the half tiles' two strips at columns
            // n0 + (fi & 3) and + 4, the row strip's 16 columns 16 tl + fi, the column strip's 16 TR + (fi & 3) -- with the role
            // in a scalar column base, a scalar lane mask and a scalar distance of the second fragment (0 where there is none:
            // two loads of elements the first two read).  Loaded in a branch per role, the fragments met behind the barrier
            // in sixteen register moves per stage and wave, the factoring wave's included.
            cplx qh[2][NKS];
            cplx (&qf)[NKS] = qh[0];                            // (the roles with one fragment)
            const bool halves = full_next && wave < TR;
            const int qcol = (full_next ? (halves ? n0 : tl * 16) : TR * 16) + (L.fi & (full_next && !halves ? 15 : 3));
            rs_load_qh_off<NKS>(W, pivoff + p0, L.fk, qcol, halves ? 4 : 0, qh);
            __syncthreads();
            if (full_next) {
                if (wave < TR) rs_lookahead_half<P, NKS>(W, colof, L, wave, p0, qh, n0);
                else if (wave == TR) rs_rowstrip_tile<P, NKS, TR, true, true>(n, W, colof, L, tl, p0, qf, n0);
            } else if (wave < T16) rs_update_tile<P, NKS, TR, true>(n, W, colof, wave, TR, p0, RS_NB, rs_opaque(L.fi), rs_opaque(L.fk), qf, n0, n0 + RS_NB);   // (once a sweep: generic form)
            __syncthreads();
            // the other columns: this role's jobs of the stage
            unsigned c = (unsigned)(jobs >> (RS_STAGE_BITS * sgi)) & ((1u << RS_STAGE_BITS) - 1u);
#pragma unroll 1
            while (c) {
                const unsigned kind = c & 3u;
                const int tj = (int)(c >> 2) & 3;
                if (kind == RS_JOB_WHOLE) rs_job_whole<P, TR, NKS, true>(n, W, pivoff, colof, L, tj, p0, RS_NB);
                else if (kind == RS_JOB_HALF) rs_job_half<P, TR>(n, W, pivoff, colof, L, tj, tj * 16 + (int)((c >> 4) & 1u) * 8, p0);
                else rs_job_strip<T16, P, TR>(n, W, pivoff, colof, L, p0);
                c >>= RS_JOB_BITS;
            }
        }
        if (wave == RS_WAVES - 1) {
            if (st && lane == 0) st[16 + 2 * (sgi + 1)] = __builtin_amdgcn_s_memrealtime();
            __builtin_amdgcn_s_setprio(3);                      // (see rs_inverse)
            // the narrow last panel in a 4-column instantiation with the arithmetic pinned: bit for bit the generic loop
            if (!full_next) rs_factor<P, 16 * T16, 4, true>(n, W, pivrow, colof, rowline, n0, n - n0, lane, avail, false, nullptr, pivoff);
            else rs_factor<P, 16 * T16>(n, W, pivrow, colof, rowline, n0, RS_NB, lane, avail, false, (st && sgi + 1 == 1) ? st + 40 : nullptr, pivoff);
            __builtin_amdgcn_s_setprio(0);
            if (st && lane == 0) st[17 + 2 * (sgi + 1)] = __builtin_amdgcn_s_memrealtime();
        }
        stamp();
        __syncthreads();
    }
    // the last stage: the narrow panel [16 TR, n) (one k-step, guarded code) on the full tiles, tile tj by role tj
    if (wave < TR) rs_job_whole<P, TR, 1, false>(n, W, pivoff, colof, L, wave, TR * 16, n - TR * 16);
    stamp();
    __syncthreads();
}

}  // namespace
