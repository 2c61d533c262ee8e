// 1-D chain contact self-energy ("decimation") for n_c <= 64, register-stationary version.
// gauNEGF/surfG1D.py:223-295 (g), :344-373 (sigma).  gfx950.
//
// A JOB is one fixed point (energy, contact); a workgroup (256 threads, 4 waves) runs one job at a time, SEVERAL
// workgroups per CU.  The fixed point is a chain of up to 2000 dependent sweeps, each a chain of 50 dependent pivot
// steps, so one workgroup can never fill a CU: the kernel is built to be small enough that three (n_c <= 57) or two
// workgroups share a CU and cover each other's latency chains.  That means ONE n x n work matrix in LDS per workgroup
// (40.8 KB at n_c = 50) and <= 168 VGPRs:
//   * B = (E + i eta) Sb - b is not stored per workgroup at all: wave w needs only row tile w of B, as
//     the A operand of T = B g (wave w owns row tile w of T) and, conjugated, as the B operand of
//     M = A - T B^H (wave w owns column tile w of M); it streams those 16 x n elements from the lead
//     matrices Sb, b (shared by all workgroups of the contact, L2-resident) a k-step ahead -- from copies of
//     them that are zero-padded to 64 x 64 at pitch 64 (ChainRsArgs::pad): a lane's element of k-step ks is an
//     immediate offset from one lane base, rows and columns >= n read zeros, nothing is clamped or selected.
//     The A of M = A - T B^H is read from the padded alpha, Salpha the same way, a row tile's loads as one batch.
//   * the iterate g is kept twice: in the work matrix at the start of a sweep (B operand of T = B g;
//     overwritten by T, then M) and as the "old" g of the mixing step, which each lane writes and
//     reads back for its own elements only (chain_mix_map.h: 10 slots per lane at n_c = 50): in a second LDS
//     matrix when two workgroups share the CU; when three do, the first slots in the unused rows of the work
//     matrix and the rest in a lane-private global scratch record (L2-resident).
//   * the in-place Gauss-Jordan inverse of M works on panels of 8 columns (RS_NB).  The wave on SIMD 0 -- the
//     CHAIN wave (rs_wave_role: the roles follow the SIMD a wave runs on, because an FP64 matrix instruction holds
//     its SIMD's vector issue) -- factors every panel: lane = row, DPP arg-max on the high word of |re| + |im|, the
//     pivot row through a 128-byte LDS line, no workgroup barrier inside.  The other three waves apply the previous
//     panel to the column tiles they OWN (the owner reads the pivot rows it needs, the Q fragment of its tile, into
//     registers before it writes: no snapshot buffer); all four bring the next panel's columns up to date first
//     (look-ahead).  Products and updates are three real matrix instructions per complex tile and k-step (3M).
//   * launches with more jobs than resident slots run them ROUND ROBIN through a device-side queue (ChainRsArgs,
//     rs_rr_pop / rs_rr_push): a persistent workgroup per slot, quanta of 100 sweeps, the iterate of a job that is
//     set aside waits in the job's output block.
// Per sweep
//     T     = B g ;  M = A - T B^H          2 complex GEMMs on the FP64 matrix cores
//     g_new = inv(M)                         blocked Gauss-Jordan, partial pivoting (izamax rule)
//     diff  = max |g_new - g| / max(|g_new|, 1e-12) ;  g = r g_new + (1-r) g
// Rows are never swapped: g_new[i][j] = W[pivrow[i]][colof[j]] is resolved when g_new is read.
// The stopping rule only needs "diff > conv" / "diff <= conv"; both are evaluated on the squares
// (|d|^2 > conv^2 max(|g_new|^2, 1e-24)), which is the same predicate without sqrt and divide.
//
// Every job stops on ITS OWN convergence (the reference's vmap runs all energies until the
// slowest lane converges; results are identical because a converged lane is frozen there).
#include "negf_common.h"
#include "chain_mix_map.h"          // the lane map of the mixing step
#include "chain_rs_inverse.h"       // the small inverse (rs_factor ... rs_inverse) and the 3M helpers, shared with k_chain1d_rd.hip
#include <algorithm>
#include <type_traits>

namespace {

struct ChainRsArgs {
    // concatenated per contact.  The kernel reads alpha, Salpha (the start matrix A) and streams everything else from `pad`;
    // the other four keep the layout of the kernel arguments: without them the compiler loads the arguments in other
    // groups and every instantiation gains 10 - 40 reloads of spilled scalars (LAB_NOTES.md, "retired variants")
    const cplx *alpha, *Salpha, *beta, *Sbeta, *tau, *Stau;
    const cplx* pad;                 // the six lead matrices, zero-padded: [matrix][contact][CHAIN_PAD][CHAIN_PAD] (SigmaProvider::d_lead_pad)
    const int* nc;
    const int* blk_off;
    int n_contacts, blk_stride;
    double eta, conv, relFactor;
    int max_iter, force_iters;
    cplx* gold;                      // [workgroups][KS][256] lane-private copies of the iterate (GOLD_GLOBAL kernels)
    int gold_lds_off;                // the first slots of a lane's copy live in LDS at this element offset
    const int* order;                // launch slot -> job (energy * n_contacts + contact), longest jobs first; or null
    // surface Green's function cache (negf_set_chain_cache): gc_mode 1 = this launch is a miss, every job stores its
    // final iterate g into gcache [energy][blk_stride] (the layout of blk); 2 = a hit, every job loads g from there and
    // only runs Sigma = t g t^H -- the same instructions on the same operands as the last pass of a miss
    cplx* gcache;
    int gc_mode;
    unsigned long long* stamps;      // diagnostic (RS_STAMPS build + NEGF_CHAIN_STAMPS): wall-clock stamps of workgroup (0,0), 10th sweep
    int stamp_sweep;                 // diagnostic: the sweep of job 0 whose phases are stamped (NEGF_CHAIN_STAMP_SWEEP, default 10)
    int simd_roles;                  // 1: wave roles follow the SIMD a wave runs on (see rs_wave_role), 0: the wave number
    // round-robin execution (rr_quantum > 0): the launch is one PERSISTENT workgroup per resident slot; the jobs wait
    // in a FIFO queue (entries 0 .. rr_jobs-1: the launch order, then rr_ring), a workgroup runs a job for rr_quantum
    // sweeps and -- if other jobs are waiting -- leaves the iterate in the job's (still unused) output block, puts the
    // job at the back of the queue and takes the one at the front.  Jobs of unknown length then finish in order of
    // their length and the chip stays full until fewer jobs than slots are left, whatever the launch order was.
    int rr_quantum;
    struct RsQueue* rr_q;            // (in device memory: its fields are only needed when a job starts or is set aside)
};
struct RsQueue {
    unsigned head, tail;             // next entry to pop / to push
    unsigned jobs, cap;              // jobs of the launch (entries 0 .. jobs-1 of the queue), entries of the ring
    unsigned long long ring[];       // (sweep count << 32) | job; ~0 = not written yet
};

// front of the job queue (lane 0 of a workgroup): (count << 32) | job, or -1 when the queue is empty.  An empty queue
// stays empty: a job is only ever pushed by a workgroup that saw other jobs waiting, so a workgroup that finds it
// empty is done (every job is then held by a running workgroup, which finishes it itself).
__device__ __forceinline__ long long rs_rr_pop(RsQueue* q, const int* order)
{
    const unsigned jobs = q->jobs;
    for (;;) {
        const unsigned h = __hip_atomic_load(&q->head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned t = __hip_atomic_load(&q->tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (h >= t) return -1;
        unsigned expect = h;
        if (!__hip_atomic_compare_exchange_strong(&q->head, &expect, h + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            continue;
        if (h < jobs) return order ? order[h] : (int)h;
        // (the pusher reserved this entry before writing it: it is a running workgroup between two instructions)
        unsigned long long v;
        do { v = __hip_atomic_load(&q->ring[h - jobs], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT); } while (v == ~0ull);
        return (long long)v;
    }
}
// are other jobs waiting (and is there room to queue this one)?
__device__ __forceinline__ bool rs_rr_waiting(RsQueue* q)
{
    const unsigned h = __hip_atomic_load(&q->head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned t = __hip_atomic_load(&q->tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return h < t && t - q->jobs + 1024u < q->cap;
}
__device__ __forceinline__ void rs_rr_push(RsQueue* q, int job, int count)
{
    const unsigned t = __hip_atomic_fetch_add(&q->tail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&q->ring[t - q->jobs], ((unsigned long long)(unsigned)count << 32) | (unsigned)job,
                       __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void rs_rr_init_kernel(RsQueue* q, unsigned cap, unsigned jobs)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) q->ring[i] = ~0ull;
    if (i == 0) { q->head = 0u; q->tail = jobs; q->jobs = jobs; q->cap = cap; }
}

// P: compile-time pitch of the work matrix (odd, >= n): every tile / k-step offset is an immediate of the
// DS instruction, a lane needs ONE address register per operand stream.  The matrix has 16*T16 rows
// of which rows >= n (and the columns >= n of a row) stay zero: operands of the padded tiles are read
// without clamps or selects and are finite.
// RR: the round-robin instantiation (a persistent workgroup that takes its jobs from the queue: every launch with more jobs
// than resident slots); the plain one -- a launch whose jobs all fit the resident slots -- carries none of the job loop (its
// per-job values are loop invariants again: equal jobs, four rounds of 768, 61.9 against 62.6 us per sweep and slot).
// a value / pointer that is the same in every lane, kept in scalar registers
__device__ __forceinline__ double rs_uniform(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// Global accesses at  scalar base + compile-time byte offset + one 32-bit lane offset:  the base is the same in every
// lane and is kept a scalar pair of its own (rs_scalar_base: opaque, so that nothing is re-associated into 64-bit vector
// arithmetic or hoisted out of the sweep), the lane offset is one register for all accesses of a phase.
typedef double rs_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned long long rs_scalar_base(const void* p)
{
    unsigned long long b = reinterpret_cast<unsigned long long>(p);
    asm volatile("" : "+s"(b));
    return b;
}
// (a base advanced by a constant is made opaque again: two scalar instructions where it is used, not a pair of scalar
//  registers per access kept alive across the sweep)
__device__ __forceinline__ unsigned long long rs_scalar_advance(unsigned long long b, long long bytes)
{
    b += (unsigned long long)bytes;
    asm volatile("" : "+s"(b));
    return b;
}
__device__ __forceinline__ cplx rs_gload(unsigned long long base, unsigned const_bytes, unsigned lane_bytes)
{
    const __attribute__((address_space(1))) char* p = reinterpret_cast<const __attribute__((address_space(1))) char*>(base) + const_bytes;
    const rs_d2 v = *reinterpret_cast<const __attribute__((address_space(1))) rs_d2*>(p + lane_bytes);
    return cmake(v.x, v.y);
}
__device__ __forceinline__ void rs_gstore(unsigned long long base, unsigned const_bytes, unsigned lane_bytes, cplx v)
{
    __attribute__((address_space(1))) char* p = reinterpret_cast<__attribute__((address_space(1))) char*>(base) + const_bytes;
    rs_d2 w; w.x = v.x; w.y = v.y;
    *reinterpret_cast<__attribute__((address_space(1))) rs_d2*>(p + lane_bytes) = w;
}

// SCHED: the inverse of a remainder-strip class follows the compile-time stage schedule (rs_inverse_sched) --
// chain1d_rs_kernel; without it the generic loop -- chain1d_rs_wn_kernel, the launches with the roles by wave number.  Two
// kernels, not one with both loops: the second copy of the inverse is 14 KB of code that a launch never runs.
template <int P, int OCC, bool GOLD_GLOBAL, bool RR, bool SCHED>
__device__ __forceinline__ void chain1d_rs_body(
    const ChainRsArgs& a, const cplx* __restrict__ E, cplx* __restrict__ blk, int* __restrict__ iters,
    int* __restrict__ converged)
{
    constexpr int T16 = (P - 1 + 15) / 16;              // 16-row tiles per dimension
    constexpr int KS = (P + 3) / 4 < 4 * T16 ? (P + 3) / 4 : 4 * T16;   // k-steps of a full-width product (n <= P)
    constexpr int WELEMS = 16 * T16 * P + 16;           // 16*T16 rows and a few elements of slack behind the last one
    constexpr int TR = T16 - 1;                         // the last tile
    constexpr bool REM = T16 >= 2 && P - 16 * TR <= 4;   // ... holds <= 4 rows / columns: strips
    constexpr int FT = REM ? TR : T16;                  // full 16 x 16 tiles per dimension
    constexpr bool M3G = T16 >= 3;                      // products in 3M form (mfma3): the 168-VGPR kernels (the updates: rs_upd_3m)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ int flags[2 * RS_WAVES];                 // per wave: any(diff > conv), all(diff <= conv)
    __shared__ int pivrow[64], colof[64];
    // the stage schedule's second pivot table, the pivot rows as byte offsets (rs_inverse_sched): 256 bytes more in classes 35 and 51 alone, whose
    // work matrix leaves them room at three workgroups per CU (class 51: 52 480 + 936 of the 53 760 bytes of 42 granules)
    constexpr bool SCHED_TABLES = SCHED && REM && rs_stage_sched(REM ? TR : -1);
    __shared__ int pivoff[SCHED_TABLES ? 64 : 1];
    __shared__ cplx rowline[RS_NB];                    // pivot row of the column step being factored

    // job of this launch slot: in launch order, or -- when the provider has seen this grid before -- in
    // the order of decreasing sweep counts of the previous evaluation (the jobs differ by up to 20x in
    // length; started longest first, the last workgroups of the grid do not leave the chip idle).
    // Round robin (a.rr_quantum > 0): the slot is a persistent workgroup and takes its jobs from the queue.
    const int slot = blockIdx.y * gridDim.x + blockIdx.x;
    __shared__ long long rr_msg;
    cplx* Ws = reinterpret_cast<cplx*>(smem_raw);       // [16*T16][P] (+ slack): g (start of a sweep), T, M, the reduced M
    const int tid = threadIdx.x, lane = tid & 63;
    // ---- wave roles.  A v_mfma_f64_16x16x4 holds its SIMD's vector issue for ~45 of its 64 cycles whatever the
    // priorities (scripts/probe/fp64_coexec_probe.hip: beside a wave that streams them, another wave's v_fma_f64 take
    // 22 cycles instead of 5.6 and an LDS round trip 230 instead of 105), so the wave that factors the panels -- a
    // chain of dependent vector and LDS instructions, the workgroup's critical path -- must not share its SIMD with
    // waves that stream matrix instructions.  The four waves of a workgroup always land on four different SIMDs
    // (scripts/probe/wave_placement_probe.hip), so the roles follow the SIMD: the wave on SIMD 0 is the CHAIN wave
    // (role 3: factors every panel; its share of the products and updates is the last tile, for n_c = 50 the
    // 2-row / 2-column remainder strip), the waves on SIMDs 1-3 are the MATRIX waves (roles 0-2).  With several
    // workgroups per CU all chain waves then sit on SIMD 0 and all matrix-instruction streams on SIMDs 1-3.
    // Only speed depends on the placement: were two waves ever to report the same SIMD, the roles fall back to
    // the wave numbers.
    int wave = tid >> 6;
    bool chain_roles = false;
    if (a.simd_roles) {
        unsigned hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        const int simd = (hwid >> 4) & 3;
        if (lane == 0) flags[wave] = simd;
        __syncthreads();
        const int seen = (1 << flags[0]) | (1 << flags[1]) | (1 << flags[2]) | (1 << flags[3]);
        chain_roles = __builtin_amdgcn_readfirstlane(seen) == 15;
        if (chain_roles) wave = simd == 0 ? RS_WAVES - 1 : simd - 1;
        wave = __builtin_amdgcn_readfirstlane(wave);
        __syncthreads();
    }
    // ---- the job: set by next_job() below -- once, or (round robin) whenever this workgroup takes another one
    int job = 0, count = 0, c = 0, b = 0, n = 1, off = 0, ksteps = 1;
    bool resume = false;                                // a job that was set aside after `count` sweeps: its iterate waits in blk
    // ---- the old iterate of the mixing step lives on the dense lane map of chain_mix_map.h (gather_mix below).  Its LDS part
    // sits at element a.gold_lds_off of the dynamic LDS -- behind the work matrix when two workgroups share the CU; when three
    // do, in the rows n_max+2 .. 16*T16-1 of the work matrix itself, which only feed discarded output rows of the padded tiles
    // and may hold any finite values -- and the rest in global scratch a.gold [slot][thread] (coalesced); with the LDS part
    // taken off, the scratch of the workgroups of an XCD fits its 4 MB L2 and is rewritten there sweep after sweep.
    const cplx *alpha = a.alpha, *Salpha = a.Salpha;    // (at pitch n: the start matrix A)
    // the padded lead matrices: matrix k (0 alpha, 1 Salpha, 2 beta, 3 Sbeta, 4 tau, 5 Stau) of the job's contact, padded.  One base and
    // one stride stay live across the sweep, not six pointers
    const cplx* pad_c = a.pad; unsigned pad_ps = 0;
    RsMixMap mm = rs_mix_map(1);                        // the job's lane map of the mixing step: scalars
    bool final_pass = false;                            // the pass that runs Sigma = t g t^H through the two products
    auto lead_p = [&](int k) __attribute__((always_inline)) { return pad_c + (size_t)k * pad_ps; };
    cplx e = cmake(0.0, 0.0), z = e;
    const double conv2 = a.conv * a.conv, rf = a.relFactor, rf1 = 1.0 - a.relFactor;
    auto sel = [](bool ok, cplx v) { return cmake(ok ? v.x : 0.0, ok ? v.y : 0.0); };
    // A = (E + i eta) Sa - a at (i, j); global loads at clamped (always valid) indices
    auto Aat = [&](int i, int j) {
        const int o = min(i, n - 1) * n + min(j, n - 1);
        return csub(cmul(z, Salpha[o]), alpha[o]);
    };

    // ---- the stationary operand of the two products: row tile `wave` of  zz * Smat - mat  in the MFMA
    // A-operand layout, element (wave*16 + fi, ks*4 + fk).  It is NOT kept in registers across the sweep
    // (52-64 VGPRs that the three-workgroups-per-CU budget does not have): each product streams it from the
    // lead matrices, which every workgroup of the contact shares (L2 / L1 resident), PF k-steps ahead.
    // Rows >= n give garbage in output rows / columns >= n only (never stored); k >= n is zeroed.
    // In the padded lead matrices a lane's element of k-step ks sits ks * 64 bytes behind its first one -- an immediate
    // offset, no clamp; rows and k >= n read zeros, and z * 0 - 0 is a zero of either sign, which multiplies finite
    // values and is added to an accumulator that starts at +0: no stored value depends on the sign.
    constexpr int PF = 1;                           // k-steps the streamed operand is requested ahead: two named buffers
    cplx opz = z;                                   // z of the sweeps, E (no eta) of the final pass
    struct Stream { cplx s[2], m[2]; };
    auto stream_row = [&](const cplx* op, int irow, int fk) __attribute__((always_inline)) {
        return op + (unsigned)(irow * CHAIN_PAD + fk);
    };
    auto stream_fetch = [&](Stream& q, const cplx* sS, const cplx* sM, int ks) __attribute__((always_inline)) {
        q.s[ks & 1] = sS[ks * 4]; q.m[ks & 1] = sM[ks * 4];
    };
    auto stream_elem = [&](const Stream& q, int ks) __attribute__((always_inline)) {
        return csub(cmul(opz, q.s[ks & 1]), q.m[ks & 1]);
    };
    // k-steps of this job's products: in a remainder-strip class every contact reaches into the strip (the launcher's
    // class rule), n > 16 TR, so all KS k-steps run and the loops below carry no branch
    const auto ksteps_of = [&]() __attribute__((always_inline)) { return REM ? KS : ksteps; };

    // wave w: acc[tj] = sum_k Op[w*16 + fi][k] * Ws[k][tj*16 + fi]  (row tile w of  Op Ws).  The padding of
    // Ws is zero / finite, output columns >= n are never stored.
    auto gemm_rowtile = [&](d4 (&accr)[T16], d4 (&acci)[T16], d4 (&accc)[T16]) __attribute__((always_inline)) {
        const int fi = rs_opaque(lane & 15), fk = rs_opaque(lane >> 4);
        const bool strip_wave = REM && wave == TR;      // this wave's row tile is the row strip
        const cplx* bb = Ws + fk * P + fi;
        const cplx* bb4 = Ws + fk * P + (fi & 3);       // column-strip B operand: column TR*16 + (l&3) in every block
        const int irow = strip_wave ? TR * 16 + (fi & 3) : wave * 16 + fi;
        const cplx* sS = stream_row(lead_p(final_pass ? 5 : 3), irow, fk);
        const cplx* sM = stream_row(lead_p(final_pass ? 4 : 2), irow, fk);
        const int ksteps = ksteps_of();
        Stream q;
#pragma unroll
        for (int ks = 0; ks < PF; ++ks) stream_fetch(q, sS, sM, ks);
#pragma unroll
        for (int tj = 0; tj < T16; ++tj) { accr[tj] = (d4){0, 0, 0, 0}; acci[tj] = (d4){0, 0, 0, 0}; accc[tj] = (d4){0, 0, 0, 0}; }
        // the LDS operands (B fragments of the work matrix) of k-step ks+1 are requested in front of the matrix
        // instructions of k-step ks: an LDS round trip is ~300 cycles on a CU whose LDS three workgroups share
        cplx qbuf[2][T16];
        auto load_qb = [&](int ks, cplx (&qb)[T16]) __attribute__((always_inline)) {
#pragma unroll
            for (int tj = 0; tj < FT; ++tj) qb[tj] = bb[ks * 4 * P + tj * 16];
            if (REM) qb[TR] = strip_wave ? bb[ks * 4 * P + TR * 16] : bb4[ks * 4 * P + TR * 16];
        };
        load_qb(0, qbuf[0]);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks < ksteps) {
                const cplx pa = stream_elem(q, ks);
                const double ps = pa.x + pa.y;
                if (ks + PF < KS) stream_fetch(q, sS, sM, ks + PF);
                cplx (&qb)[T16] = qbuf[ks & 1];
                if (ks + 1 < KS && ks + 1 < ksteps) load_qb(ks + 1, qbuf[(ks + 1) & 1]);
                if (strip_wave) {
#pragma unroll
                    for (int tj = 0; tj < T16; ++tj) { if (M3G) RS_M3S(accr[tj], acci[tj], accc[tj], pa.x, pa.y, ps, qb[tj].x, qb[tj].y, qb[tj].x + qb[tj].y); else RS_ZMFMA4(accr[tj], acci[tj], pa, qb[tj]); }
                } else {
#pragma unroll
                    for (int tj = 0; tj < FT; ++tj) { if (M3G) mfma3(accr[tj], acci[tj], accc[tj], pa.x, pa.y, ps, qb[tj].x, qb[tj].y, qb[tj].x + qb[tj].y); else zmfma(accr[tj], acci[tj], pa, qb[tj]); }
                    if (REM) { if (M3G) RS_M3S(accr[TR], acci[TR], accc[TR], pa.x, pa.y, ps, qb[TR].x, qb[TR].y, qb[TR].x + qb[TR].y); else RS_ZMFMA4(accr[TR], acci[TR], pa, qb[TR]); }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // wave w: acc[ti] = sum_k Ws[ti*16 + fi][k] * conj(Op[w*16 + fi][k])  (column tile w of  Ws Op^H)
    auto gemm_coltile = [&](d4 (&accr)[T16], d4 (&acci)[T16], d4 (&accc)[T16]) __attribute__((always_inline)) {
        const int fi = rs_opaque(lane & 15), fk = rs_opaque(lane >> 4);
        const bool strip_wave = REM && wave == TR;      // this wave's column tile is the column strip
        const cplx* ab = Ws + fi * P + fk;
        const cplx* ab4 = Ws + (fi & 3) * P + fk;       // row-strip A operand: row TR*16 + (l&3) in every block
        const int irow = strip_wave ? TR * 16 + (fi & 3) : wave * 16 + fi;
        const cplx* sS = stream_row(lead_p(final_pass ? 5 : 3), irow, fk);
        const cplx* sM = stream_row(lead_p(final_pass ? 4 : 2), irow, fk);
        const int ksteps = ksteps_of();
        Stream q;
#pragma unroll
        for (int ks = 0; ks < PF; ++ks) stream_fetch(q, sS, sM, ks);
#pragma unroll
        for (int ti = 0; ti < T16; ++ti) { accr[ti] = (d4){0, 0, 0, 0}; acci[ti] = (d4){0, 0, 0, 0}; accc[ti] = (d4){0, 0, 0, 0}; }
        cplx pbuf[2][T16];                               // A fragments of the work matrix, double buffered (see gemm_rowtile)
        auto load_pa = [&](int ks, cplx (&pa)[T16]) __attribute__((always_inline)) {
#pragma unroll
            for (int ti = 0; ti < FT; ++ti) pa[ti] = ab[ti * 16 * P + ks * 4];
            if (REM) pa[TR] = ab4[TR * 16 * P + ks * 4];
        };
        load_pa(0, pbuf[0]);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks < ksteps) {
                const cplx br = stream_elem(q, ks);
                const double bd = br.x - br.y;
                if (ks + PF < KS) stream_fetch(q, sS, sM, ks + PF);
                cplx (&pa)[T16] = pbuf[ks & 1];
                if (ks + 1 < KS && ks + 1 < ksteps) load_pa(ks + 1, pbuf[(ks + 1) & 1]);
                // pa * conj(b)
                if (strip_wave) {
#pragma unroll
                    for (int ti = 0; ti < T16; ++ti) { if (M3G) RS_M3S(accr[ti], acci[ti], accc[ti], pa[ti].x, pa[ti].y, pa[ti].x + pa[ti].y, br.x, br.y, bd); else RS_ZMFMA4C(accr[ti], acci[ti], pa[ti], br); }
                } else {
#pragma unroll
                    for (int ti = 0; ti < FT; ++ti) {
                        if (M3G) mfma3(accr[ti], acci[ti], accc[ti], pa[ti].x, pa[ti].y, pa[ti].x + pa[ti].y, br.x, br.y, bd);
                        else {
                            accr[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[ti].x, br.x, accr[ti], 0, 0, 0);
                            accr[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[ti].y, br.y, accr[ti], 0, 0, 0);
                            acci[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[ti].y, br.x, acci[ti], 0, 0, 0);
                            acci[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[ti].x, br.y, acci[ti], 0, 0, 0);
                        }
                    }
                    if (REM) { if (M3G) RS_M3S(accr[TR], acci[TR], accc[TR], pa[TR].x, pa[TR].y, pa[TR].x + pa[TR].y, br.x, br.y, bd); else RS_ZMFMA4C(accr[TR], acci[TR], pa[TR], br); }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // Where a lane's accumulator values of tile (ti, tj) live: FULL and ROW-STRIP tiles use the 16 x 16 C layout
    // (rows ti*16 + fk + 4r, column tj*16 + fi; a row strip only fills r = 0), a COLUMN-STRIP tile (tj == TR of a
    // full row tile) holds one value per lane at (ti*16 + 4 (fi>>2) + fk, TR*16 + (fi&3)).
    // f(r, i, j, re, im) is called for every element this lane holds (r: its component, a compile-time number).
    auto for_tile = [&](int ti, int tj, const d4& va, const d4& vb, const d4& vc, bool cj, int fi, int fk, auto f) __attribute__((always_inline)) {
        d4 vr, vi;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            vr[r] = !M3G ? va[r] : cj ? va[r] + vb[r] : va[r] - vb[r];
            vi[r] = !M3G ? vb[r] : cj ? vc[r] - va[r] + vb[r] : vc[r] - va[r] - vb[r];
        }
        if (REM && tj == TR && ti != TR) {
            f(0, ti * 16 + 4 * (fi >> 2) + fk, TR * 16 + (fi & 3), vr[0], vi[0]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (!(REM && ti == TR) || r == 0) f(r, ti * 16 + fk + 4 * r, tj * 16 + fi, vr[r], vi[r]);
        }
    };
    // store row tile `wave` held as accumulators (C layout: rows fk + 4r, column fi of tile tj)
    auto store_rowtile = [&](const d4 (&accr)[T16], const d4 (&acci)[T16], const d4 (&accc)[T16]) __attribute__((always_inline)) {
        const int fi = rs_opaque(lane & 15), fk = rs_opaque(lane >> 4);
        // a full tile of a remainder-strip class lies inside every contact of the launch (the launcher's class rule, as
        // rs_update_col assumes): stored without the test
        const bool inside = REM && wave < TR;
#pragma unroll
        for (int tj = 0; tj < T16; ++tj) {
            if (inside && tj < TR)
                for_tile(wave, tj, accr[tj], acci[tj], accc[tj], false, fi, fk,
                         [&](int r, int i, int j, double re, double im) { Ws[i * P + j] = cmake(re, im); });
            else
                for_tile(wave, tj, accr[tj], acci[tj], accc[tj], false, fi, fk,
                         [&](int r, int i, int j, double re, double im) { if (i < n && j < n) Ws[i * P + j] = cmake(re, im); });
        }
    };
    // g_new[k][col] = W[pivrow[k]][colof[col]] for this lane's elements; first: g = g_new, else the
    // reference's mixing and stopping test (surfG1D.py:276-284).  Leaves g in Ws and in the old iterate.
    int over = 1, allok = 0;
    // The dense lane map (chain_mix_map.h): lane t < RG n holds column t mod n of the rows t / n + RG s.
    // Slot s of the old iterate lives at [s][t]: the first MLS slots in LDS (the spare rows of the work matrix, 256 lanes
    // per slot; every slot as the compact n x n matrix behind the work matrix when two workgroups share the CU), the others
    // in the global scratch record.  Two loops in two address spaces -- no generic pointer --, the global requests first,
    // then the pivot indices as one batch, the LDS slots, the gathers.  In a remainder-strip class the slot count is
    // known up to the last slot (n > 16 TR), so the loops carry no branch but that one.
    constexpr int MIX_NLO = REM ? 16 * TR + 1 : 1;
    constexpr int MS = rs_mix_max_slots(MIX_NLO, rs_class_nmax(P)), MSMIN = rs_mix_min_slots(MIX_NLO, rs_class_nmax(P));
    constexpr int MLS = GOLD_GLOBAL ? (rs_class_lds_slots(P) < MS ? rs_class_lds_slots(P) : MS) : MS;
    static_assert(MS <= KS, "the global scratch record holds KS slots per lane");
    // where slot s of this lane's old iterate is (ta: the lane's linear index in slot 0, 0 for an idle lane)
    auto old_lds = [&](int s, int t, int ta, bool ok) __attribute__((always_inline)) -> cplx* {
        return GOLD_GLOBAL ? Ws + a.gold_lds_off + t + s * RS_MIX_LANES : Ws + a.gold_lds_off + (ok ? s * mm.stride + ta : 0);
    };
    auto old_glob = [&]() __attribute__((always_inline)) {       // this workgroup's record (a scalar base: rs_gload / rs_gstore)
        return rs_scalar_base(a.gold + (size_t)slot * KS * RS_THREADS);
    };
    constexpr unsigned GSLOT = RS_THREADS * sizeof(cplx);       // bytes of a slot of the record
    // the lazy stopping test (see gather_mix; the three-per-CU instantiations of the four-tile classes 57 and 65 keep the full test: their work matrix never
    //  fits a CU three times, so they are never launched, and with the branch their 64 - 84 bytes of scratch grow by 4 - 8)
    constexpr bool LAZY = !(T16 == 4 && OCC == 3);
    auto gather_mix = [&](bool first, unsigned long long* st) __attribute__((always_inline)) {
        const int t = rs_opaque(tid);
        const int rg0 = (int)(((unsigned)t * mm.rcp) >> 16);
        const bool active = rg0 < mm.rg;
        const int ta = active ? t : 0, rga = active ? rg0 : 0, ca = ta - rga * n;
        const int slots = mm.slots;
        auto on = [&](int s) { return s < MSMIN || s < slots; };                                  // (wave-uniform)
        auto valid = [&](int s) { return active && (s < MSMIN - 1 || rga + mm.rg * s < n); };     // only the last slot has rows >= n
        cplx go[MS], gm[MS];
        const unsigned long long gbase = GOLD_GLOBAL ? old_glob() : 0ull;
        const unsigned tb = (unsigned)t * (unsigned)sizeof(cplx);
        if (!first && GOLD_GLOBAL) {
#pragma unroll
            for (int s = MLS; s < MS; ++s) if (on(s)) go[s] = rs_gload(rs_scalar_advance(gbase, s * GSLOT), 0, tb);
        }
        int pr[MS];
#pragma unroll
        for (int s = 0; s < MS; ++s) pr[s] = on(s) ? pivrow[rga + mm.rg * s] : 0;
        const cplx* gsrc = Ws + colof[ca];
        if (!first) {
#pragma unroll
            for (int s = 0; s < MLS; ++s) if (on(s)) go[s] = *old_lds(s, t, ta, valid(s));
        }
#pragma unroll
        for (int s = 0; s < MS; ++s) gm[s] = on(s) ? gsrc[pr[s] * P] : cmake(0.0, 0.0);
        if (st && tid == 0) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); st[5] = __builtin_amdgcn_s_memrealtime(); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); st[6] = __builtin_amdgcn_s_memrealtime(); }
        bool lane_over = false, lane_ok = true;
        if (!first) {
            // The stopping test by wave (LAZY).  All it feeds are the wave's two flags: over = any element over, ok = every
            // element ok.  A lane that is over on its slot 0 (an LDS slot, valid in every active lane) settles both -- its
            // element is valid and not ok --, so the wave then skips the test of its other slots: the common case, a fixed
            // point is over in every sweep but its last few.  No lane over on slot 0 (NaN elements are neither over nor
            // ok): the other slots are tested as before.  The mixing runs for every slot either way, in its own loop.
            auto test = [&](int s) __attribute__((always_inline)) { rs_stop_test(gm[s], go[s], conv2, valid(s), lane_over, lane_ok); };
            if (LAZY) {
                test(0);
                if (__ballot(lane_over) == 0ull) {
#pragma unroll
                    for (int s = 1; s < MS; ++s) if (on(s)) test(s);
                }
#pragma unroll
                for (int s = 0; s < MS; ++s) if (on(s)) gm[s] = rs_mix(gm[s], go[s], rf, rf1);
            } else {                                    // (every slot tested and mixed in turn)
#pragma unroll
                for (int s = 0; s < MS; ++s) if (on(s)) { test(s); gm[s] = rs_mix(gm[s], go[s], rf, rf1); }
            }
        }
#pragma unroll
        for (int s = 0; s < MLS; ++s) if (on(s) && valid(s)) *old_lds(s, t, ta, true) = gm[s];
        if (GOLD_GLOBAL) {
#pragma unroll
            for (int s = MLS; s < MS; ++s) if (on(s) && valid(s)) rs_gstore(rs_scalar_advance(gbase, s * GSLOT), 0, tb, gm[s]);
        }
        if (!first) {
            const bool w_over = __ballot(lane_over) != 0ull;
            const bool w_ok = __ballot(!lane_ok) == 0ull;
            if (lane == 0) { flags[wave] = w_over ? 1 : 0; flags[RS_WAVES + wave] = w_ok ? 1 : 0; }
        }
        if (st && tid == 0) st[7] = __builtin_amdgcn_s_memrealtime();
        __syncthreads();                                // all gathers done: Ws may be overwritten
        if (st && tid == 0) st[40] = __builtin_amdgcn_s_memrealtime();
        if (tid < 64) colof[tid] = -1;                  // for the next inverse (every lane has read its colof)
        cplx* gdst = Ws + rga * P + ca;
#pragma unroll
        for (int s = 0; s < MS; ++s)
            if (on(s) && valid(s)) gdst[s * mm.rg * P] = gm[s];
        if (!first) {
            over = flags[0] | flags[1] | flags[2] | flags[3];
            allok = flags[4] & flags[5] & flags[6] & flags[7];
        }
        __syncthreads();
    };
    // a job that was set aside continues: its old iterate is the iterate itself (gather_mix leaves the mixed g in both places)
    auto resume_old = [&]() __attribute__((always_inline)) {
        const int t = rs_opaque(tid);
        const int rg0 = (int)(((unsigned)t * mm.rcp) >> 16);
        const bool active = rg0 < mm.rg;
        const int ta = active ? t : 0, rga = active ? rg0 : 0, ca = ta - rga * n;
        const unsigned long long gbase = GOLD_GLOBAL ? old_glob() : 0ull;
#pragma unroll
        for (int s = 0; s < MS; ++s) {
            if (s < mm.slots && active && rga + mm.rg * s < n) {
                const cplx v = Ws[(rga + mm.rg * s) * P + ca];
                if (s < MLS) *old_lds(s, t, ta, true) = v; else rs_gstore(rs_scalar_advance(gbase, s * GSLOT), 0, (unsigned)t * (unsigned)sizeof(cplx), v);
            }
        }
    };

    // ---- a job starts: g0 = inv(A) is the first pass through the inverse of a fresh job, so the work matrix starts as A
    // (its padding zero; it is never written afterwards).  A cache hit starts from the stored iterate instead and goes
    // straight to Sigma = t g t^H; a job that was set aside continues from its iterate with the products of its next sweep.
    const bool gc_hit = a.gc_mode == 2;
    bool first = true, skip = false;
    int q_end = 0;
    auto next_job = [&]() __attribute__((always_inline)) -> bool {
        if (RR) {
            if (tid == 0) rr_msg = rs_rr_pop(a.rr_q, a.order);
            __syncthreads();                            // (also: every wave is done with the LDS of the previous job)
            const long long ent = rr_msg;
            __syncthreads();
            if (ent < 0) return false;
            job = (int)(ent & 0xffffffffll); count = (int)(ent >> 32);
        } else {
            job = a.order ? a.order[slot] : slot; count = 0;
        }
        resume = count > 0;
        c = job % a.n_contacts; b = job / a.n_contacts;
        n = a.nc[c]; off = a.blk_off[c]; ksteps = (n + 3) >> 2;
        alpha = a.alpha + off; Salpha = a.Salpha + off;
        mm = rs_mix_map(n);
        pad_c = a.pad + (size_t)c * (CHAIN_PAD * CHAIN_PAD); pad_ps = (unsigned)a.n_contacts * (CHAIN_PAD * CHAIN_PAD);
        e = E[b]; z = cmake(e.x, e.y + a.eta);
        e = cmake(rs_uniform(e.x), rs_uniform(e.y)); z = cmake(rs_uniform(z.x), rs_uniform(z.y));   // (the same for every lane: scalar registers)
        opz = z;
        over = 1; allok = 0;
        first = !resume; skip = resume; final_pass = false;
        q_end = count + a.rr_quantum;
        if (gc_hit || resume) {
            if (resume) __threadfence();                // (acquire side of the queue entry lane 0 popped: the iterate below was
                                                        //  written by another workgroup of this launch)
            const cplx* gcj = (gc_hit ? a.gcache : blk) + (size_t)b * a.blk_stride + off;
            for (int t = tid; t < WELEMS; t += RS_THREADS) {
                const int i = t / P, j = t - i * P;
                Ws[t] = sel(i < n && j < n, gcj[min(i, n - 1) * n + min(j, n - 1)]);
            }
        } else {
            for (int t = tid; t < WELEMS; t += RS_THREADS) {
                const int i = t / P, j = t - i * P;
                Ws[t] = sel(i < n && j < n, Aat(i, j));
            }
        }
        if (resume) {
            // the old iterate of the mixing step is the iterate itself (gather_mix leaves the mixed g in both places)
            __syncthreads();
            resume_old();
        }
        if (tid < 64) { colof[tid] = -1; pivrow[tid] = 0; }
        __syncthreads();
        return true;
    };

    // One copy of every phase in the instruction stream (the loop body has to stay inside the 64 KB
    // instruction cache two CUs share): the start g0 = inv(A) is the first pass through the inverse, and
    // Sigma = t g t^H (t = E Stau - tau, no eta) runs as a last pass through the two products with t in
    // place of B:  X = t g (row tiles) -> Ws,  Sigma = X t^H (column tiles) -> global.
    bool need_job = true;
    while (true) {
        if (__builtin_expect(need_job, 0)) {
            if (!next_job()) break;                     // (round robin: the queue is empty -- every job is finished or held by a running workgroup)
            need_job = false;
        }
        unsigned long long* st = (RS_STAMPS && a.stamps && job == 0 && count == a.stamp_sweep) ? a.stamps : nullptr;
        if (st && tid == 0) st[0] = __builtin_amdgcn_s_memrealtime();
        if (!gc_hit && !skip) {
            // a remainder-strip class: the compile-time stage schedule; else, and with the roles by wave number, the generic loop
            // (role 3 factors whether the roles follow the SIMDs or, two waves having reported the same one, the wave numbers)
            if constexpr (SCHED_TABLES) rs_inverse_sched<T16, P, TR>(n, Ws, pivrow, pivoff, colof, rowline, tid, wave, st ? st + 8 : nullptr);
            else
            rs_inverse<T16, P, REM ? TR : -1>(n, Ws, pivrow, colof, rowline, tid, wave, chain_roles, st ? st + 8 : nullptr);   // st + 8: stage stamps, st + 24: factor
            if (st && tid == 0) st[1] = __builtin_amdgcn_s_memrealtime();
            if (!(RS_ABLATE & 8) || first) gather_mix(first, st);
            else { if (tid < 64) colof[tid] = -1; __syncthreads(); }
            if (st && tid == 0) st[2] = __builtin_amdgcn_s_memrealtime();
            if (!first) ++count;
            first = false;
        }
        if (__builtin_expect(skip, 0)) {
            skip = false;
        } else if (gc_hit || (a.force_iters >= 0 ? count >= a.force_iters : !(over && count < a.max_iter))) {
            final_pass = true;
            opz = e;
            if (a.gc_mode == 1) {                       // a miss leaves its final iterate in the cache (g sits in Ws, complete
                cplx* gcj = a.gcache + (size_t)b * a.blk_stride + off;                              //  since the barrier that ends gather_mix)
                for (int t = tid; t < n * n; t += RS_THREADS) { const int i = t / n; gcj[t] = Ws[i * P + (t - i * n)]; }
            }
        } else if (__builtin_expect(RR && count >= q_end, 0)) {
            // the quantum is over.  Nobody waiting: carry on.  Otherwise the iterate goes to the job's output block (g sits in
            // Ws, complete since the barrier that ends gather_mix), the job to the back of the queue, and this workgroup
            // takes the job at the front
            if (tid == 0) rr_msg = rs_rr_waiting(a.rr_q) ? 1 : 0;
            __syncthreads();
            const bool sw = rr_msg != 0;
            __syncthreads();
            if (sw) {
                cplx* gsj = blk + (size_t)b * a.blk_stride + off;
                for (int t = tid; t < n * n; t += RS_THREADS) { const int i = t / n; gsj[t] = Ws[i * P + (t - i * n)]; }
                __threadfence();                        // release side: the iterate is visible before the queue entry is
                __syncthreads();
                if (tid == 0) rs_rr_push(a.rr_q, job, count);
                need_job = true;
                continue;
            }
            q_end = count + a.rr_quantum;
        }
        d4 mr[T16], mi[T16], mc[T16];
        if (RS_ABLATE & 4) {
#pragma unroll
            for (int t = 0; t < T16; ++t) { mr[t] = (d4){1e-3, 0, 0, 0}; mi[t] = mr[t]; mc[t] = mr[t]; }
        }
        // T = B g : row tile `wave`; g is read from Ws by every wave, so T waits in registers
        if (!(RS_ABLATE & 4)) gemm_rowtile(mr, mi, mc);
        __syncthreads();
        store_rowtile(mr, mi, mc);
        __syncthreads();
        if (st && tid == 0) st[3] = __builtin_amdgcn_s_memrealtime();
        // T B^H : column tile `wave`
        if (!(RS_ABLATE & 4)) gemm_coltile(mr, mi, mc);
        const int fis = rs_opaque(lane & 15), fks = rs_opaque(lane >> 4);
        if (final_pass) {
            cplx* out = blk + (size_t)b * a.blk_stride + off;
#pragma unroll
            for (int ti = 0; ti < T16; ++ti)
                for_tile(ti, wave, mr[ti], mi[ti], mc[ti], true, fis, fks,
                         [&](int r, int i, int j, double re, double im) { if (i < n && j < n) out[i * n + j] = cmake(re, im); });
            if (tid == 0 && !gc_hit) {                  // (a hit's counts and flags are copied from the cache by the launcher's caller)
                if (iters) iters[(size_t)b * a.n_contacts + c] = count;
                if (converged) converged[(size_t)b * a.n_contacts + c] = (count > 0 && allok) ? 1 : 0;
            }
            if (!RR) break;
            need_job = true;
            continue;
        }
        __syncthreads();
        // M = A - T B^H.  With the padded alpha, Salpha no load needs the store's guard: the (up to) eight loads of a
        // row tile go out together and are consumed in order as they arrive (a ladder of vmcnt waits, one round trip per
        // tile); those of tile ti + 1 go out after tile ti is stored (requested before it they spill: 39 VGPRs in <51,3,true,false>)
        // SC: this wave's column tile is the column strip (its tiles ti < TR use the strip's lane map, see for_tile).
        // Every element is a compile-time row offset from one lane base, in the padded alpha / Salpha and in Ws.
        // Tests: none for a full tile of a remainder-strip class (inside every contact of the launch by the launcher's
        // class rule), the strip's own rows / columns against n; every element in the other classes.
        auto mstore = [&](auto sc) __attribute__((always_inline)) {
            constexpr bool SC = decltype(sc)::value;
            const int ljn = wave * 16 + fis, lis = 4 * (fis >> 2) + fks, ljs = TR * 16 + (fis & 3);
            const unsigned lon = (unsigned)(fks * CHAIN_PAD + ljn), los = (unsigned)(lis * CHAIN_PAD + ljs);
            cplx* wn = Ws + fks * P + ljn;
            cplx* wsc = Ws + lis * P + ljs;
            auto smap = [](int ti) { return SC && ti < TR; };
            auto nel = [&](int ti) { return smap(ti) || (REM && ti == TR) ? 1 : 4; };
            auto rowc = [&](int ti, int r) { return ti * 16 + (smap(ti) ? 0 : 4 * r); };
            cplx as[4], aa[4];
            const unsigned long long bS = rs_scalar_base(lead_p(1)), bA = rs_scalar_base(lead_p(0));
            const unsigned lbn = lon * (unsigned)sizeof(cplx), lbs = los * (unsigned)sizeof(cplx);
            unsigned long long curS = bS, curA = bA;        // the bases at row cur_row
            int cur_row = 0;
            auto load_a = [&](int ti, cplx (&s)[4], cplx (&m)[4]) __attribute__((always_inline)) {
#pragma unroll
                for (int r = 0; r < nel(ti); ++r) {
                    const unsigned lb = smap(ti) ? lbs : lbn;
                    const long long adv = (long long)(rowc(ti, r) - cur_row) * CHAIN_PAD * (long long)sizeof(cplx);
                    if (adv) { curS = rs_scalar_advance(curS, adv); curA = rs_scalar_advance(curA, adv); cur_row = rowc(ti, r); }
                    s[r] = rs_gload(curS, 0, lb); m[r] = rs_gload(curA, 0, lb);
                }
            };
            load_a(0, as, aa);
            // T B^H out of the 3M sums first, in place: two values per element are live beside the A buffers, not three
            if (M3G) {
#pragma unroll
                for (int ti = 0; ti < T16; ++ti)
#pragma unroll
                    for (int r = 0; r < nel(ti); ++r) {
                        const double va = mr[ti][r], vb = mi[ti][r], vc = mc[ti][r];
                        mr[ti][r] = va + vb; mi[ti][r] = vc - va + vb;
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int ti = 0; ti < T16; ++ti) {
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r = 0; r < nel(ti); ++r) {
                    const double re = mr[ti][r], im = mi[ti][r];
                    const cplx av = csub(cmul(z, as[r]), aa[r]);
                    const int i = rowc(ti, r) + (smap(ti) ? lis : fks), j = smap(ti) ? ljs : ljn;
                    const bool ok = !REM ? (i < n && j < n) : ((ti < TR || i < n) && (!SC || j < n));
                    if (ok) (smap(ti) ? wsc : wn)[rowc(ti, r) * P] = cmake(av.x - re, av.y - im);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (ti + 1 < T16) load_a(ti + 1, as, aa);
            }
        };
        if (!REM || wave < TR) mstore(std::false_type{});
        else if (wave == TR) mstore(std::true_type{});
        // (a remainder-strip class's wave > TR owns no column of the matrix)
        __syncthreads();
        if (st && tid == 0) st[4] = __builtin_amdgcn_s_memrealtime();
    }
}

template <int P, int OCC, bool GOLD_GLOBAL, bool RR>
__global__ __launch_bounds__(RS_THREADS, OCC) void chain1d_rs_kernel(
    ChainRsArgs a, const cplx* __restrict__ E, cplx* __restrict__ blk, int* __restrict__ iters,
    int* __restrict__ converged)
{
    chain1d_rs_body<P, OCC, GOLD_GLOBAL, RR, true>(a, E, blk, iters, converged);
}

// the generic loop in the remainder-strip classes (launched with the roles by wave number; the other classes have one kernel)
template <int P, int OCC, bool GOLD_GLOBAL, bool RR>
__global__ __launch_bounds__(RS_THREADS, OCC) void chain1d_rs_wn_kernel(
    ChainRsArgs a, const cplx* __restrict__ E, cplx* __restrict__ blk, int* __restrict__ iters,
    int* __restrict__ converged)
{
    chain1d_rs_body<P, OCC, GOLD_GLOBAL, RR, false>(a, E, blk, iters, converged);
}

}  // namespace

bool chain1d_lds_supported(int nc_max) { return nc_max <= 64; }

namespace {
// sweeps a job runs before it makes room for a waiting one (0 = every job runs to its end in one go)
int rs_rr_quantum(int user)
{
    return user >= 0 ? user : 100;                   // negf_set_chain_round_robin, or the default
}
size_t rs_gold_elems(int nc_max, int n_contacts, int nb)
{
    return (size_t)rs_mix_reserved_slots(nc_max) * RS_THREADS * n_contacts * nb;     // >= KS slots per lane
}
// entries of the job queue's ring: a job is queued at most once per quantum (0: no round robin for this launch)
size_t rs_ring_entries(int n_contacts, int nb, int max_sweeps, int rr_user)
{
    const int q = rs_rr_quantum(rr_user);
    if (q <= 0 || max_sweeps <= q) return 0;
    const size_t jobs = (size_t)n_contacts * nb;
    const size_t cap = jobs * ((size_t)max_sweeps / q + 1) + 2048;
    return (cap >> 27) ? 0 : cap;
}
}  // namespace

// lane-private copies of the iterate (one set per launch slot) + the job queue of the round-robin launch
size_t chain1d_lds_scratch_elems(int nc_max, int n_contacts, int nb, int max_sweeps, int rr_quantum)
{
    return rs_gold_elems(nc_max, n_contacts, nb) + 1 + (rs_ring_entries(n_contacts, nb, max_sweeps, rr_quantum) + 1) / 2;
}

namespace {

// The launch configuration of pitch class P: workgroups per CU from the LDS share of a workgroup (+ < 1 KB of static
// LDS) -- the work matrix alone when the old iterate goes to global scratch (gold_global), both matrices otherwise
// (allocated in granules of 1280 bytes: 53.8 KB per workgroup is the most that still fits three times).
struct RsConfig { int occ; bool gold_global; size_t smem; };
template <int P>
RsConfig rs_config(int n_max, bool have_scratch, int occ_env)
{
    constexpr int T16 = (P - 1 + 15) / 16;
    constexpr int OCC_MAX = T16 <= 2 ? 4 : 3;          // register budget: 128 VGPRs (T16 <= 2), 168 above
    const size_t wmat = (size_t)(16 * T16 * P + 16) * sizeof(cplx);
    const size_t gold_lds = (size_t)n_max * n_max * sizeof(cplx);
    auto fits = [](size_t smem, int per_cu) { return ((smem + 832 + 1279) / 1280) * 1280 * per_cu <= 160 * 1024; };
    if (occ_env != 2 && fits(wmat + gold_lds, OCC_MAX)) return {OCC_MAX, false, wmat + gold_lds};
    if (occ_env != 2 && have_scratch && fits(wmat, OCC_MAX)) return {OCC_MAX, true, wmat};
    if (fits(wmat + gold_lds, 2) || !have_scratch) return {2, false, wmat + gold_lds};
    return {2, true, wmat};
}
int rs_occ_env()
{
    static int occ_env = -1;
    if (occ_env < 0) { const char* e = getenv("NEGF_CHAIN1D_OCC"); occ_env = e ? atoi(e) : 0; }
    return occ_env;
}
int rs_n_cus()
{
    static int n_cus = 0;
    if (!n_cus) {
        int dev = 0; hipDeviceProp_t prop;
        n_cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 256;
    }
    return n_cus;
}
// One instantiation per pitch class of the largest contact (smaller contacts of the same launch run
// in the same padded matrix): the smallest odd pitch of the list that holds n_max columns.  The remainder-strip
// classes (19, 35, 51: the last tile holds <= 4 rows / columns and runs on the 4x4x4 instruction) store their
// full tiles unguarded and count every k-step below the strip as inside the matrix, i.e. they assume that EVERY
// contact of the launch reaches into the strip, n > 16 TR.  A launch whose smallest contact does not (contacts of
// unequal size, e.g. n_c = (50, 40)) takes the next class without strips, whose stores and k-steps are guarded
// by the contact's own n.
// rs_class_n: the size that selects the class; RS_CLASSES(n, CASE): CASE(P) of that class.
int rs_class_n(const SigmaProvider& p)
{
    int n = p.nc_max, n_min = n;
    for (int k : p.nc) n_min = std::min(n_min, k);
    const int strip_base = n <= 16 ? -1 : n <= 19 ? 16 : (n > 32 && n <= 35) ? 32 : (n > 48 && n <= 51) ? 48 : -1;
    if (strip_base > 0 && n_min <= strip_base) n = strip_base == 16 ? 25 : strip_base == 32 ? 41 : 57;
    return n;
}
#ifdef RS_FAST_BUILD
#define RS_CLASSES(n, CASE) do { if ((n) <= 16) CASE(17); else CASE(51); } while (0)
#else
#define RS_CLASSES(n, CASE) do { \
    if ((n) <= 16) CASE(17); \
    else if ((n) <= 19) CASE(19);                /* 16 + a remainder strip */ \
    else if ((n) <= 25) CASE(25); \
    else if ((n) <= 32) CASE(33); \
    else if ((n) <= 35) CASE(35);                /* 32 + a remainder strip */ \
    else if ((n) <= 41) CASE(41); \
    else if ((n) <= 48) CASE(49); \
    else if ((n) <= 51) CASE(51); \
    else if ((n) <= 57) CASE(57); \
    else CASE(65); } while (0)
#endif
// resident slots of a launch: workgroups per CU of its class x compute units (rr_slots > 0: at most that many -- tests)
int rs_launch_slots(const SigmaProvider& p, bool have_scratch, int rr_slots)
{
    int occ = 2;
#define RS_CASE(PP) occ = rs_config<PP>(p.nc_max, have_scratch, rs_occ_env()).occ
    RS_CLASSES(rs_class_n(p), RS_CASE);
#undef RS_CASE
    const int slots = occ * rs_n_cus();
    return rr_slots > 0 ? std::min(rr_slots, slots) : slots;
}

template <int P>
void chain1d_rs_launch(hipStream_t st, ChainRsArgs a, int n_max, int n_contacts, int nb, const cplx* E, cplx* blk,
                       int* iters, int* conv, cplx* gold_scratch, int slots, unsigned rr_cap)
{
    constexpr int T16 = (P - 1 + 15) / 16;
    const RsConfig cf = rs_config<P>(n_max, gold_scratch != nullptr, rs_occ_env());
    // old iterate behind the work matrix (all slots in LDS), or its first slots in the unused rows n_max+2 .. of the
    // work matrix and the rest in global scratch
    a.gold_lds_off = cf.gold_global ? (n_max + 2) * P : 16 * T16 * P + 16;
    auto launch = [&](auto kern, auto kern_rr) {
        dim3 grid(n_contacts, nb);
        // A launch with more jobs than resident slots (a.rr_quantum > 0: launch_chain1d_lds) runs from the job queue, one
        // persistent workgroup per slot, whether or not an order is known.  On the C3 grid (4000 jobs, 768 slots; 2760 jobs
        // run to the 2000-sweep cap) the queue takes 576.4 ms per step started in the learned order and 576.1 ms in launch
        // order, the plain kernel dealt longest first 584.9 ms (spreads 1.6 - 2.3 ms, scripts/time_chain_rule.py).  The
        // likely reason, not measured on its own: under the queue the capped jobs advance together and end with the chip
        // full; dealt one by one the slots finish up to one short job apart.  The job loop itself costs 1.2 % per sweep at
        // the most (equal jobs: 62.6 against 61.9 us per sweep and slot), less than that tail.
        // A launch that fits the chip runs the plain kernel in the predicted order (648 jobs: 42 against 48 ms).
        const int jobs = n_contacts * nb;
        const bool rr = a.rr_quantum > 0;
        if (rr) {
            hipLaunchKernelGGL(rs_rr_init_kernel, dim3((rr_cap + 255) / 256), dim3(256), 0, st, a.rr_q, rr_cap, (unsigned)jobs);
            grid = dim3(slots, 1);
        }
        static int log_env = -1;
        if (log_env < 0) log_env = getenv("NEGF_CHAIN_LOG") ? 1 : 0;
        if (log_env) fprintf(stderr, "[chain launch] jobs %d slots %d quantum %d order %d gc_mode %d\n", jobs, slots, a.rr_quantum, a.order ? 1 : 0, a.gc_mode);
        auto go = [&](auto k) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024) != hipSuccess)
                (void)hipGetLastError();
            hipLaunchKernelGGL(k, grid, dim3(RS_THREADS), cf.smem, st, a, E, blk, iters, conv);
        };
        if (rr) go(kern_rr); else go(kern);
    };
    constexpr int OCC_MAX = T16 <= 2 ? 4 : 3;          // (rs_config)
#define RS_PICK(KERN) do { \
        if (cf.occ == OCC_MAX && !cf.gold_global) launch(KERN<P, OCC_MAX, false, false>, KERN<P, OCC_MAX, false, true>); \
        else if (cf.occ == OCC_MAX) launch(KERN<P, OCC_MAX, true, false>, KERN<P, OCC_MAX, true, true>); \
        else if (!cf.gold_global) launch(KERN<P, 2, false, false>, KERN<P, 2, false, true>); \
        else launch(KERN<P, 2, true, false>, KERN<P, 2, true, true>); } while (0)
    // a strip class launched with the roles by wave number runs the kernels with the generic inverse
    constexpr bool STRIPS = T16 >= 2 && P - 16 * (T16 - 1) <= 4;
    if constexpr (STRIPS && rs_stage_sched(T16 - 1)) {
        if (!a.simd_roles) { RS_PICK(chain1d_rs_wn_kernel); return; }
    }
    RS_PICK(chain1d_rs_kernel);
#undef RS_PICK
}

}  // namespace

// does this launch (a miss, with its scratch) run from the job queue?  More jobs than resident slots, and a ring to set
// jobs aside in: a quantum (rr_quantum as in launch_chain1d_lds; 0: never) below the launch's sweep cap
bool chain1d_lds_runs_queue(const SigmaProvider& p, int nb, int rr_quantum, int rr_slots)
{
    return rs_ring_entries(p.n_contacts, nb, std::max(p.max_iter, p.force_iters), rr_quantum) > 0 &&
           p.n_contacts * nb > rs_launch_slots(p, true, rr_slots);
}

void launch_chain1d_lds(hipStream_t st, const SigmaProvider& p, const int* d_nc, const int* d_blk_off, int nb,
                        const cplx* E, cplx* blk, int* iters, int* conv, cplx* gold_scratch, const int* order,
                        cplx* gcache, int gc_mode, int rr_quantum, int rr_slots)
{
    ChainRsArgs a;
    a.order = order;
    a.gcache = gcache; a.gc_mode = gcache ? gc_mode : 0;
    a.alpha = p.d_alpha; a.Salpha = p.d_Salpha; a.beta = p.d_beta; a.Sbeta = p.d_Sbeta;
    a.tau = p.d_tau; a.Stau = p.d_Stau; a.pad = p.d_lead_pad;
    a.nc = d_nc; a.blk_off = d_blk_off;
    a.n_contacts = p.n_contacts; a.blk_stride = p.blk_stride;
    a.eta = p.eta; a.conv = p.conv; a.relFactor = p.relFactor;
    a.max_iter = p.max_iter; a.force_iters = p.force_iters;
    a.gold = gold_scratch;
    // the job queue sits behind the iterate copies (chain1d_lds_scratch_elems); a cache hit runs no sweeps
    a.rr_quantum = 0; a.rr_q = nullptr;
    unsigned rr_cap = 0;
    const int slots = rs_launch_slots(p, gold_scratch != nullptr, rr_slots);
    if (gold_scratch && a.gc_mode != 2 && chain1d_lds_runs_queue(p, nb, rr_quantum, rr_slots)) {
        a.rr_q = reinterpret_cast<RsQueue*>(gold_scratch + rs_gold_elems(p.nc_max, p.n_contacts, nb));
        rr_cap = (unsigned)rs_ring_entries(p.n_contacts, nb, std::max(p.max_iter, p.force_iters), rr_quantum);
        a.rr_quantum = rs_rr_quantum(rr_quantum);
    }
    static unsigned long long* d_stamps = nullptr;
    static int want_stamps = -1;
    if (want_stamps < 0) {
        want_stamps = getenv("NEGF_CHAIN_STAMPS") ? 1 : 0;
        if (want_stamps) { (void)hipMalloc(&d_stamps, 64 * sizeof(unsigned long long)); (void)hipMemset(d_stamps, 0, 64 * sizeof(unsigned long long)); }
    }
    a.stamps = d_stamps;
    { const char* e = getenv("NEGF_CHAIN_STAMP_SWEEP"); a.stamp_sweep = e ? atoi(e) : 10; }
    static int roles_env = -1;
    if (roles_env < 0) { const char* e = getenv("NEGF_CHAIN1D_ROLES"); roles_env = e ? atoi(e) : 1; }
    a.simd_roles = roles_env;
    const int n_max = p.nc_max;
#define RS_CASE(PP) chain1d_rs_launch<PP>(st, a, n_max, p.n_contacts, nb, E, blk, iters, conv, gold_scratch, slots, rr_cap)
    RS_CLASSES(rs_class_n(p), RS_CASE);
#undef RS_CASE
    if (d_stamps) {
        (void)hipStreamSynchronize(st);
        unsigned long long h[64];
        (void)hipMemcpy(h, d_stamps, sizeof(h), hipMemcpyDeviceToHost);
        if (h[0]) {
            auto us = [&](int i) { return h[i] ? (double)(h[i] - h[0]) / 100.0 : -1.0; };
            fprintf(stderr, "[chain stamps] sweep %d (us):", a.stamp_sweep); fprintf(stderr, " inverse %.2f  diff+mix %.2f  T=Bg %.2f  M=A-TB^H %.2f  (total %.2f) | inverse stages:",
                    us(1), us(2) - us(1), us(3) - us(2), us(4) - us(3), us(4));
            for (int i = 8; i < 16 && h[i]; ++i) fprintf(stderr, " %.2f", (double)(h[i] - h[0]) / 100.0);
            fprintf(stderr, " | mix: lds %.2f vmem %.2f computed+stored %.2f barrier %.2f", us(5) - us(1), us(6) - us(1), us(7) - us(1), us(40) - us(1));
            fprintf(stderr, " | column step 4 of panel 1 (shader cycles): search %llu  pivot-row exchange %llu  reciprocal+coef %llu  64 FMAs %llu",
                    h[8 + 41] - h[8 + 40], h[8 + 42] - h[8 + 41], h[8 + 43] - h[8 + 42], h[8 + 44] - h[8 + 43]);
            fprintf(stderr, " | factor begin-end:");
            for (int i = 24; i < 38 && h[i]; i += 2) fprintf(stderr, " %.2f-%.2f", (double)(h[i] - h[0]) / 100.0, (double)(h[i + 1] - h[0]) / 100.0);
            fprintf(stderr, "\n");
        }
    }
}
