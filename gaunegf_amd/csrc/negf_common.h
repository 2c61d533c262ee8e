// Internal declarations shared by the translation units of libnegf_hip.so.
// gfx950 (MI355X) only; wavefront = 64.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <memory>
#include "../../include/negf.h"
#include "../../include/negf_layered_channels.h"

// ------------------------------------------------------------------ complex
// complex128 as an aligned pair: one 16-byte global/LDS access per element.
struct __attribute__((aligned(16))) cplx {
    double x, y;
};
static_assert(sizeof(cplx) == 16, "cplx must be 16 bytes");

__host__ __device__ __forceinline__ cplx cmake(double a, double b) { cplx r; r.x = a; r.y = b; return r; }
__host__ __device__ __forceinline__ cplx cadd(cplx a, cplx b) { return cmake(a.x + b.x, a.y + b.y); }
__host__ __device__ __forceinline__ cplx csub(cplx a, cplx b) { return cmake(a.x - b.x, a.y - b.y); }
__host__ __device__ __forceinline__ cplx cneg(cplx a) { return cmake(-a.x, -a.y); }
__host__ __device__ __forceinline__ cplx cconj(cplx a) { return cmake(a.x, -a.y); }
__host__ __device__ __forceinline__ cplx cmul(cplx a, cplx b) {
    return cmake(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// a - b*c
__host__ __device__ __forceinline__ cplx cfnma(cplx a, cplx b, cplx c) {
    return cmake(a.x - b.x * c.x + b.y * c.y, a.y - b.x * c.y - b.y * c.x);
}
// a + b*c
__host__ __device__ __forceinline__ cplx cfma(cplx a, cplx b, cplx c) {
    return cmake(a.x + b.x * c.x - b.y * c.y, a.y + b.x * c.y + b.y * c.x);
}
__host__ __device__ __forceinline__ cplx cscale(cplx a, double s) { return cmake(a.x * s, a.y * s); }
// LAPACK izamax metric |re|+|im| (what zgetrf pivots on)
__host__ __device__ __forceinline__ double cabs1(cplx a) { return fabs(a.x) + fabs(a.y); }
__host__ __device__ __forceinline__ double cabs2(cplx a) { return a.x * a.x + a.y * a.y; }
// 1/a with scaling against overflow/underflow (Smith)
__host__ __device__ __forceinline__ cplx crecip(cplx a) {
    if (fabs(a.x) >= fabs(a.y)) {
        double r = a.y / a.x;
        double d = a.x + a.y * r;
        return cmake(1.0 / d, -r / d);
    } else {
        double r = a.x / a.y;
        double d = a.x * r + a.y;
        return cmake(r / d, -1.0 / d);
    }
}

// -------------------------------------------------------------- error macros
#define NEGF_HIP_CHECK(expr)                                                          \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            fprintf(stderr, "[negf] HIP error %s at %s:%d: %s\n", #expr, __FILE__,    \
                    __LINE__, hipGetErrorString(_e));                                 \
            return NEGF_EHIP;                                                         \
        }                                                                             \
    } while (0)

// ------------------------------------------------------------------- context
// A device buffer of the context (or of a provider) that only grows: ensure_cap() / release_bufs() in negf_api.hip are
// the one place where such a buffer is allocated and freed.  Reads as the pointer it holds.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;                // elements
    operator T*() const { return p; }
};

constexpr int CHAIN_PAD = 64;      // rows and pitch of the padded lead matrices (SigmaProvider::d_lead_pad)

enum SigmaKind { SK_CONST = 0, SK_CHAIN1D = 2, SK_BETHE = 3, SK_PRECOMPUTED = 4 };

struct SigmaProvider {
    int kind = -1;
    int n_contacts = 0;
    // CONST: dense per-contact Sigma [n_contacts][n][n] and their sum, on device
    cplx* d_const_c = nullptr;     // [n_contacts][n*n]
    cplx* d_const_tot = nullptr;   // [n*n]
    cplx* d_hbase = nullptr;       // F + Sigma_tot (CONST only): A = E S - hbase
    // block providers (CHAIN1D / BETHE): contact blocks scattered at inds x inds
    std::vector<int> nc;           // block size per contact
    std::vector<int> blk_off;      // offset (in cplx) of contact c inside one energy's block record
    int blk_stride = 0;            // cplx per energy = sum nc^2
    int nc_max = 0;
    int* d_inds = nullptr;         // concatenated orbital indices
    int *d_nc = nullptr, *d_blk_off = nullptr, *d_inds_off = nullptr;   // device copies
    int *d_n_atoms = nullptr, *d_atom_off = nullptr;
    int* d_pos = nullptr;          // [n_contacts][n]: position of orbital i in contact c's index list, -1 outside (small fused path)
    std::vector<int> inds_off;     // offset of contact c in d_inds
    std::vector<int> h_inds;
    // CHAIN1D matrices, concatenated [sum nc^2] each
    cplx *d_alpha = nullptr, *d_Salpha = nullptr, *d_beta = nullptr, *d_Sbeta = nullptr,
         *d_tau = nullptr, *d_Stau = nullptr;
    // the same six matrices once more for the register-stationary chain kernel (k_chain1d_rs.hip, nc_max <= 64):
    // [matrix, in the order above][contact][CHAIN_PAD][CHAIN_PAD], zero outside n x n -- a lane reads them at compile-
    // time offsets from one base, without clamps.  Written where the six are uploaded, constant for the provider's life
    cplx* d_lead_pad = nullptr;
    // host copy of alpha | Salpha | beta | Sbeta and its 64-bit hash: what the surface Green's function depends on
    // besides eta / conv / relFactor / max_iter -- the key of the context's g(E) cache (ChainGEntry)
    std::shared_ptr<std::vector<cplx>> h_lead;     // shared with the cache entries this provider fills
    unsigned long long lead_hash = 0;
    double eta = 0, conv = 0, relFactor = 0, mix = 0;
    int max_iter = 0, force_iters = -1;
    // CHAIN1D: how the surface Green's function is found.  0 = the reference's relaxed fixed point (conv, relFactor,
    // max_iter as above), 1 = renormalisation-decimation (k_chain1d_rd.hip): conv holds its tol, max_iter its max_steps,
    // force_iters its force_steps, relFactor is unused (1)
    int solver = 0;
    // job order of the next chain launch (predicted on the device)
    DevBuf<int> d_order;
    // energies and sweep counts of the previous evaluation: the order of a NEW grid is predicted from them.
    // An evaluation may arrive in several batch chunks (m0 = 0, nb, 2 nb ...): the chunks are appended to
    // cur*, and the chunk with m0 = 0 of the NEXT evaluation promotes cur* to prev*.
    cplx *d_prevE = nullptr, *d_curE = nullptr;
    int *d_prev_iters = nullptr, *d_cur_iters = nullptr;
    int prev_n = 0, prev_cap = 0, cur_n = 0, cur_cap = 0;
    // BETHE
    std::vector<int> n_atoms;      // atoms per contact
    int* d_atom_orbs = nullptr;    // [total_atoms][9]
    int* d_nb_off = nullptr;       // [total_atoms+1]
    int* d_nb_dirs = nullptr;
    std::vector<int> atom_off;     // first atom of contact c
    double* d_H = nullptr;         // [n_contacts][81]
    double* d_Slist = nullptr;     // [n_contacts][12][81]
    double* d_Vlist = nullptr;
    cplx* d_xi = nullptr;          // [n*n] or null
    // compact coupling matrices: Gamma_c lives on the index list inds[inds_off[c] .. +nc[c]) only
    // (block providers without Xi; CONST providers whose matrices vanish outside a small support)
    bool compact_ok = false;
    cplx* d_const_blk = nullptr;   // CONST: Sigma_c restricted to its support, [blk_stride]
    // CONST: every contact's Sigma has a nonzero support and the block fields above describe it (set whenever that
    // holds, also when the supports cover more than half of the orbitals and compact_ok is false): the eigenchannel
    // path (negf_transmission_channels) reads Gamma_c on its orbital list from d_const_blk.  Without compact_ok the
    // provider keeps blk_stride = 0: it sizes the context's Sigma block staging (d_blk), which no CONST path reads
    bool has_blocks = false;
    // PRECOMPUTED
    int m_pre = 0;
    int pre_nc = 0;
    bool pre_is_gamma = false;     // d_pre_c holds the Gamma matrices themselves
    cplx* d_pre_tot = nullptr;     // [m][n*n]
    cplx* d_pre_c = nullptr;       // [m][pre_nc][n*n] or null
};

// One cached evaluation of the 1-D chain fixed point: the final iterates g(E_m) of every (energy, contact) of one
// launch, with the sweep counts and convergence flags the launch reported.  g depends on the lead cell (alpha, Salpha,
// beta, Sbeta), eta, conv, relFactor, max_iter (and force_iters) and E -- NOT on F or on the coupling blocks tau
// (surfG1D.py:256-262; setF refreshes tau only, :319-329) -- so an entry is keyed on exactly those, bitwise, and
// outlives the provider that filled it: a provider re-created after setF, the t = I variant behind surfG.g(), the two
// Sigma evaluations of GrLessInt, calculate_transmission + calculate_dos on one grid and SCF cycles at a fixed Fermi
// level all find it.  A hit runs only Sigma = t g t^H (the last pass of the chain kernel) and is bit-identical to a miss.
struct ChainGEntry {
    std::vector<int> nc;
    std::shared_ptr<std::vector<cplx>> lead;
    unsigned long long lead_hash = 0, E_hash = 0;
    double eta = 0, conv = 0, relFactor = 0;
    int max_iter = 0, force_iters = -1;
    int solver = 0;                                // (SigmaProvider::solver: an entry serves the solver that filled it only)
    std::vector<cplx> E;
    cplx* d_g = nullptr;    size_t g_cap = 0;      // [energies][blk_stride]
    int* d_it = nullptr;    int* d_cv = nullptr;   size_t it_cap = 0;   // [energies][n_contacts]
    unsigned long long used = 0;
    bool valid = false;
};

// side streams of the windowed inverse (small batches are cut into up to four stream groups, k_inverse_blocked.hip):
// owned by the context
struct GjSideStreams {
    static constexpr int MAXG = 4;
    hipStream_t s[MAXG - 1] = {};
    hipEvent_t fork = nullptr, join[MAXG - 1] = {};
    bool ok = false;
};

// What the blocked inverse launches for a shape (gj_plan, k_inverse_blocked.hip; negf_inverse_plan): the launch code
// reads this and decides nothing itself.
// window kernel ids (also the bit positions of a group's launch mask):
enum {
    GJ_WK_NONE = 0,
    GJ_WK_STRIP_256 = 1,       // gj_window_strip_kernel<1, 32, 4, 2, 4>: n <= 256, sub-windows of 32
                               // (2, 3, 4: retired strip variants, LAB_NOTES.md "retired environment switches"; unused numbers)
    GJ_WK_STRIP_512 = 5,       // gj_window_strip_kernel<2, 16, 4, 2, 1>: 257 ... 512, the lean 4-wave form
    GJ_WK_STRIP_1024 = 6,      // gj_window_strip_kernel<2, 16, 8, 1, 2>: 513 ... 1024, 8 waves
    GJ_WK_LA_6 = 7,            // gj_window_la_kernel<16, 4, 6>
    GJ_WK_LA_12 = 8,           // gj_window_la_kernel<16, 8, 12>
    GJ_WK_TEAM = 9,            // gj_window_kernel<NBI, RPT>
    GJ_WK_SINGLE = 10,         // gj_blocked_kernel (one workgroup per matrix, no windows)
};
// further bits of a group's launch mask
enum {
    GJ_BIT_UPD4 = 1 << 12,     // gj_colupdate_kernel<4> (lean)
    GJ_BIT_UPD8 = 1 << 13,     // gj_colupdate_kernel<8> (fat)
    GJ_BIT_UPD2 = 1 << 14,     // gj_colupdate2_kernel (a pair of windows)
    GJ_BIT_GATHER = 1 << 15,   // gj_gather_kernel
};
// the thresholds of the rule; gj_params() is this process's set: these numbers, and stamps from NEGF_GJ_STAMPS
struct GjParams {
    int large_min = 209;             // n from which the windowed path serves every batch
    int small_win_min = 257;         // matrices from which 100 <= n < large_min goes windowed
    int strip_min = 64;              // matrices per group from which 257 <= n <= 512 takes the strip kernel
    int strip_max = 160;             // matrices per group up to which 513 <= n < strip_always takes it
    int strip_always = 900;          // n from which the <16,2> class always takes it
    long pair_min = 256;             // count * (nblk - 2) from which windows go in pairs
    long fat_max = 256;              // workgroups of an update launch up to which it is fat ...
    long fat_total_max = 2000;       // ... if nb * nblk does not exceed this
    int grp_max = 4;                 // stream groups (<= GjSideStreams::MAXG; 1 where the context has no side streams)
    int grp_min = 12;                // matrices per group
    int stamps = 0;                  // NEGF_GJ_STAMPS: time stamps of one workgroup (one group)
};
struct GjGroup {
    int first = 0, count = 0;        // matrices [first, first + count)
    int wk = GJ_WK_NONE;             // window kernel id
    int pairs = 0;                   // windows in pairs (gj_colupdate2_kernel; an odd last window on its own)
    int upd_full = 0;                // waves per column block (4 lean, 8 fat) of the update launches over all other blocks, 0: none
    int upd_single = 0;              // ... of the single-block launches of a pair, 0: none
    unsigned mask = 0;               // the launches of this group: 1 << wk | GJ_BIT_*
};
struct GjPlan {
    int path = 0;                    // 0 = no blocked kernel serves n (unblocked), 1 = single workgroup, 2 = windowed
    int nbi = 0, rpt = 0;            // windowed: the class (sub-panel width, rows per lane)
    int nblk = 0;                    // windowed: 64-column windows
    int groups = 0;
    GjGroup g[4];
    int gather = 0;                  // gj_gather_kernel runs
    int deferred = 0;                // the result stays un-gathered for launch_accumulate_perm
};
// per context: what the last inverse really launched (each launch site adds its bit)
struct GjRecord {
    int path = -1;                   // -1: no inverse yet
    int groups = 0;
    unsigned mask[4] = {};
};
const GjParams& gj_params();
// NEGF_OK / NEGF_EINVAL (n < 1, nb < 1, win_mode outside 0 ... 2); no HIP call
int gj_plan(int n, int nb, int win_mode, bool defer, const GjParams& p, GjPlan* out);

// A layered (block-tridiagonal) system of the recursive Green's function path: an object of its own inside the context
// (negf_layered_*; defined in negf_layered_impl.h)
struct LayeredSystem;

struct ProfEntry { double ms = 0; int launches = 0; double flops_alg = 0, flops_mfma = 0; };

// Flop accounting of the dense kernels, per kernel family (negf_profile_read_flops): the launchers add, for every
// launch, the ALGORITHMIC flops (8 per complex multiply-add: 8 M N K per product -- also for a Hermitian product,
// whose mirrored half the reference computes --, 8 n^3 per inverse) and the flops actually ISSUED to the
// matrix cores (3 real products per tile and k-step in the 3M form, 16-granular tiles, K padded to the staged
// K-tile, only the block tiles on and above the diagonal of a Hermitian product).  Per process, like the context
// not thread-safe; ProfScope attributes the difference across its lifetime to its family.
struct FlopCount { double alg = 0, mfma = 0; };
extern FlopCount g_negf_flops;
inline void negf_count_flops(double alg, double mfma) { g_negf_flops.alg += alg; g_negf_flops.mfma += mfma; }

struct negf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int n = 0;
    cplx* d_F = nullptr;           // the resident system: aliases of sys[sys_cur]
    cplx* d_S = nullptr;
    // the last NEGF_SYS_SLOTS systems handed to negf_set_system stay on the device (with a host copy to recognise
    // them by): front-ends that alternate between two systems -- the two spin blocks of a blockdiag(alpha, beta)
    // Fock matrix, scf.py:177-180 -- re-select instead of re-uploading
    struct SysSlot { cplx* dF = nullptr; cplx* dS = nullptr; std::vector<cplx> hF, hS; unsigned long long used = 0, key = 0; bool valid = false; };
    static constexpr int NEGF_SYS_SLOTS = 2;
    SysSlot sys[NEGF_SYS_SLOTS];
    int sys_cur = -1;
    unsigned long long sys_clock = 0;
    int batch_user = 0;            // 0 = auto
    int batch = 0;                 // allocated workspace batch
    bool transmission_seen = false; // negf_transmission[_dev] has run on this context: size the workspace for it
    // workspace, sized for `batch` energies
    cplx* d_A = nullptr;           // [batch][n*n]   assembled matrix -> inverse in place
    cplx* d_T1 = nullptr;          // [batch][n*n]   temp products
    cplx* d_T2 = nullptr;          // [batch][n*n]
    cplx* G = nullptr;             // where the last inverse left its result (d_A or d_T1)
    cplx* W1 = nullptr;            // the other of (d_A, d_T1): free work area after the inverse
    cplx* W2 = nullptr;            // = d_T2
    DevBuf<cplx> d_blk;            // [batch][blk_stride] contact blocks of Sigma(E)
    DevBuf<cplx> d_scratch;        // per-workgroup scratch of the Sigma kernels
    int* d_ipiv = nullptr;         // [batch][2][n] pivot bookkeeping of the large-matrix inverse
    int* d_info = nullptr;         // [m_cap]
    int* d_iters = nullptr;        // [m_cap][contacts]
    int* d_conv = nullptr;
    int m_cap = 0;
    int contacts_cap = 0;
    cplx* d_E = nullptr;           // staging for host-pointer API
    cplx* d_w = nullptr;
    std::vector<cplx> h_E;         // host copy of what stage_grid put into d_E (valid while h_E_valid): the g(E) cache
    bool h_E_valid = false;        //   keys on the energies without a device round trip
    // g(E) cache of the 1-D chain providers (negf_set_chain_cache)
    std::vector<ChainGEntry> gcache;
    int gcache_max = 512;          // entries (evaluated grids) kept, 0 = off
    size_t gcache_entry_bytes_max = (size_t)4 << 30;
    size_t gcache_bytes_max = (size_t)8 << 30;     // all entries together
    unsigned long long gcache_clock = 0, gcache_hits = 0, gcache_misses = 0;
    cplx* d_acc = nullptr;         // [n*n] result staging
    double* d_scal = nullptr;      // [m_cap][8] scalar outputs
    double* d_site = nullptr;      // [batch][n] per-site DOS staging
    bool gcache_pinned = false;    // a launch holds a pointer to one of the entries: allocation failures elsewhere must not drop the cache
    bool defer_gather = false;     // negf_gr_int: the weighted sum reads the reduced matrices through the permutation (set around run_assemble_inverse)
    bool G_deferred = false;       // ... and the last run_inverse did leave its result un-gathered in W1 (with d_ipiv)
    int inverse_algo = 0;
    int gamma_algo = 0;            // 0: compact Gamma products when the provider allows, 1: always dense
    DevBuf<cplx> d_gsmall;         // small Gamma matrices of a batch (compact path)
    DevBuf<cplx> d_seg_out;        // [segments][n*n] results of negf_gr_int_seg
    DevBuf<cplx> d_ref_P;          // [integrals][n*n] running values of negf_gr_int_refine
    unsigned char* d_ref_meta = nullptr;   // its level table: ratio | maxdp | maxbits [REF_MAX_LEVELS each] | first[REF_MAX_INTS + 1] | level[REF_MAX_INTS] | nanflag[REF_MAX_LEVELS]
    DevBuf<cplx> d_small_part;     // per-workgroup partial sums of the small fused kernel
    DevBuf<cplx> d_chan;           // eigenchannel work area: G[I_L, I_R], the products and H per energy, and L^H (negf_transmission_channels)
    DevBuf<int> d_chan_rank;       // rank of the pivoted Cholesky factor per energy
    DevBuf<double> d_chan_T;       // [m][nchan] staging of the host-pointer entry point
    DevBuf<cplx> d_chan_psi;       // [m][nchan][n] staging of negf_channel_states
    DevBuf<int> d_bond_map;        // local transmission: perm [n] | goff [ng + 1] of the call's orbital -> group map
    DevBuf<double> d_bond_carry;   // [n*n] running sum of the 32-energy chunk a batch boundary cuts (negf_bond_int)
    DevBuf<double> d_bond_T;       // [m][ng][ng] staging of the host-pointer entry point (negf_population / negf_projected_dos stage here too)
    DevBuf<cplx> d_pop_W;          // projected DOS: the vectors W [k][n] of the host-pointer entry point
    DevBuf<cplx> d_pop_Wt;         // ... and their transpose Wt [n][k], the second operand of Y = M Wt
    DevBuf<cplx> d_tmat_H;         // transmission matrix: [n*n] F (CONST: F + Sigma_tot) with the call's probe blocks added
    DevBuf<cplx> d_tmat_sig;       // the probes' Sigma blocks, concatenated
    DevBuf<cplx> d_tmat_gam;       // Gamma blocks: probes and CONST contacts once | [batch][sum K_c^2] of a block provider's contacts
    DevBuf<cplx> d_tmat_work;      // [batch][K_a K_b] G_ab of the pairs that take the gather / product / trace kernels
    DevBuf<int> d_tmat_tab;        // K | ioff | goff | gstride | soff [C each] | probe order [n_probes] | orbital lists | pair lists
    DevBuf<double> d_deph_T;       // floating probes: [batch][C*C] transmission matrices of the batch
    DevBuf<double> d_deph_R;       // [batch][P][n_c] responses of the batch (negf_gless_int_probes) / [m][P][n_c] staging of negf_probe_response
    DevBuf<double> d_deph_work;    // [energies in flight][P (P + n_c)] augmented matrices of the response kernel's global class
    DevBuf<cplx> d_deph_D;         // [batch][K_U^2] dephased coupling matrices on the union of the orbitals involved
    DevBuf<cplx> d_deph_carry;     // [n*n] running sum of the 32-energy chunk a batch boundary cuts (negf_gless_int_probes)
    DevBuf<int> d_deph_tab;        // the union U [K_U] | the terminals' orbital lists as positions in U | the terminals added, in order
    GjSideStreams gj_side;
    GjRecord gj_last;              // what the last run_inverse / rgf_inverse launched (negf_inverse_last)
    int chain_rr_quantum = -1, chain_rr_slots = 0;   // negf_set_chain_round_robin
    int small_algo = 0;            // 0: n <= 96 takes the fused single-kernel path, 1: never (negf_set_small_algo)
    int channel_algo = 0;          // layered channels: 0: K <= 96 takes the LDS kernels, 1: the wide kernels at every K (negf_set_channel_algo)
    // pinned host staging of the host-pointer entry points: [E | w] up, [result | info] down, ONE synchronisation
    // (the layout: PinLayout, negf_api.hip)
    unsigned char* h_pin = nullptr;
    size_t h_pin_cap = 0;
    int last_m = 0;
    bool profiling = false;
    std::map<std::string, ProfEntry> prof;
    struct Pending { std::string name; hipEvent_t e0, e1; };
    std::vector<Pending> prof_pending;
    std::vector<hipEvent_t> ev_pool;
    std::vector<SigmaProvider*> providers;
    std::vector<LayeredSystem*> layered;       // handles of negf_layered_create: a table that only grows, like providers
};

// Profiling bracket used by the orchestration code: two hipEvents recorded on the
// context's stream around a kernel family, WITHOUT any host synchronisation (the
// timed region of bench.py runs with this enabled); elapsed times are resolved when
// negf_profile_read is called.
struct ProfScope {
    negf_ctx* c; const char* name; hipEvent_t e0 = nullptr, e1 = nullptr;
    FlopCount f0;
    ProfScope(negf_ctx* ctx, const char* nm);
    ~ProfScope();
};

// ------------------------------------------------------------ kernel launchers
// (implemented in k_*.hip; all asynchronous on `st`)

// A[b] = E[b]*S - H - (dense Sigma_b) - scatter(blocks_b)
void launch_assemble(hipStream_t st, int n, int nb, const cplx* E, const cplx* S, const cplx* H,
                     const cplx* sig_dense /*[nb][n*n] or null*/,
                     const cplx* blk /*[nb][blk_stride] or null*/, int blk_stride,
                     int n_contacts, const int* d_nc /*device [n_contacts]*/,
                     const int* d_blk_off, const int* d_inds_off, const int* d_inds,
                     cplx* A);

// in-place inverse of nb matrices; info[b] = 0 or 1-based column of a zero pivot.  false: n exceeds what the
// kernel's LDS staging holds (nothing launched)
// stride: elements between consecutive matrices (0: n * n, the dense path's layout)
bool launch_inverse_unblocked(hipStream_t st, int n, int nb, cplx* A, int* info, size_t stride = 0);
// out-of-place ping-pong between A and B (both [nb][stride]); returns true when the
// inverses end up in B, false when in A
// win_mode: 0 = the measured choice of window kernel per size and batch, 1 = the strip window kernel (gj_strip.h)
// wherever it exists, 2 = the pre-strip kernels (negf_set_inverse_algo 3 / 4)
// skip_gather (in / out): in = the caller can read the reduced matrices through the pivot bookkeeping itself
// (G[i][j] = A[pivrow[i]][colof[j]], piv = [nb][2][n]); out = the gather was left out (windowed path only) -- the return
// value then still says "B", but B was not written
// rec: receives what was launched (reset first; path 0 when the return value is false)
bool launch_inverse_blocked(hipStream_t st, int n, int nb, cplx* A, cplx* B, size_t stride, int* piv, int* info,
                            GjSideStreams* side = nullptr, int win_mode = 0, bool* skip_gather = nullptr, GjRecord* rec = nullptr);
bool inverse_blocked_supported(int n);
// of the last launch_inverse_blocked: the part of its 6 n np^2 three-real-product flops that ran on the VECTOR pipe
// (the register-strip window kernels), i.e. was not issued to the matrix cores
double inverse_blocked_vector_flops();

// acc += sum_b w[b] * X[b]   (fixed summation order, deterministic); `part` is scratch of
// accumulate_scratch_elems(n2, nb) elements (<= nb * n2 / 32)
void launch_accumulate(hipStream_t st, int n2, int nb, const cplx* w, const cplx* X, cplx* acc, cplx* part);
// the same sum over matrices still in their reduced, un-gathered form: X[b][i][j] = W[b][pivrow_b[i]][colof_b[j]] (piv = [nb][2][n];
// a matrix with info[b] != 0 counts as NaN, as its gathered form would)
void launch_accumulate_perm(hipStream_t st, int n, int nb, const cplx* w, const cplx* W, const int* piv, const int* info, cplx* acc, cplx* part);
// launch_accumulate for the batch [m0, m0 + nb) of a grid of m energies (w, X indexed from the batch's first energy), bitwise
// independent of the batch cut: the chunks are the grid's; carry [n2] lives across the batches of one grid, part holds one
// record per chunk the batch touches (at most nb).  A grid in one batch is launch_accumulate itself.
void launch_accumulate_grid(hipStream_t st, int n2, int m, int m0, int nb, const cplx* w, const cplx* X, cplx* carry, cplx* part, cplx* acc);
bool launch_accumulate_ranges(hipStream_t st, int n, bool perm, const cplx* w, const cplx* XW, const int* piv, const int* info,
                              int nranges, const int* lo, const int* hi, const int* slot, cplx* out, cplx* part);
// nested refinement on the device (density.py:239-268): see refine_levels_kernel
constexpr int REF_MAX_LEVELS = 2048, REF_MAX_INTS = 64, REF_MAX_N = 512;
void launch_refine_levels(hipStream_t st, int n2, int nint, const cplx* sums, const int* first, const double* ratio, double tol,
                          cplx* P, int* level_out, double* maxdp_out);
void launch_refine_level_wide(hipStream_t st, int n2, const cplx* inc, double ratio, cplx* Pk, int level_idx, double tol,
                              int* conv, unsigned long long* maxbits, int* nanflag, double* maxdp_slot);
void launch_cadd(hipStream_t st, size_t count, const cplx* a, const cplx* b, cplx* out);
size_t accumulate_scratch_elems(int n2, int nb);

// C[b] (M x N) = A[b] (M x K) * op(B[b]);  a batch stride of 0 broadcasts one matrix.
// opB bit 1 (value 1): op(B) = B^H with B stored N x K (ldb >= K), else B is K x N (ldb >= N); bit 2 (value 2): the
// caller states that the (square) product is Hermitian -- block tiles above the diagonal are computed and mirrored, those
// below skipped; bit 4 (value 4): the result is stored conjugate-transposed, C = (A op(B))^H (N x M; not with bit 2).
void launch_zgemm(hipStream_t st, int M, int N, int K, int nb,
                  const cplx* A, int lda, size_t strideA,
                  const cplx* B, int ldb, size_t strideB, int opB,
                  cplx* C, int ldc, size_t strideC);
// the same with the kernel and the Hermitian switch chosen by the caller instead of the rule and the environment
// (negf_zgemm_batched); zgemm_plan: what such a launch does with a shape, computed on the host (negf_zgemm_plan)
enum { ZGEMM_AUTO = 0, ZGEMM_MFMA = 1, ZGEMM_FLEX = 2, ZGEMM_VALU = 3 };
void launch_zgemm_as(hipStream_t st, int kernel, bool herm_on, int M, int N, int K, int nb,
                     const cplx* A, int lda, size_t strideA,
                     const cplx* B, int ldb, size_t strideB, int opB,
                     cplx* C, int ldc, size_t strideC);
int zgemm_plan(int M, int N, int K, int opB, int nb, int kernel, int* kernel_used, int* opB_eff, int* blocks, int* grid,
               int* decode, int decode_cap);

// out[b*out_stride] = Re sum_{i<nr, j<ncol} X[b][i*ldx+j] * conj(G[b][i*ldg+j])
void launch_trace_dot(hipStream_t st, int nr, int ncol, int nb, const cplx* X, int ldx,
                      size_t strideX, const cplx* G, int ldg, size_t strideG,
                      double* out, int out_stride);

// dos_site[b][i] = -Im G[b]_ii / pi ; dos_tot[b] = sum_i
void launch_dos(hipStream_t st, int n, int nb, const cplx* G, double* dos_tot, double* dos_site);

// Gamma = i (Sigma - Sigma^H) for nb dense matrices (stride 0 allowed on input)
void launch_gamma_dense(hipStream_t st, int n, int nb, const cplx* sig, size_t stride_sig, cplx* gam);
void launch_gamma_small(hipStream_t st, int K, int c0, int c1, int nb, const int* d_nc, const int* d_blk_off,
                        const int* d_inds_off, const cplx* blk, size_t blk_stride, cplx* out, size_t out_stride);
void launch_gather_block(hipStream_t st, int n, int nr, int nc, int nb, const cplx* G, size_t strideG,
                         const int* ridx, const int* cidx, cplx* out, size_t out_stride);

// dense Sigma from contact blocks: out[b] = scatter-add of selected contacts (contact<0: all)
void launch_scatter_blocks(hipStream_t st, int n, int nb, const cplx* blk, int blk_stride,
                           int n_contacts, const int* d_nc, const int* d_blk_off,
                           const int* d_inds_off, const int* d_inds, int contact, cplx* out);

// 1-D chain decimation: one workgroup per (energy, contact)
void launch_chain1d(hipStream_t st, const SigmaProvider& p, const int* d_nc, const int* d_blk_off,
                    int nb, const cplx* E, cplx* blk, int* iters, int* conv, cplx* scratch,
                    size_t scratch_per_wg);
size_t chain1d_scratch_per_wg(int nc_max);
// register-stationary MFMA version for n_c <= 64 (k_chain1d_rs.hip)
bool chain1d_lds_supported(int nc_max);
// gold_scratch: chain1d_lds_scratch_elems() complex values of lane-private scratch (may be null:
// the kernel then keeps the old iterate in LDS at a lower occupancy)
// (+ the job queue of a round-robin launch: rr_quantum < 0 = the default, 100 sweeps)
size_t chain1d_lds_scratch_elems(int nc_max, int n_contacts, int nb, int max_sweeps, int rr_quantum);
// does a launch of nb energies that runs its fixed points (no cache hit, scratch given) run round robin: more jobs than
// resident slots, and a quantum below its sweep cap?  Such a launch needs no order (rr_quantum / rr_slots as below)
bool chain1d_lds_runs_queue(const SigmaProvider& p, int nb, int rr_quantum, int rr_slots);
// order: launch slot -> job (energy * n_contacts + contact) or null for launch order
// gcache / gc_mode: see ChainGEntry -- 0 no cache, 1 store the final iterates, 2 load them and only form Sigma
// rr_quantum / rr_slots: round-robin execution of a launch with more jobs than resident slots (ChainRsArgs; < 0 / 0:
// the defaults -- 100 sweeps, every slot of the device; rr_quantum 0: never)
void launch_chain1d_lds(hipStream_t st, const SigmaProvider& p, const int* d_nc, const int* d_blk_off, int nb,
                        const cplx* E, cplx* blk, int* iters, int* conv, cplx* gold_scratch, const int* order,
                        cplx* gcache = nullptr, int gc_mode = 0, int rr_quantum = -1, int rr_slots = 0);
// renormalisation-decimation solver (k_chain1d_rd.hip; p.conv = tol, p.max_iter = max_steps, p.force_iters = force_steps).
// scratch: chain1d_rd_scratch_elems() complex values; gcache / gc_mode as in launch_chain1d_lds (n_c <= 64 only)
size_t chain1d_rd_scratch_elems(int nc_max, int n_contacts, int nb);
void launch_chain1d_rd(hipStream_t st, const SigmaProvider& p, const int* d_nc, const int* d_blk_off, int nb,
                       const cplx* E, cplx* blk, int* iters, int* conv, cplx* scratch, cplx* gcache, int gc_mode);
// order[0..count) = jobs by decreasing sweep count predicted from the previous evaluation (k_chain1d_order.hip)
bool chain1d_order_supported(int count);
void launch_chain1d_predict_order(hipStream_t st, const cplx* prevE, const int* prev_iters, int prev_n, int n_contacts,
                                  const cplx* E, int nb, int* order);

// Bethe lattice: one workgroup per (energy, contact); writes per-atom 9x9 blocks
void launch_bethe(hipStream_t st, const SigmaProvider& p, int nb, const cplx* E, cplx* blk,
                  int* iters, int* conv);

void launch_bethe_raw(hipStream_t st, const double* d_H, const double* d_S, const double* d_V, double eta,
                      double conv, double mix, int max_iter, int force_iters, int which, int nb,
                      const cplx* E, cplx* out, int* iters, int* converged);

int run_mfma_selftest(hipStream_t st, double* max_err);

// Small systems (n <= 96): assemble + invert (+ accumulate) in one kernel, k_small_fused.hip
struct SmallFusedArgs {
    int n = 0, m = 0, gp = 0;
    const cplx* E = nullptr;          // [m]
    const cplx* w = nullptr;          // [m]   (accumulate mode)
    const cplx* S = nullptr;          // [n*n]
    const cplx* H = nullptr;          // [n*n]  F, or F + Sigma_tot of a constant provider
    const cplx* sig_dense = nullptr;  // [m][sig_stride] dense Sigma per energy, or null
    size_t sig_stride = 0;
    const cplx* blk = nullptr;        // [m][blk_stride] contact blocks of Sigma(E), or null (then n_contacts = 0)
    int blk_stride = 0, n_contacts = 0;
    const int* pos = nullptr;         // [n_contacts][n] position of an orbital in the contact's index list, -1 outside
    const int* nc = nullptr;          // [n_contacts]
    const int* blk_off = nullptr;     // [n_contacts]
    cplx* partial = nullptr;          // [small_fused_grid(n, m)][n*n] scratch (accumulate mode)
    cplx* out = nullptr;              // [n*n] sum_m w_m G(E_m)   (accumulate mode)
    cplx* Gout = nullptr;             // non-null: STORE mode, G(E_m) -> Gout + m * g_stride
    size_t g_stride = 0;
    int* info = nullptr;              // [m]
    int nseg = 0;                     // > 0: the energies are nseg consecutive segments ending at seg_end[s] (HOST array);
    const int* seg_end = nullptr;     //      out holds one n x n sum per segment
};
// Eigenchannels (k_channels.hip): one workgroup per matrix, K <= channels_kmax().
// Eigenvalues of the Hermitian matrices in the lower triangles of A[b] (their leading rank[b] x rank[b] blocks when
// rank is non-null; rank[b * rank_stride], 0 = one rank for all), sorted ascending or descending into w[b * ldw + 0 .. nout), exact zeros at positions >= rank[b].
// info[b]: chk_in -> a nonzero info[b] on entry yields a NaN row and is kept; else flag_sign * (0 converged,
// 1 non-finite input -> NaN row, 2 not converged within the sweep limit).  false: K out of range (nothing launched).
int channels_kmax();
bool launch_eigvalsh_batched(hipStream_t st, int K, int nb, const cplx* A, int lda, size_t strideA, const int* rank,
                             int rank_stride, double* w, int ldw, int nout, bool descending, int* info, bool chk_in, int flag_sign);
// The same solver with the rotations accumulated, X = X0 J_1 J_2 ... (K rows; the eigenvalues are bitwise those of
// launch_eigvalsh_batched).  x0 (null: the identity, X = the eigenvectors): element (i, j) of X0, i < K, j < rank, at
// x0[b * x0_stride + i * x0_ri + j * x0_cj], conjugated when x0_conj (L is read out of a stored L^H that way).
// out: column `pos` of the sorted result (the position its eigenvalue is written at) goes to out[b * out_stride +
// i * out_ri + pos * out_cj], conjugated when out_conj, for pos < ncol; columns rank <= pos < ncol are zeros, and a NaN
// row of w comes with NaN in all ncol of them.  xg: nb * eigh_scratch_elems(K) values of scratch (none for the K
// whose X fits in LDS).  rows, xg_stride: set by the launcher.
struct JacVec {
    const cplx* x0; size_t x0_stride; int x0_ri, x0_cj, x0_conj;
    cplx* xg; size_t xg_stride;
    cplx* out; size_t out_stride; int out_ri, out_cj, out_conj;
    int rows, ncol;
};
size_t eigh_scratch_elems(int K);
bool launch_eigh_batched(hipStream_t st, int K, int nb, const cplx* A, int lda, size_t strideA, const int* rank,
                         int rank_stride, double* w, int ldw, int nout, bool descending, int* info, bool chk_in, int flag_sign,
                         JacVec vec);
// psi[b][c][0..n), c < nchan, from Pc[b * strideP + c * n + i] = conj(psi_c[i]) (c < nce): phase fixed so that the
// component of largest modulus is real positive (lowest index on ties); zeros for c >= min(rank, nce), NaN where
// info[b] is neither 0 nor -2
void launch_channel_gauge(hipStream_t st, int n, int nce, int nchan, int nb, const cplx* Pc, size_t strideP, const int* rank,
                          int rank_stride, const int* info, cplx* psi);
// Pivoted Cholesky of the Hermitian PSD K x K matrices G[b]: Lh[b] = L^H (K x K, rows >= rank[b] zero), G ~ L L^H
bool launch_pivoted_cholesky(hipStream_t st, int K, int nb, const cplx* G, size_t strideG, cplx* Lh, size_t strideL,
                             int* rank);
// The wide forms (k_eig_wide.hip), K <= eig_wide_kmax() = 512: the same contracts -- launch_pivoted_cholesky_wide writes
// launch_pivoted_cholesky's L^H and rank, launch_eigvalsh_wide launch_eigvalsh_batched's values (its flag 2 does not
// occur) -- with the matrix in global memory: `work` holds nb * eig_wide_work_elems(K) values, private to the launch.
int eig_wide_kmax();
size_t eig_wide_work_elems(int K);
bool launch_eigvalsh_wide(hipStream_t st, int K, int nb, const cplx* A, int lda, size_t strideA, const int* rank,
                          int rank_stride, double* w, int ldw, int nout, bool descending, int* info, bool chk_in, int flag_sign,
                          cplx* work);
bool launch_pivoted_cholesky_wide(hipStream_t st, int K, int nb, const cplx* G, size_t strideG, cplx* Lh, size_t strideL,
                                  int* rank);

// Local (bond) transmission (k_bond.hip): flow[i][j] = 2 Im[(E S - F)_ij conj(A_ij)] from the Hermitian A = G Gamma_c G^H.
// launch_bond_tables: per-energy tables out [nb][ng][ng]; perm / goff (device, [n] / [ng + 1]) = the orbitals sorted by
// group and the groups' offsets, perm == null: every orbital its own group (ng = n).  info[b] != 0 -> a NaN table.
// false: n exceeds bond_max_n() (nothing launched).
int bond_max_n();
bool launch_bond_tables(hipStream_t st, int n, int nb, const cplx* E, const cplx* S, const cplx* F, const cplx* A,
                        const int* info, int ng, const int* perm, const int* goff, double* out);
// out [n2] += sum_b w[b] flow_b for the batch [m0, m0 + nb) of a grid of m energies (E, w, A indexed from the batch's
// first energy), bitwise independent of the batch cut; carry [n2] lives across the batches of one grid, part is
// scratch of bond_int_scratch_doubles(n2, nb) doubles (<= 2 nb n2)
size_t bond_int_scratch_doubles(int n2, int nb);
void launch_bond_int(hipStream_t st, int n2, int m, int m0, int nb, const cplx* E, const double* w, const cplx* S,
                     const cplx* F, const cplx* A, double* carry, double* part, double* out);

// Overlap / Hamilton populations and projected DOS (k_population.hip).  M = G (retarded: -(1/pi) Im[M_ij conj(X_ij)]) or
// the Hermitian A_c = G Gamma_c G^H (contact: (1/2 pi) Re[M_ij conj(X_ij)]), X = S or F.
// launch_population: out [nb][ng][ng] (rows_only = 0) or [nb][ng] (rows_only = 1: the sums of the table's rows, in one pass,
// the table never stored); perm / goff as in launch_bond_tables (null: every orbital its own group, ng = n).
// info[b] != 0 -> NaN.  false: n exceeds bond_max_n(), or the LDS of the row kernel could not be had (nothing launched).
bool launch_population(hipStream_t st, int n, int nb, bool retarded, const cplx* X, const cplx* M, const int* info,
                       int rows_only, int ng, const int* perm, const int* goff, double* out);
// Wt [n][k] = the transpose of W [k][n];  out[b][a] = factor * Im / Re [sum_i conj(Wt[i][a]) Y[b][i][a]], Y [nb][n][k] = M Wt
void launch_pop_transpose_w(hipStream_t st, int n, int k, const cplx* W, cplx* Wt);
void launch_pop_coldot(hipStream_t st, int n, int k, int nb, bool retarded, const cplx* Wt, const cplx* Y, size_t strideY,
                       const int* info, double* out);

// Multi-terminal transmission matrix (k_tmatrix.hip).  Terminal tables on the device, C entries each: tK = block size,
// ioff = start of the orbital list in idx, goff / gstride = where Gamma_t of energy b sits in gam (gam + b * gstride[t] +
// goff[t]; gstride 0: one block for all energies), soff = where Sigma_t sits in the source of launch_tmat_gamma.
constexpr int TMAT_SMALL_K = 15, TMAT_TINY_ELEMS = 128, TMAT_LDS_ELEMS = 1536, TMAT_MAX_TERMINALS = 1024;
// Gamma_t = i (Sigma_t - Sigma_t^H) for the terminals [t0, t0 + nt) and nb energies (src_stride 0, nb 1: constant blocks)
void launch_tmat_gamma(hipStream_t st, int t0, int nt, int nb, const int* tK, const int* soff, const int* goff,
                       const int* gstride, const cplx* src, size_t src_stride, cplx* dst);
// H[I_p, I_p] += Sigma_p for the probes order[0 .. n_probes) (terminal numbers), one after the other
void launch_tmat_add_probes(hipStream_t st, int n, int n_probes, const int* order, const int* tK, const int* ioff,
                            const int* soff, const int* idx, const cplx* sig, cplx* H);
// 0: the pair (K_a, K_b) takes the gather / product / trace kernels, 1 / 2: launch_tmat_pairs with 64 / 256 threads
int tmat_pair_class(int Ka, int Kb);
// T[b][a][b'] for the pairs (a * C + b') of one class and nb energies; max_elems >= K_a K_b of every pair listed
void launch_tmat_pairs(hipStream_t st, int cls, int n, int C, int npairs, int max_elems, int nb, const int* pairs,
                       const int* tK, const int* ioff, const int* goff, const int* gstride, const int* idx, const cplx* G,
                       const cplx* gam, double* T);
// T[b][..] = NaN where info[b] != 0
void launch_tmat_nan(hipStream_t st, int C, int nb, const int* info, double* T);

// Floating dephasing probes (k_dephase.hip).  The response kernel keeps its augmented matrix [W | rhs] in LDS for
// P <= DEPH_LDS_MAX_P probes and n_c <= DEPH_LDS_MAX_RHS contacts (80 x 96 doubles = 60 KiB), otherwise in `work`
// (deph_response_work_doubles per energy).  order [P]: the probes' terminal indices in content order.
constexpr int DEPH_LDS_MAX_P = 80, DEPH_LDS_MAX_RHS = 16;
constexpr size_t DEPH_WORK_BYTES = (size_t)256 << 20;      // the global class' work area: energies go through in chunks that fit
bool deph_response_in_lds(int P, int nc);
size_t deph_response_work_doubles(int P, int nc);
// T [nb][C][C] -> R [nb][P][nc]; an energy whose T holds a non-finite entry gives a NaN R
void launch_deph_response(hipStream_t st, int C, int nc, int nb, const int* order, const double* T, double* work, double* R);
// D[b] [KU][KU] = sum over the terminals list[0 .. nlist), in that order, of weight * Gamma_t scattered through pos (the
// terminal's orbital list as positions in U, at ioff[t]); weight = 1 for col < 0 and for contacts, R[b][t - nc][col] for probes
void launch_deph_coupling(hipStream_t st, int KU, int nc, int P, int col, int nlist, int nb, const int* list, const int* tK,
                          const int* ioff, const int* goff, const int* gstride, const int* pos, const cplx* gam,
                          const double* R, cplx* D, size_t strideD);

// Recursive Green's function passes (k_rgf.hip).  Matrices of a batch are compact row-major at the batch stride given.
constexpr int RGF_MAX_TERM = 8;                 // terminals on one end layer
// the terminals scattered into an end layer: pos[k] [n] = position of a layer orbital in terminal k's list (-1 outside),
// sig[k] + b * stride[k] = its K[k] x K[k] block at energy b (stride 0: one block for all energies)
struct RgfTermArgs { int count = 0; const int* pos[RGF_MAX_TERM]; const cplx* sig[RGF_MAX_TERM]; size_t stride[RGF_MAX_TERM]; int K[RGF_MAX_TERM]; };
// D[b] = E_b S - F - P[b] - sum_k scatter(Sigma_k,b)   (n x n; P null: no Schur term)
void launch_rgf_diag(hipStream_t st, int n, int nb, const cplx* E, const cplx* S, const cplx* F, const cplx* P,
                     size_t strideP, const RgfTermArgs& t, cplx* D, size_t strideD);
// C[b] = F - E_b S over `count` elements: the negated coupling block
void launch_rgf_coupling(hipStream_t st, int count, int nb, const cplx* E, const cplx* S, const cplx* F, cplx* C,
                         size_t strideC);
// G[b] = g[b] + W[b]
void launch_rgf_add(hipStream_t st, int count, int nb, const cplx* g, size_t strideg, const cplx* W, size_t strideW,
                    cplx* G, size_t strideG);
// out[b] = i (sig[b] - sig[b]^H), K x K
void launch_rgf_gamma(hipStream_t st, int K, int nb, const cplx* sig, size_t stride_sig, cplx* out, size_t stride_out);
// site[b * site_stride + r] = -Im G[b][r][r] / pi
void launch_rgf_dos_diag(hipStream_t st, int n, int nb, const cplx* G, size_t strideG, double* site, size_t site_stride);
// site[b * site_stride + r] (+)= -Im sum_k G[b][r][k] conj(X[r][k]) / pi   (G, X nr x nk)
void launch_rgf_dos_rows(hipStream_t st, int nr, int nk, int nb, const cplx* G, size_t strideG, const cplx* X,
                         double* site, size_t site_stride, bool accumulate);
void launch_rgf_dos_total(hipStream_t st, int N, int nb, const double* site, size_t site_stride, double* tot);
// acc[i] += sum_b w[b] X[b][i], one chain per element with b ascending
void launch_rgf_accumulate(hipStream_t st, int count, int nb, const cplx* w, const cplx* X, size_t strideX, cplx* acc);
// G Gamma G^H on the pattern of S (negf_layered_gless_int, negf_layered_contact_dos):
// out[b][r][a] = G[b][r][idx[a]]   (G n x n, out n x K compact)
void launch_rgf_gather_cols(hipStream_t st, int n, int K, int nb, const cplx* G, size_t strideG, const int* idx, cplx* out,
                            size_t stride_out);
// out[b] (KJ x KJ) = sum_k of i (Sigma_k - Sigma_k^H) scattered into the union list J (layer orbitals, ascending), k in
// the order of `t`
void launch_rgf_gamma_union(hipStream_t st, int KJ, int nb, const int* J, const RgfTermArgs& t, cplx* out, size_t stride_out);
// acc[c][r] += sum_b w[b] conj(X[b][r][c])   (X nr x nc, acc nc x nr), one chain per element with b ascending
void launch_rgf_accumulate_ct(hipStream_t st, int nr, int nc, int nb, const cplx* w, const cplx* X, size_t strideX, cplx* acc);
// row_site[b * site_stride + r] (+)= sum_k Re[A[b][r][k] conj(X[r][k])] / 2 pi, and, col_site given,
// col_site[b * site_stride + k] += sum_r of the same terms   (A, X nr x nk)
void launch_rgf_pop_block(hipStream_t st, int nr, int nk, int nb, const cplx* A, size_t strideA, const cplx* X,
                          double* row_site, bool accumulate_rows, double* col_site, size_t site_stride);
void launch_rgf_merge_info(hipStream_t st, int nb, int offset, const int* linfo, int* info);
// Bond currents and local transmission on the pattern of S (negf_layered_local_transmission, negf_layered_bond_int):
// flow = 2 Im[(E_b S - F) conj(A[b])] element by element; info[b] != 0 -> NaN.
// out[b * stride_out + i] = flow over `count` elements (a diagonal or an upper block)
void launch_rgf_bond_flow(hipStream_t st, int count, int nb, const cplx* E, const cplx* S, const cplx* F, const cplx* A,
                          size_t strideA, const int* info, double* out, size_t stride_out);
// the lower block from the upper A (nr x nc): out[b][c][r] = 2 Im[(E_b Sl - Fl)[c][r] A[b][r][c]]   (Sl, Fl, out nc x nr)
void launch_rgf_bond_flow_t(hipStream_t st, int nr, int nc, int nb, const cplx* E, const cplx* Sl, const cplx* Fl,
                            const cplx* A, size_t strideA, const int* info, double* out, size_t stride_out);
// group table of a block with nc columns: rperm / rgoff, cperm / cgoff = the orbitals of its row / column layer sorted by
// group and the groups' offsets (device).  lower false: out[b][a][g] (ngr x ngc) of the block (S, F, A) itself; true: S, F,
// A are the UPPER block and out[b][g][a] (ngc x ngr) is the lower block's table
void launch_rgf_bond_group(hipStream_t st, int nc, int ngr, int ngc, int nb, bool lower, const cplx* E, const cplx* S,
                           const cplx* F, const cplx* A, size_t strideA, const int* info, const int* rperm, const int* rgoff,
                           const int* cperm, const int* cgoff, double* out, size_t stride_out);
// A[b] = (A[b] + A[b]^H) / 2 in place (n x n): elements (r, c) and (c, r) leave as exact conjugates
void launch_rgf_bond_hermitize(hipStream_t st, int n, int nb, cplx* A, size_t strideA);
// acc[i] += sum_b w[b] flow_b[i] with real w, one chain per element with b ascending; _t: the lower block from the upper A
void launch_rgf_bond_accumulate(hipStream_t st, int count, int nb, const cplx* E, const double* w, const cplx* S,
                                const cplx* F, const cplx* A, size_t strideA, double* acc);
void launch_rgf_bond_accumulate_t(hipStream_t st, int nr, int nc, int nb, const cplx* E, const double* w, const cplx* Sl,
                                  const cplx* Fl, const cplx* A, size_t strideA, double* acc);
// Transmission matrix with probes on any layer (negf_layered_transmission_matrix):
// the columns idx of G into the first K columns of a strip of width ld (out[b][r * ld + a] = G[b][r][idx[a]])
void launch_rgf_strip_head(hipStream_t st, int n, int K, int ld, int nb, const cplx* G, size_t strideG, const int* idx,
                           cplx* out, size_t stride_out);
// D[b][I_p, I_p] -= Sigma_p for the probes order[0 .. n_probes) of one layer, one after the other (tables as k_tmatrix's,
// rows = the orbitals counted inside the layer)
void launch_rgf_sub_probes(hipStream_t st, int n, int n_probes, int nb, const int* order, const int* tK, const int* ioff,
                           const int* soff, const int* rows, const cplx* sig, cplx* D, size_t strideD);
// T[b][a][b'] for the pairs (a * C + b') of one layer level and one class (tmat_pair_class 1 / 2) from the level's column
// strip (n_i x ld at strideS): row rows[ioff[a] + i], column tcol[b'] - col0 + cpos[ioff[b'] + j]; max_elems >= K_a K_b
void launch_rgf_strip_pairs(hipStream_t st, int cls, int C, int npairs, int max_elems, int nb, const int* pairs,
                            const int* tK, const int* ioff, const int* goff, const int* gstride, const int* tcol, int col0,
                            const int* rows, const int* cpos, const cplx* strip, int ld, size_t strideS, const cplx* gstat,
                            const cplx* gdyn, double* T);
// Floating probes on a layered device (k_rgf_deph.hip; negf_layered_gless_int_probes).  D[b] = the blocks D_q (nJ[q] x nJ[q]
// at Doff[q]) of the dephased coupling, one workgroup per (layer, energy): the end terminals sel[0 .. nsel) that sit on the
// layer, then its probes porder[poff[q] .. poff[q + 1]) weighted with R[b][p][col] (col < 0: every weight 1), through cpos
void launch_rgf_deph_coupling(hipStream_t st, int L, int nb, int nt, int P, int col, int nsel, const int* sel,
                              const int* tlayer, const int* porder, const int* poff, const int* nJ, const int* Doff,
                              const int* tK, const int* ioff, const int* goff, const int* gstride, const int* cpos,
                              const cplx* gstat, const cplx* gdyn, const double* R, cplx* D, size_t strideD);
// Y_i[b] = Cfull_i[b] blockdiag(D_q[b]) for all layers, column blocks and energies in one launch; Cfull and Y [L][nb_max][cs],
// n_i x Ktot each; ctile [nct][2]: (q, first column inside J_q) of every column tile (rgf_blockdiag_tile_cols() wide)
int rgf_blockdiag_row_tiles(int nmax);
int rgf_blockdiag_col_tiles(int KJ);
int rgf_blockdiag_tile_cols();
void launch_rgf_blockdiag_mm(hipStream_t st, int L, int nmax, int nct, int Ktot, int nb, int nb_max, size_t cs,
                             const int* nl, const int* nJ, const int* Joff, const int* Doff, const int* ctile,
                             const cplx* Cfull, const cplx* D, size_t strideD, cplx* Y);

bool small_fused_supported(int n);
int small_fused_grid(int n, int m);
void launch_small_fused(hipStream_t st, SmallFusedArgs a);
