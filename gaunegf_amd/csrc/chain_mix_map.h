// Lane map of the mixing step of the 1-D chain fixed-point kernel (k_chain1d_rs.hip, gather_mix): which element of the
// n x n iterate a lane of the 256-thread workgroup holds in which slot.  Pure index arithmetic, host and device
// (tests/test_chain_mix_map_host.py compiles it with the host compiler and checks it exhaustively).
//
// The phase reads g_new from LDS through the pivot tables and writes g back after a barrier, so its layout is free of
// the tiles the waves own.  Dense map: with RG = floor(256 / n) row groups (at most 64), lane t < RG n holds column
// c = t mod n of the rows rg + RG s, rg = floor(t / n), s = 0 .. ceil(n / RG) - 1.  Element (row, c) is then the
// linear index row n + c = s RG n + t of the compact row-major matrix: slot s of lane t is element s RG n + t, valid
// while that is < n n.  Lanes t >= RG n hold nothing.  Only the last slot has rows >= n.
//
// Where the old iterate lives, slot by slot: slot s < lds_slots at [s][t] (256 lanes per slot) in the spare rows of the
// work matrix, the others at [s][t] of the workgroup's global scratch record, which reserves rs_mix_reserved_slots
// slots per lane.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RS_MIX_HD __host__ __device__
#else
#define RS_MIX_HD
#endif

constexpr int RS_MIX_LANES = 256;

struct RsMixMap {
    int n;           // matrix size, 1 .. 64
    int rg;          // row groups
    int slots;       // slots per lane
    int stride;      // rg * n: lanes that hold elements = linear-index distance of two slots
    unsigned rcp;    // floor(t / n) == (t * rcp) >> 16 for t < 256
};

RS_MIX_HD constexpr RsMixMap rs_mix_map(int n)
{
    const int rg = RS_MIX_LANES / n < 64 ? RS_MIX_LANES / n : 64;
    return RsMixMap{n, rg, (n + rg - 1) / rg, rg * n, (65536u + (unsigned)n - 1u) / (unsigned)n};
}
RS_MIX_HD constexpr int rs_mix_row_group(const RsMixMap& m, int t) { return (int)(((unsigned)t * m.rcp) >> 16); }
RS_MIX_HD constexpr int rs_mix_col(const RsMixMap& m, int t) { return t - rs_mix_row_group(m, t) * m.n; }
RS_MIX_HD constexpr bool rs_mix_active(const RsMixMap& m, int t) { return rs_mix_row_group(m, t) < m.rg; }
RS_MIX_HD constexpr int rs_mix_row(const RsMixMap& m, int t, int s) { return rs_mix_row_group(m, t) + m.rg * s; }
RS_MIX_HD constexpr bool rs_mix_valid(const RsMixMap& m, int t, int s) { return rs_mix_active(m, t) && rs_mix_row(m, t, s) < m.n; }

// pitch-class quantities of the kernel (template parameter P: the odd pitch of the work matrix, n <= P - 1 or, in the
// classes with a remainder strip, n <= P)
RS_MIX_HD constexpr int rs_class_tiles(int P) { return (P - 1 + 15) / 16; }
RS_MIX_HD constexpr int rs_class_ksteps(int P) { return (P + 3) / 4 < 4 * rs_class_tiles(P) ? (P + 3) / 4 : 4 * rs_class_tiles(P); }
RS_MIX_HD constexpr int rs_class_welems(int P) { return 16 * rs_class_tiles(P) * P + 16; }
RS_MIX_HD constexpr int rs_class_nmax(int P) { return P < 16 * rs_class_tiles(P) ? P : 16 * rs_class_tiles(P); }
// spare elements of the work matrix behind row n_max + 1, at least (any n_max <= P)
RS_MIX_HD constexpr int rs_class_spare(int P) { return rs_class_welems(P) - (P + 2) * P > 0 ? rs_class_welems(P) - (P + 2) * P : 0; }
// whole slots of 256 lanes that fit the spare rows: the LDS slots of the kernels that keep the rest in global scratch
RS_MIX_HD constexpr int rs_class_lds_slots(int P) { return rs_class_spare(P) / RS_MIX_LANES; }
RS_MIX_HD constexpr int rs_mix_lds_slots(const RsMixMap& m, int P) { return rs_class_lds_slots(P) < m.slots ? rs_class_lds_slots(P) : m.slots; }
RS_MIX_HD constexpr int rs_mix_global_slots(const RsMixMap& m, int P) { return m.slots - rs_mix_lds_slots(m, P); }
// slots per lane the global scratch record reserves (rs_gold_elems)
RS_MIX_HD constexpr int rs_mix_reserved_slots(int nc_max) { return 4 * ((nc_max + 15) >> 4); }
// most / fewest slots of any n in [n_lo, n_hi]
RS_MIX_HD constexpr int rs_mix_max_slots(int n_lo, int n_hi)
{
    int v = 0;
    for (int n = n_lo; n <= n_hi; ++n) v = rs_mix_map(n).slots > v ? rs_mix_map(n).slots : v;
    return v;
}
RS_MIX_HD constexpr int rs_mix_min_slots(int n_lo, int n_hi)
{
    int v = 1 << 20;
    for (int n = n_lo; n <= n_hi; ++n) v = rs_mix_map(n).slots < v ? rs_mix_map(n).slots : v;
    return v;
}
