// The compile-time stage schedule of the small inverse (chain_rs_inverse.h, rs_inverse_sched) in a remainder-strip
// class: TR full 16 x 16 tiles per dimension and a strip of 1 .. 4 rows / columns behind them, panels of 8, the
// factoring wave fixed (role 3).  Every contact of such a launch has 16 TR < n <= 16 TR + 4, so stage sgi < 2 TR
// applies a panel that is exactly 8 wide and lies inside a full tile, and stage 2 TR the narrow last one.
//
// Pure index arithmetic without device code: the kernel includes it, tests/chain_rs_sched_check.cpp prints it, and
// tests/test_chain_rs_sched_host.py compares that with the tile walk of the generic loop (rs_inverse).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RS_SCHED_HD __host__ __device__
#else
#define RS_SCHED_HD
#endif

// kinds of a column-tile job of the trailing update
constexpr unsigned RS_JOB_NONE = 0;      // (no job)
constexpr unsigned RS_JOB_WHOLE = 1;     // a whole full tile: 16 columns, 16 x 16 x 4 instruction
constexpr unsigned RS_JOB_HALF = 2;      // 8 columns of a full tile: two 16 x 4 column strips per row tile
constexpr unsigned RS_JOB_STRIP = 3;     // the column strip, tile TR
// a job in 5 bits: kind | tile << 2 | (upper half of the tile) << 4;  a role's two jobs of a stage in 10 bits (first job
// low; a role owns jobs role and role + 3 of the walk, and no stage has more than TR + 1 <= 4 jobs);  a role's stages
// 0 .. 2 TR - 1 in one 64-bit word, stage sgi at bit 10 sgi (TR <= 3: 60 bits)
constexpr int RS_JOB_BITS = 5, RS_STAGE_BITS = 10;
constexpr int RS_SCHED_TEAM = 3;         // the three roles that do not factor share the jobs of a stage

// job idx (in the order of the generic loop's walk over the column tiles) of stage sgi, 0 <= sgi < 2 TR.
//   even stage (the panel is the lower half of tile tp = sgi / 2, the look-ahead takes the upper half): tile tp is
//     consumed completely; the other full tiles are whole jobs, then the column strip.
//   odd stage (the panel is the upper half of tp, the look-ahead the lower half of tl = tp + 1): the lower half of tp
//     and the upper half of tl remain as half-tile jobs, the other full tiles are whole, then the column strip --
//     unless tl IS the strip: the look-ahead has then updated all of its columns.
RS_SCHED_HD constexpr unsigned rs_sched_job(int TR, int sgi, int idx)
{
    const int tp = sgi >> 1, odd = sgi & 1, tl = tp + odd;
    int cnt = 0;
    for (int tj = 0; tj <= TR; ++tj) {
        unsigned code = RS_JOB_NONE;
        if (!odd) {
            if (tj == tp) continue;
            code = (tj == TR ? RS_JOB_STRIP : RS_JOB_WHOLE) | (unsigned)tj << 2;
        } else if (tj == tp) {
            code = RS_JOB_HALF | (unsigned)tj << 2;
        } else if (tj == tl) {
            if (tl == TR) continue;
            code = RS_JOB_HALF | (unsigned)tj << 2 | 1u << 4;
        } else {
            code = (tj == TR ? RS_JOB_STRIP : RS_JOB_WHOLE) | (unsigned)tj << 2;
        }
        if (cnt++ == idx) return code;
    }
    return RS_JOB_NONE;
}

RS_SCHED_HD constexpr unsigned long long rs_sched_word(int TR, int role)
{
    unsigned long long w = 0;
    for (int sgi = 0; sgi < 2 * TR; ++sgi) {
        const unsigned long long st = rs_sched_job(TR, sgi, role) | (unsigned long long)rs_sched_job(TR, sgi, role + RS_SCHED_TEAM) << RS_JOB_BITS;
        w |= st << (RS_STAGE_BITS * sgi);
    }
    return w;
}

// what the packing relies on: no stage has a job beyond the second of a role, and a role's second job never precedes
// an empty first one
RS_SCHED_HD constexpr bool rs_sched_fits(int TR)
{
    if (TR < 1 || 2 * TR * RS_STAGE_BITS > 64) return false;
    for (int sgi = 0; sgi < 2 * TR; ++sgi) {
        if (rs_sched_job(TR, sgi, 2 * RS_SCHED_TEAM) != RS_JOB_NONE) return false;
        for (int role = 0; role < RS_SCHED_TEAM; ++role)
            if (rs_sched_job(TR, sgi, role) == RS_JOB_NONE && rs_sched_job(TR, sgi, role + RS_SCHED_TEAM) != RS_JOB_NONE) return false;
    }
    return true;
}
static_assert(rs_sched_fits(1) && rs_sched_fits(2) && rs_sched_fits(3), "stage schedule of the strip classes");
