// Stand-alone dump of gaunegf_amd/csrc/chain_rs_sched.h (built and run by tests/test_chain_rs_sched_host.py, also with
// -fsanitize=address,undefined): the compile-time stage schedule of the chain kernels' small inverse in the
// remainder-strip classes, as the kernel decodes it from the packed words.  One line per job:
//     job <TR> <stage> <role> <slot> <kind> <tile> <upper half>
// and one per word:  word <TR> <role> <hex>.
#include <cstdio>

#include "chain_rs_sched.h"

int main()
{
    int fails = 0;
    for (int TR = 1; TR <= 3; ++TR) {
        if (!rs_sched_fits(TR)) { std::printf("FAIL rs_sched_fits(%d)\n", TR); ++fails; }
        for (int role = 0; role < RS_SCHED_TEAM; ++role) {
            const unsigned long long w = rs_sched_word(TR, role);
            std::printf("word %d %d %llx\n", TR, role, w);
            for (int sgi = 0; sgi < 2 * TR; ++sgi) {
                // the kernel's decoding (rs_inverse_sched)
                unsigned c = (unsigned)(w >> (RS_STAGE_BITS * sgi)) & ((1u << RS_STAGE_BITS) - 1u);
                int slot = 0;
                while (c) {
                    std::printf("job %d %d %d %d %u %u %u\n", TR, sgi, role, slot, c & 3u, (c >> 2) & 3u, (c >> 4) & 1u);
                    if (rs_sched_job(TR, sgi, role + RS_SCHED_TEAM * slot) != (c & ((1u << RS_JOB_BITS) - 1u))) { std::printf("FAIL packing %d %d %d\n", TR, sgi, role); ++fails; }
                    c >>= RS_JOB_BITS;
                    ++slot;
                }
            }
            // nothing behind the last stage
            if (2 * TR * RS_STAGE_BITS < 64 && (w >> (2 * TR * RS_STAGE_BITS)) != 0) { std::printf("FAIL tail %d %d\n", TR, role); ++fails; }
        }
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
