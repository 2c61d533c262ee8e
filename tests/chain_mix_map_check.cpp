// Stand-alone check of gaunegf_amd/csrc/chain_mix_map.h (built and run by tests/test_chain_mix_map_host.py, also with
// -fsanitize=address,undefined): for every n = 1 .. 64 and every pitch class that can serve it, the lane map of the
// chain kernel's mixing step covers the n x n iterate exactly once and stays inside the storage the kernel has.
#include <cstdio>
#include <vector>

#include "chain_mix_map.h"

static const int CLASSES[] = {17, 19, 25, 33, 35, 41, 49, 51, 57, 65};
static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the launcher's class of a launch whose largest contact is n_max (all contacts equal) ...
static int class_of(int n_max) { for (int P : CLASSES) if (n_max <= rs_class_nmax(P)) return P; return -1; }
// ... and the class it moves to when a smaller contact does not reach into the remainder strip
static int bumped_class_of(int n_max) { const int P = class_of(n_max); return P == 19 ? 25 : P == 35 ? 41 : P == 51 ? 57 : P; }

int main()
{
    int pairs = 0;
    for (int n = 1; n <= 64; ++n) {
        const RsMixMap m = rs_mix_map(n);
        CHECK(m.rg >= 1 && m.rg <= 64 && m.stride == m.rg * n && m.stride <= RS_MIX_LANES, "n %d", n);
        CHECK(n < 4 || m.rg >= 4, "n %d rg %d", n, m.rg);
        CHECK(m.slots * m.rg >= n && (m.slots - 1) * m.rg < n, "n %d slots %d", n, m.slots);
        for (int t = 0; t < RS_MIX_LANES; ++t) {
            CHECK(rs_mix_row_group(m, t) == t / n, "n %d t %d", n, t);
            CHECK(rs_mix_col(m, t) == t % n, "n %d t %d", n, t);
            CHECK(rs_mix_active(m, t) == (t < m.stride), "n %d t %d", n, t);
        }
        std::vector<int> held((size_t)n * n, 0);
        for (int t = 0; t < RS_MIX_LANES; ++t)
            for (int s = 0; s < m.slots; ++s) {
                if (!rs_mix_valid(m, t, s)) {
                    // only idle lanes and rows past the matrix in the LAST slot hold nothing
                    CHECK(!rs_mix_active(m, t) || s == m.slots - 1, "n %d t %d s %d", n, t, s);
                    continue;
                }
                const int row = rs_mix_row(m, t, s), col = rs_mix_col(m, t);
                CHECK(row >= 0 && row < n && col >= 0 && col < n, "n %d t %d s %d -> (%d, %d)", n, t, s, row, col);
                CHECK(row * n + col == s * m.stride + t, "n %d t %d s %d linear index", n, t, s);
                if (row >= 0 && row < n && col >= 0 && col < n) ++held[(size_t)row * n + col];
            }
        for (int e = 0; e < n * n; ++e) CHECK(held[e] == 1, "n %d element (%d, %d) held %d times", n, e / n, e % n, held[e]);
        // the pivot table (64 entries) is read at the row of every slot of every active lane, valid or not
        for (int t = 0; t < m.stride; ++t) CHECK(rs_mix_row(m, t, m.slots - 1) < 64, "n %d t %d pivot-table index", n, t);
        // every launch this n can be part of: largest contact n_max >= n, its class or the bumped one
        for (int n_max = n; n_max <= 64; ++n_max) {
            const int cls[2] = {class_of(n_max), bumped_class_of(n_max)};
            for (int k = 0; k < (cls[0] == cls[1] ? 1 : 2); ++k) {
                const int P = cls[k];
                if (k == 0 && n != n_max && P != bumped_class_of(n_max) && n <= 16 * (rs_class_tiles(P) - 1)) continue;   // (this launch is bumped)
                ++pairs;
                const int lds = rs_mix_lds_slots(m, P), glob = rs_mix_global_slots(m, P);
                const int spare = rs_class_welems(P) - (n_max + 2) * P;       // what the launcher leaves behind row n_max + 1
                CHECK(n_max <= rs_class_nmax(P), "n_max %d P %d", n_max, P);
                CHECK(lds >= 0 && glob >= 0 && lds + glob == m.slots, "n %d P %d", n, P);
                CHECK(lds == 0 || lds * RS_MIX_LANES <= spare, "n %d n_max %d P %d: %d LDS slots, spare %d", n, n_max, P, lds, spare);
                CHECK(m.slots <= rs_class_ksteps(P), "n %d P %d: %d slots, %d k-steps", n, P, m.slots, rs_class_ksteps(P));
                CHECK(rs_class_ksteps(P) <= rs_mix_reserved_slots(n_max), "n_max %d P %d", n_max, P);
                CHECK(m.slots <= rs_mix_max_slots(1, rs_class_nmax(P)), "n %d P %d", n, P);
            }
        }
    }
    // the table of the change that introduced the map
    CHECK(rs_mix_map(50).slots == 10 && rs_mix_map(49).slots == 10 && rs_mix_map(51).slots == 11, "n 49-51");
    CHECK(rs_mix_map(41).slots == 7 && rs_mix_map(33).slots == 5 && rs_mix_map(35).slots == 5, "n 33-41");
    CHECK(rs_mix_map(57).slots == 15 && rs_mix_map(64).slots == 16, "n 57-64");
    CHECK(rs_class_lds_slots(51) == 2, "class 51 LDS slots");
    std::printf("%d (n, class) pairs checked, %d failures\n", pairs, fails);
    return fails ? 1 : 0;
}
