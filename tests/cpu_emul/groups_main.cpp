// TEST INFRASTRUCTURE: the split of a batch's slots over the scenario groups of csrc/hpf_groups.hpp on the host (tests/test_groups_host.py): the
// properties the enqueue relies on, for every count in 1..4096 and every n_groups in 1..8, and the pinned splits.  Prints "groups clean" when
// every check holds.
#include <stdio.h>

#include <vector>

#include "hpf_groups.hpp"
using namespace hpf;

static int fails = 0;
#define CHECK(c)                                                                                        \
    do {                                                                                                \
        if (!(c)) {                                                                                     \
            if (++fails <= 20) printf("FAIL %s:%d  %s  (count %d, n_groups %d)\n", __FILE__, __LINE__, #c, count, n_groups); \
        }                                                                                               \
    } while (0)

static void pinned(int count, int n_groups, const std::vector<int>& want) {
    const int G = group_count(true, n_groups, count);
    CHECK(G + 1 == (int)want.size());
    for (int g = 0; g <= G && g < (int)want.size(); ++g) CHECK(group_bound(count, G, g) == want[g]);
}

int main() {
    for (int count = 1; count <= 4096; ++count)
        for (int n_groups = 1; n_groups <= 8; ++n_groups) {
            CHECK(group_count(false, n_groups, count) == 1);           // (dense solver, meshed network: no groups)
            const int G = group_count(true, n_groups, count);
            CHECK(G >= 1 && G <= n_groups);
            if (count < 64) CHECK(G == 1);
            CHECK(group_bound(count, G, 0) == 0);
            CHECK(group_bound(count, G, G) == count);
            CHECK(group_bound(count, G, G + 1) == count);
            for (int g = 0; g < G; ++g) {
                const int b0 = group_bound(count, G, g), b1 = group_bound(count, G, g + 1);
                CHECK(b0 <= b1);
                if (g > 0) CHECK(b0 % 16 == 0);
                if (G > 1) CHECK(b1 - b0 >= 16);
            }
        }
    pinned(128, 3, {0, 48, 80, 128});                                  // 3 + 2 + 3 tiles of 16 scenarios, not 43 + 43 + 42
    pinned(128, 4, {0, 32, 64, 96, 128});
    pinned(80, 4, {0, 48, 80});
    pinned(63, 4, {0, 63});
    pinned(1024, 8, {0, 128, 256, 384, 512, 640, 768, 896, 1024});
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("groups clean\n");
    return 0;
}
