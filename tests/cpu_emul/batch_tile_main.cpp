// TEST INFRASTRUCTURE: the role mapping of the scenario-batched factor bodies (csrc/hpf_batch_tile.hpp) on the host
// (tests/test_batch_tile_host.py): for blocks of 12, 28 and 52 rows and tiles of 16 and 8 scenarios every (scenario, row) and every
// (scenario, harmonic) has exactly one owner among the 256 threads, tiles of 16 are today's (tid >> 4, tid & 15, l16 + 16 pz) assignment, and
// the tile follows the group size.  Prints "batch tile clean" when every check holds.
#include <stdio.h>
#include <string.h>

#include "hpf_batch_tile.hpp"
using namespace hpf;

static int fails = 0;
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c);  \
            ++fails;                                             \
        }                                                        \
    } while (0)

template <int SB>
static void owners(int B) {
    using TL = BatchTile<SB>;
    const int H2 = B / 2, QI = TL::harmonics(H2);
    static int row_owner[16][BATCH_ROWS], harm_owner[16][64];
    memset(row_owner, 0, sizeof row_owner);
    memset(harm_owner, 0, sizeof harm_owner);
    CHECK(TL::TPS * SB == BATCH_WG && TL::ROWS * TL::TPS == BATCH_ROWS);
    CHECK(QI * TL::TPS >= H2 && (QI - 1) * TL::TPS < H2);
    for (int tid = 0; tid < BATCH_WG; ++tid) {
        const int sc = TL::scenario(tid), lt = TL::lane(tid);
        CHECK(sc >= 0 && sc < SB && lt >= 0 && lt < TL::TPS && sc * TL::TPS + lt == tid);
        CHECK((tid >> 6) == (sc * TL::TPS) >> 6);                      // a scenario's threads share a wavefront
        CHECK(lt >= 16 || ((tid & 63) >> 4) == ((tid - lt) & 63) >> 4);  // ... and its first 16 one DPP row (the pivot search of T)
        for (int pz = 0; pz < TL::ROWS; ++pz) {
            const int row = TL::row(tid, pz);
            CHECK(row >= 0 && row < BATCH_ROWS);
            ++row_owner[sc][row];
        }
        for (int it = 0; it < QI; ++it) {
            const int q = TL::harmonic(tid, it);
            CHECK(q >= 0 && q < 64);
            ++harm_owner[sc][q];
        }
        if (lt == 0) CHECK(TL::harmonic(tid, 0) == 0 && TL::row(tid, 0) == 0);      // harmonic 0 and row 0: the scenario's first thread
        if (SB == 16) {                                                 // today's assignment
            const int l16 = tid & 15;
            CHECK(sc == tid >> 4 && lt == l16);
            for (int pz = 0; pz < 4; ++pz) CHECK(TL::row(tid, pz) == l16 + 16 * pz);
            for (int it = 0; it < QI; ++it) CHECK(TL::harmonic(tid, it) == l16 + 16 * it);
            CHECK(TL::ROWS == 4 && QI == (H2 + 15) / 16);
        }
    }
    for (int sc = 0; sc < SB; ++sc) {
        for (int row = 0; row < BATCH_ROWS; ++row) CHECK(row_owner[sc][row] == 1);     // (every row of the LDS arrays, the padding included)
        for (int q = 0; q < H2; ++q) CHECK(harm_owner[sc][q] == 1);
    }
    for (int sc = SB; sc < 16; ++sc)
        for (int row = 0; row < BATCH_ROWS; ++row) CHECK(row_owner[sc][row] == 0);
    CHECK(TL::tiles(0) == 0 && TL::tiles(1) == 1 && TL::tiles(SB) == 1 && TL::tiles(SB + 1) == 2 && TL::tiles(19) == (19 + SB - 1) / SB);
}

int main() {
    const int blocks[] = {12, 28, 52};
    for (int B : blocks) {
        owners<16>(B);
        owners<8>(B);
    }
    static_assert(BatchTile<8>::TPS == 32 && BatchTile<8>::ROWS == 2 && BatchTile<8>::harmonics(26) == 1 && BatchTile<16>::harmonics(26) == 2, "");
    CHECK(batch_tile_of(1, 0) == 16 && batch_tile_of(32, 0) == 16);             // 0: never
    CHECK(batch_tile_of(1, 32) == 8 && batch_tile_of(32, 32) == 8 && batch_tile_of(33, 32) == 16);
    if (!fails) printf("batch tile clean\n");
    return fails != 0;
}
