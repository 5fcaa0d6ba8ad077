// Role mapping of the scenario-batched factor bodies (leaf_batch_body / sleaf_batch_body, hpf_leafbatch.hpp): which thread of the 256-thread
// workgroup serves which (scenario, row) and (scenario, harmonic) of a tile of SB scenarios.  SB = 16: 16 threads per scenario, four rows and
// ceil(H2 / 16) harmonics each; SB = 8: 32 threads per scenario, two rows and ceil(H2 / 32) harmonics each -- half the sequential walk per
// thread, for launches too narrow to fill the chip (HPF_BATCH_TILE8_MAX).  Plain C++ (host and device): the host tests compile it on its own.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HPF_TILE_HD __host__ __device__
#else
#define HPF_TILE_HD
#endif

namespace hpf {

constexpr int BATCH_WG = 256;         // threads of a batched workgroup
constexpr int BATCH_ROWS = 64;        // rows of the [row][scenario] arrays (blocks of up to 52 rows, padded to the MFMA tiles)
constexpr int BATCH_COLS = 16;        // B-operand columns of an MFMA: the scenarios of a tile (columns SB.. are zero)

template <int SB>
struct BatchTile {
    static_assert(SB == 16 || SB == 8, "scenario tiles of 16 or 8");
    static constexpr int TPS = BATCH_WG / SB;                  // threads per scenario
    static constexpr int ROWS = BATCH_ROWS / TPS;              // rows per thread
    static HPF_TILE_HD constexpr int harmonics(int H2) { return (H2 + TPS - 1) / TPS; }      // harmonics per thread
    static HPF_TILE_HD constexpr int scenario(int tid) { return tid / TPS; }                 // scenario of the tile
    static HPF_TILE_HD constexpr int lane(int tid) { return tid % TPS; }                     // the thread's place among its scenario's
    static HPF_TILE_HD constexpr int row(int tid, int pz) { return lane(tid) + TPS * pz; }   // pz < ROWS
    static HPF_TILE_HD constexpr int harmonic(int tid, int it) { return lane(tid) + TPS * it; }   // it < harmonics(H2)
    static HPF_TILE_HD constexpr int tiles(int scenarios) { return (scenarios + SB - 1) / SB; }   // workgroups per bus
};

// the tile a launch of S scenarios takes: 8 up to tile8_max (0: never), else 16
HPF_TILE_HD constexpr int batch_tile_of(int S, int tile8_max) { return S <= tile8_max ? 8 : 16; }

}  // namespace hpf
