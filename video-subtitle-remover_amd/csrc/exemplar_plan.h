// Host-side plan of --opencv-fill exemplar: the PatchMatch exemplar fill of tests/_exemplar_statement.py.
// Pyramid sizes, valid sources, targets, tiles and the coarsest level's interpolation offsets depend on the mask alone, so they are
// built once per mask here and every frame runs the kernels of exemplar_kernels.hip over them.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace vsr {

constexpr int EX_R = 3;                  // patches are 7 x 7 x 3 bytes
constexpr int EX_P = 2 * EX_R + 1;
constexpr int EX_MAX_LEVELS = 6;
constexpr int EX_MIN_SIDE = 28;
constexpr int EX_ITERS = 4, EX_PASSES = 4;
constexpr int EX_TILE = 16;
constexpr int EX_INIT_ITER = 255, EX_ANY_SLOT = 63;

// bits of one pixel of a level's class map
enum : uint8_t { EX_HOLE = 1, EX_VALID = 2, EX_TARGET = 4 };

struct ExemplarLevel {
    int H = 0, W = 0;
    int by0 = 0, bx0 = 0, bh = 0, bw = 0;    // bounding box of the targets: the match fields cover it
    std::vector<uint8_t> cls;                // [H][W] EX_* bits
    std::vector<int16_t> src;                // [ns][2] (y, x) valid sources, raster order
    std::vector<int16_t> tgt;                // [nt][2] targets, raster order
    std::vector<int32_t> tiles;              // [ntiles][2] (ty, tx): the 16 x 16 cells that hold a target, raster order
    int64_t nhole = 0;
};

struct ExemplarPlan {
    int H = 0, W = 0;
    std::vector<ExemplarLevel> levels;       // finest first; empty for an empty mask
    std::vector<int32_t> init;               // [nhole of the coarsest][6]: y, x, distance to the known pixel left, right, above, below (0: none)
};

// mask: uint8 [H][W], non-zero = fill.  false + err: bad arguments, or a set mask that leaves no valid source at level 0.
bool exemplar_build_plan(const uint8_t* mask, int H, int W, ExemplarPlan& plan, std::string& err);

}  // namespace vsr
