// Host-side schedule ("plan") of --inpaint-mode opencv: OpenCV's INPAINT_TELEA restated (tests/_telea_statement.py is the
// readable statement; DESIGN.md has the section).  The fast-marching order, T, every "known at that step" flag and every tap
// weight depend on the mask alone, so the serial sweep runs once per mask here and the frames replay it level by level on the
// GPU (telea_kernels.hip).
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace vsr {

constexpr int TELEA_MAX_RADIUS = 5;
constexpr int TELEA_MAX_TAPS = (2 * TELEA_MAX_RADIUS + 1) * (2 * TELEA_MAX_RADIUS + 1) - 1;

// flag bits of one (pixel, tap)
enum : uint8_t { TELEA_TAP = 1, TELEA_RIGHT = 2, TELEA_LEFT = 4, TELEA_DOWN = 8, TELEA_UP = 16 };

struct TeleaPlan {
    int H = 0, W = 0, radius = 3;
    int64_t P = 0;                       // scheduled (= reached) masked pixels
    int L = 0;                           // levels
    int NT = 0;                          // taps per pixel: (dk, dl) != 0 with dk^2 + dl^2 <= radius^2, in the serial k, l order
    int8_t tap_dk[TELEA_MAX_TAPS] = {}, tap_dl[TELEA_MAX_TAPS] = {};
    // per pixel, sorted by (level, step): what the kernel walks
    std::vector<int32_t> yx;             // [P][2]
    std::vector<int32_t> step;           // [P] index in the serial fill order
    std::vector<float> T;                // [P]
    std::vector<int32_t> level;          // [P] 1-based
    std::vector<int32_t> level_off;      // [L+1] into the arrays above
    std::vector<float> w;                // [NT][P] tap weight |dst lev dir| (0 where the tap does not count)
    std::vector<uint8_t> flags;          // [NT][P] TELEA_* bits
    std::vector<float> tmap;             // [(H+2)(W+2)] T after the pass (padded)
};

// mask: uint8 [H][W], non-zero = fill.  false + err on bad arguments.
bool telea_build_plan(const uint8_t* mask, int H, int W, int radius, TeleaPlan& plan, std::string& err);

}  // namespace vsr
