// The plan of --opencv-fill exemplar (exemplar_plan.h): tests/_exemplar_statement.plan restated for the host.
#include "exemplar_plan.h"

#include <algorithm>

namespace vsr {
namespace {

// square dilation by k, clipped to the frame: a pixel is set if its (2k+1)^2 window holds a hole pixel
std::vector<uint8_t> dilate(const std::vector<uint8_t>& hole, int H, int W, int k)
{
    std::vector<int32_t> c((size_t)(H + 1) * (W + 1), 0);                  // integral image of the hole
    for (int y = 0; y < H; ++y) {
        int32_t run = 0;
        for (int x = 0; x < W; ++x) {
            run += hole[(size_t)y * W + x];
            c[(size_t)(y + 1) * (W + 1) + x + 1] = c[(size_t)y * (W + 1) + x + 1] + run;
        }
    }
    std::vector<uint8_t> out((size_t)H * W);
    for (int y = 0; y < H; ++y) {
        const int y0 = std::max(y - k, 0), y1 = std::min(y + k + 1, H);
        for (int x = 0; x < W; ++x) {
            const int x0 = std::max(x - k, 0), x1 = std::min(x + k + 1, W);
            const int32_t s = c[(size_t)y1 * (W + 1) + x1] - c[(size_t)y0 * (W + 1) + x1] - c[(size_t)y1 * (W + 1) + x0] + c[(size_t)y0 * (W + 1) + x0];
            out[(size_t)y * W + x] = s > 0;
        }
    }
    return out;
}

// whether the hole survives k 4-neighbour erosions, outside the frame counting as hole
bool depth_exceeds(std::vector<uint8_t> hole, int H, int W, int k)
{
    std::vector<uint8_t> next(hole.size());
    auto at = [&](int y, int x) -> uint8_t { return (y < 0 || y >= H || x < 0 || x >= W) ? 1 : hole[(size_t)y * W + x]; };
    for (int it = 0; it < k; ++it) {
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                next[(size_t)y * W + x] = at(y, x) & at(y - 1, x) & at(y + 1, x) & at(y, x - 1) & at(y, x + 1);
        hole.swap(next);
    }
    return std::any_of(hole.begin(), hole.end(), [](uint8_t v) { return v != 0; });
}

std::vector<uint8_t> down_hole(const std::vector<uint8_t>& hole, int H, int W)
{
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    std::vector<uint8_t> out((size_t)Hc * Wc);
    for (int y = 0; y < Hc; ++y)
        for (int x = 0; x < Wc; ++x) {
            const int y1 = std::min(2 * y + 1, H - 1), x1 = std::min(2 * x + 1, W - 1);
            out[(size_t)y * Wc + x] = hole[(size_t)(2 * y) * W + 2 * x] | hole[(size_t)(2 * y) * W + x1] | hole[(size_t)y1 * W + 2 * x] | hole[(size_t)y1 * W + x1];
        }
    return out;
}

void build_level(const std::vector<uint8_t>& hole, int H, int W, int level, ExemplarLevel& lv)
{
    lv.H = H;
    lv.W = W;
    lv.cls.assign((size_t)H * W, 0);
    const std::vector<uint8_t> meets = dilate(hole, H, W, EX_R), close = dilate(hole, H, W, std::max(8, 32 >> level));
    int y0 = H, x0 = W, y1 = -1, x1 = -1;
    const int tw = (W + EX_TILE - 1) / EX_TILE, th = (H + EX_TILE - 1) / EX_TILE;
    std::vector<uint8_t> tile_has((size_t)th * tw, 0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const bool centre = y >= EX_R && y < H - EX_R && x >= EX_R && x < W - EX_R;
            uint8_t c = hole[i] ? EX_HOLE : 0;
            if (hole[i]) ++lv.nhole;
            if (centre && !meets[i] && close[i]) {
                c |= EX_VALID;
                lv.src.push_back((int16_t)y);
                lv.src.push_back((int16_t)x);
            }
            if (centre && meets[i]) {
                c |= EX_TARGET;
                lv.tgt.push_back((int16_t)y);
                lv.tgt.push_back((int16_t)x);
                tile_has[(size_t)(y / EX_TILE) * tw + x / EX_TILE] = 1;
                y0 = std::min(y0, y); y1 = std::max(y1, y); x0 = std::min(x0, x); x1 = std::max(x1, x);
            }
            lv.cls[i] = c;
        }
    for (int ty = 0; ty < th; ++ty)
        for (int tx = 0; tx < tw; ++tx)
            if (tile_has[(size_t)ty * tw + tx]) {
                lv.tiles.push_back(ty);
                lv.tiles.push_back(tx);
            }
    if (y1 >= 0) { lv.by0 = y0; lv.bx0 = x0; lv.bh = y1 - y0 + 1; lv.bw = x1 - x0 + 1; }
}

void build_init(const std::vector<uint8_t>& hole, int H, int W, std::vector<int32_t>& table)
{
    static const int DY[4] = {0, 0, -1, 1}, DX[4] = {-1, 1, 0, 0};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            if (!hole[(size_t)y * W + x]) continue;
            int32_t d[4] = {0, 0, 0, 0};
            for (int k = 0; k < 4; ++k) {
                int yy = y + DY[k], xx = x + DX[k], s = 1;
                while (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                    if (!hole[(size_t)yy * W + xx]) { d[k] = s; break; }
                    yy += DY[k]; xx += DX[k]; ++s;
                }
            }
            table.insert(table.end(), {y, x, d[0], d[1], d[2], d[3]});
        }
}

}  // namespace

bool exemplar_build_plan(const uint8_t* mask, int H, int W, ExemplarPlan& plan, std::string& err)
{
    if (!mask || H < 1 || W < 1 || H > 32767 || W > 32767) {
        err = "exemplar: the frame must be 1..32767 pixels a side";
        return false;
    }
    plan = ExemplarPlan();
    plan.H = H;
    plan.W = W;
    std::vector<uint8_t> hole((size_t)H * W);
    bool any = false;
    for (size_t i = 0; i < hole.size(); ++i) { hole[i] = mask[i] != 0; any |= hole[i] != 0; }
    if (!any) return true;                                                 // an empty mask: no level, nothing is filled
    plan.levels.emplace_back();
    build_level(hole, H, W, 0, plan.levels[0]);
    if (plan.levels[0].src.empty()) {
        plan = ExemplarPlan();
        err = "exemplar: the mask leaves no 7x7 patch of known pixels near the hole to copy from (a whole-frame mask, or a frame smaller than 7x7)";
        return false;
    }
    int h = H, w = W;
    while ((int)plan.levels.size() < EX_MAX_LEVELS && depth_exceeds(hole, h, w, 2) && std::min(h, w) >= EX_MIN_SIDE) {
        std::vector<uint8_t> nh = down_hole(hole, h, w);
        ExemplarLevel lv;
        build_level(nh, (h + 1) / 2, (w + 1) / 2, (int)plan.levels.size(), lv);
        if (lv.src.empty()) break;
        plan.levels.push_back(std::move(lv));
        hole.swap(nh);
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    build_init(hole, h, w, plan.init);
    return true;
}

}  // namespace vsr
