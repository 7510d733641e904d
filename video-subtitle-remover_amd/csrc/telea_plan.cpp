// The mask schedule of the Telea fill (telea_plan.h).  Every rule below is spelled out in tests/_telea_statement.py, which the
// not-gpu suite compares this file with pixel by pixel (tests/test_telea_plan.py).
#include "telea_plan.h"

#include <math.h>
#include <algorithm>
#include <numeric>
#include <queue>

// weights are fp32 products the tests reproduce bit for bit in numpy: no fused multiply-add
#pragma clang fp contract(off)

namespace vsr {
namespace {

enum : uint8_t { KNOWN = 0, BAND = 1, INSIDE = 2 };

struct Item {
    float T;
    uint64_t seq;                        // first in, first out among equal T
    int i, j;
    bool operator>(const Item& o) const { return T > o.T || (T == o.T && seq > o.seq); }
};
using Heap = std::priority_queue<Item, std::vector<Item>, std::greater<Item>>;

struct Grid {
    int rows, cols;
    std::vector<uint8_t> f;
    std::vector<float> t;
    uint8_t& F(int i, int j) { return f[(size_t)i * cols + j]; }
    float& Tt(int i, int j) { return t[(size_t)i * cols + j]; }
};

float solve(Grid& g, int i1, int j1, int i2, int j2)
{
    const double a11 = g.Tt(i1, j1), a22 = g.Tt(i2, j2), m12 = std::min(a11, a22);
    double sol;
    if (g.F(i1, j1) != INSIDE) {
        if (g.F(i2, j2) != INSIDE)
            sol = fabs(a11 - a22) >= 1.0 ? 1 + m12 : (a11 + a22 + sqrt(2 - (a11 - a22) * (a11 - a22))) * 0.5;
        else
            sol = 1 + a11;
    } else if (g.F(i2, j2) != INSIDE) {
        sol = 1 + a22;
    } else {
        sol = 1 + m12;
    }
    return (float)sol;
}

float min4(Grid& g, int i, int j)
{
    return std::min(std::min(solve(g, i - 1, j, i, j - 1), solve(g, i + 1, j, i, j - 1)),
                    std::min(solve(g, i - 1, j, i, j + 1), solve(g, i + 1, j, i, j + 1)));
}

const int NB[4][2] = {{-1, 0}, {0, -1}, {1, 0}, {0, 1}};      // up, left, down, right

}  // namespace

bool telea_build_plan(const uint8_t* mask, int H, int W, int radius, TeleaPlan& plan, std::string& err)
{
    if (!mask || H < 3 || W < 3 || H > 32766 || W > 32766) { err = "telea: mask must be uint8 [H][W] with 3 <= H, W <= 32766"; return false; }
    if (radius < 1 || radius > TELEA_MAX_RADIUS) { err = "telea: radius must be 1.." + std::to_string(TELEA_MAX_RADIUS); return false; }
    const int R = radius, rows = H + 2, cols = W + 2;
    const size_t N = (size_t)rows * cols;
    plan = TeleaPlan();
    plan.H = H; plan.W = W; plan.radius = R;
    for (int dk = -R; dk <= R; ++dk)
        for (int dl = -R; dl <= R; ++dl)
            if ((dk || dl) && dk * dk + dl * dl <= R * R) { plan.tap_dk[plan.NT] = (int8_t)dk; plan.tap_dl[plan.NT] = (int8_t)dl; ++plan.NT; }
    const int NT = plan.NT;
    float tap_dst[TELEA_MAX_TAPS];
    for (int tp = 0; tp < NT; ++tp) {
        const float rx = (float)-plan.tap_dl[tp], ry = (float)-plan.tap_dk[tp];
        const float vl = sqrtf(rx * rx + ry * ry);
        tap_dst[tp] = (float)(1.0 / ((double)vl * sqrt((double)vl)));
    }

    std::vector<uint8_t> m(N, 0), band(N, 0);
    auto at = [cols](int i, int j) { return (size_t)i * cols + j; };
    int64_t masked = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (mask[(size_t)y * W + x]) { m[at(y + 1, x + 1)] = 1; ++masked; }
    for (int i = 1; i < rows - 1; ++i)
        for (int j = 1; j < cols - 1; ++j)
            if (!m[at(i, j)] && (m[at(i - 1, j)] || m[at(i + 1, j)] || m[at(i, j - 1)] || m[at(i, j + 1)])) band[at(i, j)] = 1;

    // outer pass: the ring of `radius` pixels around the mask, marched outwards from the band, then negated
    Grid g{rows, cols, std::vector<uint8_t>(N, KNOWN), std::vector<float>(N, 1.0e6f)};
    {
        std::vector<uint8_t> rowdil(N, 0);                   // square dilation, separably
        for (int i = 0; i < rows; ++i)
            for (int j = 0; j < cols; ++j)
                if (m[at(i, j)])
                    for (int jj = std::max(0, j - R); jj <= std::min(cols - 1, j + R); ++jj) rowdil[at(i, jj)] = 1;
        for (int i = 0; i < rows; ++i)
            for (int j = 0; j < cols; ++j)
                if (rowdil[at(i, j)])
                    for (int ii = std::max(0, i - R); ii <= std::min(rows - 1, i + R); ++ii)
                        if (ii > 0 && ii < rows - 1 && j > 0 && j < cols - 1 && !m[at(ii, j)] && !band[at(ii, j)]) g.F(ii, j) = INSIDE;
    }
    Heap heap;
    uint64_t seq = 0;
    std::vector<Item> first;
    for (int i = 1; i < rows - 1; ++i)
        for (int j = 1; j < cols - 1; ++j)
            if (band[at(i, j)]) { g.Tt(i, j) = 0.0f; first.push_back(Item{0.0f, seq++, i, j}); }
    for (const Item& it : first) heap.push(it);
    std::vector<std::pair<int, int>> changed;
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        changed.emplace_back(it.i, it.j);
        for (auto& d : NB) {
            const int i = it.i + d[0], j = it.j + d[1];
            if (i <= 0 || j <= 0 || i >= rows - 1 || j >= cols - 1) continue;
            if (g.F(i, j) != INSIDE) continue;
            const float dist = min4(g, i, j);
            g.Tt(i, j) = dist;
            g.F(i, j) = BAND;
            heap.push(Item{dist, seq++, i, j});
        }
    }
    for (auto& c : changed) g.Tt(c.first, c.second) = -g.Tt(c.first, c.second);

    // main pass
    for (size_t q = 0; q < N; ++q) g.f[q] = m[q] ? INSIDE : (band[q] ? BAND : KNOWN);
    for (const Item& it : first) heap.push(it);
    std::vector<int32_t> lev(N, 0), war(N, 0);
    std::vector<int32_t> s_yx, s_level;
    std::vector<float> s_T, s_w;
    std::vector<uint8_t> s_fl;
    s_yx.reserve((size_t)masked * 2); s_level.reserve(masked); s_T.reserve(masked);
    s_w.reserve((size_t)masked * NT); s_fl.reserve((size_t)masked * NT);
    std::vector<size_t> unfilled;
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        g.F(it.i, it.j) = KNOWN;
        for (auto& d : NB) {
            const int i = it.i + d[0], j = it.j + d[1];
            if (i <= 0 || j <= 0 || i >= rows - 1 || j >= cols - 1) continue;
            if (g.F(i, j) != INSIDE) continue;
            const float ti = min4(g, i, j);
            g.Tt(i, j) = ti;
            float gx, gy;
            if (g.F(i, j + 1) != INSIDE) gx = g.F(i, j - 1) != INSIDE ? (g.Tt(i, j + 1) - g.Tt(i, j - 1)) * 0.5f : g.Tt(i, j + 1) - ti;
            else gx = g.F(i, j - 1) != INSIDE ? ti - g.Tt(i, j - 1) : 0.0f;
            if (g.F(i + 1, j) != INSIDE) gy = g.F(i - 1, j) != INSIDE ? (g.Tt(i + 1, j) - g.Tt(i - 1, j)) * 0.5f : g.Tt(i + 1, j) - ti;
            else gy = g.F(i - 1, j) != INSIDE ? ti - g.Tt(i - 1, j) : 0.0f;
            int32_t Lv = war[at(i, j)];
            unfilled.clear();
            for (int tp = 0; tp < NT; ++tp) {
                const int k = i + plan.tap_dk[tp], l = j + plan.tap_dl[tp];
                float w = 0.0f;
                uint8_t fl = 0;
                if (k > 0 && l > 0 && k < rows - 1 && l < cols - 1 && g.F(k, l) != INSIDE) {
                    const float ry = (float)(i - k), rx = (float)(j - l);
                    const float lv = (float)(1.0 / (1.0 + fabs((double)(g.Tt(k, l) - ti))));
                    float dr = rx * gx + ry * gy;
                    if (fabs((double)dr) <= 0.01) dr = 0.000001f;
                    w = fabsf(tap_dst[tp] * lv * dr);
                    const bool a = g.F(k, l + 1) != INSIDE, b = g.F(k, l - 1) != INSIDE, a2 = g.F(k + 1, l) != INSIDE, b2 = g.F(k - 1, l) != INSIDE;
                    fl = (uint8_t)(TELEA_TAP | (a ? TELEA_RIGHT : 0) | (b ? TELEA_LEFT : 0) | (a2 ? TELEA_DOWN : 0) | (b2 ? TELEA_UP : 0));
                    // the pixels this tap reads (unpadded, OpenCV's clamped indices) decide the level
                    const int km = k - 1 + (k == 1), kp = k - 1 - (k == rows - 2), lm = l - 1 + (l == 1), lp = l - 1 - (l == cols - 2);
                    int rd[7][2], nr = 0;
                    auto add = [&](int y, int x) { rd[nr][0] = y; rd[nr][1] = x; ++nr; };
                    add(km, lm);
                    if (a) { add(km, lp + 1); if (b) add(km, lm - 1); }
                    else if (b) { add(km, lp); add(km, lm - 1); }
                    if (a2) { add(kp + 1, lm); if (b2) add(km - 1, lm); }
                    else if (b2) { add(kp, lm); add(km - 1, lm); }
                    for (int q = 0; q < nr; ++q) {
                        const size_t p = at(rd[q][0] + 1, rd[q][1] + 1);
                        if (!m[p]) continue;
                        if (g.f[p] != INSIDE) Lv = std::max(Lv, lev[p]);
                        else unfilled.push_back(p);
                    }
                }
                s_w.push_back(w);
                s_fl.push_back(fl);
            }
            ++Lv;
            lev[at(i, j)] = Lv;
            for (size_t p : unfilled) war[p] = std::max(war[p], Lv);     // read while unfilled: its writer goes to a later level
            s_yx.push_back(i - 1); s_yx.push_back(j - 1);
            s_T.push_back(ti);
            s_level.push_back(Lv);
            g.F(i, j) = BAND;
            heap.push(Item{ti, seq++, i, j});
        }
    }

    const int64_t P = (int64_t)s_level.size();
    plan.P = P;
    plan.tmap = g.t;
    std::vector<int32_t> order((size_t)P);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return s_level[a] < s_level[b]; });
    plan.L = P ? *std::max_element(s_level.begin(), s_level.end()) : 0;
    plan.yx.resize((size_t)P * 2); plan.step.resize(P); plan.T.resize(P); plan.level.resize(P);
    plan.w.resize((size_t)P * NT); plan.flags.resize((size_t)P * NT);
    plan.level_off.assign((size_t)plan.L + 1, 0);
    for (int64_t q = 0; q < P; ++q) {
        const int32_t s = order[q];
        plan.yx[2 * q] = s_yx[2 * (size_t)s]; plan.yx[2 * q + 1] = s_yx[2 * (size_t)s + 1];
        plan.step[q] = s; plan.T[q] = s_T[s]; plan.level[q] = s_level[s];
        plan.level_off[s_level[s]] = (int32_t)(q + 1);
        for (int tp = 0; tp < NT; ++tp) {
            plan.w[(size_t)tp * P + q] = s_w[(size_t)s * NT + tp];
            plan.flags[(size_t)tp * P + q] = s_fl[(size_t)s * NT + tp];
        }
    }
    for (int l = 1; l <= plan.L; ++l) plan.level_off[l] = std::max(plan.level_off[l], plan.level_off[l - 1]);
    return true;
}

}  // namespace vsr
