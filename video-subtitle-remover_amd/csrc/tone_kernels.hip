// --tone-match: the fill's tone levelled to the picture across the seam of the composite mask (the statement is
// tests/_tone_statement.py).  Integer arithmetic only.
//
//   k_tone_sets     C (uint8 [H][W], non-zero = the plugin blends here) and the sample rows [r0, r1) -> a byte map of the picture:
//                   bit 0 = E (C == 0, a non-zero within Chebyshev distance 2), bit 1 = M (C != 0, a zero within Chebyshev distance 2),
//                   both only at r0 <= y < r1 and counted; bit 2 = C != 0.  A wave owns one level-3 cell (8 x 8 pixels, a lane each)
//                   and lists it when one of its bytes is non-zero.  Once per mask.
//   k_tone_cells    per listed cell and frame: the number and the per-channel sum of src over E and of the fill over M, and whether
//                   the fill differs from src on a pixel of C.  A wave per cell, packed 16-bit partial sums, wave reductions; no
//                   atomics (every wave of a frame setting one "changed" word made this kernel five times as long as the other two).
//   k_tone_levels   one workgroup per frame walks the cell pyramid with barriers (the precedent: the Telea replay): the listed cells
//                   are added into their level-4 parents, every level above is the sum of its 2 x 2 children, the top cell's means
//                   start the push, which blends each level's own mean with the bilinear upsample of the level above by the number of
//                   samples the cell holds; at level 3 the clamped difference of the two sets' fields is kept.  Integer sums and
//                   integer atomics: whatever order the threads arrive in, the same words.
//   k_tone_offset   in place on the frames that hold the fill: fill + (S * h + d / 2) / d on the pixels of C, h the bilinear
//                   interpolation of the level-3 difference between the four nearest cell centres.
//
// The frames hold `rows` rows of the picture starting at its row y0 (the whole picture, or sttn-auto's strip rows); the map and the
// cells are the whole picture's.  A frame is rows * W * 3 contiguous bytes at any alignment, frames and src have their own strides.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "plan_c.h"
#include "tone_kernels.h"

namespace {

constexpr int TN_BAND = 2, TN_MAX_PERCENT = 100, TN_FINEST = 3, TN_MAX_LEVELS = 28;       // levels 3 .. 30: max(H, W) < 2^31 / 3
constexpr int TN_CLAMP = 24 * 64, TN_DEN = 100 * 64 * 256;
constexpr int TN_THREADS = 256, TN_WAVES = TN_THREADS / 64, TN_LEVEL_THREADS = 1024;
constexpr int TN_MAX_GY = 1024, TN_MAX_GX = 2048;
constexpr uint8_t BIT_E = 1, BIT_M = 2, BIT_C = 4;

// the cell grids of one picture: level k is gh[k - 3] x gw[k - 3]; the levels 4 .. K lie one after the other in the workspace's upper
// arrays, level k from cell off[k - 3] on; `upper` cells in all
struct ToneGeom {
    int K;
    int gh[TN_MAX_LEVELS], gw[TN_MAX_LEVELS];
    int64_t off[TN_MAX_LEVELS];
    int64_t upper;
};

ToneGeom geometry(int H, int W)
{
    ToneGeom g{};
    g.K = TN_FINEST;
    while ((1ll << g.K) < (H > W ? H : W)) ++g.K;
    for (int k = TN_FINEST; k <= g.K; ++k) {
        g.gh[k - TN_FINEST] = (int)((H + (1ll << k) - 1) >> k);
        g.gw[k - TN_FINEST] = (int)((W + (1ll << k) - 1) >> k);
        g.off[k - TN_FINEST] = g.upper;
        if (k > TN_FINEST) g.upper += (int64_t)g.gh[k - TN_FINEST] * g.gw[k - TN_FINEST];
    }
    return g;
}

// the workspace of n frames: per frame two flag words (changed, touched), then the arrays below, every frame's part after the other
struct ToneSpace {
    int32_t* flags;       // [n][2]          written by k_tone_levels, read by k_tone_offset
    int64_t* usum;        // [n][upper][6]   the sums of the levels above 3: E's three channels, then M's
    int32_t* l3;          // [n][ncells][8]  per listed cell: |E| (bit 16: a pixel of C changed), |M|, E's sums, M's sums
    int32_t* ucnt;        // [n][upper][2]
    int32_t* uv;          // [n][upper][6]   V of the levels above 3, in 1/64 levels
    int32_t* h3;          // [n][g3][3]      the clamped difference at level 3
};

int64_t frame_bytes(const ToneGeom& g) { return 8 + 80 * g.upper + 44 * (int64_t)g.gh[0] * g.gw[0]; }

ToneSpace carve(void* workspace, const ToneGeom& g, int n)
{
    const int64_t g3 = (int64_t)g.gh[0] * g.gw[0];
    char* p = (char*)workspace;
    ToneSpace s;
    s.flags = (int32_t*)p;  p += (int64_t)n * 8;
    s.usum = (int64_t*)p;   p += (int64_t)n * g.upper * 48;
    s.l3 = (int32_t*)p;     p += (int64_t)n * g3 * 32;
    s.ucnt = (int32_t*)p;   p += (int64_t)n * g.upper * 8;
    s.uv = (int32_t*)p;     p += (int64_t)n * g.upper * 24;
    s.h3 = (int32_t*)p;
    return s;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                            // lane 0 holds the sum
}

// a wave per level-3 cell, a lane per pixel of it
__global__ __launch_bounds__(TN_THREADS) void k_tone_sets(const uint8_t* __restrict__ cmask, int H, int W, int r0, int r1, int gw3, int g3,
                                                          uint8_t* __restrict__ map, unsigned long long* __restrict__ counts,
                                                          int32_t* __restrict__ cells)
{
    const int cell = blockIdx.x * TN_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (cell >= g3) return;
    const int y = (cell / gw3) * 8 + (lane >> 3), x = (cell % gw3) * 8 + (lane & 7);
    uint32_t byte = 0;
    if (y < H && x < W) {
        const bool in = cmask[(int64_t)y * W + x] != 0;
        bool other = false;                                  // a pixel of the picture within TN_BAND that lies on the other side
        for (int dy = -TN_BAND; dy <= TN_BAND; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -TN_BAND; dx <= TN_BAND; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= W) continue;
                other |= (cmask[(int64_t)yy * W + xx] != 0) != in;
            }
        }
        const bool band = other && y >= r0 && y < r1;
        byte = (band && !in ? BIT_E : 0) | (band && in ? BIT_M : 0) | (in ? BIT_C : 0);
        map[(int64_t)y * W + x] = (uint8_t)byte;
    }
    const uint32_t ne = (uint32_t)__popcll(__ballot((byte & BIT_E) != 0)), nm = (uint32_t)__popcll(__ballot((byte & BIT_M) != 0));
    const bool any = __ballot(byte != 0) != 0;
    if (lane == 0 && any) {
        if (ne) atomicAdd(counts + 0, (unsigned long long)ne);
        if (nm) atomicAdd(counts + 1, (unsigned long long)nm);
        cells[atomicAdd(counts + 2, 1ull)] = cell;           // at most g3 cells arrive here
    }
}

// grid.x: the listed cells, a wave each; grid.y strides the frames
__global__ __launch_bounds__(TN_THREADS) void k_tone_cells(const uint8_t* __restrict__ frames, int64_t frame_stride,
                                                           const uint8_t* __restrict__ src, int64_t src_frame_stride,
                                                           const uint8_t* __restrict__ map, const int32_t* __restrict__ cells, int ncells,
                                                           int n, int H, int W, int y0, int rows, int gw3, int g3, ToneSpace ws)
{
    const int i = blockIdx.x * TN_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= ncells) return;
    const int cell = cells[i];
    uint32_t m = 0;
    int64_t at = 0;
    if (cell >= 0 && cell < g3) {
        const int y = (cell / gw3) * 8 + (lane >> 3), x = (cell % gw3) * 8 + (lane & 7);
        if (y < H && x < W && y >= y0 && y - y0 < rows) {
            m = map[(int64_t)y * W + x];
            at = ((int64_t)(y - y0) * W + x) * 3;
        }
    }
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* __restrict__ fill = frames + (int64_t)f * frame_stride + at;
        const uint8_t* __restrict__ s = src + (int64_t)f * src_frame_stride + at;
        uint32_t e01 = 0, e2n = 0, m01 = 0, m2n = 0;         // two 16-bit partial sums a word: a cell's sum stays below 64 * 255
        bool changed = false;
        if (m & BIT_E) {
            e01 = (uint32_t)s[0] | ((uint32_t)s[1] << 16);
            e2n = (uint32_t)s[2] | (1u << 16);
        }
        if (m & BIT_C) {
            const uint32_t f0 = fill[0], f1 = fill[1], f2 = fill[2];
            changed = f0 != s[0] || f1 != s[1] || f2 != s[2];
            if (m & BIT_M) {
                m01 = f0 | (f1 << 16);
                m2n = f2 | (1u << 16);
            }
        }
        e01 = wave_sum(e01);
        e2n = wave_sum(e2n);
        m01 = wave_sum(m01);
        m2n = wave_sum(m2n);
        const bool any_changed = __ballot(changed) != 0;
        if (lane == 0) {
            int32_t* rec = ws.l3 + ((int64_t)f * ncells + i) * 8;
            rec[0] = (int32_t)(e2n >> 16) | (any_changed ? 1 << 16 : 0);
            rec[1] = (int32_t)(m2n >> 16);
            rec[2] = (int32_t)(e01 & 0xffff);
            rec[3] = (int32_t)(e01 >> 16);
            rec[4] = (int32_t)(e2n & 0xffff);
            rec[5] = (int32_t)(m01 & 0xffff);
            rec[6] = (int32_t)(m01 >> 16);
            rec[7] = (int32_t)(m2n & 0xffff);
        }
    }
}

// (64 sum + N / 2) / N in 1/64 levels, 0 for an empty cell
__device__ __forceinline__ int64_t mean64(int64_t count, int64_t sum) { return count > 0 ? (64 * sum + count / 2) / count : 0; }

// the 2x bilinear upsample of the level above (v: [ph][pw][6]) at the centre of the cell (Y, X): 9/3/3/1, a numerator over 16
__device__ __forceinline__ void upsample(const int32_t* __restrict__ v, int ph, int pw, int Y, int X, int32_t* u)
{
    const int ya = Y >> 1, xa = X >> 1;
    const int yb = min(max(ya + ((Y & 1) ? 1 : -1), 0), ph - 1), xb = min(max(xa + ((X & 1) ? 1 : -1), 0), pw - 1);
    const int32_t* aa = v + ((int64_t)ya * pw + xa) * 6;
    const int32_t* ab = v + ((int64_t)ya * pw + xb) * 6;
    const int32_t* ba = v + ((int64_t)yb * pw + xa) * 6;
    const int32_t* bb = v + ((int64_t)yb * pw + xb) * 6;
#pragma unroll
    for (int j = 0; j < 6; ++j) u[j] = 9 * aa[j] + 3 * (ab[j] + ba[j]) + bb[j];
}

// V_k = (16 w mean_k + (T - w) U + 8 T) / (16 T), T = 2 * 2^k, w = min(N, T)
__device__ __forceinline__ int32_t blend(int64_t count, int64_t sum, int32_t u, int64_t T)
{
    const int64_t w = count < T ? count : T;
    return (int32_t)((16 * w * mean64(count, sum) + (T - w) * (int64_t)u + 8 * T) / (16 * T));
}

// One workgroup per frame.  Every phase ends in a barrier; what a phase reads, an earlier phase of this workgroup wrote.
__global__ __launch_bounds__(TN_LEVEL_THREADS) void k_tone_levels(const int32_t* __restrict__ cells, int ncells, ToneGeom g, ToneSpace ws)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    const int K = g.K, gw3 = g.gw[0];
    const int64_t g3 = (int64_t)g.gh[0] * gw3;
    int32_t* flags = ws.flags + (int64_t)f * 2;
    const int32_t* __restrict__ l3 = ws.l3 + (int64_t)f * ncells * 8;
    int64_t* usum = ws.usum + (int64_t)f * g.upper * 6;
    int32_t* ucnt = ws.ucnt + (int64_t)f * g.upper * 2;
    int32_t* uv = ws.uv + (int64_t)f * g.upper * 6;
    int32_t* h3 = ws.h3 + (int64_t)f * g3 * 3;

    // did the call inpaint the frame?
    int differs = 0;
    for (int i = tid; i < ncells; i += TN_LEVEL_THREADS) differs |= l3[(int64_t)i * 8] >> 16;
    const bool changed = __syncthreads_or(differs) != 0;

    // pull: level 3 -> 4 from the list, then level by level
    if (K > TN_FINEST) {
        const int gw4 = g.gw[1];
        const int64_t g4 = (int64_t)g.gh[1] * gw4;
        for (int64_t c = tid; c < g4; c += TN_LEVEL_THREADS) {
            ucnt[c * 2] = ucnt[c * 2 + 1] = 0;
#pragma unroll
            for (int j = 0; j < 6; ++j) usum[c * 6 + j] = 0;
        }
        __syncthreads();
        for (int i = tid; i < ncells; i += TN_LEVEL_THREADS) {
            const int cell = cells[i];
            if (cell < 0 || cell >= g3) continue;
            const int32_t* rec = l3 + (int64_t)i * 8;
            const int64_t p = (int64_t)((cell / gw3) >> 1) * gw4 + ((cell % gw3) >> 1);
            if (rec[0] & 0xffff) atomicAdd(ucnt + p * 2, rec[0] & 0xffff);
            if (rec[1]) atomicAdd(ucnt + p * 2 + 1, rec[1]);
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (rec[2 + j]) atomicAdd((unsigned long long*)(usum + p * 6 + j), (unsigned long long)rec[2 + j]);
        }
        __syncthreads();
        for (int k = TN_FINEST + 2; k <= K; ++k) {
            const int l = k - TN_FINEST, gh = g.gh[l], gw = g.gw[l], ch = g.gh[l - 1], cw = g.gw[l - 1];
            const int64_t cells_k = (int64_t)gh * gw, to = g.off[l], from = g.off[l - 1];
            for (int64_t c = tid; c < cells_k; c += TN_LEVEL_THREADS) {
                const int Y = (int)(c / gw), X = (int)(c % gw);
                int32_t cnt[2] = {0, 0};
                int64_t sum[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int cy = 2 * Y + (d >> 1), cx = 2 * X + (d & 1);
                    if (cy >= ch || cx >= cw) continue;      // a child that does not exist
                    const int64_t q = from + (int64_t)cy * cw + cx;
                    cnt[0] += ucnt[q * 2];
                    cnt[1] += ucnt[q * 2 + 1];
#pragma unroll
                    for (int j = 0; j < 6; ++j) sum[j] += usum[q * 6 + j];
                }
                ucnt[(to + c) * 2] = cnt[0];
                ucnt[(to + c) * 2 + 1] = cnt[1];
#pragma unroll
                for (int j = 0; j < 6; ++j) usum[(to + c) * 6 + j] = sum[j];
            }
            __syncthreads();
        }
    }

    // the top cell: is there anything to level?  (the same words for every thread: the whole workgroup stays or leaves)
    const int64_t top = g.off[K - TN_FINEST];
    int64_t top_e = 0, top_m = 0;
    if (K > TN_FINEST) {
        top_e = ucnt[top * 2];
        top_m = ucnt[top * 2 + 1];
    } else if (ncells > 0) {
        top_e = l3[0] & 0xffff;
        top_m = l3[1];
    }
    const bool touched = top_e > 0 && top_m > 0 && changed;
    if (tid == 0) {
        flags[0] = changed ? 1 : 0;
        flags[1] = touched ? 1 : 0;
    }
    if (!touched) return;

    // push: V_K = mean_K, then down to level 4
    if (K > TN_FINEST) {
        if (tid < 6) uv[top * 6 + tid] = (int32_t)mean64(tid < 3 ? top_e : top_m, usum[top * 6 + tid]);
        __syncthreads();
        for (int k = K - 1; k > TN_FINEST; --k) {
            const int l = k - TN_FINEST, gh = g.gh[l], gw = g.gw[l];
            const int64_t cells_k = (int64_t)gh * gw, at = g.off[l], T = 2ll << k;
            const int32_t* above = uv + g.off[l + 1] * 6;
            for (int64_t c = tid; c < cells_k; c += TN_LEVEL_THREADS) {
                int32_t u[6];
                upsample(above, g.gh[l + 1], g.gw[l + 1], (int)(c / gw), (int)(c % gw), u);
#pragma unroll
                for (int j = 0; j < 6; ++j) uv[(at + c) * 6 + j] = blend(ucnt[(at + c) * 2 + j / 3], usum[(at + c) * 6 + j], u[j], T);
            }
            __syncthreads();
        }
        // level 3, every cell as an empty one first: V_3 = (U + 8) / 16
        const int32_t* above = uv + g.off[1] * 6;
        for (int64_t c = tid; c < g3; c += TN_LEVEL_THREADS) {
            int32_t u[6];
            upsample(above, g.gh[1], g.gw[1], (int)(c / gw3), (int)(c % gw3), u);
#pragma unroll
            for (int j = 0; j < 3; ++j) h3[c * 3 + j] = min(max(((u[j] + 8) >> 4) - ((u[3 + j] + 8) >> 4), -TN_CLAMP), TN_CLAMP);
        }
        __syncthreads();
    }
    // ... then the listed cells with their own samples
    for (int i = tid; i < ncells; i += TN_LEVEL_THREADS) {
        const int cell = cells[i];
        if (cell < 0 || cell >= g3) continue;
        const int32_t* rec = l3 + (int64_t)i * 8;
        int32_t v[6];
        if (K > TN_FINEST) {
            int32_t u[6];
            upsample(uv + g.off[1] * 6, g.gh[1], g.gw[1], cell / gw3, cell % gw3, u);
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = blend(rec[j / 3] & 0xffff, rec[2 + j], u[j], 2ll << TN_FINEST);
        } else {
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = (int32_t)mean64(rec[j / 3] & 0xffff, rec[2 + j]);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) h3[(int64_t)cell * 3 + j] = min(max(v[j] - v[3 + j], -TN_CLAMP), TN_CLAMP);
    }
}

// grid.x strides the pixels of the local rows [la, lb) (the rows of C's bounding rows that the frames hold), grid.y the frames
__global__ __launch_bounds__(TN_THREADS) void k_tone_offset(uint8_t* __restrict__ frames, int64_t frame_stride, const uint8_t* __restrict__ map,
                                                            int n, int W, int y0, int la, int lb, int gh3, int gw3, int S, ToneSpace ws)
{
    const uint32_t npix = (uint32_t)(lb - la) * (uint32_t)W;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        if (!ws.flags[(int64_t)f * 2 + 1]) continue;          // the frame stays as it is
        const int32_t* __restrict__ h3 = ws.h3 + (int64_t)f * gh3 * gw3 * 3;
        uint8_t* __restrict__ dst = frames + (int64_t)f * frame_stride;
        for (uint32_t p = blockIdx.x * TN_THREADS + threadIdx.x; p < npix; p += gridDim.x * TN_THREADS) {
            const int ly = la + (int)(p / (uint32_t)W), x = (int)(p % (uint32_t)W), y = y0 + ly;
            if (!(map[(int64_t)y * W + x] & BIT_C)) continue;
            // the cell whose centre (8 X + 3.5) lies before the pixel, and the next: odd sixteenths, indices clamped
            const int cy = (y + 4) / 8 - 1, cx = (x + 4) / 8 - 1;
            const int wy1 = 2 * ((y + 4) & 7) + 1, wx1 = 2 * ((x + 4) & 7) + 1, wy0 = 16 - wy1, wx0 = 16 - wx1;
            const int ya = max(cy, 0), yb = min(cy + 1, gh3 - 1), xa = max(cx, 0), xb = min(cx + 1, gw3 - 1);
            const int32_t* aa = h3 + ((int64_t)ya * gw3 + xa) * 3;
            const int32_t* ab = h3 + ((int64_t)ya * gw3 + xb) * 3;
            const int32_t* ba = h3 + ((int64_t)yb * gw3 + xa) * 3;
            const int32_t* bb = h3 + ((int64_t)yb * gw3 + xb) * 3;
            uint8_t* px = dst + ((int64_t)ly * W + x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int h = wy0 * (wx0 * aa[c] + wx1 * ab[c]) + wy1 * (wx0 * ba[c] + wx1 * bb[c]);         // |h| <= 256 * 24 * 64
                const int num = S * h + TN_DEN / 2;
                int q = num / TN_DEN;
                if (num % TN_DEN < 0) --q;                   // floor
                if (q) px[c] = (uint8_t)min(255, max(0, (int)px[c] + q));
            }
        }
    }
}

int gfail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

const char* bad_picture(int H, int W)
{
    if (H <= 0 || W <= 0) return "tone match: H and W must be positive";
    if ((int64_t)H * W * 3 > 0x7fffffffll) return "tone match: a frame of H * W * 3 >= 2^31 bytes is not supported";
    return nullptr;
}

}  // namespace

extern "C" int vsr_tone_launch_sets(const uint8_t* cmask, int H, int W, int r0, int r1, uint8_t* map, uint64_t* counts, int32_t* cells,
                                    void* stream)
{
    if (hipMemsetAsync(counts, 0, 3 * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) return -1;
    const ToneGeom g = geometry(H, W);
    const int g3 = g.gh[0] * g.gw[0];                         // < 2^31 / 3 / 8
    hipLaunchKernelGGL(k_tone_sets, dim3((unsigned)((g3 + TN_WAVES - 1) / TN_WAVES)), dim3(TN_THREADS), 0, (hipStream_t)stream, cmask, H, W, r0,
                       r1, g.gw[0], g3, map, (unsigned long long*)counts, cells);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int vsr_tone_launch_apply(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride, const uint8_t* map,
                                     const int32_t* cells, int ncells, int n, int H, int W, int y0, int rows, int c0, int c1, int S,
                                     void* workspace, void* stream)
{
    const int la = c0 - y0 > 0 ? c0 - y0 : 0;
    const int lb = c1 - y0 < rows ? c1 - y0 : rows;
    if (lb <= la) return 0;                                  // the frames hold no pixel of the mask
    const ToneGeom g = geometry(H, W);
    const ToneSpace ws = carve(workspace, g, n);
    const int g3 = g.gh[0] * g.gw[0];
    const int gy = n < TN_MAX_GY ? n : TN_MAX_GY;
    hipLaunchKernelGGL(k_tone_cells, dim3((unsigned)((ncells + TN_WAVES - 1) / TN_WAVES), (unsigned)gy), dim3(TN_THREADS), 0, (hipStream_t)stream,
                       frames, frame_stride, src, src_frame_stride, map, cells, ncells, n, H, W, y0, rows, g.gw[0], g3, ws);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_tone_levels, dim3((unsigned)n), dim3(TN_LEVEL_THREADS), 0, (hipStream_t)stream, cells, ncells, g, ws);
    if (hipGetLastError() != hipSuccess) return -1;
    const int64_t blocks = ((int64_t)(lb - la) * W + TN_THREADS - 1) / TN_THREADS;
    hipLaunchKernelGGL(k_tone_offset, dim3((unsigned)(blocks < TN_MAX_GX ? blocks : TN_MAX_GX), (unsigned)gy), dim3(TN_THREADS), 0,
                       (hipStream_t)stream, frames, frame_stride, map, n, W, y0, la, lb, g.gh[0], g.gw[0], S, ws);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int vsr_tone_sets(const uint8_t* cmask_dev, int H, int W, int r0, int r1, uint8_t* map_dev, uint64_t* counts_dev, int32_t* cells_dev,
                  void* stream)
{
    if (!cmask_dev || !map_dev || !counts_dev || !cells_dev) return gfail(VSR_ERR_ARG, "tone match: null pointer");
    if (const char* why = bad_picture(H, W)) return gfail(VSR_ERR_ARG, why);
    if (r0 < 0 || r1 < r0 || r1 > H)
        return gfail(VSR_ERR_ARG, "tone match: sample rows [" + std::to_string(r0) + ", " + std::to_string(r1) + ") outside the frame");
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_tone_launch_sets(cmask_dev, H, W, r0, r1, map_dev, counts_dev, cells_dev, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("tone match sets launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

int64_t vsr_tone_workspace_bytes(int H, int W, int n)
{
    if (n < 0) return gfail(VSR_ERR_ARG, "tone match: negative frame count");
    if (const char* why = bad_picture(H, W)) return gfail(VSR_ERR_ARG, why);
    const int64_t per = frame_bytes(geometry(H, W));
    if (n > 0 && per > INT64_MAX / n) return gfail(VSR_ERR_ARG, "tone match: the workspace of so many frames has no size");
    return per * n;
}

int vsr_tone_apply(uint8_t* frames_dev, int64_t frame_stride, const uint8_t* src_dev, int64_t src_frame_stride, const uint8_t* map_dev,
                   const int32_t* cells_dev, int ncells, int n, int H, int W, int y0, int rows, int c0, int c1, int S, void* workspace_dev,
                   void* stream)
{
    if (!frames_dev || !src_dev || !map_dev || !cells_dev || !workspace_dev) return gfail(VSR_ERR_ARG, "tone match: null pointer");
    if (n < 0) return gfail(VSR_ERR_ARG, "tone match: negative frame count");
    if (const char* why = bad_picture(H, W)) return gfail(VSR_ERR_ARG, why);
    if (y0 < 0 || rows <= 0 || y0 > H - rows) return gfail(VSR_ERR_ARG, "tone match: the rows held must lie inside the frame");
    if (c0 < 0 || c1 < c0 || c1 > H) return gfail(VSR_ERR_ARG, "tone match: the mask's rows must lie inside the frame");
    if (S < 0 || S > TN_MAX_PERCENT)
        return gfail(VSR_ERR_ARG, "tone match: S = " + std::to_string(S) + ", 0 <= S <= " + std::to_string(TN_MAX_PERCENT) + " are possible");
    const int64_t N = (int64_t)rows * W * 3;
    if (frame_stride < N || src_frame_stride < N) return gfail(VSR_ERR_ARG, "tone match: frame stride smaller than a frame");
    if (ncells < 0 || ncells > (int64_t)((H + 7) / 8) * ((W + 7) / 8)) return gfail(VSR_ERR_ARG, "tone match: more cells listed than the picture has");
    if ((uintptr_t)workspace_dev % 8) return gfail(VSR_ERR_ARG, "tone match: the workspace must be 8-byte aligned");
    if (n == 0 || S == 0 || ncells == 0) return 0;
    if (n > 0 && frame_bytes(geometry(H, W)) > INT64_MAX / n) return gfail(VSR_ERR_ARG, "tone match: the workspace of so many frames has no size");
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_tone_launch_apply(frames_dev, frame_stride, src_dev, src_frame_stride, map_dev, cells_dev, ncells, n, H, W, y0, rows, c0, c1, S,
                              workspace_dev, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("tone match launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // extern "C"
