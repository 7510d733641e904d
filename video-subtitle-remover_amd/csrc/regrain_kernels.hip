// --regrain: the source's grain, measured next to the mask, put back inside the inpainted pixels (the statement is
// tests/_regrain_statement.py).  All integer arithmetic.
//
//   k_regrain_sets      C (uint8 [H][W], non-zero = the plugin blends here) and the sample rows [r0, r1) -> a byte map of the frame:
//                       bit 0 = E (3x3 neighbourhood all outside C, within Chebyshev distance 16 of C), bit 1 = I (3x3 neighbourhood
//                       all inside C), both only at r0 + 1 <= y < r1 - 1, 1 <= x < W - 1; bit 2 = C != 0.  |E| and |I| are counted.
//                       Separable through LDS: flags of the tile and a 16-pixel halo, then rows, then columns.  Once per mask.
//   k_regrain_measure   per frame A_src = sum over E of L(src), A_fill = sum over I of L(fill), L = sum over the channels of
//                       |[[1,-2,1],[-2,4,-2],[1,-2,1]] * x|, and the number of pixels of C where fill != src.  Integer sums: whatever
//                       order the workgroups arrive in, the same numbers.
//   k_regrain_apply     in place on the frames that hold the fill: r = isqrt(max(0, q_src^2 - q_fill^2)) from the device stats, then
//                       fill + ((r * P * GAIN * z(y, x, seed) + 2^39) >> 40), clamped, on the pixels of C.
//
// The frames hold `rows` rows of the picture starting at its row y0 (the whole picture, or sttn-auto's strip rows); the map is the
// whole picture's.  A frame is rows * W * 3 contiguous bytes at any alignment, frames and src have their own strides.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "plan_c.h"
#include "regrain_kernels.h"

namespace {

constexpr int RG_RING = 16, RG_MAX_PERCENT = 200;
constexpr int64_t RG_GAIN = 60701;       // round(2^40 * (sqrt(pi / 2) / 6) / (sqrt(65535 / 3) * 100 * 256))
constexpr int RG_THREADS = 256, RG_WAVES = RG_THREADS / 64;
constexpr int RS_TX = 64, RS_TY = 32, RS_SW = RS_TX + 2 * RG_RING, RS_SH = RS_TY + 2 * RG_RING;
constexpr int RM_ROWS = 8;               // rows one lane of k_regrain_measure walks down its column
constexpr int RG_MAX_GY = 1024, RA_MAX_GX = 2048;
constexpr uint8_t BIT_E = 1, BIT_I = 2, BIT_C = 4;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                            // lane 0 holds the sum
}

// the sum over the workgroup, valid in thread 0; part: RG_WAVES words of LDS
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* part)
{
    v = wave_sum(v);
    __syncthreads();                     // (part may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < RG_WAVES; ++w) s += part[w];
    return s;
}

// One workgroup owns RS_TY x RS_TX pixels.  nz: C != 0 on the tile and RG_RING pixels around it (outside the frame: 0);
// hz: per row of nz, bit 0 = a non-zero within RG_RING along the row, bit 1 = x-1, x, x+1 all non-zero, bit 2 = all zero.
__global__ __launch_bounds__(RG_THREADS) void k_regrain_sets(const uint8_t* __restrict__ cmask, int H, int W, int r0, int r1,
                                                             uint8_t* __restrict__ map, unsigned long long* __restrict__ counts)
{
    __shared__ uint8_t nz[RS_SH * RS_SW];
    __shared__ uint8_t hz[RS_SH * RS_TX];
    __shared__ uint32_t part[RG_WAVES];
    const int x0 = blockIdx.x * RS_TX, y0 = blockIdx.y * RS_TY;
    for (int i = threadIdx.x; i < RS_SH * RS_SW; i += RG_THREADS) {
        const int y = y0 - RG_RING + i / RS_SW, x = x0 - RG_RING + i % RS_SW;
        nz[i] = (y >= 0 && y < H && x >= 0 && x < W && cmask[(int64_t)y * W + x] != 0) ? 1 : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RS_SH * RS_TX; i += RG_THREADS) {
        const uint8_t* row = nz + (i / RS_TX) * RS_SW + (i % RS_TX) + RG_RING;
        int any = 0;
#pragma unroll
        for (int k = -RG_RING; k <= RG_RING; ++k) any |= row[k];
        const int a = row[-1], b = row[0], c = row[1];
        hz[i] = (uint8_t)(any | ((a & b & c) << 1) | (((a | b | c) ^ 1) << 2));
    }
    __syncthreads();
    uint32_t ne = 0, ni = 0;
    for (int i = threadIdx.x; i < RS_TY * RS_TX; i += RG_THREADS) {
        const int ly = i / RS_TX, lx = i % RS_TX;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        const uint8_t* col = hz + (ly + RG_RING) * RS_TX + lx;
        int near = 0;
#pragma unroll
        for (int dy = -RG_RING; dy <= RG_RING; ++dy) near |= col[dy * RS_TX];
        const int three = col[-RS_TX] & col[0] & col[RS_TX];
        const bool inner = y >= r0 + 1 && y < r1 - 1 && x >= 1 && x < W - 1;
        const uint32_t e = inner && (three & 4) && (near & 1), in = inner && (three & 2);
        map[(int64_t)y * W + x] = (uint8_t)((e ? BIT_E : 0) | (in ? BIT_I : 0) | (nz[(ly + RG_RING) * RS_SW + lx + RG_RING] ? BIT_C : 0));
        ne += e;
        ni += in;
    }
    ne = block_sum(ne, part);
    ni = block_sum(ni, part);
    if (threadIdx.x == 0) {
        if (ne) atomicAdd(counts + 0, (unsigned long long)ne);
        if (ni) atomicAdd(counts + 1, (unsigned long long)ni);
    }
}

// sum of L(img) over the rows ly0 + i (bit i of `want`) of column x: the second difference along the row is kept for three rows
// (before, at, after) and differenced again down the column.  A wanted row has all nine neighbours inside the rows held.
__device__ __forceinline__ uint32_t level_column(const uint8_t* __restrict__ img, int W, int ly0, int x, uint32_t want)
{
    uint32_t sum = 0;
    int before[3] = {0, 0, 0}, at[3] = {0, 0, 0};
#pragma unroll
    for (int j = -1; j <= RM_ROWS; ++j) {
        int after[3] = {0, 0, 0};
        if (((want << 2) >> (j + 1)) & 7u) {                 // row j is a neighbour of, or is, a wanted row
            const uint8_t* p = img + ((int64_t)(ly0 + j) * W + x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) after[c] = (int)p[c - 3] - 2 * (int)p[c] + (int)p[c + 3];
        }
        if (j >= 1 && ((want >> (j - 1)) & 1u)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sum += (uint32_t)abs(before[c] - 2 * at[c] + after[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { before[c] = at[c]; at[c] = after[c]; }
    }
    return sum;
}

// stats: per frame four 64-bit words: A_src, A_fill, the number of pixels of C with fill != src, unused.
// grid.x: column tiles x row tiles over the local rows [la, lb); grid.y strides the frames.  A workgroup's sums stay below 2^25.
__global__ __launch_bounds__(RG_THREADS) void k_regrain_measure(const uint8_t* __restrict__ frames, int64_t frame_stride,
                                                                const uint8_t* __restrict__ src, int64_t src_frame_stride,
                                                                const uint8_t* __restrict__ map, int n, int W, int y0, int rows, int la, int lb,
                                                                int col_tiles, unsigned long long* __restrict__ stats)
{
    __shared__ uint32_t part[RG_WAVES];
    const int x = (blockIdx.x % col_tiles) * RG_THREADS + threadIdx.x;
    const int ly0 = la + (blockIdx.x / col_tiles) * RM_ROWS;
    uint32_t want_e = 0, want_i = 0, want_c = 0;
    if (x < W) {
        const bool xin = x >= 1 && x < W - 1;
#pragma unroll
        for (int i = 0; i < RM_ROWS; ++i) {
            const int ly = ly0 + i;
            if (ly >= lb) break;
            const uint32_t m = map[(int64_t)(y0 + ly) * W + x];
            const bool fits = xin && ly >= 1 && ly < rows - 1;                  // (the map says so already: E and I lie in `inner`)
            want_e |= (uint32_t)(fits && (m & BIT_E)) << i;
            want_i |= (uint32_t)(fits && (m & BIT_I)) << i;
            want_c |= (uint32_t)((m & BIT_C) != 0) << i;
        }
    }
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* __restrict__ fill = frames + (int64_t)f * frame_stride;
        const uint8_t* __restrict__ s = src + (int64_t)f * src_frame_stride;
        uint32_t a_src = want_e ? level_column(s, W, ly0, x, want_e) : 0u;
        uint32_t a_fill = want_i ? level_column(fill, W, ly0, x, want_i) : 0u;
        uint32_t changed = 0;
#pragma unroll
        for (int i = 0; i < RM_ROWS; ++i) {
            if ((want_c >> i) & 1u) {
                const int64_t o = ((int64_t)(ly0 + i) * W + x) * 3;
                changed += (fill[o] != s[o]) | (fill[o + 1] != s[o + 1]) | (fill[o + 2] != s[o + 2]);
            }
        }
        a_src = block_sum(a_src, part);
        a_fill = block_sum(a_fill, part);
        changed = block_sum(changed, part);
        if (threadIdx.x == 0) {
            unsigned long long* st = stats + (int64_t)f * 4;
            if (a_src) atomicAdd(st + 0, (unsigned long long)a_src);
            if (a_fill) atomicAdd(st + 1, (unsigned long long)a_fill);
            if (changed) atomicAdd(st + 2, (unsigned long long)changed);
        }
    }
}

__device__ __forceinline__ uint64_t isqrt64(uint64_t v)       // floor(sqrt(v)), v < 2^52: a float estimate, corrected in integers
{
    uint64_t r = (uint64_t)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

__device__ __forceinline__ uint32_t mix32(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

// grid.x strides the pixels of the local rows [la, lb) (the rows of C's bounding rows that the frames hold), grid.y the frames
__global__ __launch_bounds__(RG_THREADS) void k_regrain_apply(uint8_t* __restrict__ frames, int64_t frame_stride, const uint8_t* __restrict__ map,
                                                              const unsigned long long* __restrict__ counts,
                                                              const unsigned long long* __restrict__ stats, int n, int W, int y0, int la, int lb,
                                                              int percent)
{
    __shared__ int64_t s_gain;
    __shared__ uint32_t s_seed;
    const uint32_t npix = (uint32_t)(lb - la) * (uint32_t)W;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        __syncthreads();                                     // (the previous frame's values are read by now)
        if (threadIdx.x == 0) {
            const uint64_t ne = counts[0], ni = counts[1];
            const uint64_t* st = (const uint64_t*)(stats + (int64_t)f * 4);
            int64_t gain = 0;
            if (ne && ni && st[2]) {
                const uint64_t qs = (st[0] << 8) / (3 * ne), qf = (st[1] << 8) / (3 * ni);
                const uint64_t r = qs > qf ? isqrt64(qs * qs - qf * qf) : 0;
                gain = (int64_t)r * percent * RG_GAIN;       // < 2^20 * 2^8 * 2^16
            }
            s_gain = gain;
            s_seed = (uint32_t)st[0] ^ (uint32_t)(st[0] >> 32);
        }
        __syncthreads();
        const int64_t gain = s_gain;
        if (gain == 0) continue;                             // the frame stays as it is
        const uint32_t seed = s_seed;
        uint8_t* __restrict__ dst = frames + (int64_t)f * frame_stride;
        for (uint32_t p = blockIdx.x * RG_THREADS + threadIdx.x; p < npix; p += gridDim.x * RG_THREADS) {
            const uint32_t ly = (uint32_t)la + p / (uint32_t)W, x = p % (uint32_t)W;
            const uint32_t at = ((uint32_t)y0 + ly) * (uint32_t)W + x;           // < 2^31 / 3
            if (!(map[at] & BIT_C)) continue;
            const uint32_t h = mix32(mix32(at ^ seed) + 0x9e3779b9u);
            const int z = (int)((h & 0xff) + ((h >> 8) & 0xff) + ((h >> 16) & 0xff) + (h >> 24)) - 510;
            const int g = (int)((gain * z + (1ll << 39)) >> 40);
            if (g == 0) continue;
            uint8_t* px = dst + ((int64_t)ly * W + x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = (uint8_t)min(255, max(0, (int)px[c] + g));
        }
    }
}

int gfail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

// the checks the three entry points share; nullptr = fine
const char* bad_geometry(int n, int H, int W, int y0, int rows, int c0, int c1)
{
    if (n < 0) return "regrain: negative frame count";
    if (H <= 0 || W <= 0) return "regrain: H and W must be positive";
    if ((int64_t)H * W * 3 > 0x7fffffffll) return "regrain: a frame of H * W * 3 >= 2^31 bytes is not supported";
    if (y0 < 0 || rows <= 0 || y0 > H - rows) return "regrain: the rows held must lie inside the frame";
    if (c0 < 0 || c1 < c0 || c1 > H) return "regrain: the mask's rows must lie inside the frame";
    return nullptr;
}

}  // namespace

extern "C" int vsr_regrain_launch_sets(const uint8_t* cmask, int H, int W, int r0, int r1, uint8_t* map, uint64_t* counts, void* stream)
{
    if (hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) return -1;
    const dim3 grid((W + RS_TX - 1) / RS_TX, (H + RS_TY - 1) / RS_TY);
    hipLaunchKernelGGL(k_regrain_sets, grid, dim3(RG_THREADS), 0, (hipStream_t)stream, cmask, H, W, r0, r1, map, (unsigned long long*)counts);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int vsr_regrain_launch_measure(const uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride,
                                          const uint8_t* map, int n, int W, int y0, int rows, int c0, int c1, uint64_t* stats, void* stream)
{
    if (hipMemsetAsync(stats, 0, (size_t)n * 4 * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) return -1;
    // the local rows that can hold a sample or a pixel of C: C's rows and the ring (and its 3x3 neighbourhoods) around them
    const int la = c0 - RG_RING - 1 - y0 > 0 ? c0 - RG_RING - 1 - y0 : 0;
    const int lb = c1 + RG_RING + 1 - y0 < rows ? c1 + RG_RING + 1 - y0 : rows;
    if (lb <= la) return 0;
    const int col_tiles = (W + RG_THREADS - 1) / RG_THREADS, row_tiles = (lb - la + RM_ROWS - 1) / RM_ROWS;
    const dim3 grid((unsigned)(col_tiles * row_tiles), (unsigned)(n < RG_MAX_GY ? n : RG_MAX_GY));
    hipLaunchKernelGGL(k_regrain_measure, grid, dim3(RG_THREADS), 0, (hipStream_t)stream, frames, frame_stride, src, src_frame_stride, map, n, W,
                       y0, rows, la, lb, col_tiles, (unsigned long long*)stats);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int vsr_regrain_launch_apply(uint8_t* frames, int64_t frame_stride, const uint8_t* map, const uint64_t* counts, const uint64_t* stats,
                                        int n, int W, int y0, int rows, int c0, int c1, int percent, void* stream)
{
    const int la = c0 - y0 > 0 ? c0 - y0 : 0;
    const int lb = c1 - y0 < rows ? c1 - y0 : rows;
    if (lb <= la) return 0;
    const int64_t blocks = ((int64_t)(lb - la) * W + RG_THREADS - 1) / RG_THREADS;
    const int gy = n < RG_MAX_GY ? n : RG_MAX_GY;
    const dim3 grid((unsigned)(blocks < RA_MAX_GX ? blocks : RA_MAX_GX), (unsigned)gy);
    hipLaunchKernelGGL(k_regrain_apply, grid, dim3(RG_THREADS), 0, (hipStream_t)stream, frames, frame_stride, map,
                       (const unsigned long long*)counts, (const unsigned long long*)stats, n, W, y0, la, lb, percent);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int vsr_regrain_sets(const uint8_t* cmask_dev, int H, int W, int r0, int r1, uint8_t* map_dev, uint64_t* counts_dev, void* stream)
{
    if (!cmask_dev || !map_dev || !counts_dev) return gfail(VSR_ERR_ARG, "regrain: null pointer");
    if (const char* why = bad_geometry(0, H, W, 0, 1, 0, 0)) return gfail(VSR_ERR_ARG, why);
    if (r0 < 0 || r1 < r0 || r1 > H)
        return gfail(VSR_ERR_ARG, "regrain: sample rows [" + std::to_string(r0) + ", " + std::to_string(r1) + ") outside the frame");
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_regrain_launch_sets(cmask_dev, H, W, r0, r1, map_dev, counts_dev, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("regrain sets launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

int vsr_regrain_measure(const uint8_t* frames_dev, int64_t frame_stride, const uint8_t* src_dev, int64_t src_frame_stride,
                        const uint8_t* map_dev, int n, int H, int W, int y0, int rows, int c0, int c1, uint64_t* stats_dev, void* stream)
{
    if (!frames_dev || !src_dev || !map_dev || !stats_dev) return gfail(VSR_ERR_ARG, "regrain: null pointer");
    if (const char* why = bad_geometry(n, H, W, y0, rows, c0, c1)) return gfail(VSR_ERR_ARG, why);
    const int64_t N = (int64_t)rows * W * 3;
    if (frame_stride < N || src_frame_stride < N) return gfail(VSR_ERR_ARG, "regrain: frame stride smaller than a frame");
    if (n == 0) return 0;
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_regrain_launch_measure(frames_dev, frame_stride, src_dev, src_frame_stride, map_dev, n, W, y0, rows, c0, c1, stats_dev, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("regrain measure launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

int vsr_regrain_apply(uint8_t* frames_dev, int64_t frame_stride, const uint8_t* map_dev, const uint64_t* counts_dev, const uint64_t* stats_dev,
                      int n, int H, int W, int y0, int rows, int c0, int c1, int percent, void* stream)
{
    if (!frames_dev || !map_dev || !counts_dev || !stats_dev) return gfail(VSR_ERR_ARG, "regrain: null pointer");
    if (const char* why = bad_geometry(n, H, W, y0, rows, c0, c1)) return gfail(VSR_ERR_ARG, why);
    if (percent < 0 || percent > RG_MAX_PERCENT)
        return gfail(VSR_ERR_ARG, "regrain: P = " + std::to_string(percent) + ", 0 <= P <= " + std::to_string(RG_MAX_PERCENT) + " are possible");
    if (frame_stride < (int64_t)rows * W * 3) return gfail(VSR_ERR_ARG, "regrain: frame stride smaller than a frame");
    if (n == 0 || percent == 0) return 0;
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_regrain_launch_apply(frames_dev, frame_stride, map_dev, counts_dev, stats_dev, n, W, y0, rows, c0, c1, percent, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("regrain apply launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // extern "C"
