// --deflicker: the fill steadied over time inside the inpainted pixels, gated by how much the real picture around them moved
// (the statement is tests/_deflicker_statement.py).  All integer arithmetic.
//
//   k_deflicker_pairs   per frame t and k = 1..R (t + k < n): S[t][k] = sum over E (bit 0 of vsr_regrain_sets' map) and the channels of
//                       |src_t - src_{t+k}|.  Integer sums: whatever order the workgroups arrive in, the same numbers.
//   k_deflicker_apply   in place on the frames that hold the fill, reading a snapshot of the unsmoothed fill: per frame the pair weights
//                       a(t, k) in 0..16 from S, the stats of vsr_regrain_measure and |E| (one lane, on the device), then per pixel of C
//                       out = (16 TH fill_t + sum_s a (TH - D_s) fill_s + den / 2) / den over the neighbours s with D_s < TH.
//
// The frames hold `rows` rows of the picture starting at its row y0 (the whole picture, or sttn-auto's strip rows); the map is the
// whole picture's.  A frame is rows * W * 3 contiguous bytes at any alignment; frames, src and the snapshot have their own strides.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "plan_c.h"
#include "deflicker_kernels.h"

namespace {

constexpr int DF_RING = 16;              // E reaches this far from C (regrain_kernels.hip)
constexpr int DF_MAX_R = 8, DF_TH = 24, DF_FULL = 16;
constexpr uint64_t DF_GRAIN = 15447;     // round(2^16 * sqrt(2) / 6)
constexpr int DF_THREADS = 256, DF_WAVES = DF_THREADS / 64;
constexpr int DP_ROWS = 8;               // rows one lane of k_deflicker_pairs walks down its column
constexpr int DF_MAX_GY = 1024, DA_MAX_GX = 2048;
constexpr uint8_t BIT_E = 1, BIT_C = 4;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                            // lane 0 holds the sum
}

// grid.x: column tiles x row tiles over the local rows [la, lb) (the rows that can hold E); grid.y strides the frames.  A lane keeps
// its column's samples of frame t and meets the R frames behind it; a workgroup's sums stay below 2^21.
__global__ __launch_bounds__(DF_THREADS) void k_deflicker_pairs(const uint8_t* __restrict__ src, int64_t src_frame_stride,
                                                                const uint8_t* __restrict__ map, int n, int W, int y0, int la, int lb,
                                                                int col_tiles, int R, unsigned long long* __restrict__ pairs)
{
    __shared__ uint32_t part[DF_MAX_R][DF_WAVES];
    const int x = (blockIdx.x % col_tiles) * DF_THREADS + threadIdx.x;
    const int ly0 = la + (blockIdx.x / col_tiles) * DP_ROWS;
    uint32_t want = 0;
    if (x < W) {
#pragma unroll
        for (int i = 0; i < DP_ROWS; ++i) {
            const int ly = ly0 + i;
            if (ly >= lb) break;
            want |= (uint32_t)(map[(int64_t)(y0 + ly) * W + x] & BIT_E) << i;
        }
    }
    if (!__syncthreads_or(want != 0)) return;                // no sample in this tile (most tiles over the mask's own rows)
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const int kmax = R < n - 1 - f ? R : n - 1 - f;
        if (kmax <= 0) continue;
        const uint8_t* __restrict__ s = src + (int64_t)f * src_frame_stride;
        uint32_t mine[DP_ROWS];
#pragma unroll
        for (int i = 0; i < DP_ROWS; ++i) {
            mine[i] = 0;
            if ((want >> i) & 1u) {
                const uint8_t* p = s + ((int64_t)(ly0 + i) * W + x) * 3;
                mine[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
            }
        }
        for (int k = 1; k <= kmax; ++k) {
            const uint8_t* __restrict__ u = s + (int64_t)k * src_frame_stride;
            uint32_t sum = 0;
#pragma unroll
            for (int i = 0; i < DP_ROWS; ++i) {
                if ((want >> i) & 1u) {
                    const uint8_t* p = u + ((int64_t)(ly0 + i) * W + x) * 3;
                    sum += (uint32_t)abs((int)(mine[i] & 0xff) - (int)p[0]) + (uint32_t)abs((int)((mine[i] >> 8) & 0xff) - (int)p[1]) +
                           (uint32_t)abs((int)(mine[i] >> 16) - (int)p[2]);
                }
            }
            sum = wave_sum(sum);
            if ((threadIdx.x & 63) == 0) part[k - 1][threadIdx.x >> 6] = sum;
        }
        __syncthreads();
        if ((int)threadIdx.x < kmax) {
            uint32_t total = 0;
            for (int w = 0; w < DF_WAVES; ++w) total += part[threadIdx.x][w];
            if (total) atomicAdd(pairs + (int64_t)f * R + threadIdx.x, (unsigned long long)total);
        }
        __syncthreads();                                     // (part is written again for the next frame)
    }
}

// grid.x strides the pixels of the local rows [la, lb) (the rows of C's bounding rows that the frames hold; the snapshot's rows), grid.y
// the frames.  stats: vsr_regrain_measure's four words per frame (word 0 = A, word 2 = changed); counts[0] = |E|.
__global__ __launch_bounds__(DF_THREADS) void k_deflicker_apply(uint8_t* __restrict__ frames, int64_t frame_stride,
                                                                const uint8_t* __restrict__ snap, int64_t snap_stride,
                                                                const uint8_t* __restrict__ map, const unsigned long long* __restrict__ counts,
                                                                const unsigned long long* __restrict__ stats,
                                                                const unsigned long long* __restrict__ pairs, int n, int W, int y0, int la,
                                                                int lb, int R)
{
    __shared__ int s_w[2 * DF_MAX_R + 1];                    // s_w[j]: a(t, s) of the neighbour s = t - R + j; 0: takes no part
    __shared__ int s_any;
    const uint32_t npix = (uint32_t)(lb - la) * (uint32_t)W;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        __syncthreads();                                     // (the previous frame's values are read by now)
        if (threadIdx.x == 0) {
            const uint64_t m = 3 * (uint64_t)counts[0];
            const uint64_t a_t = stats[(int64_t)f * 4], changed_t = stats[(int64_t)f * 4 + 2];
            int any = 0;
            for (int j = 0; j <= 2 * R; ++j) {
                const int s = f - R + j;
                int a = 0;
                if (m && changed_t && s >= 0 && s < n && s != f && stats[(int64_t)s * 4 + 2]) {
                    const int lo = s < f ? s : f, k = s < f ? f - s : s - f;
                    const uint64_t sum = pairs[(int64_t)lo * R + (k - 1)];
                    const uint64_t floor = (DF_GRAIN * (a_t + (uint64_t)stats[(int64_t)s * 4])) >> 17;
                    const uint64_t moved = sum > floor ? sum - floor : 0;
                    if (moved < 4 * m) {
                        const uint64_t q = (DF_FULL * (4 * m - moved)) / (3 * m);
                        a = q < (uint64_t)DF_FULL ? (int)q : DF_FULL;
                    }
                }
                s_w[j] = a;
                any |= a;
            }
            s_any = any;
        }
        __syncthreads();
        if (!s_any) continue;                                // the frame stays as it is
        const uint8_t* __restrict__ own = snap + (int64_t)f * snap_stride;
        uint8_t* __restrict__ dst = frames + (int64_t)f * frame_stride;
        for (uint32_t p = blockIdx.x * DF_THREADS + threadIdx.x; p < npix; p += gridDim.x * DF_THREADS) {
            const uint32_t lr = p / (uint32_t)W, x = p % (uint32_t)W;            // lr: the row of the snapshot
            if (!(map[((uint32_t)(y0 + la) + lr) * (uint32_t)W + x] & BIT_C)) continue;     // (the index is < 2^31 / 3)
            const int64_t so = (int64_t)p * 3;
            const int b0 = own[so], b1 = own[so + 1], b2 = own[so + 2];
            uint32_t den = DF_FULL * DF_TH;
            uint32_t n0 = den * b0, n1 = den * b1, n2 = den * b2;
            for (int j = 0; j <= 2 * R; ++j) {
                const int a = s_w[j];
                if (a == 0) continue;
                const uint8_t* __restrict__ q = snap + (int64_t)(f - R + j) * snap_stride + so;
                const int v0 = q[0], v1 = q[1], v2 = q[2];
                const int d = max(max(abs(v0 - b0), abs(v1 - b1)), abs(v2 - b2));
                if (d >= DF_TH) continue;                    // other content at this pixel, not flicker
                const uint32_t w = (uint32_t)(a * (DF_TH - d));
                n0 += w * v0;
                n1 += w * v1;
                n2 += w * v2;
                den += w;
            }
            if (den == (uint32_t)(DF_FULL * DF_TH)) continue;                    // no neighbour: the pixel is the fill's
            uint8_t* px = dst + ((int64_t)la * W) * 3 + so;
            px[0] = (uint8_t)((n0 + den / 2) / den);
            px[1] = (uint8_t)((n1 + den / 2) / den);
            px[2] = (uint8_t)((n2 + den / 2) / den);
        }
    }
}

int gfail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

// the checks the two entry points share; nullptr = fine
const char* bad_geometry(int n, int H, int W, int y0, int rows, int c0, int c1, int R)
{
    if (n < 0) return "deflicker: negative frame count";
    if (H <= 0 || W <= 0) return "deflicker: H and W must be positive";
    if ((int64_t)H * W * 3 > 0x7fffffffll) return "deflicker: a frame of H * W * 3 >= 2^31 bytes is not supported";
    if (y0 < 0 || rows <= 0 || y0 > H - rows) return "deflicker: the rows held must lie inside the frame";
    if (c0 < 0 || c1 < c0 || c1 > H) return "deflicker: the mask's rows must lie inside the frame";
    if (R < 0 || R > DF_MAX_R) return "deflicker: R outside 0..8";
    return nullptr;
}

// the local rows of the frames that hold a row of [c0, c1): the snapshot's rows
inline void mask_rows(int y0, int rows, int c0, int c1, int* la, int* lb)
{
    *la = c0 - y0 > 0 ? c0 - y0 : 0;
    *lb = c1 - y0 < rows ? c1 - y0 : rows;
}

}  // namespace

extern "C" int vsr_deflicker_launch_pairs(const uint8_t* src, int64_t src_frame_stride, const uint8_t* map, int n, int W, int y0, int rows,
                                          int c0, int c1, int R, uint64_t* pairs, void* stream)
{
    if (hipMemsetAsync(pairs, 0, (size_t)n * R * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) return -1;
    // the local rows that can hold a sample: C's rows and the ring around them
    const int la = c0 - DF_RING - 1 - y0 > 0 ? c0 - DF_RING - 1 - y0 : 0;
    const int lb = c1 + DF_RING + 1 - y0 < rows ? c1 + DF_RING + 1 - y0 : rows;
    if (lb <= la || n < 2) return 0;
    const int col_tiles = (W + DF_THREADS - 1) / DF_THREADS, row_tiles = (lb - la + DP_ROWS - 1) / DP_ROWS;
    const dim3 grid((unsigned)(col_tiles * row_tiles), (unsigned)(n < DF_MAX_GY ? n : DF_MAX_GY));
    hipLaunchKernelGGL(k_deflicker_pairs, grid, dim3(DF_THREADS), 0, (hipStream_t)stream, src, src_frame_stride, map, n, W, y0, la, lb,
                       col_tiles, R, (unsigned long long*)pairs);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int vsr_deflicker_launch_apply(uint8_t* frames, int64_t frame_stride, const uint8_t* snap, int64_t snap_stride, const uint8_t* map,
                                          const uint64_t* counts, const uint64_t* stats, const uint64_t* pairs, int n, int W, int y0, int rows,
                                          int c0, int c1, int R, void* stream)
{
    int la, lb;
    mask_rows(y0, rows, c0, c1, &la, &lb);
    if (lb <= la || n < 2) return 0;
    const int64_t blocks = ((int64_t)(lb - la) * W + DF_THREADS - 1) / DF_THREADS;
    const int gy = n < DF_MAX_GY ? n : DF_MAX_GY;
    const dim3 grid((unsigned)(blocks < DA_MAX_GX ? blocks : DA_MAX_GX), (unsigned)gy);
    hipLaunchKernelGGL(k_deflicker_apply, grid, dim3(DF_THREADS), 0, (hipStream_t)stream, frames, frame_stride, snap, snap_stride, map,
                       (const unsigned long long*)counts, (const unsigned long long*)stats, (const unsigned long long*)pairs, n, W, y0, la,
                       lb, R);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int vsr_deflicker_pairs(const uint8_t* src_dev, int64_t src_frame_stride, const uint8_t* map_dev, int n, int H, int W, int y0, int rows,
                        int c0, int c1, int R, uint64_t* pairs_dev, void* stream)
{
    if (!src_dev || !map_dev || !pairs_dev) return gfail(VSR_ERR_ARG, "deflicker: null pointer");
    if (const char* why = bad_geometry(n, H, W, y0, rows, c0, c1, R)) return gfail(VSR_ERR_ARG, why);
    if (src_frame_stride < (int64_t)rows * W * 3) return gfail(VSR_ERR_ARG, "deflicker: frame stride smaller than a frame");
    if (n == 0 || R == 0) return 0;
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_deflicker_launch_pairs(src_dev, src_frame_stride, map_dev, n, W, y0, rows, c0, c1, R, pairs_dev, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("deflicker pairs launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

int vsr_deflicker_apply(uint8_t* frames_dev, int64_t frame_stride, const uint8_t* snap_dev, int64_t snap_stride, const uint8_t* map_dev,
                        const uint64_t* counts_dev, const uint64_t* stats_dev, const uint64_t* pairs_dev, int n, int H, int W, int y0,
                        int rows, int c0, int c1, int R, void* stream)
{
    if (!frames_dev || !snap_dev || !map_dev || !counts_dev || !stats_dev || !pairs_dev) return gfail(VSR_ERR_ARG, "deflicker: null pointer");
    if (const char* why = bad_geometry(n, H, W, y0, rows, c0, c1, R)) return gfail(VSR_ERR_ARG, why);
    if (frame_stride < (int64_t)rows * W * 3) return gfail(VSR_ERR_ARG, "deflicker: frame stride smaller than a frame");
    int la, lb;
    mask_rows(y0, rows, c0, c1, &la, &lb);
    if (lb > la && snap_stride < (int64_t)(lb - la) * W * 3)
        return gfail(VSR_ERR_ARG, "deflicker: snapshot stride smaller than the mask's rows of a frame");
    if (n == 0 || R == 0) return 0;
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_deflicker_launch_apply(frames_dev, frame_stride, snap_dev, snap_stride, map_dev, counts_dev, stats_dev, pairs_dev, n, W, y0, rows,
                                   c0, c1, R, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("deflicker apply launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // extern "C"
