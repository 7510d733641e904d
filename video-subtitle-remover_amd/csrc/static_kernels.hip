// --logo-scan: where an edge pattern stays put while the picture around it moves (the statement is
// tests/_static_statement.py).  Integer arithmetic only; the host (backend/tools/logo_scan.py) labels the grown map with
// vsr_det_launch_ccl and chooses the components.
//
//   k_static_accum     per tile of 64 columns x 32 rows, ONE workgroup for all n sampled frames: per frame the luma
//                      Y = (29 B + 150 G + 77 R + 128) >> 8 of the tile and a one-pixel halo into LDS -- the halo's coordinates clamp at the
//                      frame's borders, not at the tile's, so a gradient across a tile seam reads the neighbour's pixel -- then per pixel
//                      g = |Y[y][x + 1] - Y[y][x - 1]| + |Y[y + 1][x] - Y[y - 1][x]| from LDS.  A thread owns 8 pixels (one column, 8 rows)
//                      and keeps their lo = min Y, hi = max Y and e = #(g >= ge) in registers across the frames; the state planes are
//                      read (first == 0) and written once per launch.  Two LDS tiles alternate, so a frame costs one barrier, and the
//                      next frame's bytes are fetched into registers in front of that barrier, so they travel under this frame's sums.
//                      A frame's bytes are read once but for the halo (34 x 66 lumas per 32 x 64 pixels, served by the caches).
//   k_static_classify  per tile of 64 x 32: seed = edges >= need of the tile and a halo of `grow` pixels (outside the frame: 0) in LDS, the
//                      OR over 2 grow + 1 columns, then over 2 grow + 1 rows: the seeds dilated by `grow` pixels of Chebyshev distance,
//                      written as 1.0f / 0.0f for vsr_det_launch_ccl; and moving = hi - lo >= mv.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "plan_c.h"
#include "static_kernels.h"

namespace {

constexpr int ST_THREADS = 256, ST_WAVES = ST_THREADS / 64, ST_TW = 64, ST_TH = 32, ST_PER = ST_TH / ST_WAVES;   // rows of a tile: 8 per wave
constexpr int ST_YROWS = ST_TH + 2, ST_YCOLS = ST_TW + 2, ST_YPITCH = 68;       // the luma tile with its halo; a row padded to whole dwords
constexpr int ST_FILL = (ST_YROWS * ST_YCOLS + ST_THREADS - 1) / ST_THREADS;   // lumas of the tile and its halo a thread stages per frame
constexpr int ST_MAX_GROW = 16, ST_MAX_N = 65535;
constexpr int ST_SROWS = ST_TH + 2 * ST_MAX_GROW, ST_SCOLS = ST_TW + 2 * ST_MAX_GROW;

// grid.x: tiles of 64 columns, grid.y: tiles of 32 rows
__global__ __launch_bounds__(ST_THREADS) void k_static_accum(const uint8_t* __restrict__ frames, int64_t frame_stride, const int32_t* __restrict__ idx,
                                                             int n, int H, int W, int ge, int first, uint8_t* __restrict__ lo_p,
                                                             uint8_t* __restrict__ hi_p, uint16_t* __restrict__ edges_p)
{
    __shared__ uint8_t Y[2][ST_YROWS * ST_YPITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * ST_TW, y0 = blockIdx.y * ST_TH;
    const int x = x0 + lane, yt = y0 + wave * ST_PER;                           // this thread's column and its first row
    int lo[ST_PER], hi[ST_PER], e[ST_PER];
#pragma unroll
    for (int j = 0; j < ST_PER; ++j) {
        lo[j] = 255, hi[j] = 0, e[j] = 0;
        if (!first && x < W && yt + j < H) {
            const int64_t at = (int64_t)(yt + j) * W + x;
            lo[j] = lo_p[at], hi[j] = hi_p[at], e[j] = edges_p[at];
        }
    }
    // the lumas this thread stages: their place in a frame (the same in every frame; H * W * 3 < 2^31) and in the LDS tile; -1: none
    int from[ST_FILL], to[ST_FILL], raw[ST_FILL][3];
#pragma unroll
    for (int s = 0; s < ST_FILL; ++s) {
        const int i = tid + s * ST_THREADS;
        const int ry = i / ST_YCOLS, rx = i - ry * ST_YCOLS;
        const int gy = min(max(y0 - 1 + ry, 0), H - 1), gx = min(max(x0 - 1 + rx, 0), W - 1);
        from[s] = (gy * W + gx) * 3, to[s] = i < ST_YROWS * ST_YCOLS ? ry * ST_YPITCH + rx : -1;
    }
    auto fetch = [&](int k) {                                                   // frame k's bytes into registers; nothing waits for them here
        const uint8_t* __restrict__ fp = frames + (int64_t)idx[k] * frame_stride;
#pragma unroll
        for (int s = 0; s < ST_FILL; ++s)
            if (to[s] >= 0) raw[s][0] = fp[from[s]], raw[s][1] = fp[from[s] + 1], raw[s][2] = fp[from[s] + 2];
    };
    fetch(0);
    for (int k = 0; k < n; ++k) {
        uint8_t* __restrict__ Yk = Y[k & 1];
#pragma unroll
        for (int s = 0; s < ST_FILL; ++s)
            if (to[s] >= 0) Yk[to[s]] = (uint8_t)((29 * raw[s][0] + 150 * raw[s][1] + 77 * raw[s][2] + 128) >> 8);
        if (k + 1 < n) fetch(k + 1);                                            // the next frame travels under this frame's sums
        __syncthreads();                                                        // (the other tile is free: every thread has passed frame k - 1's sums)
        const uint8_t* q = Yk + (wave * ST_PER + 1) * ST_YPITCH + lane + 1;    // this thread's first pixel
#pragma unroll
        for (int j = 0; j < ST_PER; ++j, q += ST_YPITCH) {
            const int c = q[0];
            const int g = abs((int)q[1] - (int)q[-1]) + abs((int)q[ST_YPITCH] - (int)q[-ST_YPITCH]);
            lo[j] = min(lo[j], c), hi[j] = max(hi[j], c), e[j] += g >= ge;
        }
    }
    if (x >= W) return;
#pragma unroll
    for (int j = 0; j < ST_PER; ++j) {
        if (yt + j >= H) break;
        const int64_t at = (int64_t)(yt + j) * W + x;
        lo_p[at] = (uint8_t)lo[j], hi_p[at] = (uint8_t)hi[j], edges_p[at] = (uint16_t)min(e[j], 65535);
    }
}

// grid.x: tiles of 64 columns, grid.y: tiles of 32 rows; 0 <= grow <= ST_MAX_GROW
__global__ __launch_bounds__(ST_THREADS) void k_static_classify(const uint8_t* __restrict__ lo_p, const uint8_t* __restrict__ hi_p,
                                                                const uint16_t* __restrict__ edges_p, int H, int W, int need, int mv, int grow,
                                                                float* __restrict__ grown, uint8_t* __restrict__ moving)
{
    __shared__ uint8_t S[ST_SROWS * ST_SCOLS];              // the seeds of the tile and its halo, pitch ST_TW + 2 grow
    __shared__ uint8_t R[ST_SROWS * ST_TW];                 // the same rows, every seed spread over 2 grow + 1 columns
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * ST_TW, y0 = blockIdx.y * ST_TH;
    const int srows = ST_TH + 2 * grow, scols = ST_TW + 2 * grow;
    for (int i = tid; i < srows * scols; i += ST_THREADS) {
        const int ry = i / scols, rx = i - ry * scols;
        const int y = y0 - grow + ry, x = x0 - grow + rx;
        S[i] = (y >= 0 && y < H && x >= 0 && x < W && (int)edges_p[(int64_t)y * W + x] >= need) ? 1 : 0;
    }
    __syncthreads();
    for (int i = tid; i < srows * ST_TW; i += ST_THREADS) {
        const int ry = i / ST_TW, cx = i - ry * ST_TW;
        const uint8_t* s = S + ry * scols + cx;             // the column cx - grow of the picture's tile
        int any = 0;
        for (int d = 0; d <= 2 * grow; ++d) any |= s[d];
        R[i] = (uint8_t)any;
    }
    __syncthreads();
    const int x = x0 + lane;
    if (x >= W) return;
    for (int j = 0; j < ST_PER; ++j) {
        const int ry = wave * ST_PER + j, y = y0 + ry;
        if (y >= H) break;
        int any = 0;
        for (int d = 0; d <= 2 * grow; ++d) any |= R[(ry + d) * ST_TW + lane];
        const int64_t at = (int64_t)y * W + x;
        grown[at] = any ? 1.0f : 0.0f;
        moving[at] = ((int)hi_p[at] - (int)lo_p[at] >= mv) ? 1 : 0;
    }
}

int sfail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

const char* bad_picture(int H, int W)
{
    if (H <= 0 || W <= 0) return "logo scan: H and W must be positive";
    if ((int64_t)H * W * 3 > 0x7fffffffll) return "logo scan: a frame of H * W * 3 >= 2^31 bytes is not supported";
    return nullptr;
}

dim3 tiles(int H, int W) { return dim3((unsigned)((W + ST_TW - 1) / ST_TW), (unsigned)((H + ST_TH - 1) / ST_TH)); }

}  // namespace

extern "C" int vsr_static_accum_launch(const uint8_t* frames, int64_t frame_stride, const int32_t* idx, int n, int H, int W, int ge, int first,
                                       uint8_t* lo, uint8_t* hi, uint16_t* edges, void* stream)
{
    hipLaunchKernelGGL(k_static_accum, tiles(H, W), dim3(ST_THREADS), 0, (hipStream_t)stream, frames, frame_stride, idx, n, H, W, ge, first, lo, hi,
                       edges);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int vsr_static_classify_launch(const uint8_t* lo, const uint8_t* hi, const uint16_t* edges, int H, int W, int need, int mv, int grow,
                                          float* grown, uint8_t* moving, void* stream)
{
    hipLaunchKernelGGL(k_static_classify, tiles(H, W), dim3(ST_THREADS), 0, (hipStream_t)stream, lo, hi, edges, H, W, need, mv, grow, grown, moving);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int vsr_static_accum(const uint8_t* frames_dev, int64_t frame_stride, const int32_t* idx_dev, int n, int H, int W, int ge, int first,
                     uint8_t* lo_dev, uint8_t* hi_dev, uint16_t* edges_dev, void* stream)
{
    if (!frames_dev || !idx_dev || !lo_dev || !hi_dev || !edges_dev) return sfail(VSR_ERR_ARG, "logo scan: null pointer");
    if (n < 1 || n > ST_MAX_N)
        return sfail(VSR_ERR_ARG, "logo scan: n = " + std::to_string(n) + " frames, 1 <= n <= " + std::to_string(ST_MAX_N) + " are possible");
    if (const char* why = bad_picture(H, W)) return sfail(VSR_ERR_ARG, why);
    if (ge < 0 || ge > 510) return sfail(VSR_ERR_ARG, "logo scan: ge = " + std::to_string(ge) + ", a gradient lies in 0..510");
    if (first != 0 && first != 1) return sfail(VSR_ERR_ARG, "logo scan: first must be 0 or 1");
    if (frame_stride < (int64_t)H * W * 3) return sfail(VSR_ERR_ARG, "logo scan: frame stride smaller than a frame");
    if ((uintptr_t)edges_dev % 2 || (uintptr_t)idx_dev % 4) return sfail(VSR_ERR_ARG, "logo scan: the edge plane or the frame numbers are misaligned");
    if (vsr_device_count() <= 0) return sfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_static_accum_launch(frames_dev, frame_stride, idx_dev, n, H, W, ge, first, lo_dev, hi_dev, edges_dev, stream) != 0)
        return sfail(VSR_ERR_HIP, std::string("logo scan accumulate launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

int vsr_static_classify(const uint8_t* lo_dev, const uint8_t* hi_dev, const uint16_t* edges_dev, int H, int W, int need, int mv, int grow,
                        float* grown_dev, uint8_t* moving_dev, void* stream)
{
    if (!lo_dev || !hi_dev || !edges_dev || !grown_dev || !moving_dev) return sfail(VSR_ERR_ARG, "logo scan: null pointer");
    if (const char* why = bad_picture(H, W)) return sfail(VSR_ERR_ARG, why);
    if (need < 0 || need > 65536) return sfail(VSR_ERR_ARG, "logo scan: need = " + std::to_string(need) + ", 0 <= need <= 65536 are possible");
    if (mv < 0 || mv > 256) return sfail(VSR_ERR_ARG, "logo scan: mv = " + std::to_string(mv) + ", 0 <= mv <= 256 are possible");
    if (grow < 0 || grow > ST_MAX_GROW)
        return sfail(VSR_ERR_ARG, "logo scan: grow = " + std::to_string(grow) + ", 0 <= grow <= " + std::to_string(ST_MAX_GROW) + " are possible");
    if ((uintptr_t)edges_dev % 2 || (uintptr_t)grown_dev % 4) return sfail(VSR_ERR_ARG, "logo scan: the edge plane or the grown map is misaligned");
    if (vsr_device_count() <= 0) return sfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_static_classify_launch(lo_dev, hi_dev, edges_dev, H, W, need, mv, grow, grown_dev, moving_dev, stream) != 0)
        return sfail(VSR_ERR_HIP, std::string("logo scan classify launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // extern "C"
