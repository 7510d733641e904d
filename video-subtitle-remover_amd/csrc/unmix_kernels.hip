// --logo-unblend: a translucent overlay I = (1 - a) B + a L is un-mixed, B = (I - o) / g (the statement is
// tests/_unmix_statement.py).  Integer arithmetic only; the host (backend/tools/unblend.py) solves for the planes g and o between the two.
//
//   k_unmix_accum  the moments S1 = sum F and S2 = sum F^2 of every byte of Gbox (an area grown by its ring) over the n sampled frames.
//                  A row of Gbox is 3 gw consecutive bytes of a frame and the same run of the planes, so the kernel works on bytes: a
//                  workgroup owns 256 byte columns x 4 rows for ALL n frames, a thread one byte column and its 4 rows; the 8 sums stay in
//                  registers, the planes are read (first == 0) and written once per launch, no atomics.  The next frame's bytes are
//                  fetched in front of this frame's sums, so they travel under them.
//   k_unmix_apply  per pixel of the box inside the rows held, per frame: g < 64 (opaque) writes nothing; else per channel
//                  num = 256 (16 I - o), den = 16 g, out = 0 if num < 0 else min(255, (num + den / 2) / den) by the integer divide, read
//                  from src and written to frames at the same place -- a thread reads its pixel before it writes it, so src == frames works.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "plan_c.h"
#include "unmix_kernels.h"

namespace {

constexpr int UM_THREADS = 256, UM_ROWS = 4, UM_MAX_N = 65535, UM_GMIN = 64;

// grid.x: runs of 256 bytes of a row of Gbox, grid.y: runs of 4 rows; row_bytes = 3 (gx1 - gx0)
__global__ __launch_bounds__(UM_THREADS) void k_unmix_accum(const uint8_t* __restrict__ frames, int64_t frame_stride, const int32_t* __restrict__ idx,
                                                            int n, int W, int gy0, int gh, int gx0, int row_bytes, int first,
                                                            uint32_t* __restrict__ S1, uint32_t* __restrict__ S2)
{
    const int j = blockIdx.x * UM_THREADS + threadIdx.x, r0 = blockIdx.y * UM_ROWS;
    if (j >= row_bytes) return;
    uint32_t s1[UM_ROWS], s2[UM_ROWS];
    int from[UM_ROWS];                                                          // the byte's place in a frame (H * W * 3 < 2^31); -1: no such row
#pragma unroll
    for (int r = 0; r < UM_ROWS; ++r) {
        const bool in = r0 + r < gh;
        from[r] = in ? ((gy0 + r0 + r) * W + gx0) * 3 + j : -1;
        s1[r] = s2[r] = 0;
        if (in && !first) {
            const int64_t at = (int64_t)(r0 + r) * row_bytes + j;
            s1[r] = S1[at], s2[r] = S2[at];
        }
    }
    uint32_t raw[UM_ROWS];
    auto fetch = [&](int k) {
        const uint8_t* __restrict__ fp = frames + (int64_t)idx[k] * frame_stride;
#pragma unroll
        for (int r = 0; r < UM_ROWS; ++r) raw[r] = from[r] >= 0 ? fp[from[r]] : 0;
    };
    fetch(0);
    for (int k = 0; k < n; ++k) {
        uint32_t v[UM_ROWS];
#pragma unroll
        for (int r = 0; r < UM_ROWS; ++r) v[r] = raw[r];
        if (k + 1 < n) fetch(k + 1);
#pragma unroll
        for (int r = 0; r < UM_ROWS; ++r) s1[r] += v[r], s2[r] += v[r] * v[r];
    }
#pragma unroll
    for (int r = 0; r < UM_ROWS; ++r) {
        if (from[r] < 0) break;
        const int64_t at = (int64_t)(r0 + r) * row_bytes + j;
        S1[at] = s1[r], S2[at] = s2[r];
    }
}

// grid.x: runs of 256 pixels of the box's rows [lo, hi) (picture rows), grid.y: frames.  frames / src hold the picture's rows from y0 on.
__global__ __launch_bounds__(UM_THREADS) void k_unmix_apply(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_stride,
                                                            const uint16_t* __restrict__ g16, const int16_t* __restrict__ o16, int W, int y0, int lo,
                                                            int hi, int by0, int bx0, int bw)
{
    const int p = blockIdx.x * UM_THREADS + threadIdx.x;
    if (p >= (hi - lo) * bw) return;
    const int ry = p / bw, x = p - ry * bw, y = lo + ry;                       // the picture's row y, the box's column x
    const int at = (y - by0) * bw + x;
    const int g = g16[at];
    if (g < UM_GMIN) return;
    const int64_t px = ((int64_t)(y - y0) * W + bx0 + x) * 3;
    const uint8_t* s = src + (int64_t)blockIdx.y * src_stride + px;
    uint8_t* f = frames + (int64_t)blockIdx.y * frame_stride + px;
    const uint32_t den = 16u * (uint32_t)g;
    int I[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) I[c] = s[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int num = 256 * (16 * I[c] - (int)o16[at * 3 + c]);
        f[c] = num < 0 ? (uint8_t)0 : (uint8_t)min(255u, ((uint32_t)num + den / 2) / den);
    }
}

int ufail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

const char* bad_picture(int H, int W)
{
    if (H <= 0 || W <= 0) return "logo unblend: H and W must be positive";
    if ((int64_t)H * W * 3 > 0x7fffffffll) return "logo unblend: a frame of H * W * 3 >= 2^31 bytes is not supported";
    return nullptr;
}

}  // namespace

extern "C" int vsr_unmix_accum_launch(const uint8_t* frames, int64_t frame_stride, const int32_t* idx, int n, int H, int W, int gy0, int gy1, int gx0,
                                      int gx1, int first, uint32_t* S1, uint32_t* S2, void* stream)
{
    (void)H;
    const int gh = gy1 - gy0, row_bytes = 3 * (gx1 - gx0);
    const dim3 grid((unsigned)((row_bytes + UM_THREADS - 1) / UM_THREADS), (unsigned)((gh + UM_ROWS - 1) / UM_ROWS));
    hipLaunchKernelGGL(k_unmix_accum, grid, dim3(UM_THREADS), 0, (hipStream_t)stream, frames, frame_stride, idx, n, W, gy0, gh, gx0, row_bytes, first,
                       S1, S2);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int vsr_unmix_apply_launch(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_stride, const uint16_t* g16,
                                      const int16_t* o16, int n, int W, int y0, int lo, int hi, int by0, int bx0, int bw, void* stream)
{
    const dim3 grid((unsigned)(((int64_t)(hi - lo) * bw + UM_THREADS - 1) / UM_THREADS), (unsigned)n);
    hipLaunchKernelGGL(k_unmix_apply, grid, dim3(UM_THREADS), 0, (hipStream_t)stream, frames, frame_stride, src, src_stride, g16, o16, W, y0, lo, hi,
                       by0, bx0, bw);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int vsr_unmix_accum(const uint8_t* frames_dev, int64_t frame_stride, const int32_t* idx_dev, int n, int H, int W, int gy0, int gy1, int gx0, int gx1,
                    int first, uint32_t* s1_dev, uint32_t* s2_dev, void* stream)
{
    if (!frames_dev || !idx_dev || !s1_dev || !s2_dev) return ufail(VSR_ERR_ARG, "logo unblend: null pointer");
    if (n < 1 || n > UM_MAX_N)
        return ufail(VSR_ERR_ARG, "logo unblend: n = " + std::to_string(n) + " frames, 1 <= n <= " + std::to_string(UM_MAX_N) +
                                      " are possible (the sum of squares of more could overflow)");
    if (const char* why = bad_picture(H, W)) return ufail(VSR_ERR_ARG, why);
    if (gy0 < 0 || gy1 > H || gy0 >= gy1 || gx0 < 0 || gx1 > W || gx0 >= gx1)
        return ufail(VSR_ERR_ARG, "logo unblend: the grown box [" + std::to_string(gy0) + ", " + std::to_string(gy1) + ") x [" + std::to_string(gx0) +
                                      ", " + std::to_string(gx1) + ") is empty or leaves the frame");
    if (first != 0 && first != 1) return ufail(VSR_ERR_ARG, "logo unblend: first must be 0 or 1");
    if (frame_stride < (int64_t)H * W * 3) return ufail(VSR_ERR_ARG, "logo unblend: frame stride smaller than a frame");
    if ((uintptr_t)s1_dev % 4 || (uintptr_t)s2_dev % 4 || (uintptr_t)idx_dev % 4)
        return ufail(VSR_ERR_ARG, "logo unblend: the moment planes or the frame numbers are misaligned");
    if (vsr_device_count() <= 0) return ufail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_unmix_accum_launch(frames_dev, frame_stride, idx_dev, n, H, W, gy0, gy1, gx0, gx1, first, s1_dev, s2_dev, stream) != 0)
        return ufail(VSR_ERR_HIP, std::string("logo unblend accumulate launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

int vsr_unmix_apply(uint8_t* frames_dev, int64_t frame_stride, const uint8_t* src_dev, int64_t src_stride, const uint16_t* g16_dev,
                    const int16_t* o16_dev, int n, int H, int W, int y0, int rows, const int32_t* box, void* stream)
{
    if (!frames_dev || !src_dev || !g16_dev || !o16_dev || !box) return ufail(VSR_ERR_ARG, "logo unblend: null pointer");
    if (n < 0) return ufail(VSR_ERR_ARG, "logo unblend: n = " + std::to_string(n) + " frames");
    if (const char* why = bad_picture(H, W)) return ufail(VSR_ERR_ARG, why);
    if (y0 < 0 || rows <= 0 || y0 > H - rows)
        return ufail(VSR_ERR_ARG, "logo unblend: the rows [" + std::to_string(y0) + ", " + std::to_string((int64_t)y0 + rows) + ") leave the frame");
    const int by0 = box[0], by1 = box[1], bx0 = box[2], bx1 = box[3];
    if (by0 < 0 || by1 > H || by0 >= by1 || bx0 < 0 || bx1 > W || bx0 >= bx1)
        return ufail(VSR_ERR_ARG, "logo unblend: the box [" + std::to_string(by0) + ", " + std::to_string(by1) + ") x [" + std::to_string(bx0) + ", " +
                                      std::to_string(bx1) + ") is empty or leaves the frame");
    if (frame_stride < (int64_t)rows * W * 3 || src_stride < (int64_t)rows * W * 3)
        return ufail(VSR_ERR_ARG, "logo unblend: frame stride smaller than the rows held");
    if ((uintptr_t)g16_dev % 2 || (uintptr_t)o16_dev % 2) return ufail(VSR_ERR_ARG, "logo unblend: the gain or the offset plane is misaligned");
    const int lo = by0 > y0 ? by0 : y0, hi = by1 < y0 + rows ? by1 : y0 + rows;
    if (n == 0 || lo >= hi) return 0;                                           // nothing of the box in these rows: no launch
    if (n > UM_MAX_N) return ufail(VSR_ERR_ARG, "logo unblend: n = " + std::to_string(n) + " frames, at most " + std::to_string(UM_MAX_N) + " a call");
    if (vsr_device_count() <= 0) return ufail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_unmix_apply_launch(frames_dev, frame_stride, src_dev, src_stride, g16_dev, o16_dev, n, W, y0, lo, hi, by0, bx0, bx1 - bx0, stream) != 0)
        return ufail(VSR_ERR_HIP, std::string("logo unblend apply launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // extern "C"
