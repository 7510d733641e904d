// --seam-feather: the mask-exact, feathered composite every inpaint mode can end with (the statement is
// tests/_feather_statement.py).  All integer arithmetic.
//
//   k_feather_alpha       C (uint8 [H][W], non-zero = the plugin blends here) -> d = min(F, Chebyshev distance to the nearest zero
//                         of C inside the frame).  Separable and exact: h = clipped distance along the row, then
//                         d(y,x) = min over |dy| < F of max(|dy|, h(y+dy,x)), rows outside the frame counting as h = F (the frame
//                         border is no zero: no ramp along it).  Once per mask, not per frame.
//   k_feather_composite   in place on the frames that hold the fill: d == F nothing is touched (no read of src, no store), d == 0
//                         the source byte is stored, else (d * fill + (F - d) * src + F / 2) / F.
//
// Both are streaming kernels.  A frame is H * W * 3 contiguous bytes whose start may have any alignment (a batch is a slice of a
// larger tensor, W * 3 is no multiple of 4 in general), so the composite walks a frame as a flat byte array: a scalar head up to
// the first 16-byte boundary of the DESTINATION, 16-byte chunks, a scalar tail.  The source of a chunk has whatever alignment it
// has; its 16 bytes are read through memcpy, which the compiler lowers to what the target allows.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "feather_kernels.h"
#include "plan_c.h"

namespace {

constexpr int FEATHER_MAX = 64;
constexpr int FA_TX = 64, FA_TY = 32, FA_THREADS = 256;
constexpr int FC_THREADS = 256, FC_MAX_BLOCKS = 2048, FC_MAX_GY = 64;

// One workgroup owns FA_TY x FA_TX pixels.  Pass 1 fills LDS with h for its rows and F - 1 rows above and below, pass 2 reads the
// column out of LDS.  C is read at in-frame coordinates only; columns >= W of the tile hold h = F and are never written out.
__global__ __launch_bounds__(FA_THREADS) void k_feather_alpha(const uint8_t* __restrict__ cmask, int H, int W, int F,
                                                              uint8_t* __restrict__ alpha)
{
    __shared__ uint8_t hrow[(FA_TY + 2 * (FEATHER_MAX - 1)) * FA_TX];
    const int x0 = blockIdx.x * FA_TX, y0 = blockIdx.y * FA_TY;
    const int halo = F - 1, rows = FA_TY + 2 * halo;
    for (int i = threadIdx.x; i < rows * FA_TX; i += FA_THREADS) {
        const int ly = i / FA_TX, lx = i % FA_TX;
        const int y = y0 - halo + ly, x = x0 + lx;
        int h = F;
        if (y >= 0 && y < H && x < W) {
            const uint8_t* row = cmask + (int64_t)y * W;
            if (row[x] == 0) {
                h = 0;
            } else {
                for (int k = 1; k < F; ++k)
                    if ((x - k >= 0 && row[x - k] == 0) || (x + k < W && row[x + k] == 0)) { h = k; break; }
            }
        }
        hrow[i] = (uint8_t)h;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < FA_TY * FA_TX; i += FA_THREADS) {
        const int ly = i / FA_TX, lx = i % FA_TX;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        const uint8_t* col = hrow + (ly + halo) * FA_TX + lx;
        int d = col[0];
        for (int dy = 1; dy < d; ++dy)                     // a row |dy| >= d away cannot lower d; dy < d <= F keeps inside the halo
            d = min(d, max(dy, (int)min(col[-dy * FA_TX], col[dy * FA_TX])));
        alpha[(int64_t)y * W + x] = (uint8_t)d;
    }
}

// x / F for 0 <= x <= 64 * 255 + 32 and 2 <= F <= 64, magic = ceil(2^32 / F): exact, since x * (magic * F - 2^32) < 2^32
__device__ __forceinline__ uint32_t div_feather(uint32_t x, uint32_t magic) { return __umulhi(x, magic); }

__device__ __forceinline__ void feather_byte(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t o, int d, int F, uint32_t magic)
{
    if (d >= F) return;
    const uint32_t s = src[o];
    dst[o] = d == 0 ? (uint8_t)s : (uint8_t)div_feather((uint32_t)d * dst[o] + (uint32_t)(F - d) * s + (uint32_t)(F >> 1), magic);
}

// N = H * W * 3 bytes per frame, below 2^31 (the entry point refuses larger frames): offsets inside a frame are 32-bit, frame starts 64-bit
using idx_t = uint32_t;
__global__ __launch_bounds__(FC_THREADS) void k_feather_composite(uint8_t* __restrict__ frames, int64_t frame_stride,
                                                                  const uint8_t* __restrict__ src, int64_t src_frame_stride,
                                                                  const uint8_t* __restrict__ alpha, int n, idx_t N, int F, uint32_t magic)
{
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        uint8_t* __restrict__ dst = frames + (int64_t)f * frame_stride;
        const uint8_t* __restrict__ s = src + (int64_t)f * src_frame_stride;
        const idx_t to_boundary = (idx_t)((16 - ((uintptr_t)dst & 15)) & 15);
        const idx_t head = to_boundary < N ? to_boundary : N;
        const idx_t nb = (N - head) / 16;
        const idx_t step = (idx_t)gridDim.x * FC_THREADS;
        for (idx_t c = (idx_t)blockIdx.x * FC_THREADS + threadIdx.x; c <= nb; c += step) {
            if (c == nb) {                                   // one lane per frame: the bytes in front of and behind the chunks
                for (idx_t o = 0; o < head; ++o) feather_byte(dst, s, o, alpha[o / 3], F, magic);
                for (idx_t o = head + nb * 16; o < N; ++o) feather_byte(dst, s, o, alpha[o / 3], F, magic);
                break;
            }
            const idx_t o = head + c * 16;                   // o + 15 < N: the six pixels p0 .. p0 + 5 the chunk touches all exist
            const idx_t p0 = o / 3;
            const int r = (int)(o - p0 * 3);
            const uint8_t* a = alpha + p0;
            const uint32_t a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
            const uint32_t lo = min(min(min(a0, a1), min(a2, a3)), min(a4, a5));
            if (lo >= (uint32_t)F) continue;                  // the fill stays: nothing is read from src, nothing stored
            if ((a0 | a1 | a2 | a3 | a4 | a5) == 0) {         // the source comes back
                uint4 v;
                __builtin_memcpy(&v, s + o, 16);
                *reinterpret_cast<uint4*>(dst + o) = v;
                continue;
            }
            const uint64_t packed = (uint64_t)(a0 | (a1 << 8) | (a2 << 16) | (a3 << 24)) | ((uint64_t)(a4 | (a5 << 8)) << 32);
#pragma unroll
            for (int j = 0; j < 16; ++j)
                feather_byte(dst, s, o + j, (int)((packed >> (8 * ((r + j) / 3))) & 0xff), F, magic);
        }
    }
}

int ffail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

}  // namespace

extern "C" int vsr_feather_launch_alpha(const uint8_t* cmask, int H, int W, int feather, uint8_t* alpha, void* stream)
{
    const dim3 grid((W + FA_TX - 1) / FA_TX, (H + FA_TY - 1) / FA_TY);
    hipLaunchKernelGGL(k_feather_alpha, grid, dim3(FA_THREADS), 0, (hipStream_t)stream, cmask, H, W, feather, alpha);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int vsr_feather_launch_composite(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride,
                                            const uint8_t* alpha, int n, int H, int W, int feather, void* stream)
{
    const int64_t N = (int64_t)H * W * 3;
    const int64_t items = N / 16 + 1;                        // chunks per frame (an upper bound) + the head / tail lane
    const int gy = n < FC_MAX_GY ? n : FC_MAX_GY;
    int64_t gx = (items + FC_THREADS - 1) / FC_THREADS;
    const int64_t cap = FC_MAX_BLOCKS / gy > 0 ? FC_MAX_BLOCKS / gy : 1;
    if (gx > cap) gx = cap;                                  // a memory-bound kernel: ~2048 workgroups, the rest by grid stride
    const uint32_t magic = feather >= 2 ? (uint32_t)(((1ull << 32) + feather - 1) / feather) : 0u;      // F = 1 never divides
    const dim3 grid((unsigned)gx, (unsigned)gy);
    hipLaunchKernelGGL(k_feather_composite, grid, dim3(FC_THREADS), 0, (hipStream_t)stream, frames, frame_stride, src, src_frame_stride,
                       alpha, n, (uint32_t)N, feather, magic);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int vsr_feather_alpha(const uint8_t* cmask_dev, int H, int W, int feather, uint8_t* alpha_dev, void* stream)
{
    if (!cmask_dev || !alpha_dev) return ffail(VSR_ERR_ARG, "feather: null pointer");
    if (H <= 0 || W <= 0) return ffail(VSR_ERR_ARG, "feather: H and W must be positive, got " + std::to_string(H) + " x " + std::to_string(W));
    if (feather < 1 || feather > FEATHER_MAX)
        return ffail(VSR_ERR_ARG, "feather: F = " + std::to_string(feather) + ", 1 <= F <= " + std::to_string(FEATHER_MAX) + " are possible");
    if (vsr_device_count() <= 0) return ffail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_feather_launch_alpha(cmask_dev, H, W, feather, alpha_dev, stream) != 0)
        return ffail(VSR_ERR_HIP, std::string("feather alpha launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

int vsr_feather_composite(uint8_t* frames_dev, int64_t frame_stride, const uint8_t* src_dev, int64_t src_frame_stride,
                          const uint8_t* alpha_dev, int n, int H, int W, int feather, void* stream)
{
    if (!frames_dev || !src_dev || !alpha_dev) return ffail(VSR_ERR_ARG, "feather: null pointer");
    if (n < 0) return ffail(VSR_ERR_ARG, "feather: negative frame count");
    if (H <= 0 || W <= 0) return ffail(VSR_ERR_ARG, "feather: H and W must be positive, got " + std::to_string(H) + " x " + std::to_string(W));
    if (feather < 1 || feather > FEATHER_MAX)
        return ffail(VSR_ERR_ARG, "feather: F = " + std::to_string(feather) + ", 1 <= F <= " + std::to_string(FEATHER_MAX) + " are possible");
    const int64_t N = (int64_t)H * W * 3;
    if (N > 0x7fffffffll) return ffail(VSR_ERR_ARG, "feather: a frame of H * W * 3 >= 2^31 bytes is not supported");
    if (frame_stride < N || src_frame_stride < N) return ffail(VSR_ERR_ARG, "feather: frame stride smaller than a frame");
    if (n == 0) return 0;
    if (vsr_device_count() <= 0) return ffail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_feather_launch_composite(frames_dev, frame_stride, src_dev, src_frame_stride, alpha_dev, n, H, W, feather, stream) != 0)
        return ffail(VSR_ERR_HIP, std::string("feather composite launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // extern "C"
