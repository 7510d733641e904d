// Colour conversion of the raw-container frame transport: planar 8-bit YCbCr <-> packed BGR.
// In the reference this is libswscale's work on both sides of the pipe: cv2.VideoCapture.read() hands out BGR frames
// (backend/inpaint/sttn_auto_inpaint.py:254-262, backend/main.py:171-176) and FFmpegVideoWriter feeds bgr24 frames to an encoder
// that converts them to yuv420p (backend/tools/video_io.py:54-81).  Here the *.y4m reader / writer (backend/tools/video_io.py)
// keep the planes as they are on disk, and these kernels do the BT.601 integer conversion on the GPU: a 1080p frame costs the
// host 47 ms in numpy -- seven times the inpainting itself -- and 10 us here.  Integer work, HBM-bound, bit-exact against the
// numpy statement of the same matrices (video_io._yuv_to_bgr / _bgr_to_yuv; tests/test_gpu_io.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/vsr_hip.h"

#define DONE() return hipGetLastError() == hipSuccess ? 0 : VSR_ERR_HIP

__device__ __forceinline__ int clip_u8(int v) { return min(max(v, 0), 255); }

// 16.16 fixed-point BT.601 (the constants of libswscale / OpenCV): studio swing unless `full`
__device__ __forceinline__ void yuv2bgr_px(int y, int u, int v, bool full, int& b, int& g, int& r)
{
    u -= 128;
    v -= 128;
    if (full) {
        const int c = y << 16;
        r = (c + 91881 * v + 32768) >> 16;
        g = (c - 22554 * u - 46802 * v + 32768) >> 16;
        b = (c + 116130 * u + 32768) >> 16;
    } else {
        const int c = 76309 * (y - 16);
        r = (c + 104597 * v + 32768) >> 16;
        g = (c - 25675 * u - 53279 * v + 32768) >> 16;
        b = (c + 132201 * u + 32768) >> 16;
    }
    b = clip_u8(b);
    g = clip_u8(g);
    r = clip_u8(r);
}

__device__ __forceinline__ void bgr2yuv_px(int b, int g, int r, bool full, int& y, int& u, int& v)
{
    if (full) {
        y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
        u = ((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128;
        v = ((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128;
    } else {
        y = ((16829 * r + 33039 * g + 6416 * b + 32768) >> 16) + 16;
        u = ((-9714 * r - 19070 * g + 28784 * b + 32768) >> 16) + 128;
        v = ((28784 * r - 24103 * g - 4681 * b + 32768) >> 16) + 128;
    }
    y = clip_u8(y);
    u = clip_u8(u);
    v = clip_u8(v);
}

// One thread = 4 horizontally adjacent pixels: one 32-bit luma load, 12 output bytes as three 32-bit stores when the row is
// aligned.  Chroma is replicated (nearest), sx / sy = log2 of the sub-sampling; cw == 0: no chroma planes (mono).
// src = frames of [Y: H*W][U: ch*cw][V: ch*cw] contiguous, `frameBytes` apart; dst BGR [n][H][W][3].
__global__ void __launch_bounds__(256) k_io_yuv_to_bgr(const uint8_t* __restrict__ src, int64_t frameBytes, int H, int W, int cw, int ch,
                                                       int sx, int sy, int full, uint8_t* __restrict__ dst, int nframes)
{
    const int wq = (W + 3) >> 2;
    const int64_t total = (int64_t)nframes * H * wq;
    for (int64_t t = blockIdx.x * (int64_t)256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int xq = (int)(t % wq);
        const int yy = (int)((t / wq) % H);
        const int f = (int)(t / ((int64_t)wq * H));
        const uint8_t* Y = src + f * frameBytes + (int64_t)yy * W;
        const uint8_t* U = src + f * frameBytes + (int64_t)H * W + (int64_t)min(yy >> sy, max(ch - 1, 0)) * cw;
        const uint8_t* V = U + (int64_t)ch * cw;
        uint8_t* o = dst + ((int64_t)f * H + yy) * W * 3;
        const int x0 = xq * 4;
        uint8_t out[12];
        const int n = min(4, W - x0);
        for (int j = 0; j < n; ++j) {
            const int x = x0 + j;
            int u = 128, v = 128;
            if (cw > 0) {
                const int xc = min(x >> sx, cw - 1);
                u = U[xc];
                v = V[xc];
            }
            int b, g, r;
            yuv2bgr_px(Y[x], u, v, full != 0, b, g, r);
            if (cw == 0) g = r = b;                          // mono: the reader repeats the blue channel (video_io.Y4mVideo.read)
            out[3 * j] = (uint8_t)b;
            out[3 * j + 1] = (uint8_t)g;
            out[3 * j + 2] = (uint8_t)r;
        }
        uint8_t* p = o + (int64_t)x0 * 3;
        if (n == 4 && (((uintptr_t)p) & 3) == 0) {
            uint32_t* p32 = reinterpret_cast<uint32_t*>(p);
            p32[0] = out[0] | (out[1] << 8) | (out[2] << 16) | ((uint32_t)out[3] << 24);
            p32[1] = out[4] | (out[5] << 8) | (out[6] << 16) | ((uint32_t)out[7] << 24);
            p32[2] = out[8] | (out[9] << 8) | (out[10] << 16) | ((uint32_t)out[11] << 24);
        } else {
            for (int j = 0; j < 3 * n; ++j) p[j] = out[j];
        }
    }
}

// BGR [n][H][W][3] -> planar frames [Y: H*W][U][V], chroma 4:4:4 (sub == 0) or 4:2:0 (sub == 1: the rounded mean of the 2x2 block of
// per-pixel u8 chroma values, edge pixels repeated for odd sizes -- video_io.Y4mWriter).  One thread = one 2x2 block.
__global__ void __launch_bounds__(256) k_io_bgr_to_yuv(const uint8_t* __restrict__ src, int H, int W, int sub, int full, uint8_t* __restrict__ dst,
                                                       int64_t frameBytes, int nframes)
{
    const int bw = (W + 1) >> 1, bh = (H + 1) >> 1;
    const int cw = sub ? bw : W, chh = sub ? bh : H;
    const int64_t total = (int64_t)nframes * bh * bw;
    for (int64_t t = blockIdx.x * (int64_t)256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int bx = (int)(t % bw);
        const int by = (int)((t / bw) % bh);
        const int f = (int)(t / ((int64_t)bw * bh));
        const uint8_t* in = src + (int64_t)f * H * W * 3;
        uint8_t* Y = dst + f * frameBytes;
        uint8_t* U = Y + (int64_t)H * W;
        uint8_t* V = U + (int64_t)chh * cw;
        int us = 0, vs = 0;
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int y = by * 2 + dy, x = bx * 2 + dx;
                const int yc = min(y, H - 1), xc = min(x, W - 1);       // edge padding of the sub-sampler
                const uint8_t* p = in + ((int64_t)yc * W + xc) * 3;
                int yv, u, v;
                bgr2yuv_px(p[0], p[1], p[2], full != 0, yv, u, v);
                us += u;
                vs += v;
                if (y < H && x < W) {
                    Y[(int64_t)y * W + x] = (uint8_t)yv;
                    if (!sub) {
                        U[(int64_t)y * W + x] = (uint8_t)u;
                        V[(int64_t)y * W + x] = (uint8_t)v;
                    }
                }
            }
        if (sub) {
            U[(int64_t)by * cw + bx] = (uint8_t)((us + 2) >> 2);
            V[(int64_t)by * cw + bx] = (uint8_t)((vs + 2) >> 2);
        }
    }
}

static inline int grid_for(int64_t total)
{
    const int64_t b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

extern "C" int vsr_io_yuv_to_bgr(const uint8_t* planes_dev, int64_t frame_bytes, int H, int W, int chroma_w, int chroma_h, int full_range,
                                 uint8_t* bgr_dev, int nframes, void* stream)
{
    if (planes_dev == nullptr || bgr_dev == nullptr || H <= 0 || W <= 0 || nframes < 0) return VSR_ERR_ARG;
    if (nframes == 0) return 0;
    int sx = 0, sy = 0;
    if (chroma_w > 0) {
        if (chroma_w == W) sx = 0; else if (chroma_w == (W + 1) / 2) sx = 1; else return VSR_ERR_ARG;
        if (chroma_h == H) sy = 0; else if (chroma_h == (H + 1) / 2) sy = 1; else return VSR_ERR_ARG;
    }
    if (frame_bytes < (int64_t)H * W + 2 * (int64_t)chroma_w * chroma_h) return VSR_ERR_ARG;
    const int64_t total = (int64_t)nframes * H * ((W + 3) / 4);
    hipLaunchKernelGGL(k_io_yuv_to_bgr, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, planes_dev, frame_bytes, H, W, chroma_w,
                       chroma_h, sx, sy, full_range, bgr_dev, nframes);
    DONE();
}

extern "C" int vsr_io_bgr_to_yuv(const uint8_t* bgr_dev, int H, int W, int subsample_420, int full_range, uint8_t* planes_dev,
                                 int64_t frame_bytes, int nframes, void* stream)
{
    if (planes_dev == nullptr || bgr_dev == nullptr || H <= 0 || W <= 0 || nframes < 0) return VSR_ERR_ARG;
    if (nframes == 0) return 0;
    const int64_t cw = subsample_420 ? (W + 1) / 2 : W, ch = subsample_420 ? (H + 1) / 2 : H;
    if (frame_bytes < (int64_t)H * W + 2 * cw * ch) return VSR_ERR_ARG;
    const int64_t total = (int64_t)nframes * ((H + 1) / 2) * ((W + 1) / 2);
    hipLaunchKernelGGL(k_io_bgr_to_yuv, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, bgr_dev, H, W, subsample_420, full_range,
                       planes_dev, frame_bytes, nframes);
    DONE();
}

// ------------------------------------------------------------------------------------------------------------------------------
// The source's own format: 8 / 10 / 12-bit planes (16-bit little-endian samples above 8 bits), 4:4:4 / 4:2:2 / 4:2:0 /
// mono, both ranges, and the KEEP RULE of the writer -- a sample whose decoded colour the inpainting did not change is copied from
// the source record, not re-encoded (video_io.keep_record is the definition; tests/test_gpu_y4m_formats.py holds the kernels to it
// bit for bit).  The per-depth constants are made once on the host (io_color below: double, floor(x + 0.5), the expression
// video_io.color_constants uses) and reach the kernels as an argument.  int32 is enough: the largest accumulator is 5.6e8 at 12 bits.
// ------------------------------------------------------------------------------------------------------------------------------
struct IoColor {
    int ky, krv, kgu, kgv, kbu;      // decode: c = ky * (Y - yoff); R = c + krv V'; G = c + kgu U' + kgv V'; B = c + kbu U'
    int e[9];                        // encode rows Y, U, V over (R, G, B)
    int yoff, coff, peak, s;         // luma offset, chroma offset, 2^depth - 1, depth - 8
};

__device__ __forceinline__ void dec_px(const IoColor& k, int y, int u, int v, int& b, int& g, int& r)
{
    y = min(y, k.peak);              // stored samples above the peak come from outside the program
    u = min(u, k.peak) - k.coff;
    v = min(v, k.peak) - k.coff;
    const int c = k.ky * (y - k.yoff), rnd = 1 << (15 + k.s), sh = 16 + k.s;
    r = clip_u8((c + k.krv * v + rnd) >> sh);
    g = clip_u8((c + k.kgu * u + k.kgv * v + rnd) >> sh);
    b = clip_u8((c + k.kbu * u + rnd) >> sh);
}

__device__ __forceinline__ void enc_px(const IoColor& k, int b, int g, int r, int& y, int& u, int& v)
{
    const int rnd = 1 << (15 - k.s), sh = 16 - k.s;
    y = min(max(((k.e[0] * r + k.e[1] * g + k.e[2] * b + rnd) >> sh) + k.yoff, 0), k.peak);
    u = min(max(((k.e[3] * r + k.e[4] * g + k.e[5] * b + rnd) >> sh) + k.coff, 0), k.peak);
    v = min(max(((k.e[6] * r + k.e[7] * g + k.e[8] * b + rnd) >> sh) + k.coff, 0), k.peak);
}

// N consecutive samples of a plane row starting at p, the first n (1 <= n <= N) real, the rest repeating the last real one (the edge
// replication of the sub-sampler): one 4 / 8 / 16-byte access when all N are there and the address allows it
template <typename T, int N>
__device__ __forceinline__ void load_row(const T* p, int n, int (&out)[N])
{
    constexpr int NW = N * (int)sizeof(T) / 4, PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    if (n == N && (((uintptr_t)p) & (NW * 4 - 1)) == 0) {
        uint32_t w[NW];
        if constexpr (NW == 1) {
            w[0] = *reinterpret_cast<const uint32_t*>(p);
        } else if constexpr (NW == 2) {
            const uint2 t = *reinterpret_cast<const uint2*>(p);
            w[0] = t.x; w[1] = t.y;
        } else {
            const uint4 t = *reinterpret_cast<const uint4*>(p);
            w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < N; ++j) out[j] = (int)((w[j / PER] >> (BITS * (j % PER))) & ((1u << BITS) - 1u));
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) out[j] = (int)p[min(j, n - 1)];
    }
}

template <typename T, int N>
__device__ __forceinline__ void store_row(T* p, int n, const int (&val)[N])
{
    constexpr int NW = N * (int)sizeof(T) / 4, PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    if (n == N && (((uintptr_t)p) & (NW * 4 - 1)) == 0) {
        uint32_t w[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) w[j / PER] |= (uint32_t)val[j] << (BITS * (j % PER));
        if constexpr (NW == 1) *reinterpret_cast<uint32_t*>(p) = w[0];
        else if constexpr (NW == 2) *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
        else *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j < n) p[j] = (T)val[j];
    }
}

// planes (T = uint8_t at 8 bits, uint16_t above) -> BGR.  One thread = 4 adjacent pixels, as k_io_yuv_to_bgr: one 4- or 8-byte luma
// load, three 32-bit stores.
template <typename T>
__global__ void __launch_bounds__(256) k_io_planes_to_bgr(const uint8_t* __restrict__ src, int64_t frameBytes, int H, int W, int cw, int ch,
                                                          int sx, int sy, IoColor k, uint8_t* __restrict__ dst, int nframes)
{
    const int wq = (W + 3) >> 2;
    const int64_t total = (int64_t)nframes * H * wq;
    for (int64_t t = blockIdx.x * (int64_t)256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int xq = (int)(t % wq);
        const int yy = (int)((t / wq) % H);
        const int f = (int)(t / ((int64_t)wq * H));
        const T* Y = reinterpret_cast<const T*>(src + f * frameBytes) + (int64_t)yy * W;
        const T* U = reinterpret_cast<const T*>(src + f * frameBytes) + (int64_t)H * W + (int64_t)min(yy >> sy, max(ch - 1, 0)) * cw;
        const T* V = U + (int64_t)ch * cw;
        const int x0 = xq * 4, n = min(4, W - x0);
        int ys[4];
        load_row<T, 4>(Y + x0, n, ys);
        uint32_t out[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = min(x0 + j, W - 1);
            int u = k.coff, v = k.coff;
            if (cw > 0) {
                const int xc = min(x >> sx, cw - 1);
                u = U[xc];
                v = V[xc];
            }
            int b, g, r;
            dec_px(k, ys[j], u, v, b, g, r);
            out[3 * j] = (uint32_t)b;
            out[3 * j + 1] = (uint32_t)g;
            out[3 * j + 2] = (uint32_t)r;
        }
        uint8_t* p = dst + (((int64_t)f * H + yy) * W + x0) * 3;
        if (n == 4 && (((uintptr_t)p) & 3) == 0) {
            uint32_t* p32 = reinterpret_cast<uint32_t*>(p);
            p32[0] = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
            p32[1] = out[4] | (out[5] << 8) | (out[6] << 16) | (out[7] << 24);
            p32[2] = out[8] | (out[9] << 8) | (out[10] << 16) | (out[11] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j)
                if (j < 3 * n) p[j] = (uint8_t)out[j];
        }
    }
}

// BGR -> planes, with the keep rule when KEEP.  One thread = a tile of 8 pixels x (1 << SY) rows = whole chroma blocks (1x1, 2x1, 1x2
// or 2x2: SX / SY = log2 of the sub-sampling), so the decision "every pixel of this block kept its colour" needs no communication.
// Per row: 24 bytes of BGR as six 32-bit words, 8 source luma samples and 8 luma samples out as one 8- or 16-byte access.  The
// chroma mean is the writer's: (sum + half) >> (SX + SY) over the block with the edge pixels repeated.  In place (dst == src, same
// stride) is fine: a thread reads the source samples of its own tile only, before it writes them.
template <typename T, int SX, int SY, bool KEEP>
__global__ void __launch_bounds__(256) k_io_bgr_to_planes(const uint8_t* __restrict__ bgr, int H, int W, int cw, int ch, IoColor k,
                                                          const uint8_t* srcp, int64_t srcBytes, uint8_t* dstp, int64_t dstBytes, int nframes)
{
    constexpr int R = 1 << SY, NC = 8 >> SX;
    const int tw = (W + 7) >> 3, th = (H + R - 1) >> SY;
    const bool mono = cw == 0;
    const int64_t total = (int64_t)nframes * th * tw;
    for (int64_t t = blockIdx.x * (int64_t)256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int tx = (int)(t % tw);
        const int ty = (int)((t / tw) % th);
        const int f = (int)(t / ((int64_t)tw * th));
        const int x0 = tx * 8, n = min(8, W - x0);
        const int cx0 = x0 >> SX, nc = mono ? 0 : min(NC, cw - cx0);
        const int cy = min(ty, max(ch - 1, 0));                    // (SY == 0: ty is the row itself)
        T* Yd = reinterpret_cast<T*>(dstp + f * dstBytes);
        T* Ud = Yd + (int64_t)H * W + (int64_t)cy * cw + cx0;
        T* Vd = Ud + (int64_t)ch * cw;
        const T* Ys = reinterpret_cast<const T*>(srcp + f * srcBytes);
        int usrc[NC], vsrc[NC], us[NC], vs[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) us[c] = vs[c] = 0, usrc[c] = vsrc[c] = k.coff;
        if (KEEP && !mono) {
            const T* Us = Ys + (int64_t)H * W + (int64_t)cy * cw + cx0;
            load_row<T, NC>(Us, nc, usrc);
            load_row<T, NC>(Us + (int64_t)ch * cw, nc, vsrc);
        }
        unsigned kept = 0xffu;                                     // bit c: every pixel of chroma block c decodes to the frame's colour
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int y = ty * R + r, yc = min(y, H - 1);
            const uint8_t* p = bgr + (((int64_t)f * H + yc) * W + x0) * 3;
            int px[24];
            if (n == 8 && (((uintptr_t)p) & 3) == 0) {
                const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p);
                uint32_t w[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) w[i] = p32[i];
#pragma unroll
                for (int i = 0; i < 24; ++i) px[i] = (int)((w[i >> 2] >> (8 * (i & 3))) & 255u);
            } else {
#pragma unroll
                for (int i = 0; i < 24; ++i) px[i] = (int)p[3 * min(i / 3, n - 1) + i % 3];
            }
            int ysrc[8], yout[8];
            if (KEEP) load_row<T, 8>(Ys + (int64_t)yc * W + x0, n, ysrc);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int ye, ue, ve;
                enc_px(k, px[3 * j], px[3 * j + 1], px[3 * j + 2], ye, ue, ve);
                bool same = false;
                if (KEEP) {
                    int b, g, rr;
                    dec_px(k, ysrc[j], usrc[j >> SX], vsrc[j >> SX], b, g, rr);
                    same = b == px[3 * j] && g == px[3 * j + 1] && rr == px[3 * j + 2];
                    if (!same) kept &= ~(1u << (j >> SX));
                }
                yout[j] = same ? ysrc[j] : ye;
                us[j >> SX] += ue;
                vs[j >> SX] += ve;
            }
            if (y < H) store_row<T, 8>(Yd + (int64_t)y * W + x0, n, yout);
        }
        if (!mono) {
            constexpr int HALF = (1 << (SX + SY)) >> 1;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const bool kc = KEEP && ((kept >> c) & 1u);
                us[c] = kc ? usrc[c] : (us[c] + HALF) >> (SX + SY);
                vs[c] = kc ? vsrc[c] : (vs[c] + HALF) >> (SX + SY);
            }
            store_row<T, NC>(Ud, nc, us);
            store_row<T, NC>(Vd, nc, vs);
        }
    }
}

// the constants of one depth and range: at 8 bits the ones of yuv2bgr_px / bgr2yuv_px; studio range keeps them at every depth (the
// shifts move); full range rescales them by 255 * 2^s / (2^depth - 1) (decode) and its inverse (encode), since peak white is
// 2^depth - 1 and not 255 << s
static bool io_color(int depth, int full, IoColor* c)
{
    if (depth != 8 && depth != 10 && depth != 12) return false;
    static const int dec_studio[5] = {76309, 104597, -25675, -53279, 132201}, dec_full[5] = {65536, 91881, -22554, -46802, 116130};
    static const int enc_studio[9] = {16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681};
    static const int enc_full[9] = {19595, 38470, 7471, -11059, -21709, 32768, 32768, -27439, -5329};
    const int s = depth - 8;
    c->s = s;
    c->peak = (1 << depth) - 1;
    c->coff = 128 << s;
    c->yoff = full ? 0 : 16 << s;
    int d[5];
    for (int i = 0; i < 5; ++i) d[i] = full ? (int)floor((double)dec_full[i] * (double)(255 << s) / (double)c->peak + 0.5) : dec_studio[i];
    c->ky = d[0]; c->krv = d[1]; c->kgu = d[2]; c->kgv = d[3]; c->kbu = d[4];
    for (int i = 0; i < 9; ++i) c->e[i] = full ? (int)floor((double)enc_full[i] * (double)c->peak / (double)(255 << s) + 0.5) : enc_studio[i];
    return true;
}

// chroma geometry of a record: cw == 0 mono; else cw in {W, (W+1)/2}, ch in {H, (H+1)/2}
static bool io_geometry(int H, int W, int cw, int ch, int* sx, int* sy)
{
    *sx = *sy = 0;
    if (cw < 0 || ch < 0) return false;
    if (cw == 0) return true;
    if (cw != W) { if (cw != (W + 1) / 2) return false; *sx = 1; }
    if (ch != H) { if (ch != (H + 1) / 2) return false; *sy = 1; }
    return true;
}

extern "C" int vsr_io_color_constants(int depth, int full_range, int32_t* out18)
{
    IoColor c;
    if (out18 == nullptr || !io_color(depth, full_range, &c)) return VSR_ERR_ARG;
    const int v[18] = {c.ky, c.krv, c.kgu, c.kgv, c.kbu, c.e[0], c.e[1], c.e[2], c.e[3], c.e[4], c.e[5], c.e[6], c.e[7], c.e[8],
                       c.yoff, c.coff, c.peak, c.s};
    for (int i = 0; i < 18; ++i) out18[i] = v[i];
    return 0;
}

extern "C" int vsr_io_planes_to_bgr(const void* planes_dev, int64_t frame_bytes, int H, int W, int chroma_w, int chroma_h, int depth,
                                    int full_range, uint8_t* bgr_dev, int nframes, void* stream)
{
    IoColor c;
    int sx, sy;
    if (planes_dev == nullptr || bgr_dev == nullptr || H <= 0 || W <= 0 || nframes < 0) return VSR_ERR_ARG;
    if (!io_color(depth, full_range, &c) || !io_geometry(H, W, chroma_w, chroma_h, &sx, &sy)) return VSR_ERR_ARG;
    const int bps = depth > 8 ? 2 : 1;
    if (frame_bytes < bps * ((int64_t)H * W + 2 * (int64_t)chroma_w * chroma_h)) return VSR_ERR_ARG;
    if (bps == 2 && ((((uintptr_t)planes_dev) | (uintptr_t)frame_bytes) & 1)) return VSR_ERR_ARG;
    if (nframes == 0) return 0;
    const int64_t total = (int64_t)nframes * H * ((W + 3) / 4);
    const uint8_t* src = static_cast<const uint8_t*>(planes_dev);
    if (bps == 1)
        hipLaunchKernelGGL(k_io_planes_to_bgr<uint8_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, frame_bytes, H, W,
                           chroma_w, chroma_h, sx, sy, c, bgr_dev, nframes);
    else
        hipLaunchKernelGGL(k_io_planes_to_bgr<uint16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, frame_bytes, H, W,
                           chroma_w, chroma_h, sx, sy, c, bgr_dev, nframes);
    DONE();
}

template <typename T, int SX, int SY>
static void launch_bgr_to_planes(bool keep, int64_t total, hipStream_t st, const uint8_t* bgr, int H, int W, int cw, int ch, const IoColor& c,
                                 const uint8_t* src, int64_t srcBytes, uint8_t* dst, int64_t dstBytes, int n)
{
    if (keep)
        hipLaunchKernelGGL((k_io_bgr_to_planes<T, SX, SY, true>), dim3(grid_for(total)), dim3(256), 0, st, bgr, H, W, cw, ch, c, src, srcBytes,
                           dst, dstBytes, n);
    else
        hipLaunchKernelGGL((k_io_bgr_to_planes<T, SX, SY, false>), dim3(grid_for(total)), dim3(256), 0, st, bgr, H, W, cw, ch, c, src, srcBytes,
                           dst, dstBytes, n);
}

extern "C" int vsr_io_bgr_to_planes(const uint8_t* bgr_dev, int H, int W, int chroma_w, int chroma_h, int depth, int full_range,
                                    const void* src_planes_dev, int64_t src_frame_bytes, void* planes_dev, int64_t frame_bytes, int nframes,
                                    void* stream)
{
    IoColor c;
    int sx, sy;
    if (planes_dev == nullptr || bgr_dev == nullptr || H <= 0 || W <= 0 || nframes < 0) return VSR_ERR_ARG;
    if (!io_color(depth, full_range, &c) || !io_geometry(H, W, chroma_w, chroma_h, &sx, &sy)) return VSR_ERR_ARG;
    const int bps = depth > 8 ? 2 : 1;
    const int64_t need = bps * ((int64_t)H * W + 2 * (int64_t)chroma_w * chroma_h);
    if (frame_bytes < need || (src_planes_dev != nullptr && src_frame_bytes < need)) return VSR_ERR_ARG;
    if (bps == 2 && ((((uintptr_t)planes_dev) | (uintptr_t)frame_bytes) & 1)) return VSR_ERR_ARG;
    if (bps == 2 && src_planes_dev != nullptr && ((((uintptr_t)src_planes_dev) | (uintptr_t)src_frame_bytes) & 1)) return VSR_ERR_ARG;
    const uint8_t* src = static_cast<const uint8_t*>(src_planes_dev);
    uint8_t* dst = static_cast<uint8_t*>(planes_dev);
    if (src != nullptr && !(src == dst && src_frame_bytes == frame_bytes)) {      // in place is fine; any other overlap is not
        const uint8_t* se = src + (int64_t)nframes * src_frame_bytes;
        const uint8_t* de = dst + (int64_t)nframes * frame_bytes;
        if (src < de && dst < se) return VSR_ERR_ARG;
    }
    if (nframes == 0) return 0;
    const int64_t total = (int64_t)nframes * ((H + sy) >> sy) * ((W + 7) / 8);
    const hipStream_t st = (hipStream_t)stream;
    const bool keep = src != nullptr;
#define VSR_IO_GO(T)                                                                                                                     \
    do {                                                                                                                                 \
        if (sx && sy) launch_bgr_to_planes<T, 1, 1>(keep, total, st, bgr_dev, H, W, chroma_w, chroma_h, c, src, src_frame_bytes, dst, frame_bytes, nframes); \
        else if (sx) launch_bgr_to_planes<T, 1, 0>(keep, total, st, bgr_dev, H, W, chroma_w, chroma_h, c, src, src_frame_bytes, dst, frame_bytes, nframes);  \
        else if (sy) launch_bgr_to_planes<T, 0, 1>(keep, total, st, bgr_dev, H, W, chroma_w, chroma_h, c, src, src_frame_bytes, dst, frame_bytes, nframes);  \
        else launch_bgr_to_planes<T, 0, 0>(keep, total, st, bgr_dev, H, W, chroma_w, chroma_h, c, src, src_frame_bytes, dst, frame_bytes, nframes);          \
    } while (0)
    if (bps == 1) VSR_IO_GO(uint8_t); else VSR_IO_GO(uint16_t);
#undef VSR_IO_GO
    DONE();
}
