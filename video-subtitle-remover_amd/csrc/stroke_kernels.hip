// --text-detect strokes: a weight-free detector of stroke-like text (the statement is tests/_strokes_statement.py).
// Integer arithmetic only; the host (backend/tools/stroke_det.py) labels the text map with vsr_det_launch_ccl, one call per frame, and
// chooses the boxes.
//
//   k_strokes_cells<F>  per tile of 64 x 32 analysis pixels of one frame (grid.z: the frame): the luma Y = (29 B + 150 G + 77 R + 128) >> 8
//                       of every source pixel, averaged over F x F with rounding, of the tile and a halo of S analysis pixels into LDS --
//                       the halo's coordinates clamp at the frame's borders, not at the tile's.  A thread owns one column and 8 rows:
//                       its column of 8 + 2 S lumas goes to registers once (the vertical test slides over it), the horizontal test
//                       reads its 2 S neighbours from LDS.  A pixel is a V-stroke pixel when it is a ridge along the row (brighter
//                       by C than the minima of the S pixels on BOTH sides, or darker by C than the maxima on both sides), an
//                       H-stroke pixel when it is one along the column.  The flags of 4 rows are summed in registers, the 4 columns
//                       of a cell sit in 4 neighbouring lanes and are summed by two lane exchanges; lane 4 b writes the cell.  No
//                       atomics.  A thread's staging loads stand ahead of the first LDS store in the source; at F = 1 the compiler keeps
//                       all 45 in flight (156 VGPRs), at larger F (15 * 3 F F loads, 86 VGPRs) it issues them in groups.  Beyond that
//                       the workgroups of a CU (3.8 KB of LDS each) overlap one tile's loads with another's tests.
//   k_strokes_text      per tile of 64 x 32 cells of one frame: both count planes with a halo of (WX, WY) cells (outside the frame: 0)
//                       in LDS, the sums over 2 WX + 1 columns, then over 2 WY + 1 rows; text = sv >= NV and sh >= NH as 1.0f / 0.0f
//                       for vsr_det_launch_ccl.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "plan_c.h"
#include "stroke_kernels.h"

namespace {

constexpr int SK_THREADS = 256, SK_WAVES = SK_THREADS / 64, SK_TW = 64, SK_TH = 32, SK_PER = SK_TH / SK_WAVES;   // rows of a tile: 8 per wave
constexpr int SK_MAX_S = 8, SK_MAX_F = 8, SK_MAX_WIN = 8, SK_MAX_N = 65535, SK_CELL = 4;
constexpr int SK_YROWS = SK_TH + 2 * SK_MAX_S, SK_YCOLS = SK_TW + 2 * SK_MAX_S;                  // the luma tile with the widest halo
constexpr int SK_FILL = (SK_YROWS * SK_YCOLS + SK_THREADS - 1) / SK_THREADS;                     // analysis pixels a thread stages
constexpr int SK_CROWS = SK_TH + 2 * SK_MAX_WIN, SK_CCOLS = SK_TW + 2 * SK_MAX_WIN;

// grid.x: tiles of 64 analysis columns, grid.y: tiles of 32 analysis rows, grid.z: the frame.  h = H / F, w = W / F; 1 <= S <= SK_MAX_S
template <int F>
__global__ __launch_bounds__(SK_THREADS) void k_strokes_cells(const uint8_t* __restrict__ frames, int64_t frame_stride, int W, int h, int w,
                                                              int S, int C, int hc, int wc, uint8_t* __restrict__ cv_p,
                                                              uint8_t* __restrict__ ch_p)
{
    __shared__ uint8_t Y[SK_YROWS * SK_YCOLS];              // rows y0 - S .. y0 + 31 + S, columns x0 - S .. x0 + 63 + S, pitch 64 + 2 S
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * SK_TW, y0 = blockIdx.y * SK_TH;
    const uint8_t* __restrict__ fp = frames + (int64_t)blockIdx.z * frame_stride;
    const int cols = SK_TW + 2 * S, count = (SK_TH + 2 * S) * cols;
    // the source bytes of this thread's analysis pixels, summed per pixel ahead of the LDS stores (H * W * 3 < 2^31)
    int sum[SK_FILL];
#pragma unroll
    for (int s = 0; s < SK_FILL; ++s) {
        const int i = tid + s * SK_THREADS;
        sum[s] = 0;
        if (i < count) {
            const int ry = i / cols, rx = i - ry * cols;
            const int gy = min(max(y0 - S + ry, 0), h - 1), gx = min(max(x0 - S + rx, 0), w - 1);
            const uint8_t* __restrict__ q = fp + ((gy * F) * W + gx * F) * 3;
#pragma unroll
            for (int fy = 0; fy < F; ++fy)
#pragma unroll
                for (int fx = 0; fx < F; ++fx) {
                    const uint8_t* __restrict__ b = q + (fy * W + fx) * 3;
                    sum[s] += (29 * (int)b[0] + 150 * (int)b[1] + 77 * (int)b[2] + 128) >> 8;
                }
        }
    }
#pragma unroll
    for (int s = 0; s < SK_FILL; ++s) {
        const int i = tid + s * SK_THREADS;
        if (i < count) Y[i] = (uint8_t)((sum[s] + F * F / 2) / (F * F));
    }
    __syncthreads();
    // this thread's column: rows yt - 8 .. yt + 15 of the picture in col[0..23], of which yt - S .. yt + 7 + S are read
    const uint8_t* me = Y + (S + wave * SK_PER) * cols + S + lane;             // this thread's first pixel
    int col[SK_PER + 2 * SK_MAX_S];
#pragma unroll
    for (int i = 0; i < SK_PER + 2 * SK_MAX_S; ++i) {
        const int d = i - SK_MAX_S;                                            // the row's distance from yt
        col[i] = (d >= -S && d < SK_PER + S) ? (int)me[d * cols] : 0;
    }
    const int x = x0 + lane, yt = y0 + wave * SK_PER;
    int nv[2] = {0, 0}, nh[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < SK_PER; ++j) {
        const uint8_t* q = me + j * cols;
        const int c = col[SK_MAX_S + j];
        int loL = 255, loR = 255, hiL = 0, hiR = 0, loU = 255, loD = 255, hiU = 0, hiD = 0;
#pragma unroll
        for (int k = 1; k <= SK_MAX_S; ++k)
            if (k <= S) {
                const int l = q[-k], r = q[k], u = col[SK_MAX_S + j - k], d = col[SK_MAX_S + j + k];
                loL = min(loL, l), hiL = max(hiL, l), loR = min(loR, r), hiR = max(hiR, r);
                loU = min(loU, u), hiU = max(hiU, u), loD = min(loD, d), hiD = max(hiD, d);
            }
        const bool in = x < w && yt + j < h;
        const bool v = c - max(loL, loR) >= C || min(hiL, hiR) - c >= C;
        const bool hz = c - max(loU, loD) >= C || min(hiU, hiD) - c >= C;
        nv[j / SK_CELL] += in && v, nh[j / SK_CELL] += in && hz;
    }
    // a cell's 4 columns are 4 neighbouring lanes (x0 is a multiple of 4): every lane takes part, lane 4 b writes
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        nv[m] += __shfl_xor(nv[m], 1), nh[m] += __shfl_xor(nh[m], 1);
        nv[m] += __shfl_xor(nv[m], 2), nh[m] += __shfl_xor(nh[m], 2);
    }
    if ((lane & 3) != 0) return;
    const int b = x / SK_CELL;
    if (b >= wc) return;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int a = yt / SK_CELL + m;
        if (a >= hc) break;
        const int64_t at = ((int64_t)blockIdx.z * hc + a) * wc + b;
        cv_p[at] = (uint8_t)nv[m], ch_p[at] = (uint8_t)nh[m];
    }
}

// grid.x: tiles of 64 cell columns, grid.y: tiles of 32 cell rows, grid.z: the frame; 0 <= WX, WY <= SK_MAX_WIN
__global__ __launch_bounds__(SK_THREADS) void k_strokes_text(const uint8_t* __restrict__ cv_p, const uint8_t* __restrict__ ch_p, int hc, int wc,
                                                             int WX, int WY, int NV, int NH, float* __restrict__ text)
{
    __shared__ uint8_t V[SK_CROWS * SK_CCOLS], Hz[SK_CROWS * SK_CCOLS];        // the counts of the tile and its halo, pitch 64 + 2 WX
    __shared__ uint16_t RV[SK_CROWS * SK_TW], RH[SK_CROWS * SK_TW];           // the same rows, summed over 2 WX + 1 columns (<= 17 * 16)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * SK_TW, y0 = blockIdx.y * SK_TH;
    const int srows = SK_TH + 2 * WY, scols = SK_TW + 2 * WX;
    const int64_t plane = (int64_t)blockIdx.z * hc * wc;
    for (int i = tid; i < srows * scols; i += SK_THREADS) {
        const int ry = i / scols, rx = i - ry * scols;
        const int y = y0 - WY + ry, x = x0 - WX + rx;
        const bool in = y >= 0 && y < hc && x >= 0 && x < wc;
        const int64_t at = plane + (int64_t)y * wc + x;
        V[i] = in ? cv_p[at] : 0, Hz[i] = in ? ch_p[at] : 0;
    }
    __syncthreads();
    for (int i = tid; i < srows * SK_TW; i += SK_THREADS) {
        const int ry = i / SK_TW, cx = i - ry * SK_TW;
        const int at = ry * scols + cx;                     // the column cx - WX of the plane's tile
        int sv = 0, sh = 0;
        for (int d = 0; d <= 2 * WX; ++d) sv += V[at + d], sh += Hz[at + d];
        RV[i] = (uint16_t)sv, RH[i] = (uint16_t)sh;
    }
    __syncthreads();
    const int x = x0 + lane;
    if (x >= wc) return;
    for (int j = 0; j < SK_PER; ++j) {
        const int ry = wave * SK_PER + j, y = y0 + ry;
        if (y >= hc) break;
        int sv = 0, sh = 0;
        for (int d = 0; d <= 2 * WY; ++d) sv += RV[(ry + d) * SK_TW + lane], sh += RH[(ry + d) * SK_TW + lane];
        text[plane + (int64_t)y * wc + x] = (sv >= NV && sh >= NH) ? 1.0f : 0.0f;
    }
}

int kfail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

dim3 tiles(int rows, int cols, int n) { return dim3((unsigned)((cols + SK_TW - 1) / SK_TW), (unsigned)((rows + SK_TH - 1) / SK_TH), (unsigned)n); }

template <int F>
void launch_cells(const uint8_t* frames, int64_t frame_stride, int n, int H, int W, int S, int C, uint8_t* cv, uint8_t* ch, hipStream_t stream)
{
    const int h = H / F, w = W / F, hc = (h + SK_CELL - 1) / SK_CELL, wc = (w + SK_CELL - 1) / SK_CELL;
    hipLaunchKernelGGL(k_strokes_cells<F>, tiles(h, w, n), dim3(SK_THREADS), 0, stream, frames, frame_stride, W, h, w, S, C, hc, wc, cv, ch);
}

}  // namespace

extern "C" int vsr_strokes_cells_launch(const uint8_t* frames, int64_t frame_stride, int n, int H, int W, int F, int S, int C, uint8_t* cv,
                                        uint8_t* ch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    switch (F) {
    case 1: launch_cells<1>(frames, frame_stride, n, H, W, S, C, cv, ch, s); break;
    case 2: launch_cells<2>(frames, frame_stride, n, H, W, S, C, cv, ch, s); break;
    case 3: launch_cells<3>(frames, frame_stride, n, H, W, S, C, cv, ch, s); break;
    case 4: launch_cells<4>(frames, frame_stride, n, H, W, S, C, cv, ch, s); break;
    case 5: launch_cells<5>(frames, frame_stride, n, H, W, S, C, cv, ch, s); break;
    case 6: launch_cells<6>(frames, frame_stride, n, H, W, S, C, cv, ch, s); break;
    case 7: launch_cells<7>(frames, frame_stride, n, H, W, S, C, cv, ch, s); break;
    case 8: launch_cells<8>(frames, frame_stride, n, H, W, S, C, cv, ch, s); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

extern "C" int vsr_strokes_text_launch(const uint8_t* cv, const uint8_t* ch, int n, int hc, int wc, int WX, int WY, int NV, int NH, float* text,
                                       void* stream)
{
    hipLaunchKernelGGL(k_strokes_text, tiles(hc, wc, n), dim3(SK_THREADS), 0, (hipStream_t)stream, cv, ch, hc, wc, WX, WY, NV, NH, text);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int vsr_strokes_cells(const uint8_t* frames_dev, int64_t frame_stride, int n, int H, int W, int F, int S, int C, uint8_t* cv_dev, uint8_t* ch_dev,
                      void* stream)
{
    if (!frames_dev || !cv_dev || !ch_dev) return kfail(VSR_ERR_ARG, "strokes: null pointer");
    if (n < 1 || n > SK_MAX_N)
        return kfail(VSR_ERR_ARG, "strokes: n = " + std::to_string(n) + " frames, 1 <= n <= " + std::to_string(SK_MAX_N) + " are possible");
    if (H <= 0 || W <= 0) return kfail(VSR_ERR_ARG, "strokes: H and W must be positive");
    if ((int64_t)H * W * 3 > 0x7fffffffll) return kfail(VSR_ERR_ARG, "strokes: a frame of H * W * 3 >= 2^31 bytes is not supported");
    if (F < 1 || F > SK_MAX_F) return kfail(VSR_ERR_ARG, "strokes: F = " + std::to_string(F) + ", 1 <= F <= 8 are possible");
    if (H / F < 1 || W / F < 1) return kfail(VSR_ERR_ARG, "strokes: the frame is smaller than one analysis pixel");
    if (S < 1 || S > SK_MAX_S) return kfail(VSR_ERR_ARG, "strokes: S = " + std::to_string(S) + ", 1 <= S <= 8 are possible");
    if (C < 1 || C > 255) return kfail(VSR_ERR_ARG, "strokes: C = " + std::to_string(C) + ", a contrast lies in 1..255");
    if (frame_stride < (int64_t)H * W * 3) return kfail(VSR_ERR_ARG, "strokes: frame stride smaller than a frame");
    if (vsr_device_count() <= 0) return kfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (const int err = vsr_strokes_cells_launch(frames_dev, frame_stride, n, H, W, F, S, C, cv_dev, ch_dev, stream))
        return kfail(VSR_ERR_HIP, std::string("strokes cells launch failed: ") + hipGetErrorString((hipError_t)err));
    return 0;
}

int vsr_strokes_text(const uint8_t* cv_dev, const uint8_t* ch_dev, int n, int hc, int wc, int WX, int WY, int NV, int NH, float* text_dev,
                     void* stream)
{
    if (!cv_dev || !ch_dev || !text_dev) return kfail(VSR_ERR_ARG, "strokes: null pointer");
    if (n < 1 || n > SK_MAX_N)
        return kfail(VSR_ERR_ARG, "strokes: n = " + std::to_string(n) + " frames, 1 <= n <= " + std::to_string(SK_MAX_N) + " are possible");
    if (hc <= 0 || wc <= 0 || (int64_t)hc * wc > 0x7fffffffll / 5) return kfail(VSR_ERR_ARG, "strokes: hc and wc must be positive, hc * wc below 2^31 / 5");
    if (WX < 0 || WX > SK_MAX_WIN || WY < 0 || WY > SK_MAX_WIN)
        return kfail(VSR_ERR_ARG, "strokes: WX = " + std::to_string(WX) + ", WY = " + std::to_string(WY) + ", 0 <= WX, WY <= 8 are possible");
    if (NV < 0 || NV > 65535 || NH < 0 || NH > 65535) return kfail(VSR_ERR_ARG, "strokes: NV and NH lie in 0..65535");
    if ((uintptr_t)text_dev % 4) return kfail(VSR_ERR_ARG, "strokes: the text map is misaligned");
    if (vsr_device_count() <= 0) return kfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (const int err = vsr_strokes_text_launch(cv_dev, ch_dev, n, hc, wc, WX, WY, NV, NH, text_dev, stream))
        return kfail(VSR_ERR_HIP, std::string("strokes text launch failed: ") + hipGetErrorString((hipError_t)err));
    return 0;
}

}  // extern "C"
