// --borrow: the fill replaced by the real picture of a neighbouring frame of the same call (the statement is
// tests/_borrow_statement.py).  Integer arithmetic only, bit-parallel on the glyph key's 64-bit seed words (key_kernels.hip).
//
//   k_key_seeds     the key's own kernel, through vsr_key_seeds_launch: bitmap 1 = the seeds at T of every frame.
//   k_borrow_near   per frame and tile of one word x 32 rows of the bitmap: the words of the tile's rows +- (G + R - 1) with the words to the
//                   left and right in LDS, every row's word dilated by G + R - 1 bits to either side with the carries across the word
//                   boundaries, then the OR over the rows y - (G + R - 1) .. y + (G + R - 1): bitmap 2 = N, the pixels where the key's
//                   weight is not 0.  Rows beyond the bitmap's hold no seed; every word of the bitmap's rows is written.
//   k_borrow_take   per frame and tile of 64 columns x 32 rows of C's rows: one thread turns the frame's pair sums, the ring's noise sums
//                   and |E| into the thresholds (24 b) >> 4 of its up to 2 B lenders, in the order t-1, t+1, t-2, .. (the only division);
//                   a wave works per row, a lane per pixel.  A lane with its N_t bit and C != 0 walks the lenders: N_s's word of the
//                   row is one address per wave, the first lender with its bit clear and max_c |src_s - fill_t| under the threshold gives
//                   its three source bytes.  A pixel reads its own fill bytes and src only: in place, no snapshot.
//
// The frames hold `rows` rows of the picture starting at its row y0 (the whole picture, or sttn-auto's strip rows); C is the whole
// picture's.  The bitmaps' rows are the key's, [sa, sb) = the rows [c0 - 1, c1 + 1) of the picture that the frames hold.  A frame is
// rows * W * 3 contiguous bytes at any alignment, frames and src have their own strides.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "borrow_kernels.h"
#include "key_kernels.h"
#include "plan_c.h"

namespace {

constexpr int BW_REACH = 7;                                  // G + R - 1 of the key
constexpr int BW_MAX_B = 8, BW_MAX_T = 128, BW_TH = 24, BW_FULL = 16;
constexpr uint64_t BW_GRAIN = 15447;                         // round(2^16 * sqrt(2) / 6), deflicker's
constexpr int BW_THREADS = 256, BW_WAVES = BW_THREADS / 64, BW_TILE = 32;       // rows of a tile: 8 per wave
constexpr int BW_HROWS = BW_TILE + 2 * BW_REACH;             // rows of the seed bitmap a tile of k_borrow_near reads
constexpr int BW_MAX_GZ = 1024;

// grid.x: the words of a row, grid.y: tiles of 32 rows of the bitmap, grid.z strides the frames
__global__ __launch_bounds__(BW_THREADS) void k_borrow_near(const unsigned long long* __restrict__ seeds, unsigned long long* __restrict__ near,
                                                            int n, int srows, int nw)
{
    __shared__ unsigned long long S[BW_HROWS * 3];          // the seed words: left, own, right
    __shared__ unsigned long long Hd[BW_HROWS];
    const int tid = threadIdx.x, w = blockIdx.x, r0 = blockIdx.y * BW_TILE;     // the tile's first row of the bitmap
    const int64_t per = (int64_t)srows * nw;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        if (tid < BW_HROWS * 3) {
            const int hr = tid / 3, side = tid - hr * 3;
            const int y = r0 - BW_REACH + hr, ww = w - 1 + side;
            S[tid] = (y >= 0 && y < srows && ww >= 0 && ww < nw) ? seeds[f * per + (int64_t)y * nw + ww] : 0ull;
        }
        __syncthreads();
        if (tid < BW_HROWS) {
            const unsigned long long l = S[tid * 3], c = S[tid * 3 + 1], r = S[tid * 3 + 2];
            unsigned long long h = c;
#pragma unroll
            for (int j = 1; j <= BW_REACH; ++j) h |= (c << j) | (l >> (64 - j)) | (c >> j) | (r << (64 - j));
            Hd[tid] = h;
        }
        __syncthreads();
        if (tid < BW_TILE && r0 + tid < srows) {
            unsigned long long v = 0;
#pragma unroll
            for (int d = 0; d <= 2 * BW_REACH; ++d) v |= Hd[tid + d];
            near[f * per + (int64_t)(r0 + tid) * nw + w] = v;
        }
        __syncthreads();                                     // the next frame's words
    }
}

// grid.x: the words of a row, grid.y: tiles of 32 rows of [la, lb) (the rows of C's bounding rows that the frames hold), grid.z strides the
// frames.  stats: vsr_regrain_measure's four words per frame (word 0 = A); counts[0] = |E|; pairs: vsr_deflicker_pairs' with R = B
__global__ __launch_bounds__(BW_THREADS) void k_borrow_take(uint8_t* __restrict__ frames, int64_t frame_stride, const uint8_t* __restrict__ src,
                                                            int64_t src_stride, const uint8_t* __restrict__ cmask,
                                                            const unsigned long long* __restrict__ counts,
                                                            const unsigned long long* __restrict__ stats,
                                                            const unsigned long long* __restrict__ pairs, int n, int W, int y0, int la, int lb,
                                                            int sa, int srows, int nw, int B, const unsigned long long* __restrict__ near)
{
    __shared__ int s_thr[2 * BW_MAX_B];                      // the threshold of lender j; 0: lends nothing
    __shared__ int s_frame[2 * BW_MAX_B];                    // its frame
    __shared__ int s_any;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = blockIdx.x, r0 = la + blockIdx.y * BW_TILE;
    const int x = w * 64 + lane;
    const int64_t per = (int64_t)srows * nw;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        __syncthreads();                                     // (the previous frame's values are read by now)
        if (tid == 0) {
            const uint64_t m = 3 * (uint64_t)counts[0];
            const uint64_t a_t = stats[(int64_t)f * 4];
            int any = 0;
            for (int j = 0; j < 2 * B; ++j) {
                const int k = (j >> 1) + 1, s = (j & 1) ? f + k : f - k;
                int thr = 0;
                if (m && s >= 0 && s < n) {
                    const int lo = s < f ? s : f;
                    const uint64_t sum = pairs[(int64_t)lo * B + (k - 1)];
                    const uint64_t floor = (BW_GRAIN * (a_t + (uint64_t)stats[(int64_t)s * 4])) >> 17;
                    const uint64_t moved = sum > floor ? sum - floor : 0;
                    if (moved < 4 * m) {
                        const uint64_t q = (BW_FULL * (4 * m - moved)) / (3 * m);
                        thr = (BW_TH * (q < (uint64_t)BW_FULL ? (int)q : BW_FULL)) >> 4;
                    }
                }
                s_thr[j] = thr;
                s_frame[j] = s;
                any |= thr;
            }
            s_any = any;
        }
        __syncthreads();
        if (!s_any) continue;                                // every pair closed: the frame stays as it is
        uint8_t* __restrict__ fp = frames + (int64_t)f * frame_stride;
        for (int i = 0; i < BW_TILE / BW_WAVES; ++i) {
            const int ly = r0 + wave * (BW_TILE / BW_WAVES) + i;                // (wave-uniform)
            if (ly >= lb) break;
            const int64_t word = (int64_t)(ly - sa) * nw + w;
            const unsigned long long own = near[f * per + word];
            bool want = ((own >> lane) & 1ull) && x < W && cmask[(int64_t)(y0 + ly) * W + x] != 0;
            if (!__any(want)) continue;
            const int64_t at = ((int64_t)ly * W + x) * 3;
            int b0 = 0, b1 = 0, b2 = 0;
            if (want) {
                b0 = fp[at];
                b1 = fp[at + 1];
                b2 = fp[at + 2];
            }
            for (int j = 0; j < 2 * B; ++j) {
                const int thr = s_thr[j];
                if (thr == 0) continue;
                const int s = s_frame[j];
                const unsigned long long theirs = near[s * per + word];         // one address per wave and lender (a vector load: s comes from LDS)
                if (want && !((theirs >> lane) & 1ull)) {
                    const uint8_t* __restrict__ q = src + (int64_t)s * src_stride + at;
                    const int v0 = q[0], v1 = q[1], v2 = q[2];
                    if (max(max(abs(v0 - b0), abs(v1 - b1)), abs(v2 - b2)) < thr) {
                        fp[at] = (uint8_t)v0;
                        fp[at + 1] = (uint8_t)v1;
                        fp[at + 2] = (uint8_t)v2;
                        want = false;
                    }
                }
                if (!__any(want)) break;
            }
        }
    }
}

static_assert(BW_HROWS * 3 <= BW_THREADS, "a thread per seed word of a tile");

int gfail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

const char* bad_picture(int H, int W)
{
    if (H <= 0 || W <= 0) return "borrow: H and W must be positive";
    if ((int64_t)H * W * 3 > 0x7fffffffll) return "borrow: a frame of H * W * 3 >= 2^31 bytes is not supported";
    return nullptr;
}

}  // namespace

// three launches.  The workspace holds the two bitmaps [n][sb - sa][nw] one behind the other
extern "C" int vsr_borrow_launch(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride, const uint8_t* cmask,
                                 const uint64_t* counts, const uint64_t* stats, const uint64_t* pairs, int n, int H, int W, int y0, int rows,
                                 int c0, int c1, int T, int B, void* workspace, void* stream)
{
    (void)H;
    const int la = c0 - y0 > 0 ? c0 - y0 : 0;
    const int lb = c1 - y0 < rows ? c1 - y0 : rows;
    if (lb <= la) return 0;                                  // the frames hold no pixel of the mask
    const int sa = la > 0 ? la - 1 : 0, sb = lb < rows ? lb + 1 : rows;
    const int nw = (W + 63) / 64, srows = sb - sa;
    const unsigned gz = (unsigned)(n < BW_MAX_GZ ? n : BW_MAX_GZ);
    unsigned long long* seeds = (unsigned long long*)workspace;
    unsigned long long* near = seeds + (int64_t)n * srows * nw;
    if (vsr_key_seeds_launch(frames, frame_stride, src, src_frame_stride, cmask, n, W, y0, rows, sa, sb, T, seeds, stream) != 0) return -1;
    hipLaunchKernelGGL(k_borrow_near, dim3((unsigned)nw, (unsigned)((srows + BW_TILE - 1) / BW_TILE), gz), dim3(BW_THREADS), 0,
                       (hipStream_t)stream, seeds, near, n, srows, nw);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_borrow_take, dim3((unsigned)nw, (unsigned)((lb - la + BW_TILE - 1) / BW_TILE), gz), dim3(BW_THREADS), 0,
                       (hipStream_t)stream, frames, frame_stride, src, src_frame_stride, cmask, (const unsigned long long*)counts,
                       (const unsigned long long*)stats, (const unsigned long long*)pairs, n, W, y0, la, lb, sa, srows, nw, B, near);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int64_t vsr_borrow_workspace_bytes(int H, int W, int n)
{
    if (n < 0) return gfail(VSR_ERR_ARG, "borrow: negative frame count");
    if (const char* why = bad_picture(H, W)) return gfail(VSR_ERR_ARG, why);
    const int64_t per = (int64_t)H * ((W + 63) / 64) * 16;   // two bitmaps of the key's
    if (n > 0 && per > INT64_MAX / n) return gfail(VSR_ERR_ARG, "borrow: the workspace of so many frames has no size");
    return per * n;
}

int vsr_borrow_apply(uint8_t* frames_dev, int64_t frame_stride, const uint8_t* src_dev, int64_t src_frame_stride, const uint8_t* cmask_dev,
                     const uint64_t* counts_dev, const uint64_t* stats_dev, const uint64_t* pairs_dev, int n, int H, int W, int y0, int rows,
                     int c0, int c1, int T, int B, void* workspace_dev, void* stream)
{
    if (!frames_dev || !src_dev || !cmask_dev || !counts_dev || !stats_dev || !pairs_dev || !workspace_dev)
        return gfail(VSR_ERR_ARG, "borrow: null pointer");
    if (n < 0) return gfail(VSR_ERR_ARG, "borrow: negative frame count");
    if (const char* why = bad_picture(H, W)) return gfail(VSR_ERR_ARG, why);
    if (y0 < 0 || rows <= 0 || y0 > H - rows) return gfail(VSR_ERR_ARG, "borrow: the rows held must lie inside the frame");
    if (c0 < 0 || c1 < c0 || c1 > H) return gfail(VSR_ERR_ARG, "borrow: the mask's rows must lie inside the frame");
    if (T < 1 || T > BW_MAX_T)
        return gfail(VSR_ERR_ARG, "borrow: T = " + std::to_string(T) + ", 1 <= T <= " + std::to_string(BW_MAX_T) + " are possible");
    if (B < 1 || B > BW_MAX_B)
        return gfail(VSR_ERR_ARG, "borrow: B = " + std::to_string(B) + ", 1 <= B <= " + std::to_string(BW_MAX_B) + " are possible");
    const int64_t N = (int64_t)rows * W * 3;
    if (frame_stride < N || src_frame_stride < N) return gfail(VSR_ERR_ARG, "borrow: frame stride smaller than a frame");
    if ((uintptr_t)workspace_dev % 8) return gfail(VSR_ERR_ARG, "borrow: the workspace must be 8-byte aligned");
    if (n < 2 || c0 == c1) return 0;                         // one frame has no neighbour
    if (vsr_borrow_workspace_bytes(H, W, n) < 0) return VSR_ERR_ARG;
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_borrow_launch(frames_dev, frame_stride, src_dev, src_frame_stride, cmask_dev, counts_dev, stats_dev, pairs_dev, n, H, W, y0, rows,
                          c0, c1, T, B, workspace_dev, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("borrow launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // extern "C"
