// --glyph-key: the source kept wherever the fill only repeats it (the statement is tests/_key_statement.py).  Integer
// arithmetic only, bit-parallel where a wave's ballot makes it so: 64 pixels of a row are one 64-bit word.
//
//   k_key_seeds     per frame and tile of 64 columns x 32 rows: D = max over the channels of |src - fill| where C != 0 (src and the fill
//                   are read nowhere else), the tile with a one-pixel halo in LDS, the 3 x 3 sum A per pixel, and per row of the tile
//                   one ballot of A >= 9 T: a word of the seed bitmap [n][s1 - s0][ceil(W / 64)], bit i = column 64 w + i.  Every word
//                   of the bitmap's rows is written, so the workspace needs no zeroing.
//   k_key_apply     per frame and tile of 64 columns x 32 rows of C's rows: the bitmap's words of the tile's rows +- (G + R - 1), with
//                   the words to the left and right, in LDS; H_k = the row's word dilated by k bits to either side with carries across
//                   the word boundaries, V_k(y) = the OR of H_k over the rows y - k .. y + k, for k = 0 .. G + R - 1; a pixel's
//                   weight is min(R, the number of k whose V_k has its bit): V_k grows with k, so that number is G + R - e.  Then
//                   (a fill + (R - a) src + R / 2) / R on the pixels of C, in place: a pixel writes from its own bytes only.
//
// --glyph-hold K (the statement is tests/_hold_statement.py) holds a weak seed while a neighbouring frame of the call
// is strongly different at that place:
//   k_key_seeds2    k_key_seeds with two ballots per row, A >= 9 T and A >= 9 ((T + 1) / 2): the strong and the weak bitmap.
//   k_key_hold      per frame and tile of one word x 32 rows of the bitmap: the OR of the strong words of the frames within K of f, f
//                   itself left out, dilated by one pixel; held = strong | (weak & that), a third bitmap that k_key_apply then reads.
//
// The frames hold `rows` rows of the picture starting at its row y0 (the whole picture, or sttn-auto's strip rows); C is the whole
// picture's.  A seed needs a pixel of C in its 3 x 3 neighbourhood, so the bitmap's rows are [s0, s1) = the rows [c0 - 1, c1 + 1) of
// the picture that the frames hold; rows beyond them hold no seed.  A frame is rows * W * 3 contiguous bytes at any alignment, frames
// and src have their own strides.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "key_kernels.h"
#include "plan_c.h"

namespace {

constexpr int KY_G = 4, KY_R = 4, KY_REACH = KY_G + KY_R - 1, KY_K = KY_G + KY_R, KY_MAX_T = 128, KY_MAX_K = 8;
constexpr int KY_THREADS = 256, KY_WAVES = KY_THREADS / 64, KY_TILE = 32;       // rows of a tile: 8 per wave
constexpr int KY_DPITCH = 68;                                                    // bytes of a row of D in LDS: 64 + 2 of halo, padded
constexpr int KY_HROWS = KY_TILE + 2 * KY_REACH;                                 // rows of the bitmap a tile of k_key_apply reads
constexpr int KY_MAX_GZ = 1024;

// the body of both seed kernels.  HOLD: a second ballot per row, A >= T9lo, into `weak` (the same layout); without it T9lo and weak are
// not read and the code is k_key_seeds' of before
template <bool HOLD>
__device__ __forceinline__ void key_seeds(const uint8_t* __restrict__ frames, int64_t frame_stride, const uint8_t* __restrict__ src,
                                          int64_t src_stride, const uint8_t* __restrict__ cmask, int n, int W, int y0, int rows, int sa, int sb,
                                          int nw, int T9, int T9lo, unsigned long long* __restrict__ bitmap,
                                          unsigned long long* __restrict__ weak)
{
    __shared__ uint8_t D[(KY_TILE + 2) * KY_DPITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * 64, r0 = sa + blockIdx.y * KY_TILE;             // the tile's first column and first row of the frames
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const uint8_t* __restrict__ fp = frames + (int64_t)f * frame_stride;
        const uint8_t* __restrict__ sp = src + (int64_t)f * src_stride;
        for (int i = tid; i < (KY_TILE + 2) * 66; i += KY_THREADS) {
            const int ry = i / 66, rx = i - ry * 66;
            const int ly = r0 - 1 + ry, x = x0 - 1 + rx;
            int d = 0;
            if (ly >= 0 && ly < rows && x >= 0 && x < W && cmask[(int64_t)(y0 + ly) * W + x]) {
                const int64_t at = ((int64_t)ly * W + x) * 3;
                const int d0 = abs((int)sp[at] - (int)fp[at]), d1 = abs((int)sp[at + 1] - (int)fp[at + 1]);
                const int d2 = abs((int)sp[at + 2] - (int)fp[at + 2]);
                d = max(d0, max(d1, d2));
            }
            D[ry * KY_DPITCH + rx] = (uint8_t)d;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KY_TILE / KY_WAVES; ++j) {
            const int ry = wave * (KY_TILE / KY_WAVES) + j, ly = r0 + ry;       // (wave-uniform)
            if (ly >= sb) break;
            const uint8_t* q = D + ry * KY_DPITCH + lane;                      // the row above, its column to the left
            const int A = q[0] + q[1] + q[2] + q[KY_DPITCH] + q[KY_DPITCH + 1] + q[KY_DPITCH + 2] + q[2 * KY_DPITCH] +
                          q[2 * KY_DPITCH + 1] + q[2 * KY_DPITCH + 2];
            const unsigned long long word = __ballot(x0 + lane < W && A >= T9);
            if (lane == 0) bitmap[((int64_t)f * (sb - sa) + (ly - sa)) * nw + blockIdx.x] = word;
            if constexpr (HOLD) {
                const unsigned long long low = __ballot(x0 + lane < W && A >= T9lo);
                if (lane == 0) weak[((int64_t)f * (sb - sa) + (ly - sa)) * nw + blockIdx.x] = low;
            }
        }
        __syncthreads();                                                        // the next frame's D
    }
}

// grid.x: the words of a row, grid.y: tiles of 32 rows of the bitmap, grid.z strides the frames.  [sa, sb): the bitmap's rows, as rows
// of the frames
__global__ __launch_bounds__(KY_THREADS) void k_key_seeds(const uint8_t* __restrict__ frames, int64_t frame_stride, const uint8_t* __restrict__ src,
                                                          int64_t src_stride, const uint8_t* __restrict__ cmask, int n, int W, int y0, int rows,
                                                          int sa, int sb, int nw, int T9, unsigned long long* __restrict__ bitmap)
{
    key_seeds<false>(frames, frame_stride, src, src_stride, cmask, n, W, y0, rows, sa, sb, nw, T9, 0, bitmap, nullptr);
}

// the same grid; two ballots per row: `strong` takes A >= T9 (k_key_seeds' bitmap), `weak` A >= T9lo
__global__ __launch_bounds__(KY_THREADS) void k_key_seeds2(const uint8_t* __restrict__ frames, int64_t frame_stride, const uint8_t* __restrict__ src,
                                                           int64_t src_stride, const uint8_t* __restrict__ cmask, int n, int W, int y0, int rows,
                                                           int sa, int sb, int nw, int T9, int T9lo, unsigned long long* __restrict__ strong,
                                                           unsigned long long* __restrict__ weak)
{
    key_seeds<true>(frames, frame_stride, src, src_stride, cmask, n, W, y0, rows, sa, sb, nw, T9, T9lo, strong, weak);
}

// grid.x: the words of a row, grid.y: tiles of 32 rows of the bitmap, grid.z strides the frames.  U = the OR of the strong words of the
// frames g != f, |g - f| <= K, 0 <= g < n, for the tile's rows +- 1 and the words to the left and right (beyond the bitmap: 0), in LDS;
// per row the OR of the three rows' words, dilated by one bit to either side with the carries from the neighbouring words; then
// held = strong(f) | (weak(f) & that).  Every word of the bitmap's rows is written; strong(f) is still read by the frames around f, so
// `held` is a bitmap of its own
__global__ __launch_bounds__(KY_THREADS) void k_key_hold(const unsigned long long* __restrict__ strong, const unsigned long long* __restrict__ weak,
                                                         unsigned long long* __restrict__ held, int n, int K, int srows, int nw)
{
    __shared__ unsigned long long U[(KY_TILE + 2) * 3];     // left, own, right
    const int tid = threadIdx.x, w = blockIdx.x, r0 = blockIdx.y * KY_TILE;     // the tile's first row of the bitmap
    const int64_t per = (int64_t)srows * nw;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        if (tid < (KY_TILE + 2) * 3) {
            const int hr = tid / 3, side = tid - hr * 3;
            const int y = r0 - 1 + hr, ww = w - 1 + side;
            unsigned long long u = 0;
            if (y >= 0 && y < srows && ww >= 0 && ww < nw) {
                const int ga = f - K > 0 ? f - K : 0, gb = f + K < n - 1 ? f + K : n - 1;
                const unsigned long long* __restrict__ at = strong + (int64_t)y * nw + ww;
                for (int g = ga; g <= gb; ++g)
                    if (g != f) u |= at[g * per];
            }
            U[tid] = u;
        }
        __syncthreads();
        if (tid < KY_TILE && r0 + tid < srows) {
            const unsigned long long* q = U + tid * 3;                          // the row above
            const unsigned long long l = q[0] | q[3] | q[6], c = q[1] | q[4] | q[7], r = q[2] | q[5] | q[8];
            const unsigned long long near = c | (c << 1) | (l >> 63) | (c >> 1) | (r << 63);
            const int64_t i = f * per + (int64_t)(r0 + tid) * nw + w;
            held[i] = strong[i] | (weak[i] & near);
        }
        __syncthreads();                                                        // the next frame's U
    }
}

// grid.x: the words of a row, grid.y: tiles of 32 rows of [la, lb) (the rows of C's bounding rows that the frames hold), grid.z strides the
// frames
__global__ __launch_bounds__(KY_THREADS) void k_key_apply(uint8_t* __restrict__ frames, int64_t frame_stride, const uint8_t* __restrict__ src,
                                                          int64_t src_stride, const uint8_t* __restrict__ cmask, int n, int W, int y0, int la,
                                                          int lb, int sa, int sb, int nw, const unsigned long long* __restrict__ bitmap)
{
    __shared__ unsigned long long S[KY_HROWS * 3];          // the seed words: left, own, right
    __shared__ unsigned long long Hk[KY_HROWS * KY_K];
    __shared__ unsigned long long V[KY_TILE * KY_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = blockIdx.x, r0 = la + blockIdx.y * KY_TILE;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const unsigned long long* __restrict__ bm = bitmap + (int64_t)f * (sb - sa) * nw;
        if (tid < KY_HROWS * 3) {
            const int hr = tid / 3, side = tid - hr * 3;
            const int ly = r0 - KY_REACH + hr, ww = w - 1 + side;
            S[tid] = (ly >= sa && ly < sb && ww >= 0 && ww < nw) ? bm[(int64_t)(ly - sa) * nw + ww] : 0ull;
        }
        __syncthreads();
        for (int i = tid; i < KY_HROWS * KY_K; i += KY_THREADS) {
            const int hr = i / KY_K, k = i - hr * KY_K;
            const unsigned long long l = S[hr * 3], c = S[hr * 3 + 1], r = S[hr * 3 + 2];
            unsigned long long h = c;
            for (int j = 1; j <= k; ++j) h |= (c << j) | (l >> (64 - j)) | (c >> j) | (r << (64 - j));
            Hk[i] = h;
        }
        __syncthreads();
        {
            const int ry = tid / KY_K, k = tid - ry * KY_K;                    // KY_THREADS == KY_TILE * KY_K
            unsigned long long v = 0;
            for (int d = -k; d <= k; ++d) v |= Hk[(ry + KY_REACH + d) * KY_K + k];
            V[tid] = v;
        }
        __syncthreads();
        uint8_t* __restrict__ fp = frames + (int64_t)f * frame_stride;
        const uint8_t* __restrict__ sp = src + (int64_t)f * src_stride;
        const int x = w * 64 + lane;
#pragma unroll
        for (int j = 0; j < KY_TILE / KY_WAVES; ++j) {
            const int ry = wave * (KY_TILE / KY_WAVES) + j, ly = r0 + ry;       // (wave-uniform)
            if (ly >= lb) break;
            int a = 0;
#pragma unroll
            for (int k = 0; k < KY_K; ++k) a += (int)((V[ry * KY_K + k] >> lane) & 1ull);
            a = min(a, KY_R);
            if (a == KY_R || x >= W || !cmask[(int64_t)(y0 + ly) * W + x]) continue;
            const int64_t at = ((int64_t)ly * W + x) * 3;
            if (a == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) fp[at + c] = sp[at + c];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) fp[at + c] = (uint8_t)((a * (int)fp[at + c] + (KY_R - a) * (int)sp[at + c] + KY_R / 2) / KY_R);
            }
        }
        __syncthreads();                                                        // the next frame's words
    }
}

static_assert(KY_THREADS == KY_TILE * KY_K, "a thread per (row, k) of a tile");
static_assert(KY_HROWS * 3 <= KY_THREADS, "a thread per seed word of a tile");

int gfail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

const char* bad_picture(int H, int W)
{
    if (H <= 0 || W <= 0) return "glyph key: H and W must be positive";
    if ((int64_t)H * W * 3 > 0x7fffffffll) return "glyph key: a frame of H * W * 3 >= 2^31 bytes is not supported";
    return nullptr;
}

}  // namespace

extern "C" int vsr_key_launch(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride, const uint8_t* cmask, int n,
                              int H, int W, int y0, int rows, int c0, int c1, int T, void* workspace, void* stream)
{
    (void)H;
    const int la = c0 - y0 > 0 ? c0 - y0 : 0;
    const int lb = c1 - y0 < rows ? c1 - y0 : rows;
    if (lb <= la) return 0;                                  // the frames hold no pixel of the mask
    const int sa = la > 0 ? la - 1 : 0, sb = lb < rows ? lb + 1 : rows;
    const int nw = (W + 63) / 64;
    const unsigned gz = (unsigned)(n < KY_MAX_GZ ? n : KY_MAX_GZ);
    unsigned long long* bitmap = (unsigned long long*)workspace;
    hipLaunchKernelGGL(k_key_seeds, dim3((unsigned)nw, (unsigned)((sb - sa + KY_TILE - 1) / KY_TILE), gz), dim3(KY_THREADS), 0,
                       (hipStream_t)stream, frames, frame_stride, src, src_frame_stride, cmask, n, W, y0, rows, sa, sb, nw, 9 * T, bitmap);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_key_apply, dim3((unsigned)nw, (unsigned)((lb - la + KY_TILE - 1) / KY_TILE), gz), dim3(KY_THREADS), 0,
                       (hipStream_t)stream, frames, frame_stride, src, src_frame_stride, cmask, n, W, y0, la, lb, sa, sb, nw, bitmap);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// k_key_seeds alone, for --borrow (borrow_kernels.hip): the bitmap [n][sb - sa][nw] of the rows [sa, sb) of the frames, every word written
extern "C" int vsr_key_seeds_launch(const uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride,
                                    const uint8_t* cmask, int n, int W, int y0, int rows, int sa, int sb, int T, void* bitmap, void* stream)
{
    const int nw = (W + 63) / 64;
    const unsigned gz = (unsigned)(n < KY_MAX_GZ ? n : KY_MAX_GZ);
    hipLaunchKernelGGL(k_key_seeds, dim3((unsigned)nw, (unsigned)((sb - sa + KY_TILE - 1) / KY_TILE), gz), dim3(KY_THREADS), 0,
                       (hipStream_t)stream, frames, frame_stride, src, src_frame_stride, cmask, n, W, y0, rows, sa, sb, nw, 9 * T,
                       (unsigned long long*)bitmap);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// three launches: the strong and the weak seeds, the held seeds, k_key_apply on the held seeds.  The workspace holds the three bitmaps
// [n][sb - sa][nw] one behind the other
extern "C" int vsr_key_hold_launch(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride, const uint8_t* cmask, int n,
                                   int H, int W, int y0, int rows, int c0, int c1, int T, int K, void* workspace, void* stream)
{
    (void)H;
    const int la = c0 - y0 > 0 ? c0 - y0 : 0;
    const int lb = c1 - y0 < rows ? c1 - y0 : rows;
    if (lb <= la) return 0;                                  // the frames hold no pixel of the mask
    const int sa = la > 0 ? la - 1 : 0, sb = lb < rows ? lb + 1 : rows;
    const int nw = (W + 63) / 64;
    const unsigned gz = (unsigned)(n < KY_MAX_GZ ? n : KY_MAX_GZ);
    const int64_t words = (int64_t)n * (sb - sa) * nw;
    unsigned long long* strong = (unsigned long long*)workspace;
    unsigned long long *weak = strong + words, *held = weak + words;
    const dim3 seed_grid((unsigned)nw, (unsigned)((sb - sa + KY_TILE - 1) / KY_TILE), gz);
    hipLaunchKernelGGL(k_key_seeds2, seed_grid, dim3(KY_THREADS), 0, (hipStream_t)stream, frames, frame_stride, src, src_frame_stride, cmask, n, W,
                       y0, rows, sa, sb, nw, 9 * T, 9 * ((T + 1) / 2), strong, weak);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_key_hold, seed_grid, dim3(KY_THREADS), 0, (hipStream_t)stream, strong, weak, held, n, K, sb - sa, nw);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_key_apply, dim3((unsigned)nw, (unsigned)((lb - la + KY_TILE - 1) / KY_TILE), gz), dim3(KY_THREADS), 0,
                       (hipStream_t)stream, frames, frame_stride, src, src_frame_stride, cmask, n, W, y0, la, lb, sa, sb, nw, held);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int64_t vsr_key_workspace_bytes(int H, int W, int n)
{
    if (n < 0) return gfail(VSR_ERR_ARG, "glyph key: negative frame count");
    if (const char* why = bad_picture(H, W)) return gfail(VSR_ERR_ARG, why);
    const int64_t per = (int64_t)H * ((W + 63) / 64) * 8;
    if (n > 0 && per > INT64_MAX / n) return gfail(VSR_ERR_ARG, "glyph key: the workspace of so many frames has no size");
    return per * n;
}

// the refusals of vsr_key_apply and vsr_key_apply_hold: 0, or the error code with its message set
static int key_refusal(const void* frames_dev, int64_t frame_stride, const void* src_dev, int64_t src_frame_stride, const void* cmask_dev, int n,
                       int H, int W, int y0, int rows, int c0, int c1, int T, const void* workspace_dev)
{
    if (!frames_dev || !src_dev || !cmask_dev || !workspace_dev) return gfail(VSR_ERR_ARG, "glyph key: null pointer");
    if (n < 0) return gfail(VSR_ERR_ARG, "glyph key: negative frame count");
    if (const char* why = bad_picture(H, W)) return gfail(VSR_ERR_ARG, why);
    if (y0 < 0 || rows <= 0 || y0 > H - rows) return gfail(VSR_ERR_ARG, "glyph key: the rows held must lie inside the frame");
    if (c0 < 0 || c1 < c0 || c1 > H) return gfail(VSR_ERR_ARG, "glyph key: the mask's rows must lie inside the frame");
    if (T < 1 || T > KY_MAX_T)
        return gfail(VSR_ERR_ARG, "glyph key: T = " + std::to_string(T) + ", 1 <= T <= " + std::to_string(KY_MAX_T) + " are possible");
    const int64_t N = (int64_t)rows * W * 3;
    if (frame_stride < N || src_frame_stride < N) return gfail(VSR_ERR_ARG, "glyph key: frame stride smaller than a frame");
    if ((uintptr_t)workspace_dev % 8) return gfail(VSR_ERR_ARG, "glyph key: the workspace must be 8-byte aligned");
    return 0;
}

int vsr_key_apply(uint8_t* frames_dev, int64_t frame_stride, const uint8_t* src_dev, int64_t src_frame_stride, const uint8_t* cmask_dev, int n,
                  int H, int W, int y0, int rows, int c0, int c1, int T, void* workspace_dev, void* stream)
{
    if (int rc = key_refusal(frames_dev, frame_stride, src_dev, src_frame_stride, cmask_dev, n, H, W, y0, rows, c0, c1, T, workspace_dev)) return rc;
    if (n == 0 || c0 == c1) return 0;
    if (vsr_key_workspace_bytes(H, W, n) < 0) return VSR_ERR_ARG;
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_key_launch(frames_dev, frame_stride, src_dev, src_frame_stride, cmask_dev, n, H, W, y0, rows, c0, c1, T, workspace_dev, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("glyph key launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

int64_t vsr_key_hold_workspace_bytes(int H, int W, int n)
{
    const int64_t one = vsr_key_workspace_bytes(H, W, n);
    if (one < 0) return one;
    if (one > INT64_MAX / 3) return gfail(VSR_ERR_ARG, "glyph key: the workspace of so many frames has no size");
    return 3 * one;
}

int vsr_key_apply_hold(uint8_t* frames_dev, int64_t frame_stride, const uint8_t* src_dev, int64_t src_frame_stride, const uint8_t* cmask_dev,
                       int n, int H, int W, int y0, int rows, int c0, int c1, int T, int K, void* workspace_dev, void* stream)
{
    if (int rc = key_refusal(frames_dev, frame_stride, src_dev, src_frame_stride, cmask_dev, n, H, W, y0, rows, c0, c1, T, workspace_dev)) return rc;
    if (K < 1 || K > KY_MAX_K)
        return gfail(VSR_ERR_ARG, "glyph key: hold K = " + std::to_string(K) + ", 1 <= K <= " + std::to_string(KY_MAX_K) + " are possible");
    if (n == 0 || c0 == c1) return 0;
    if (vsr_key_hold_workspace_bytes(H, W, n) < 0) return VSR_ERR_ARG;
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_key_hold_launch(frames_dev, frame_stride, src_dev, src_frame_stride, cmask_dev, n, H, W, y0, rows, c0, c1, T, K, workspace_dev,
                            stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("glyph key launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // extern "C"
