// --borrow-pan: --borrow made to follow a camera that pans by whole pixels (the statement is
// tests/_borrow_pan_statement.py).  Integer arithmetic only.  borrow_kernels.hip serves P = 0 and stays as it is.
//
//   k_pan_search1   level k = 1, a lane per candidate shift.  A workgroup owns a tile of 16 rows x 32 columns of the rows that can hold E.
//                   Once: the tile's E samples, compacted into LDS.  Per frame t: the samples of src_t as one dword per pixel with their
//                   offset in the other tile, and the tile of src_{t+1} with a halo of 8, a dword per pixel whose top byte says "no valid
//                   target" (off the rows held, or C != 0).  The row pitch of that tile is = 2 P + 1 mod 32 dwords, so that the lanes of
//                   two rows of candidates read distinct banks.  A lane walks the samples: the sample is an LDS broadcast (one
//                   ds_read_b64), the shifted one a ds_read_b32, then one v_sad_u8 into a private sum; at the end one atomic pair per
//                   lane and workgroup.
//   k_pan_searchk   level k >= 2, a lane per pixel of a tile of 8 rows x 32 columns, ten candidates.  Every workgroup finds the centre
//                   itself: the best of level k - 1 of frame t and of level 1 of frame t + k - 1 from the table (pan_best, integer, the
//                   same in every workgroup), and stores it behind the row's slots for the next level and for k_pan_resolve.
//   k_pan_resolve   per pair (t, k): R, b_0, b_R, the chosen shift D and the threshold (24 w) >> 4, one packed word.
//   k_pan_near      k_borrow_near (borrow_kernels.hip): N, the seed bitmap dilated by 7.
//   k_pan_take      k_borrow_take with a shift per lender: one thread unpacks the frame's up to 2 B words into LDS; a lane with its N_t
//                   bit and C != 0 walks the lenders, q = p +- D: inside the rows held, C[q] == 0 or the N_s bit of q clear, and
//                   max_c |src_s[q] - fill_t[p]| under the threshold.  A pixel reads its own fill bytes and src only: in place.
//
// Tiles without an E sample leave at once.  The sums are integer: the order the workgroups arrive in does not matter.
//
// The workspace: the table [n][B][NC + 1][2] of 64-bit words, (S, cnt) per slot, NC = max((2 P + 1)^2, 10), the pair behind the slots
// holding the level's centre; then n * B words of k_pan_resolve; then the two bitmaps of borrow_kernels.hip.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "borrow_pan_kernels.h"
#include "key_kernels.h"
#include "plan_c.h"

namespace {

typedef unsigned long long u64;

constexpr int PN_REACH = 7;                                  // G + R - 1 of the key
constexpr int PN_RING = 16;                                  // E reaches this far from C (regrain_kernels.hip)
constexpr int PN_MAX_B = 8, PN_MAX_P = 8, PN_MAX_T = 128, PN_TH = 24, PN_FULL = 16;
constexpr u64 PN_GRAIN = 15447;                              // round(2^16 * sqrt(2) / 6), deflicker's
constexpr uint8_t BIT_E = 1, BIT_C = 4;                      // of vsr_regrain_sets' map
constexpr int PN_LATER = 10;                                 // the slots of a level k >= 2
constexpr int PN_MAX_GZ = 1024;

// k_pan_search1
constexpr int S1_THREADS = 320;                              // 289 candidates at P = 8
constexpr int S1_TW = 32, S1_TH = 16, S1_N = S1_TW * S1_TH;
constexpr int S1_HW = S1_TW + 2 * PN_MAX_P, S1_HH = S1_TH + 2 * PN_MAX_P;
constexpr int S1_MAX_PITCH = S1_HW + 31;
constexpr uint32_t S1_INVALID = 0xff000000u;
// k_pan_searchk, k_pan_resolve
constexpr int SK_THREADS = 256, SK_WAVES = SK_THREADS / 64, SK_TW = 32, SK_TH = 8;
// k_pan_near, k_pan_take
constexpr int BW_THREADS = 256, BW_WAVES = BW_THREADS / 64, BW_TILE = 32;
constexpr int BW_HROWS = BW_TILE + 2 * PN_REACH;

__host__ __device__ inline int pan_slots(int P) { return (2 * P + 1) * (2 * P + 1) > PN_LATER ? (2 * P + 1) * (2 * P + 1) : PN_LATER; }

__device__ __forceinline__ int pack_shift(int dy, int dx) { return (int)(((uint32_t)dy & 0xffffu) | ((uint32_t)dx << 16)); }
__device__ __forceinline__ int shift_y(int s) { return (int)(short)(s & 0xffff); }
__device__ __forceinline__ int shift_x(int s) { return s >> 16; }

// ascending (max(|dy|,|dx|), |dy|+|dx|, dy, dx)
__device__ __forceinline__ int order_key(int dy, int dx)
{
    const int ay = abs(dy), ax = abs(dx);
    return ((((ay > ax ? ay : ax) << 8 | (ay + ax)) << 8 | (dy + 128)) << 8) | (dx + 128);
}

struct Best {
    u64 S, cnt;                                              // cnt == 0: none
    int d;                                                   // packed shift
};

__device__ __forceinline__ bool beats(const Best& a, const Best& b)
{
    if (a.cnt == 0) return false;
    if (b.cnt == 0) return true;
    const u64 l = a.S * b.cnt, r = b.S * a.cnt;
    if (l != r) return l < r;
    return order_key(shift_y(a.d), shift_x(a.d)) < order_key(shift_y(b.d), shift_x(b.d));
}

// the shift of slot i of a level, false: the slot is empty
__device__ __forceinline__ bool slot_shift(int i, int level, int P, int centre, int* dy, int* dx)
{
    if (level == 1) {
        const int side = 2 * P + 1;
        *dy = i / side - P;
        *dx = i % side - P;
        return true;
    }
    if (i == PN_LATER - 1) {
        *dy = *dx = 0;
        return true;
    }
    *dy = shift_y(centre) + i / 3 - 1;
    *dx = shift_x(centre) + i % 3 - 1;
    const int ay = abs(*dy), ax = abs(*dx);
    return (ay > ax ? ay : ax) <= level * P && (*dy | *dx) != 0;
}

// R of one table row, by the whole workgroup (SK_THREADS threads, all of them call): the eligible slot that no other beats; cnt == 0 and
// d = 0 where none is eligible.  The result is the same in every thread.
__device__ Best pan_best(const u64* __restrict__ row, int level, int P, int nc, u64 n_e, Best* sh)
{
    const int tid = threadIdx.x;
    Best mine = {0, 0, 0};
    const int centre = level > 1 ? (int)row[2 * nc] : 0;
    for (int i = tid; i < (level == 1 ? (2 * P + 1) * (2 * P + 1) : PN_LATER); i += SK_THREADS) {
        int dy, dx;
        if (!slot_shift(i, level, P, centre, &dy, &dx)) continue;
        const Best c = {row[2 * i], row[2 * i + 1], pack_shift(dy, dx)};
        if (n_e == 0 || 2 * c.cnt < n_e) continue;
        if (beats(c, mine)) mine = c;
    }
    __syncthreads();                                         // (sh is read by the previous call)
    sh[tid] = mine;
    __syncthreads();
    for (int o = SK_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o && beats(sh[tid + o], sh[tid])) sh[tid] = sh[tid + o];
        __syncthreads();
    }
    Best out = sh[0];
    if (out.cnt == 0) out.d = 0;
    return out;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                                // lane 0 holds the sum
}

// b_d
__device__ __forceinline__ int pan_weight(u64 S, u64 cnt, u64 a_t, u64 a_u, u64 n_e)
{
    if (n_e == 0 || cnt == 0) return 0;
    const u64 m = 3 * cnt;
    const u64 floor = (((PN_GRAIN * (a_t + a_u)) >> 17) * cnt) / n_e;
    const u64 moved = S > floor ? S - floor : 0;
    if (moved >= 4 * m) return 0;
    const u64 q = (PN_FULL * (4 * m - moved)) / (3 * m);
    return q < (u64)PN_FULL ? (int)q : PN_FULL;
}

// grid.x: column tiles x row tiles over the local rows [la, lb) (the rows that can hold E); grid.y strides the frames t, t + 1 < n
__global__ __launch_bounds__(S1_THREADS) void k_pan_search1(const uint8_t* __restrict__ src, int64_t src_frame_stride,
                                                            const uint8_t* __restrict__ map, int n, int W, int y0, int rows, int la, int lb,
                                                            int col_tiles, int P, int pitch, int B, int ncw, u64* __restrict__ table)
{
    __shared__ uint16_t s_pos[S1_N];                         // the tile's E samples: ty * 32 + tx
    __shared__ uint2 s_smp[S1_N];                            // (the sample of src_t, its offset in s_tgt)
    __shared__ uint32_t s_tgt[S1_HH * S1_MAX_PITCH];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int x0 = (blockIdx.x % col_tiles) * S1_TW, ly0 = la + (blockIdx.x / col_tiles) * S1_TH;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i = tid; i < S1_N; i += S1_THREADS) {
        const int ly = ly0 + i / S1_TW, x = x0 + i % S1_TW;
        if (ly < lb && x < W && (map[(int64_t)(y0 + ly) * W + x] & BIT_E)) s_pos[atomicAdd(&s_n, 1)] = (uint16_t)i;
    }
    __syncthreads();
    const int cnt_e = s_n;
    if (cnt_e == 0) return;                                  // no sample in this tile
    const int side = 2 * P + 1, nc1 = side * side;
    const int base = (PN_MAX_P + tid / side - P) * pitch + PN_MAX_P + tid % side - P;      // of the lane's shift in s_tgt
    for (int f = blockIdx.y; f + 1 < n; f += gridDim.y) {
        const uint8_t* __restrict__ s = src + (int64_t)f * src_frame_stride;
        const uint8_t* __restrict__ u = s + src_frame_stride;
        for (int i = tid; i < cnt_e; i += S1_THREADS) {
            const int ty = s_pos[i] / S1_TW, tx = s_pos[i] % S1_TW;
            const uint8_t* p = s + ((int64_t)(ly0 + ty) * W + x0 + tx) * 3;
            s_smp[i] = make_uint2((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16), (uint32_t)(ty * pitch + tx));
        }
        for (int i = tid; i < S1_HH * S1_HW; i += S1_THREADS) {
            const int hy = i / S1_HW, hx = i % S1_HW;
            const int ly = ly0 - PN_MAX_P + hy, x = x0 - PN_MAX_P + hx;
            uint32_t v = S1_INVALID;
            if (ly >= 0 && ly < rows && x >= 0 && x < W && !(map[(int64_t)(y0 + ly) * W + x] & BIT_C)) {
                const uint8_t* p = u + ((int64_t)ly * W + x) * 3;
                v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
            }
            s_tgt[hy * pitch + hx] = v;
        }
        __syncthreads();
        if (tid < nc1) {
            uint32_t sum = 0, cnt = 0;
            for (int i = 0; i < cnt_e; ++i) {
                const uint2 a = s_smp[i];
                const uint32_t b = s_tgt[base + a.y];
                if (b < 0x01000000u) {
                    sum = __builtin_amdgcn_sad_u8(a.x, b, sum);
                    ++cnt;
                }
            }
            if (cnt) {
                u64* e = table + (((int64_t)f * B) * ncw + tid) * 2;
                if (sum) atomicAdd(e, (u64)sum);
                atomicAdd(e + 1, (u64)cnt);
            }
        }
        __syncthreads();                                     // (the tiles are written again for the next frame)
    }
}

// grid.x: column tiles x row tiles of 8 rows over [la, lb); grid.y strides the frames t, t + k < n.  k >= 2
__global__ __launch_bounds__(SK_THREADS) void k_pan_searchk(const uint8_t* __restrict__ src, int64_t src_frame_stride,
                                                            const uint8_t* __restrict__ map, const u64* __restrict__ counts, int n, int W, int y0,
                                                            int rows, int la, int lb, int col_tiles, int P, int B, int ncw, int k,
                                                            u64* __restrict__ table)
{
    __shared__ Best s_best[SK_THREADS];
    __shared__ uint32_t s_part[PN_LATER][SK_WAVES][2];
    const int tid = threadIdx.x;
    const int x = (blockIdx.x % col_tiles) * SK_TW + tid % SK_TW, ly = la + (blockIdx.x / col_tiles) * SK_TH + tid / SK_TW;
    const bool want = ly < lb && x < W && (map[(int64_t)(y0 + ly) * W + x] & BIT_E);
    if (!__syncthreads_or(want)) return;                     // no sample in this tile
    const u64 n_e = counts[0];
    const int nc = ncw - 1;
    for (int f = blockIdx.y; f + k < n; f += gridDim.y) {
        u64* row = table + ((int64_t)f * B + (k - 1)) * ncw * 2;
        const Best before = pan_best(table + ((int64_t)f * B + (k - 2)) * ncw * 2, k - 1, P, nc, n_e, s_best);
        const Best step = pan_best(table + ((int64_t)(f + k - 1) * B) * ncw * 2, 1, P, nc, n_e, s_best);
        const int centre = pack_shift(shift_y(before.d) + shift_y(step.d), shift_x(before.d) + shift_x(step.d));
        if (tid == 0) row[2 * nc] = (u64)(uint32_t)centre;   // (every workgroup writes the same word)
        const uint8_t* __restrict__ s = src + (int64_t)f * src_frame_stride;
        const uint8_t* __restrict__ u = s + (int64_t)k * src_frame_stride;
        int m0 = 0, m1 = 0, m2 = 0;
        if (want) {
            const uint8_t* p = s + ((int64_t)ly * W + x) * 3;
            m0 = p[0];
            m1 = p[1];
            m2 = p[2];
        }
#pragma unroll 1
        for (int j = 0; j < PN_LATER; ++j) {
            int dy, dx;
            uint32_t sum = 0, cnt = 0;
            if (slot_shift(j, k, P, centre, &dy, &dx) && want) {         // (the slot is the workgroup's, `want` the lane's)
                const int qy = ly + dy, qx = x + dx;
                if (qy >= 0 && qy < rows && qx >= 0 && qx < W && !(map[(int64_t)(y0 + qy) * W + qx] & BIT_C)) {
                    const uint8_t* p = u + ((int64_t)qy * W + qx) * 3;
                    sum = (uint32_t)(abs(m0 - (int)p[0]) + abs(m1 - (int)p[1]) + abs(m2 - (int)p[2]));
                    cnt = 1;
                }
            }
            sum = wave_sum(sum);
            cnt = wave_sum(cnt);
            if ((tid & 63) == 0) {
                s_part[j][tid >> 6][0] = sum;
                s_part[j][tid >> 6][1] = cnt;
            }
        }
        __syncthreads();
        if (tid < PN_LATER) {
            uint32_t sum = 0, cnt = 0;
            for (int w = 0; w < SK_WAVES; ++w) {
                sum += s_part[tid][w][0];
                cnt += s_part[tid][w][1];
            }
            if (cnt) {
                if (sum) atomicAdd(row + 2 * tid, (u64)sum);
                atomicAdd(row + 2 * tid + 1, (u64)cnt);
            }
        }
        __syncthreads();                                     // (s_part is written again for the next frame)
    }
}

// grid: (n, B).  resolved[t * B + k - 1] = dy (int8) | dx (int8) << 8 | threshold << 16 of the pair (t, t + k); 0 where t + k >= n
__global__ __launch_bounds__(SK_THREADS) void k_pan_resolve(const u64* __restrict__ table, const u64* __restrict__ counts,
                                                            const u64* __restrict__ stats, int n, int B, int P, int ncw,
                                                            u64* __restrict__ resolved)
{
    __shared__ Best s_best[SK_THREADS];
    const int t = blockIdx.x, k = blockIdx.y + 1;
    if (t + k >= n) {
        if (threadIdx.x == 0) resolved[(int64_t)t * B + k - 1] = 0;
        return;
    }
    const u64 n_e = counts[0];
    const u64* __restrict__ row = table + ((int64_t)t * B + (k - 1)) * ncw * 2;
    const Best r = pan_best(row, k, P, ncw - 1, n_e, s_best);
    if (threadIdx.x != 0) return;
    const int still = k == 1 ? P * (2 * P + 1) + P : PN_LATER - 1;
    const u64 a_t = stats[(int64_t)t * 4], a_u = stats[(int64_t)(t + k) * 4];
    const int b0 = pan_weight(row[2 * still], row[2 * still + 1], a_t, a_u, n_e);
    int d = 0, w = b0;
    if (b0 != PN_FULL && r.d != 0) {
        const int br = pan_weight(r.S, r.cnt, a_t, a_u, n_e);
        if (br > b0) {
            d = r.d;
            w = br;
        }
    }
    resolved[(int64_t)t * B + k - 1] = (u64)(uint32_t)((shift_y(d) & 0xff) | ((shift_x(d) & 0xff) << 8) | (((PN_TH * w) >> 4) << 16));
}

// k_borrow_near of borrow_kernels.hip.  grid.x: the words of a row, grid.y: tiles of 32 rows of the bitmap, grid.z strides the frames
__global__ __launch_bounds__(BW_THREADS) void k_pan_near(const u64* __restrict__ seeds, u64* __restrict__ near, int n, int srows, int nw)
{
    __shared__ u64 S[BW_HROWS * 3];                          // the seed words: left, own, right
    __shared__ u64 Hd[BW_HROWS];
    const int tid = threadIdx.x, w = blockIdx.x, r0 = blockIdx.y * BW_TILE;
    const int64_t per = (int64_t)srows * nw;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        if (tid < BW_HROWS * 3) {
            const int hr = tid / 3, side = tid - hr * 3;
            const int y = r0 - PN_REACH + hr, ww = w - 1 + side;
            S[tid] = (y >= 0 && y < srows && ww >= 0 && ww < nw) ? seeds[f * per + (int64_t)y * nw + ww] : 0ull;
        }
        __syncthreads();
        if (tid < BW_HROWS) {
            const u64 l = S[tid * 3], c = S[tid * 3 + 1], r = S[tid * 3 + 2];
            u64 h = c;
#pragma unroll
            for (int j = 1; j <= PN_REACH; ++j) h |= (c << j) | (l >> (64 - j)) | (c >> j) | (r << (64 - j));
            Hd[tid] = h;
        }
        __syncthreads();
        if (tid < BW_TILE && r0 + tid < srows) {
            u64 v = 0;
#pragma unroll
            for (int d = 0; d <= 2 * PN_REACH; ++d) v |= Hd[tid + d];
            near[f * per + (int64_t)(r0 + tid) * nw + w] = v;
        }
        __syncthreads();                                     // the next frame's words
    }
}

// grid.x: the words of a row, grid.y: tiles of 32 rows of [la, lb) (the rows of C's bounding rows that the frames hold), grid.z strides the
// frames.  resolved: k_pan_resolve's
__global__ __launch_bounds__(BW_THREADS) void k_pan_take(uint8_t* __restrict__ frames, int64_t frame_stride, const uint8_t* __restrict__ src,
                                                         int64_t src_stride, const uint8_t* __restrict__ cmask,
                                                         const u64* __restrict__ resolved, int n, int W, int y0, int rows, int la, int lb, int sa,
                                                         int srows, int nw, int B, const u64* __restrict__ near)
{
    __shared__ int s_thr[2 * PN_MAX_B];                      // the threshold of lender j; 0: lends nothing
    __shared__ int s_frame[2 * PN_MAX_B];                    // its frame
    __shared__ int s_dy[2 * PN_MAX_B], s_dx[2 * PN_MAX_B];   // where it is read: q = p + (dy, dx)
    __shared__ int s_any;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = blockIdx.x, r0 = la + blockIdx.y * BW_TILE;
    const int x = w * 64 + lane;
    const int64_t per = (int64_t)srows * nw;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        __syncthreads();                                     // (the previous frame's values are read by now)
        if (tid == 0) {
            int any = 0;
            for (int j = 0; j < 2 * B; ++j) {
                const int k = (j >> 1) + 1, s = (j & 1) ? f + k : f - k;
                int thr = 0, dy = 0, dx = 0;
                if (s >= 0 && s < n) {
                    const uint32_t v = (uint32_t)resolved[(int64_t)(s < f ? s : f) * B + (k - 1)];
                    const int sign = s < f ? -1 : 1;
                    dy = sign * (int)(int8_t)(v & 0xff);
                    dx = sign * (int)(int8_t)((v >> 8) & 0xff);
                    thr = (int)(v >> 16);
                }
                s_thr[j] = thr;
                s_frame[j] = s;
                s_dy[j] = dy;
                s_dx[j] = dx;
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
            const u64 own = near[f * per + (int64_t)(ly - sa) * nw + w];
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
                const int s = s_frame[j], qy = ly + s_dy[j], qx = x + s_dx[j];
                if (want && qy >= 0 && qy < rows && qx >= 0 && qx < W) {
                    bool lends = cmask[(int64_t)(y0 + qy) * W + qx] == 0;                  // real picture: no bitmap row is needed
                    if (!lends)                                                            // (a pixel of C lies in the bitmap's rows)
                        lends = !((near[s * per + (int64_t)(qy - sa) * nw + (qx >> 6)] >> (qx & 63)) & 1ull);
                    if (lends) {
                        const uint8_t* __restrict__ q = src + (int64_t)s * src_stride + ((int64_t)qy * W + qx) * 3;
                        const int v0 = q[0], v1 = q[1], v2 = q[2];
                        if (max(max(abs(v0 - b0), abs(v1 - b1)), abs(v2 - b2)) < thr) {
                            fp[at] = (uint8_t)v0;
                            fp[at + 1] = (uint8_t)v1;
                            fp[at + 2] = (uint8_t)v2;
                            want = false;
                        }
                    }
                }
                if (!__any(want)) break;
            }
        }
    }
}

static_assert(BW_HROWS * 3 <= BW_THREADS, "a thread per seed word of a tile");
static_assert((2 * PN_MAX_P + 1) * (2 * PN_MAX_P + 1) <= S1_THREADS, "a lane per candidate");
static_assert(S1_N <= 65536 && PN_MAX_B * PN_MAX_P <= 127, "the packed forms");

int gfail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

const char* bad_picture(int H, int W)
{
    if (H <= 0 || W <= 0) return "borrow-pan: H and W must be positive";
    if ((int64_t)H * W * 3 > 0x7fffffffll) return "borrow-pan: a frame of H * W * 3 >= 2^31 bytes is not supported";
    return nullptr;
}

std::string bad_options(int B, int P)
{
    if (B < 1 || B > PN_MAX_B) return "borrow-pan: B = " + std::to_string(B) + ", 1 <= B <= " + std::to_string(PN_MAX_B) + " are possible";
    if (P < 1 || P > PN_MAX_P) return "borrow-pan: P = " + std::to_string(P) + ", 1 <= P <= " + std::to_string(PN_MAX_P) + " are possible";
    return "";
}

const char* bad_rows(int H, int y0, int rows, int c0, int c1)
{
    if (y0 < 0 || rows <= 0 || y0 > H - rows) return "borrow-pan: the rows held must lie inside the frame";
    if (c0 < 0 || c1 < c0 || c1 > H) return "borrow-pan: the mask's rows must lie inside the frame";
    return nullptr;
}

inline int64_t table_words(int n, int B, int P) { return (int64_t)n * B * (pan_slots(P) + 1) * 2; }

}  // namespace

extern "C" int vsr_borrow_pan_launch_search(const uint8_t* src, int64_t src_frame_stride, const uint8_t* map, const uint64_t* counts, int n, int W,
                                            int y0, int rows, int c0, int c1, int B, int P, void* workspace, void* stream)
{
    u64* table = (u64*)workspace;
    if (hipMemsetAsync(table, 0, (size_t)table_words(n, B, P) * sizeof(u64), (hipStream_t)stream) != hipSuccess) return -1;
    // the local rows that can hold a sample: C's rows and the ring around them
    const int la = c0 - PN_RING - 1 - y0 > 0 ? c0 - PN_RING - 1 - y0 : 0;
    const int lb = c1 + PN_RING + 1 - y0 < rows ? c1 + PN_RING + 1 - y0 : rows;
    if (lb <= la || n < 2) return 0;
    const int ncw = pan_slots(P) + 1;
    const int pitch = S1_HW + (((2 * P + 1 - S1_HW) % 32) + 32) % 32;          // = 2 P + 1 mod 32
    const unsigned gy = (unsigned)(n - 1 < PN_MAX_GZ ? n - 1 : PN_MAX_GZ);
    {
        const int col_tiles = (W + S1_TW - 1) / S1_TW, row_tiles = (lb - la + S1_TH - 1) / S1_TH;
        hipLaunchKernelGGL(k_pan_search1, dim3((unsigned)(col_tiles * row_tiles), gy), dim3(S1_THREADS), 0, (hipStream_t)stream, src,
                           src_frame_stride, map, n, W, y0, rows, la, lb, col_tiles, P, pitch, B, ncw, table);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    const int col_tiles = (W + SK_TW - 1) / SK_TW, row_tiles = (lb - la + SK_TH - 1) / SK_TH;
    for (int k = 2; k <= B && k < n; ++k) {
        hipLaunchKernelGGL(k_pan_searchk, dim3((unsigned)(col_tiles * row_tiles), gy), dim3(SK_THREADS), 0, (hipStream_t)stream, src,
                           src_frame_stride, map, (const u64*)counts, n, W, y0, rows, la, lb, col_tiles, P, B, ncw, k, table);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

extern "C" int vsr_borrow_pan_launch_apply(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride,
                                           const uint8_t* cmask, const uint64_t* counts, const uint64_t* stats, int n, int H, int W, int y0,
                                           int rows, int c0, int c1, int T, int B, int P, void* workspace, void* stream)
{
    (void)H;
    const int la = c0 - y0 > 0 ? c0 - y0 : 0;
    const int lb = c1 - y0 < rows ? c1 - y0 : rows;
    if (lb <= la) return 0;                                  // the frames hold no pixel of the mask
    const int sa = la > 0 ? la - 1 : 0, sb = lb < rows ? lb + 1 : rows;
    const int nw = (W + 63) / 64, srows = sb - sa;
    const unsigned gz = (unsigned)(n < PN_MAX_GZ ? n : PN_MAX_GZ);
    const u64* table = (const u64*)workspace;
    u64* resolved = (u64*)workspace + table_words(n, B, P);
    u64* seeds = resolved + (int64_t)n * B;
    u64* near = seeds + (int64_t)n * srows * nw;
    if (vsr_key_seeds_launch(frames, frame_stride, src, src_frame_stride, cmask, n, W, y0, rows, sa, sb, T, seeds, stream) != 0) return -1;
    hipLaunchKernelGGL(k_pan_near, dim3((unsigned)nw, (unsigned)((srows + BW_TILE - 1) / BW_TILE), gz), dim3(BW_THREADS), 0,
                       (hipStream_t)stream, seeds, near, n, srows, nw);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_pan_resolve, dim3((unsigned)n, (unsigned)B), dim3(SK_THREADS), 0, (hipStream_t)stream, table, (const u64*)counts,
                       (const u64*)stats, n, B, P, pan_slots(P) + 1, resolved);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_pan_take, dim3((unsigned)nw, (unsigned)((lb - la + BW_TILE - 1) / BW_TILE), gz), dim3(BW_THREADS), 0,
                       (hipStream_t)stream, frames, frame_stride, src, src_frame_stride, cmask, resolved, n, W, y0, rows, la, lb, sa, srows, nw,
                       B, near);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

int64_t vsr_borrow_pan_workspace_bytes(int H, int W, int n, int B, int P)
{
    if (n < 0) return gfail(VSR_ERR_ARG, "borrow-pan: negative frame count");
    if (const char* why = bad_picture(H, W)) return gfail(VSR_ERR_ARG, why);
    const std::string why = bad_options(B, P);
    if (!why.empty()) return gfail(VSR_ERR_ARG, why);
    // the table and the chosen shifts, then two bitmaps of the key's
    const int64_t per = (int64_t)H * ((W + 63) / 64) * 16 + ((int64_t)B * (pan_slots(P) + 1) * 2 + B) * 8;
    if (n > 0 && per > INT64_MAX / n) return gfail(VSR_ERR_ARG, "borrow-pan: the workspace of so many frames has no size");
    return per * n;
}

int vsr_borrow_pan_search(const uint8_t* src_dev, int64_t src_frame_stride, const uint8_t* map_dev, const uint64_t* counts_dev, int n, int H,
                          int W, int y0, int rows, int c0, int c1, int B, int P, void* workspace_dev, void* stream)
{
    if (!src_dev || !map_dev || !counts_dev || !workspace_dev) return gfail(VSR_ERR_ARG, "borrow-pan: null pointer");
    if (n < 0) return gfail(VSR_ERR_ARG, "borrow-pan: negative frame count");
    if (const char* why = bad_picture(H, W)) return gfail(VSR_ERR_ARG, why);
    if (const char* why = bad_rows(H, y0, rows, c0, c1)) return gfail(VSR_ERR_ARG, why);
    const std::string why = bad_options(B, P);
    if (!why.empty()) return gfail(VSR_ERR_ARG, why);
    if (src_frame_stride < (int64_t)rows * W * 3) return gfail(VSR_ERR_ARG, "borrow-pan: frame stride smaller than a frame");
    if ((uintptr_t)workspace_dev % 8) return gfail(VSR_ERR_ARG, "borrow-pan: the workspace must be 8-byte aligned");
    if (n < 2 || c0 == c1) return 0;                         // one frame has no neighbour
    if (vsr_borrow_pan_workspace_bytes(H, W, n, B, P) < 0) return VSR_ERR_ARG;
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_borrow_pan_launch_search(src_dev, src_frame_stride, map_dev, counts_dev, n, W, y0, rows, c0, c1, B, P, workspace_dev, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("borrow-pan search launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

int vsr_borrow_pan_apply(uint8_t* frames_dev, int64_t frame_stride, const uint8_t* src_dev, int64_t src_frame_stride, const uint8_t* cmask_dev,
                         const uint64_t* counts_dev, const uint64_t* stats_dev, int n, int H, int W, int y0, int rows, int c0, int c1, int T,
                         int B, int P, void* workspace_dev, void* stream)
{
    if (!frames_dev || !src_dev || !cmask_dev || !counts_dev || !stats_dev || !workspace_dev)
        return gfail(VSR_ERR_ARG, "borrow-pan: null pointer");
    if (n < 0) return gfail(VSR_ERR_ARG, "borrow-pan: negative frame count");
    if (const char* why = bad_picture(H, W)) return gfail(VSR_ERR_ARG, why);
    if (const char* why = bad_rows(H, y0, rows, c0, c1)) return gfail(VSR_ERR_ARG, why);
    if (T < 1 || T > PN_MAX_T)
        return gfail(VSR_ERR_ARG, "borrow-pan: T = " + std::to_string(T) + ", 1 <= T <= " + std::to_string(PN_MAX_T) + " are possible");
    const std::string why = bad_options(B, P);
    if (!why.empty()) return gfail(VSR_ERR_ARG, why);
    const int64_t N = (int64_t)rows * W * 3;
    if (frame_stride < N || src_frame_stride < N) return gfail(VSR_ERR_ARG, "borrow-pan: frame stride smaller than a frame");
    if ((uintptr_t)workspace_dev % 8) return gfail(VSR_ERR_ARG, "borrow-pan: the workspace must be 8-byte aligned");
    if (n < 2 || c0 == c1) return 0;                         // one frame has no neighbour
    if (vsr_borrow_pan_workspace_bytes(H, W, n, B, P) < 0) return VSR_ERR_ARG;
    if (vsr_device_count() <= 0) return gfail(VSR_ERR_NOGPU, "no HIP device; there is no CPU fallback");
    if (vsr_borrow_pan_launch_apply(frames_dev, frame_stride, src_dev, src_frame_stride, cmask_dev, counts_dev, stats_dev, n, H, W, y0, rows,
                                    c0, c1, T, B, P, workspace_dev, stream) != 0)
        return gfail(VSR_ERR_HIP, std::string("borrow-pan launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // extern "C"
