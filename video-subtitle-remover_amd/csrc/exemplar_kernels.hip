// --opencv-fill exemplar on the GPU: the PatchMatch exemplar fill of tests/_exemplar_statement.py and the
// vsr_exemplar_* C-ABI.
//
// Everything that depends on the mask alone comes from the plan (exemplar_plan.h).  The frames of a call go through every launch
// together (grid.y is the frame), on the caller's stream, and the launches of a call are ordered by that stream alone: no atomics, no
// flags, no grid sync.  The arithmetic is integer from end to end, so the bytes are the statement's.
//   k_ex_down    one pyramid level: 2 x 2 means
//   k_ex_init    the coarsest level's hole content, interpolated along the row and the column from the plan's offsets
//   k_ex_up      a level's initial match field, from the coarser level's or from the hash
//   k_ex_search  one synchronous pass: a workgroup is a 16 x 16 tile of targets, its 22 x 22 x 3 target bytes are staged in LDS once, a
//                lane owns a target and walks its candidates; a candidate's seven 21-byte rows are read as six aligned dwords each and
//                shifted into place, and summed against the lane's own patch (held in registers) with v_sad_u8
//   k_ex_vote    per hole pixel a gather over the at most 49 targets around it; it reads known pixels only and writes hole pixels only
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/vsr_hip.h"
#include "exemplar_kernels.h"
#include "exemplar_plan.h"
#include "plan_c.h"

namespace {

using namespace vsr;

constexpr int EX_THREADS = 256;
constexpr uint32_t EX_NONE = 0xFFFFFFFFu;
constexpr int EX_STAGE = EX_TILE + 2 * EX_R;          // 22
constexpr int EX_STAGE_WORDS = 17;                    // 22 pixels = 66 bytes, padded to 68

__device__ __forceinline__ uint32_t ex_mix(uint32_t h, uint32_t a)
{
    h ^= a;
    h *= 0x9E3779B1u;
    return h ^ (h >> 15);
}

__device__ __forceinline__ uint32_t ex_hash(uint32_t level, uint32_t it, uint32_t ps, uint32_t slot, uint32_t y, uint32_t x)
{
    uint32_t h = 0x811C9DC5u;
    h = ex_mix(h, level); h = ex_mix(h, it); h = ex_mix(h, ps); h = ex_mix(h, slot); h = ex_mix(h, y); h = ex_mix(h, x);
    h *= 0x85EBCA6Bu; h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

__device__ __forceinline__ uint32_t ex_pack(int y, int x) { return ((uint32_t)y & 0xFFFFu) | ((uint32_t)x << 16); }
__device__ __forceinline__ int ex_y(uint32_t v) { return (int)(int16_t)(v & 0xFFFFu); }
__device__ __forceinline__ int ex_x(uint32_t v) { return (int)(int16_t)(v >> 16); }

__device__ __forceinline__ uint32_t ex_any_source(const vsr_ex_level& lv, uint32_t it, uint32_t ps, uint32_t slot, int y, int x)
{
    const uint32_t i = ex_hash(lv.level, it, ps, slot, y, x) % lv.ns;
    return ex_pack(lv.src[2 * i], lv.src[2 * i + 1]);
}

// the field entry of (y, x): EX_NONE outside the box
__device__ __forceinline__ uint32_t ex_field(const uint32_t* f, const vsr_ex_level& lv, int y, int x)
{
    const int r = y - lv.by0, c = x - lv.bx0;
    if ((unsigned)r >= (unsigned)lv.bh || (unsigned)c >= (unsigned)lv.bw) return EX_NONE;
    return f[(int64_t)r * lv.bw + c];
}

__global__ __launch_bounds__(EX_THREADS) void k_ex_down(const uint8_t* __restrict__ src, int64_t src_stride, int Hs, int Ws,
                                                        uint8_t* __restrict__ dst, int64_t dst_stride)
{
    const int Hd = (Hs + 1) / 2, Wd = (Ws + 1) / 2;
    const int64_t i = (int64_t)blockIdx.x * EX_THREADS + threadIdx.x;
    if (i >= (int64_t)Hd * Wd) return;
    const int y = (int)(i / Wd), x = (int)(i % Wd);
    const int y1 = min(2 * y + 1, Hs - 1), x1 = min(2 * x + 1, Ws - 1);            // an odd size repeats its last row / column
    const uint8_t* s = src + (int64_t)blockIdx.y * src_stride;
    const uint8_t* r0 = s + (int64_t)(2 * y) * Ws * 3;
    const uint8_t* r1 = s + (int64_t)y1 * Ws * 3;
    uint8_t* d = dst + (int64_t)blockIdx.y * dst_stride + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        d[c] = (uint8_t)(((int)r0[2 * x * 3 + c] + r0[x1 * 3 + c] + r1[2 * x * 3 + c] + r1[x1 * 3 + c] + 2) >> 2);
}

__global__ __launch_bounds__(EX_THREADS) void k_ex_init(vsr_ex_level lv, const int32_t* __restrict__ table, int64_t nh)
{
    const int64_t i = (int64_t)blockIdx.x * EX_THREADS + threadIdx.x;
    if (i >= nh) return;
    const int32_t* t = table + i * 6;
    const int y = t[0], x = t[1], dl = t[2], dr = t[3], du = t[4], dd = t[5];
    uint8_t* img = lv.img + (int64_t)blockIdx.y * lv.img_stride;
    const int64_t rowb = (int64_t)lv.W * 3;
    uint8_t* p = img + y * rowb + x * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int h = -1, v = -1;
        if (dl && dr) h = (dr * (int)p[c - dl * 3] + dl * (int)p[c + dr * 3] + (dl + dr) / 2) / (dl + dr);
        else if (dl) h = p[c - dl * 3];
        else if (dr) h = p[c + dr * 3];
        if (du && dd) v = (dd * (int)p[c - du * rowb] + du * (int)p[c + dd * rowb] + (du + dd) / 2) / (du + dd);
        else if (du) v = p[c - du * rowb];
        else if (dd) v = p[c + dd * rowb];
        p[c] = (uint8_t)(h >= 0 && v >= 0 ? (h + v + 1) >> 1 : h >= 0 ? h : v >= 0 ? v : 128);
    }
}

__global__ __launch_bounds__(EX_THREADS) void k_ex_up(vsr_ex_level lv, vsr_ex_level co, int has_coarse)
{
    const int64_t i = (int64_t)blockIdx.x * EX_THREADS + threadIdx.x;
    if (i >= (int64_t)lv.bh * lv.bw) return;
    const int y = lv.by0 + (int)(i / lv.bw), x = lv.bx0 + (int)(i % lv.bw);
    uint32_t out = EX_NONE;
    if (lv.cls[(int64_t)y * lv.W + x] & EX_TARGET) {
        bool ok = false;
        if (has_coarse) {
            const int cy = min(max(y >> 1, EX_R), co.H - EX_R - 1), cx = min(max(x >> 1, EX_R), co.W - EX_R - 1);
            const uint32_t c = ex_field(co.fa + (int64_t)blockIdx.y * co.bh * co.bw, co, cy, cx);
            if (c != EX_NONE) {
                const int uy = min(max(2 * ex_y(c) + (y & 1), EX_R), lv.H - EX_R - 1);
                const int ux = min(max(2 * ex_x(c) + (x & 1), EX_R), lv.W - EX_R - 1);
                if (lv.cls[(int64_t)uy * lv.W + ux] & EX_VALID) { ok = true; out = ex_pack(uy, ux); }
            }
        }
        if (!ok) out = ex_any_source(lv, EX_INIT_ITER, 0, 0, y, x);
    }
    const int64_t o = (int64_t)blockIdx.y * lv.bh * lv.bw + i;
    lv.fa[o] = out;
    lv.fb[o] = out;
}

// 21 bytes at p as five dwords and one byte: six aligned dwords, shifted into place.  The last aligned dword read is the one that
// holds byte 20, so nothing is read beyond a dword that holds a byte of the row.
__device__ __forceinline__ void ex_row_global(const uint8_t* p, uint32_t w[6])
{
    const uint32_t k = (uint32_t)((uintptr_t)p & 3);
    const uint32_t* q = (const uint32_t*)(p - k);
    uint32_t d[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) d[j] = q[j];
    const uint32_t sh = 8 * k;
#pragma unroll
    for (int j = 0; j < 5; ++j) w[j] = (uint32_t)((((uint64_t)d[j + 1] << 32) | d[j]) >> sh);
    w[5] = (d[5] >> sh) & 0xFFu;
}

__global__ __launch_bounds__(EX_THREADS) void k_ex_search(vsr_ex_level lv, const int32_t* __restrict__ tiles, int it, int ps, int from_b)
{
    __shared__ uint32_t stage[EX_STAGE][EX_STAGE_WORDS];
    const int ty = tiles[2 * blockIdx.x], tx = tiles[2 * blockIdx.x + 1];
    const uint8_t* img = lv.img + (int64_t)blockIdx.y * lv.img_stride;
    const int64_t rowb = (int64_t)lv.W * 3;
    const int H = lv.H, W = lv.W;
    // the tile's pixels and a margin of R around them; coordinates outside the frame are clamped (no target reads those)
    uint8_t* sb = (uint8_t*)&stage[0][0];
    for (int i = threadIdx.x; i < EX_STAGE * EX_STAGE * 3; i += EX_THREADS) {
        const int r = i / (EX_STAGE * 3), b = i % (EX_STAGE * 3);
        const int gy = min(max(ty * EX_TILE - EX_R + r, 0), H - 1), gx = min(max(tx * EX_TILE - EX_R + b / 3, 0), W - 1);
        sb[r * (EX_STAGE_WORDS * 4) + b] = img[gy * rowb + gx * 3 + b % 3];
    }
    __syncthreads();
    const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
    const int y = ty * EX_TILE + ly, x = tx * EX_TILE + lx;
    if (y >= H || x >= W || !(lv.cls[(int64_t)y * W + x] & EX_TARGET)) return;

    uint32_t T[EX_P][6];                                                      // the lane's own patch, rows packed as ex_row_global packs them
    {
        const uint32_t o = lx * 3, wd = o >> 2, sh = 8 * (o & 3);
#pragma unroll
        for (int r = 0; r < EX_P; ++r) {
            uint32_t d[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) d[j] = stage[ly + r][wd + j];
#pragma unroll
            for (int j = 0; j < 5; ++j) T[r][j] = (uint32_t)((((uint64_t)d[j + 1] << 32) | d[j]) >> sh);
            T[r][5] = (d[5] >> sh) & 0xFFu;
        }
    }

    const int64_t fo = (int64_t)blockIdx.y * lv.bh * lv.bw;
    const uint32_t* fin = (from_b ? lv.fb : lv.fa) + fo;
    uint32_t* fout = (from_b ? lv.fa : lv.fb) + fo;
    const uint32_t cur = ex_field(fin, lv, y, x);
    uint32_t best = cur, best_d = 0xFFFFFFFFu;

    auto consider = [&](int cy, int cx) {
        if ((unsigned)cy >= (unsigned)H || (unsigned)cx >= (unsigned)W) return;
        if (!(lv.cls[(int64_t)cy * W + cx] & EX_VALID)) return;                // valid: the whole patch lies inside the frame
        const uint8_t* p = img + (int64_t)(cy - EX_R) * rowb + (cx - EX_R) * 3;
        uint32_t s = 0;
#pragma unroll
        for (int r = 0; r < EX_P; ++r) {
            uint32_t w[6];
            ex_row_global(p + r * rowb, w);
#pragma unroll
            for (int j = 0; j < 6; ++j) s = __builtin_amdgcn_sad_u8(T[r][j], w[j], s);
            if (s >= best_d) return;                                          // only a strictly smaller sum wins: it cannot any more
        }
        best_d = s;
        best = ex_pack(cy, cx);
    };

    consider(ex_y(cur), ex_x(cur));
    const int EY[4] = {0, 1, 0, -1}, EX[4] = {1, 0, -1, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t nb = ex_field(fin, lv, y - EY[e], x - EX[e]);
        if (nb != EX_NONE) consider(ex_y(nb) + EY[e], ex_x(nb) + EX[e]);
    }
    int k = 0;
    for (int rho = max(H, W) >> 1; rho >= 1; rho >>= 1, ++k) {
        const uint32_t span = 2 * rho + 1;
        const int oy = (int)(ex_hash(lv.level, it, ps, 2 * k, y, x) % span) - rho;
        const int ox = (int)(ex_hash(lv.level, it, ps, 2 * k + 1, y, x) % span) - rho;
        consider(ex_y(cur) + oy, ex_x(cur) + ox);
    }
    const uint32_t any = ex_any_source(lv, it, ps, EX_ANY_SLOT, y, x);
    consider(ex_y(any), ex_x(any));
    fout[(int64_t)(y - lv.by0) * lv.bw + (x - lv.bx0)] = best;
}

__global__ __launch_bounds__(EX_THREADS) void k_ex_vote(vsr_ex_level lv, int from_b, int vy0, int vx0, int vh, int vw)
{
    const int64_t i = (int64_t)blockIdx.x * EX_THREADS + threadIdx.x;
    if (i >= (int64_t)vh * vw) return;
    const int y = vy0 + (int)(i / vw), x = vx0 + (int)(i % vw);
    const int H = lv.H, W = lv.W;
    if (!(lv.cls[(int64_t)y * W + x] & EX_HOLE)) return;
    uint8_t* img = lv.img + (int64_t)blockIdx.y * lv.img_stride;
    const int64_t rowb = (int64_t)W * 3;
    const uint32_t* f = (from_b ? lv.fb : lv.fa) + (int64_t)blockIdx.y * lv.bh * lv.bw;
    uint32_t s0 = 0, s1 = 0, s2 = 0, n = 0;
    for (int dy = -EX_R; dy <= EX_R; ++dy) {
        const int qy = y + dy;
        if (qy < EX_R || qy >= H - EX_R) continue;
        for (int dx = -EX_R; dx <= EX_R; ++dx) {
            const int qx = x + dx;
            if (qx < EX_R || qx >= W - EX_R) continue;                        // an in-frame centre this close to a hole pixel is a target
            const uint32_t m = f[(int64_t)(qy - lv.by0) * lv.bw + (qx - lv.bx0)];
            const int my = ex_y(m), mx = ex_x(m);
            // a field the searches wrote holds valid sources only; one that a caller of the stage runner left unset is not followed
            if ((unsigned)my >= (unsigned)H || (unsigned)mx >= (unsigned)W || !(lv.cls[(int64_t)my * W + mx] & EX_VALID)) continue;
            const uint8_t* p = img + (int64_t)(my - dy) * rowb + (mx - dx) * 3;               // inside the match's patch: a known pixel
            s0 += p[0]; s1 += p[1]; s2 += p[2];
            ++n;
        }
    }
    if (n == 0) return;
    uint8_t* o = img + y * rowb + x * 3;
    o[0] = (uint8_t)((s0 + n / 2) / n);
    o[1] = (uint8_t)((s1 + n / 2) / n);
    o[2] = (uint8_t)((s2 + n / 2) / n);
}

inline unsigned blocks_for(int64_t items) { return (unsigned)((items + EX_THREADS - 1) / EX_THREADS); }
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

}  // namespace

extern "C" {

int vsr_ex_launch_down(const uint8_t* src, int64_t src_stride, int Hs, int Ws, uint8_t* dst, int64_t dst_stride, int n, void* stream)
{
    const int64_t items = (int64_t)((Hs + 1) / 2) * ((Ws + 1) / 2);
    if (n <= 0 || items <= 0) return 0;
    hipLaunchKernelGGL(k_ex_down, dim3(blocks_for(items), n), dim3(EX_THREADS), 0, (hipStream_t)stream, src, src_stride, Hs, Ws, dst, dst_stride);
    return launched();
}

int vsr_ex_launch_init(const vsr_ex_level* lv, const int32_t* table, int64_t nh, int n, void* stream)
{
    if (n <= 0 || nh <= 0) return 0;
    hipLaunchKernelGGL(k_ex_init, dim3(blocks_for(nh), n), dim3(EX_THREADS), 0, (hipStream_t)stream, *lv, table, nh);
    return launched();
}

int vsr_ex_launch_up(const vsr_ex_level* lv, const vsr_ex_level* coarse, int n, void* stream)
{
    const int64_t items = (int64_t)lv->bh * lv->bw;
    if (n <= 0 || items <= 0) return 0;
    hipLaunchKernelGGL(k_ex_up, dim3(blocks_for(items), n), dim3(EX_THREADS), 0, (hipStream_t)stream, *lv, coarse ? *coarse : *lv, coarse ? 1 : 0);
    return launched();
}

int vsr_ex_launch_search(const vsr_ex_level* lv, const int32_t* tiles, int ntiles, int it, int ps, int from_b, int n, void* stream)
{
    if (n <= 0 || ntiles <= 0) return 0;
    hipLaunchKernelGGL(k_ex_search, dim3(ntiles, n), dim3(EX_THREADS), 0, (hipStream_t)stream, *lv, tiles, it, ps, from_b);
    return launched();
}

int vsr_ex_launch_vote(const vsr_ex_level* lv, int from_b, int n, void* stream)
{
    // the hole pixels lie within R of the targets' box
    const int y0 = std::max(lv->by0 - EX_R, 0), x0 = std::max(lv->bx0 - EX_R, 0);
    const int y1 = std::min(lv->by0 + lv->bh + EX_R, lv->H), x1 = std::min(lv->bx0 + lv->bw + EX_R, lv->W);
    const int64_t items = (int64_t)(y1 - y0) * (x1 - x0);
    if (n <= 0 || items <= 0 || lv->bh <= 0) return 0;
    hipLaunchKernelGGL(k_ex_vote, dim3(blocks_for(items), n), dim3(EX_THREADS), 0, (hipStream_t)stream, *lv, from_b, y0, x0, y1 - y0, x1 - x0);
    return launched();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
struct vsr_exemplar {
    int device = -1;
    bool has_plan = false;
    vsr::ExemplarPlan plan;
    std::vector<uint8_t*> d_cls;
    std::vector<int16_t*> d_src;
    std::vector<int32_t*> d_tiles;
    int32_t* d_init = nullptr;
};

namespace {

int efail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

#define ECHK(expr)                                                                                     \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return efail(VSR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

void release_device(vsr_exemplar* h)
{
    if (h->device < 0) return;
    (void)hipSetDevice(h->device);
    if (!h->d_cls.empty() || h->d_init) (void)hipDeviceSynchronize();
    for (auto p : h->d_cls) if (p) (void)hipFree(p);
    for (auto p : h->d_src) if (p) (void)hipFree(p);
    for (auto p : h->d_tiles) if (p) (void)hipFree(p);
    if (h->d_init) (void)hipFree(h->d_init);
    h->d_cls.clear(); h->d_src.clear(); h->d_tiles.clear();
    h->d_init = nullptr;
}

template <typename T>
int upload(T** dst, const std::vector<T>& src)
{
    ECHK(hipMalloc((void**)dst, std::max<size_t>(src.size(), 1) * sizeof(T)));
    if (!src.empty()) ECHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

constexpr int64_t EX_ALIGN = 256;
inline int64_t align_up(int64_t v) { return (v + EX_ALIGN - 1) / EX_ALIGN * EX_ALIGN; }

// the workspace of a call of n frames: per level >= 1 its images, per level its two match fields
struct Layout {
    int64_t img[EX_MAX_LEVELS], fa[EX_MAX_LEVELS], fb[EX_MAX_LEVELS], total;
};

Layout layout_of(const vsr::ExemplarPlan& p, int n)
{
    Layout L{};
    int64_t at = 0;
    for (size_t l = 0; l < p.levels.size(); ++l) {
        const vsr::ExemplarLevel& lv = p.levels[l];
        L.img[l] = -1;
        if (l > 0) { L.img[l] = at; at = align_up(at + (int64_t)n * lv.H * lv.W * 3); }
        const int64_t fbytes = (int64_t)n * lv.bh * lv.bw * 4;
        L.fa[l] = at; at = align_up(at + fbytes);
        L.fb[l] = at; at = align_up(at + fbytes);
    }
    L.total = at;
    return L;
}

vsr_ex_level level_args(const vsr_exemplar* h, const Layout& L, int l, uint8_t* frames, int64_t frame_stride, uint8_t* ws)
{
    const vsr::ExemplarLevel& lv = h->plan.levels[l];
    vsr_ex_level a{};
    a.img = l == 0 ? frames : ws + L.img[l];
    a.img_stride = l == 0 ? frame_stride : (int64_t)lv.H * lv.W * 3;
    a.H = lv.H; a.W = lv.W; a.level = l;
    a.cls = h->d_cls[l];
    a.src = h->d_src[l];
    a.ns = (uint32_t)(lv.src.size() / 2);
    a.fa = (uint32_t*)(ws + L.fa[l]);
    a.fb = (uint32_t*)(ws + L.fb[l]);
    a.by0 = lv.by0; a.bx0 = lv.bx0; a.bh = lv.bh; a.bw = lv.bw;
    return a;
}

int check_call(const vsr_exemplar* h, const uint8_t* frames, int64_t frame_stride, int n, const void* ws, int64_t ws_bytes)
{
    if (!h || !frames || n < 0) return efail(VSR_ERR_ARG, "bad argument");
    if (h->device < 0) return efail(VSR_ERR_NOGPU, "handle was created without a HIP device; there is no CPU fallback");
    if (!h->has_plan) return efail(VSR_ERR_STATE, "exemplar: no mask set");
    if (frame_stride < (int64_t)h->plan.H * h->plan.W * 3) return efail(VSR_ERR_ARG, "exemplar: frame stride smaller than a frame");
    if (n > 65535) return efail(VSR_ERR_ARG, "exemplar: at most 65535 frames a call");
    if (n > 0 && !h->plan.levels.empty()) {
        if (!ws || ((uintptr_t)ws & 3)) return efail(VSR_ERR_ARG, "exemplar: the workspace must be a 4-byte aligned device pointer");
        if (ws_bytes < layout_of(h->plan, n).total) return efail(VSR_ERR_ARG, "exemplar: workspace smaller than vsr_exemplar_workspace_bytes");
    }
    return 0;
}

int run_stage(const vsr_exemplar* h, const Layout& L, uint8_t* frames, int64_t stride, int n, uint8_t* ws, int stage, int l, int it, int ps,
              int from_b, void* stream)
{
    const int nl = (int)h->plan.levels.size();
    const vsr_ex_level a = level_args(h, L, l, frames, stride, ws);
    int rc = 0;
    switch (stage) {
    case VSR_EX_DOWN: {
        const vsr_ex_level s = level_args(h, L, l - 1, frames, stride, ws);
        rc = vsr_ex_launch_down(s.img, s.img_stride, s.H, s.W, a.img, a.img_stride, n, stream);
        break;
    }
    case VSR_EX_INIT:
        rc = vsr_ex_launch_init(&a, h->d_init, (int64_t)(h->plan.init.size() / 6), n, stream);
        break;
    case VSR_EX_UP:
        if (l == nl - 1) rc = vsr_ex_launch_up(&a, nullptr, n, stream);
        else {
            const vsr_ex_level c = level_args(h, L, l + 1, frames, stride, ws);
            rc = vsr_ex_launch_up(&a, &c, n, stream);
        }
        break;
    case VSR_EX_SEARCH:
        rc = vsr_ex_launch_search(&a, h->d_tiles[l], (int)(h->plan.levels[l].tiles.size() / 2), it, ps, from_b, n, stream);
        break;
    case VSR_EX_VOTE:
        rc = vsr_ex_launch_vote(&a, from_b, n, stream);
        break;
    }
    if (rc != 0) return efail(VSR_ERR_HIP, std::string("exemplar launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // namespace

extern "C" {

int vsr_exemplar_create(vsr_exemplar_t** out, int device)
{
    if (!out) return efail(VSR_ERR_ARG, "null out pointer");
    if (device >= 0 && device >= vsr_device_count()) return efail(VSR_ERR_NOGPU, "no such HIP device; there is no CPU fallback");
    vsr_exemplar* h = new vsr_exemplar;
    h->device = device < 0 ? -1 : device;
    *out = h;
    return 0;
}

void vsr_exemplar_destroy(vsr_exemplar_t* h)
{
    if (!h) return;
    release_device(h);
    delete h;
}

int vsr_exemplar_set_mask(vsr_exemplar_t* h, const uint8_t* mask_host, int H, int W)
{
    if (!h || !mask_host) return efail(VSR_ERR_ARG, "bad argument");
    std::string err;
    vsr::ExemplarPlan plan;
    if (!vsr::exemplar_build_plan(mask_host, H, W, plan, err)) return efail(VSR_ERR_ARG, err);
    release_device(h);
    h->plan = std::move(plan);
    h->has_plan = true;
    if (h->device >= 0 && !h->plan.levels.empty()) {
        ECHK(hipSetDevice(h->device));
        const size_t nl = h->plan.levels.size();
        h->d_cls.assign(nl, nullptr); h->d_src.assign(nl, nullptr); h->d_tiles.assign(nl, nullptr);
        for (size_t l = 0; l < nl; ++l) {
            if (int rc = upload(&h->d_cls[l], h->plan.levels[l].cls)) return rc;
            if (int rc = upload(&h->d_src[l], h->plan.levels[l].src)) return rc;
            if (int rc = upload(&h->d_tiles[l], h->plan.levels[l].tiles)) return rc;
        }
        if (int rc = upload(&h->d_init, h->plan.init)) return rc;
    }
    return 0;
}

int vsr_exemplar_plan_levels(const vsr_exemplar_t* h) { return (h && h->has_plan) ? (int)h->plan.levels.size() : -1; }

int vsr_exemplar_plan_level_info(const vsr_exemplar_t* h, int level, int64_t* out)
{
    if (!h || !h->has_plan || !out) return efail(VSR_ERR_STATE, "exemplar: no mask set");
    if (level < 0 || level >= (int)h->plan.levels.size()) return efail(VSR_ERR_ARG, "exemplar: no such level");
    const vsr::ExemplarLevel& lv = h->plan.levels[level];
    const int64_t v[VSR_EX_INFO_LEN] = {lv.H, lv.W, (int64_t)lv.src.size() / 2, (int64_t)lv.tgt.size() / 2, (int64_t)lv.tiles.size() / 2, lv.nhole,
                                        lv.by0, lv.bx0, lv.bh, lv.bw};
    std::copy(v, v + VSR_EX_INFO_LEN, out);
    return 0;
}

int vsr_exemplar_plan_read(const vsr_exemplar_t* h, int level, int16_t* src, int16_t* tgt, int32_t* tiles, uint8_t* cls)
{
    if (!h || !h->has_plan) return efail(VSR_ERR_STATE, "exemplar: no mask set");
    if (level < 0 || level >= (int)h->plan.levels.size()) return efail(VSR_ERR_ARG, "exemplar: no such level");
    const vsr::ExemplarLevel& lv = h->plan.levels[level];
    if (src) std::copy(lv.src.begin(), lv.src.end(), src);
    if (tgt) std::copy(lv.tgt.begin(), lv.tgt.end(), tgt);
    if (tiles) std::copy(lv.tiles.begin(), lv.tiles.end(), tiles);
    if (cls) std::copy(lv.cls.begin(), lv.cls.end(), cls);
    return 0;
}

int vsr_exemplar_plan_init(const vsr_exemplar_t* h, int32_t* table)
{
    if (!h || !h->has_plan || !table) return efail(VSR_ERR_STATE, "exemplar: no mask set");
    std::copy(h->plan.init.begin(), h->plan.init.end(), table);
    return 0;
}

int64_t vsr_exemplar_workspace_bytes(const vsr_exemplar_t* h, int n)
{
    if (!h || !h->has_plan || n < 0) return -1;
    return layout_of(h->plan, n).total;
}

int vsr_exemplar_layout(const vsr_exemplar_t* h, int n, int level, int64_t* out)
{
    if (!h || !h->has_plan || !out || n < 0) return efail(VSR_ERR_STATE, "exemplar: no mask set");
    if (level < 0 || level >= (int)h->plan.levels.size()) return efail(VSR_ERR_ARG, "exemplar: no such level");
    const Layout L = layout_of(h->plan, n);
    const vsr::ExemplarLevel& lv = h->plan.levels[level];
    out[0] = L.img[level];
    out[1] = (int64_t)lv.H * lv.W * 3;
    out[2] = L.fa[level];
    out[3] = L.fb[level];
    out[4] = (int64_t)lv.bh * lv.bw * 4;
    return 0;
}

int vsr_exemplar_run_stage(vsr_exemplar_t* h, uint8_t* frames_dev, int64_t frame_stride, int n, void* workspace, int64_t workspace_bytes, int stage,
                           int level, int iteration, int pass, int from_b, void* stream)
{
    if (int rc = check_call(h, frames_dev, frame_stride, n, workspace, workspace_bytes)) return rc;
    const int nl = (int)h->plan.levels.size();
    if (level < 0 || level >= nl) return efail(VSR_ERR_ARG, "exemplar: no such level");
    if (stage < VSR_EX_DOWN || stage > VSR_EX_VOTE) return efail(VSR_ERR_ARG, "exemplar: no such stage");
    if (stage == VSR_EX_DOWN && level == 0) return efail(VSR_ERR_ARG, "exemplar: level 0 is the frame, nothing is downsampled into it");
    if (stage == VSR_EX_INIT && level != nl - 1) return efail(VSR_ERR_ARG, "exemplar: only the coarsest level is interpolated");
    if (iteration < 0 || iteration > 255 || pass < 0 || pass > 255) return efail(VSR_ERR_ARG, "exemplar: iteration and pass must be 0..255");
    if (n == 0) return 0;
    ECHK(hipSetDevice(h->device));
    return run_stage(h, layout_of(h->plan, n), frames_dev, frame_stride, n, (uint8_t*)workspace, stage, level, iteration, pass, from_b != 0, stream);
}

int vsr_exemplar_inpaint(vsr_exemplar_t* h, uint8_t* frames_dev, int64_t frame_stride, int n, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (int rc = check_call(h, frames_dev, frame_stride, n, workspace, workspace_bytes)) return rc;
    const int nl = (int)h->plan.levels.size();
    if (n == 0 || nl == 0) return 0;                                           // an empty mask: nothing is filled
    ECHK(hipSetDevice(h->device));
    const Layout L = layout_of(h->plan, n);
    uint8_t* ws = (uint8_t*)workspace;
    auto run = [&](int stage, int l, int it, int ps, int from_b) { return run_stage(h, L, frames_dev, frame_stride, n, ws, stage, l, it, ps, from_b, stream); };
    for (int l = 1; l < nl; ++l)
        if (int rc = run(VSR_EX_DOWN, l, 0, 0, 0)) return rc;
    for (int l = nl - 1; l >= 0; --l) {
        if (l == nl - 1) {
            if (int rc = run(VSR_EX_INIT, l, 0, 0, 0)) return rc;
            if (int rc = run(VSR_EX_UP, l, 0, 0, 0)) return rc;
        } else {
            if (int rc = run(VSR_EX_UP, l, 0, 0, 0)) return rc;
            if (int rc = run(VSR_EX_VOTE, l, 0, 0, 0)) return rc;
        }
        for (int it = 0; it < vsr::EX_ITERS; ++it) {
            for (int ps = 0; ps < vsr::EX_PASSES; ++ps)
                if (int rc = run(VSR_EX_SEARCH, l, it, ps, ps & 1)) return rc;
            if (int rc = run(VSR_EX_VOTE, l, 0, 0, vsr::EX_PASSES & 1)) return rc;
        }
    }
    return 0;
}

}  // extern "C"
