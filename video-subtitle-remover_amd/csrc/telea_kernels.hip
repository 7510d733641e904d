// --inpaint-mode opencv on the GPU: the level replay of the Telea schedule (telea_plan.h) and the vsr_telea_* C-ABI.
//
// One workgroup owns one frame.  It walks the levels of the plan in order; the pixels of a level are independent, a lane is
// one (pixel, channel) and sums its taps in the serial statement's own k, l order in fp32.  Everything a level reads was
// written by the same workgroup in an earlier level, so a workgroup barrier (which drains this wave's stores first) is all the
// synchronisation there is: no agent-scope fence, no grid sync, no flag in memory.  Weights and "known at that step" bits
// come from the plan (they depend on the mask alone); a tap that does not count has weight 0 and x + 0 * y == x exactly, so
// no tap is skipped and every address is legal.
//
// The result is pinned bit for bit to a float32 numpy statement (tests/test_gpu_telea.py): contraction is off for this file,
// division and square root are the correctly rounded ones, and nothing here may be built with fast-math.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vsr_hip.h"
#include "plan_c.h"
#include "telea_kernels.h"
#include "telea_plan.h"

#pragma clang fp contract(off)

namespace {

constexpr int TELEA_THREADS = 512;

struct TeleaTaps {
    int8_t dk[vsr::TELEA_MAX_TAPS], dl[vsr::TELEA_MAX_TAPS];
};

// NT_CT > 0: compile-time tap count (28 for radius 3), fully unrolled; 0: runtime `nt`
template <int NT_CT>
__global__ __launch_bounds__(TELEA_THREADS) void telea_fill_kernel(uint8_t* __restrict__ frames, int64_t frame_stride, int H, int W, int L,
                                                                   int64_t P, int nt, const int32_t* __restrict__ level_off,
                                                                   const int32_t* __restrict__ yx, const float* __restrict__ wts,
                                                                   const uint8_t* __restrict__ flags, TeleaTaps taps)
{
    uint8_t* img = frames + (int64_t)blockIdx.x * frame_stride;
    const int64_t rowb = (int64_t)W * 3;
    int beg = level_off[0];
    for (int lev = 0; lev < L; ++lev) {
        const int end = level_off[lev + 1];
        for (int q = threadIdx.x; q < (end - beg) * 3; q += TELEA_THREADS) {
            const int64_t p = beg + q / 3;
            const int c = q % 3;
            const int i = yx[2 * p] + 1, j = yx[2 * p + 1] + 1;       // padded coordinates, as in the statement
            float Ia = 0.0f, Jx = 0.0f, Jy = 0.0f, s = 0.0f;
            auto tap = [&](int tp) {
                const float w = wts[(int64_t)tp * P + p];
                const int fl = flags[(int64_t)tp * P + p];
                const int dk = taps.dk[tp], dl = taps.dl[tp];
                // a tap outside the frame has w = 0; its addresses are clamped into the frame so that the loads stay legal
                const int k = min(max(i + dk, 1), H), l = min(max(j + dl, 1), W);
                const int km = k - 1 + (k == 1), kp = k - 1 - (k == H);
                const int lm = l - 1 + (l == 1), lp = l - 1 - (l == W);
                const uint8_t* row = img + (int64_t)km * rowb + c;
                const int vC = row[lm * 3], vL = row[(lm - 1) * 3], vR = row[(lp + 1) * 3];
                const int vU = row[lm * 3 - rowb], vD = img[(int64_t)(kp + 1) * rowb + lm * 3 + c];
                const int vXP = lp == lm ? vC : vL;                   // I[km][lp]: the centre, or at the first/last column the left one
                const int vYP = kp == km ? vC : vU;                   // I[kp][lm] likewise
                const bool a = fl & vsr::TELEA_RIGHT, b = fl & vsr::TELEA_LEFT, a2 = fl & vsr::TELEA_DOWN, b2 = fl & vsr::TELEA_UP;
                const float gix = a ? (b ? (float)(vR - vL) * 2.0f : (float)(vR - vC)) : (b ? (float)(vXP - vL) : 0.0f);
                const float giy = a2 ? (b2 ? (float)(vD - vU) * 2.0f : (float)(vD - vC)) : (b2 ? (float)(vYP - vU) : 0.0f);
                const float rx = (float)-dl, ry = (float)-dk;
                Ia = Ia + w * (float)vC;
                Jx = Jx - w * (gix * rx);
                Jy = Jy - w * (giy * ry);
                s = s + w;
            };
            if constexpr (NT_CT > 0) {
#pragma unroll
                for (int tp = 0; tp < NT_CT; ++tp) tap(tp);
            } else {
                for (int tp = 0; tp < nt; ++tp) tap(tp);
            }
            // plain `/` and sqrtf: hipcc's defaults are the correctly rounded expansions (the __f*_rn intrinsics map to the 1-ulp instructions)
            const float sat = Ia / s + (Jx + Jy) / (sqrtf(Jx * Jx + Jy * Jy) + 1.0e-20f) + 0.5f;
            // saturate_cast<uchar>(float): round to nearest even, then clamp
            img[(int64_t)(i - 1) * rowb + (j - 1) * 3 + c] = (uint8_t)min(max(__float2int_rn(sat), 0), 255);
        }
        beg = end;
        // this level's stores must have left the wave before anyone in the workgroup reads them
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

}  // namespace

extern "C" int vsr_telea_launch_fill(uint8_t* frames, int64_t frame_stride, int n, int H, int W, int L, int64_t P, int NT,
                                     const int8_t* tap_dk, const int8_t* tap_dl, const int32_t* level_off, const int32_t* yx,
                                     const float* w, const uint8_t* flags, void* stream)
{
    if (n <= 0 || L <= 0 || P <= 0) return 0;
    TeleaTaps taps;
    for (int t = 0; t < vsr::TELEA_MAX_TAPS; ++t) { taps.dk[t] = t < NT ? tap_dk[t] : 0; taps.dl[t] = t < NT ? tap_dl[t] : 0; }
    hipStream_t st = (hipStream_t)stream;
    if (NT == 28)
        hipLaunchKernelGGL(telea_fill_kernel<28>, dim3(n), dim3(TELEA_THREADS), 0, st, frames, frame_stride, H, W, L, P, NT, level_off, yx, w, flags, taps);
    else
        hipLaunchKernelGGL(telea_fill_kernel<0>, dim3(n), dim3(TELEA_THREADS), 0, st, frames, frame_stride, H, W, L, P, NT, level_off, yx, w, flags, taps);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI (include/vsr_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------
struct vsr_telea {
    int device = -1, radius = 3;
    bool has_plan = false;
    vsr::TeleaPlan plan;
    int32_t* d_level_off = nullptr;
    int32_t* d_yx = nullptr;
    float* d_w = nullptr;
    uint8_t* d_flags = nullptr;
};

namespace {

int tfail(int code, const std::string& msg) { return vsr_internal_fail(code, msg.c_str()); }

#define TCHK(expr)                                                                                     \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return tfail(VSR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

void release_device(vsr_telea* h)
{
    if (h->device < 0) return;
    (void)hipSetDevice(h->device);
    if (h->d_level_off || h->d_yx || h->d_w || h->d_flags) (void)hipDeviceSynchronize();
    if (h->d_level_off) (void)hipFree(h->d_level_off);
    if (h->d_yx) (void)hipFree(h->d_yx);
    if (h->d_w) (void)hipFree(h->d_w);
    if (h->d_flags) (void)hipFree(h->d_flags);
    h->d_level_off = nullptr; h->d_yx = nullptr; h->d_w = nullptr; h->d_flags = nullptr;
}

template <typename T>
int upload(T** dst, const std::vector<T>& src)
{
    TCHK(hipMalloc((void**)dst, std::max<size_t>(src.size(), 1) * sizeof(T)));
    if (!src.empty()) TCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

extern "C" {

int vsr_telea_create(vsr_telea_t** out, int device, int radius)
{
    if (!out) return tfail(VSR_ERR_ARG, "null out pointer");
    if (radius < 1 || radius > vsr::TELEA_MAX_RADIUS) return tfail(VSR_ERR_ARG, "telea: radius must be 1.." + std::to_string(vsr::TELEA_MAX_RADIUS));
    if (device >= 0 && device >= vsr_device_count()) return tfail(VSR_ERR_NOGPU, "no such HIP device; there is no CPU fallback");
    vsr_telea* h = new vsr_telea;
    h->device = device < 0 ? -1 : device;
    h->radius = radius;
    *out = h;
    return 0;
}

void vsr_telea_destroy(vsr_telea_t* h)
{
    if (!h) return;
    release_device(h);
    delete h;
}

int vsr_telea_set_mask(vsr_telea_t* h, const uint8_t* mask_host, int H, int W)
{
    if (!h || !mask_host) return tfail(VSR_ERR_ARG, "bad argument");
    std::string err;
    vsr::TeleaPlan plan;
    if (!vsr::telea_build_plan(mask_host, H, W, h->radius, plan, err)) return tfail(VSR_ERR_ARG, err);
    release_device(h);
    h->plan = std::move(plan);
    h->has_plan = true;
    if (h->device >= 0 && h->plan.P > 0) {
        TCHK(hipSetDevice(h->device));
        if (int rc = upload(&h->d_level_off, h->plan.level_off)) return rc;
        if (int rc = upload(&h->d_yx, h->plan.yx)) return rc;
        if (int rc = upload(&h->d_w, h->plan.w)) return rc;
        if (int rc = upload(&h->d_flags, h->plan.flags)) return rc;
    }
    return 0;
}

int64_t vsr_telea_plan_pixels(const vsr_telea_t* h) { return (h && h->has_plan) ? h->plan.P : -1; }
int vsr_telea_plan_levels(const vsr_telea_t* h) { return (h && h->has_plan) ? h->plan.L : -1; }
int vsr_telea_plan_taps(const vsr_telea_t* h) { return (h && h->has_plan) ? h->plan.NT : -1; }

int vsr_telea_plan_read(const vsr_telea_t* h, int32_t* yx, int32_t* step, float* T, int32_t* level)
{
    if (!h || !h->has_plan) return tfail(VSR_ERR_STATE, "telea: no mask set");
    const vsr::TeleaPlan& p = h->plan;
    if (yx) std::copy(p.yx.begin(), p.yx.end(), yx);
    if (step) std::copy(p.step.begin(), p.step.end(), step);
    if (T) std::copy(p.T.begin(), p.T.end(), T);
    if (level) std::copy(p.level.begin(), p.level.end(), level);
    return 0;
}

int vsr_telea_plan_tmap(const vsr_telea_t* h, float* out)
{
    if (!h || !h->has_plan || !out) return tfail(VSR_ERR_STATE, "telea: no mask set");
    std::copy(h->plan.tmap.begin(), h->plan.tmap.end(), out);
    return 0;
}

int vsr_telea_plan_weights(const vsr_telea_t* h, float* w, uint8_t* flags)
{
    if (!h || !h->has_plan) return tfail(VSR_ERR_STATE, "telea: no mask set");
    if (w) std::copy(h->plan.w.begin(), h->plan.w.end(), w);
    if (flags) std::copy(h->plan.flags.begin(), h->plan.flags.end(), flags);
    return 0;
}

int vsr_telea_inpaint(vsr_telea_t* h, uint8_t* frames_dev, int64_t frame_stride, int n, void* stream)
{
    if (!h || !frames_dev || n < 0) return tfail(VSR_ERR_ARG, "bad argument");
    if (h->device < 0) return tfail(VSR_ERR_NOGPU, "handle was created without a HIP device; there is no CPU fallback");
    if (!h->has_plan) return tfail(VSR_ERR_STATE, "telea: no mask set");
    const vsr::TeleaPlan& p = h->plan;
    if (frame_stride < (int64_t)p.H * p.W * 3) return tfail(VSR_ERR_ARG, "telea: frame stride smaller than a frame");
    if (n == 0 || p.P == 0) return 0;                      // empty mask, or a mask with no band: nothing is filled
    TCHK(hipSetDevice(h->device));
    if (vsr_telea_launch_fill(frames_dev, frame_stride, n, p.H, p.W, p.L, p.P, p.NT, p.tap_dk, p.tap_dl, h->d_level_off, h->d_yx, h->d_w,
                              h->d_flags, stream) != 0)
        return tfail(VSR_ERR_HIP, std::string("telea fill launch failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // extern "C"
