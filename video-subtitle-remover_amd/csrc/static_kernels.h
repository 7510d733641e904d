// Launchers of the static-overlay kernels (static_kernels.hip): the per-pixel state of --logo-scan over the sampled frames of a clip, and
// the seed / moving maps made from it.  All pointers are device pointers; both return 0 or -1 (launch error).  The arguments are
// checked by the C-ABI entry points (vsr_static_accum, vsr_static_classify), not here.
#pragma once
#include <stdint.h>

extern "C" {
// one launch over the n frames frames + idx[k] * frame_stride: lo / hi / edges [H][W] overwritten (first != 0) or continued
int vsr_static_accum_launch(const uint8_t* frames, int64_t frame_stride, const int32_t* idx, int n, int H, int W, int ge, int first, uint8_t* lo,
                            uint8_t* hi, uint16_t* edges, void* stream);
// one launch: grown float [H][W] (1.0 within `grow` pixels of a pixel with edges >= need, else 0.0), moving uint8 [H][W] (hi - lo >= mv)
int vsr_static_classify_launch(const uint8_t* lo, const uint8_t* hi, const uint16_t* edges, int H, int W, int need, int mv, int grow, float* grown,
                               uint8_t* moving, void* stream);
}
