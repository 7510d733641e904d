// Launchers of the seam-feather kernels (feather_kernels.hip): the clipped Chebyshev distance d of a composite mask and the in-place
// composite out = (d * fill + (F - d) * src + F / 2) / F.  All pointers are device pointers; both return 0 or -1 (launch error).
// The arguments are checked by the C-ABI entry points (vsr_feather_alpha / vsr_feather_composite), not here.
#pragma once
#include <stdint.h>

extern "C" {
// cmask uint8 [H][W] (non-zero = inside) -> alpha uint8 [H][W]: d = min(F, Chebyshev distance to the nearest zero inside the frame)
int vsr_feather_launch_alpha(const uint8_t* cmask, int H, int W, int feather, uint8_t* alpha, void* stream);
// frames uint8 [n][H][W][3] hold the fill and are composited in place; frame f at frames + f * frame_stride, its source at
// src + f * src_frame_stride (bytes; any alignment)
int vsr_feather_launch_composite(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride,
                                 const uint8_t* alpha, int n, int H, int W, int feather, void* stream);
}
