// Launchers of the un-mixing kernels (unmix_kernels.hip): the moments of --logo-unblend over the sampled frames of a clip inside an area
// grown by its ring, and the un-mixed source written into the pixels of the area.  All pointers are device pointers; both return 0 or -1
// (launch error).  The arguments are checked by the C-ABI entry points (vsr_unmix_accum, vsr_unmix_apply), not here.
#pragma once
#include <stdint.h>

extern "C" {
// one launch over the n frames frames + idx[k] * frame_stride: S1 / S2 uint32 [gy1 - gy0][gx1 - gx0][3] overwritten (first != 0) or continued
int vsr_unmix_accum_launch(const uint8_t* frames, int64_t frame_stride, const int32_t* idx, int n, int H, int W, int gy0, int gy1, int gx0, int gx1,
                           int first, uint32_t* S1, uint32_t* S2, void* stream);
// one launch over the picture rows [lo, hi) of a box that starts at (by0, bx0) and is bw wide, in n frames that hold the rows from y0 on
int vsr_unmix_apply_launch(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_stride, const uint16_t* g16, const int16_t* o16,
                           int n, int W, int y0, int lo, int hi, int by0, int bx0, int bw, void* stream);
}
