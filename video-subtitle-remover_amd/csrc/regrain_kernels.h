// Launchers of the regrain kernels (regrain_kernels.hip): the sample sets of a composite mask, the per-frame noise sums and the in-place
// grain.  All pointers are device pointers; all return 0 or -1 (launch error).  The arguments are checked by the C-ABI entry points
// (vsr_regrain_sets / vsr_regrain_measure / vsr_regrain_apply), not here.  The frames hold `rows` rows of the picture from its row y0;
// [c0, c1) are the rows of the picture that hold a non-zero of the mask.
#pragma once
#include <stdint.h>

extern "C" {
// cmask uint8 [H][W] -> map uint8 [H][W] (bit 0 = E, bit 1 = I, bit 2 = cmask != 0), counts[2] = |E|, |I| (zeroed here, on the stream)
int vsr_regrain_launch_sets(const uint8_t* cmask, int H, int W, int r0, int r1, uint8_t* map, uint64_t* counts, void* stream);
// stats [n][4] = A_src, A_fill, pixels of the mask where frames != src, unused (zeroed here, on the stream)
int vsr_regrain_launch_measure(const uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride,
                               const uint8_t* map, int n, int W, int y0, int rows, int c0, int c1, uint64_t* stats, void* stream);
// in place on the frames, from counts and stats as the two launches above left them on the same stream
int vsr_regrain_launch_apply(uint8_t* frames, int64_t frame_stride, const uint8_t* map, const uint64_t* counts, const uint64_t* stats,
                             int n, int W, int y0, int rows, int c0, int c1, int percent, void* stream);
}
