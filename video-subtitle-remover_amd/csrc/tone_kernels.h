// Launchers of the tone-match kernels (tone_kernels.hip): the seam bands of a composite mask, and per call the level-3 sums, the pull and
// push through the cell pyramid and the in-place offset.  All pointers are device pointers; all return 0 or -1 (launch error).  The
// arguments are checked by the C-ABI entry points (vsr_tone_sets / vsr_tone_apply), not here.  The frames hold `rows` rows of the
// picture from its row y0; [c0, c1) are the rows of the picture that hold a non-zero of the mask.
#pragma once
#include <stdint.h>

extern "C" {
// cmask uint8 [H][W] -> map uint8 [H][W] (bit 0 = E, bit 1 = M, bit 2 = cmask != 0), counts[3] = |E|, |M|, listed cells (zeroed here,
// on the stream), cells = the level-3 cells with a non-zero byte of the map
int vsr_tone_launch_sets(const uint8_t* cmask, int H, int W, int r0, int r1, uint8_t* map, uint64_t* counts, int32_t* cells, void* stream);
// the three per-call launches, in place on the frames; workspace: vsr_tone_workspace_bytes(H, W, n) bytes, 8-byte aligned
int vsr_tone_launch_apply(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride, const uint8_t* map,
                          const int32_t* cells, int ncells, int n, int H, int W, int y0, int rows, int c0, int c1, int S, void* workspace,
                          void* stream);
}
