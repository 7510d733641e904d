// Launcher of the borrow kernels (borrow_kernels.hip): per call the glyph key's seed bitmap of every frame, the bitmap of the pixels
// within G + R - 1 of a seed, and the in-place replacement of the fill by a neighbouring frame's source pixel.  All pointers are device
// pointers; returns 0 or -1 (launch error).  The arguments are checked by the C-ABI entry point (vsr_borrow_apply), not here.  The frames
// hold `rows` rows of the picture from its row y0; [c0, c1) are the rows of the picture that hold a non-zero of the mask.
#pragma once
#include <stdint.h>

extern "C" {
// the three per-call launches, in place on the frames; counts: vsr_regrain_sets', stats: vsr_regrain_measure's, pairs:
// vsr_deflicker_pairs' with R = B; workspace: vsr_borrow_workspace_bytes(H, W, n) bytes, 8-byte aligned, uninitialised
int vsr_borrow_launch(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride, const uint8_t* cmask,
                      const uint64_t* counts, const uint64_t* stats, const uint64_t* pairs, int n, int H, int W, int y0, int rows, int c0,
                      int c1, int T, int B, void* workspace, void* stream);
}
