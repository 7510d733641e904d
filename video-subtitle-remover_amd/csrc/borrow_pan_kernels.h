// Launchers of the borrow-pan kernels (borrow_pan_kernels.hip): per call the table of shift sums over the ring, level by level, then
// the seed and near bitmaps of --borrow, the chosen shift and threshold of every pair, and the in-place replacement of the fill by a
// neighbouring frame's source pixel at the shifted position.  All pointers are device pointers; returns 0 or -1 (launch error).  The
// arguments are checked by the C-ABI entry points (vsr_borrow_pan_search / vsr_borrow_pan_apply), not here.  The frames hold `rows` rows
// of the picture from its row y0; [c0, c1) are the rows of the picture that hold a non-zero of the mask.
#pragma once
#include <stdint.h>

extern "C" {
// a memset and min(B, n - 1) launches; map, counts: vsr_regrain_sets'; workspace: vsr_borrow_pan_workspace_bytes(H, W, n, B, P) bytes,
// 8-byte aligned, uninitialised: the table at its front is cleared here
int vsr_borrow_pan_launch_search(const uint8_t* src, int64_t src_frame_stride, const uint8_t* map, const uint64_t* counts, int n, int W, int y0,
                                 int rows, int c0, int c1, int B, int P, void* workspace, void* stream);
// the four per-call launches, in place on the frames; stats: vsr_regrain_measure's; workspace: as vsr_borrow_pan_launch_search left it
int vsr_borrow_pan_launch_apply(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride, const uint8_t* cmask,
                                const uint64_t* counts, const uint64_t* stats, int n, int H, int W, int y0, int rows, int c0, int c1, int T,
                                int B, int P, void* workspace, void* stream);
}
