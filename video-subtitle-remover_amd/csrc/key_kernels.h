// Launcher of the glyph-key kernels (key_kernels.hip): per call the seed bitmap of every frame and the in-place mix of the fill and the
// source by the distance to the nearest seed.  All pointers are device pointers; returns 0 or -1 (launch error).  The arguments are
// checked by the C-ABI entry point (vsr_key_apply), not here.  The frames hold `rows` rows of the picture from its row y0; [c0, c1) are
// the rows of the picture that hold a non-zero of the mask.
#pragma once
#include <stdint.h>

extern "C" {
// the two per-call launches, in place on the frames; workspace: vsr_key_workspace_bytes(H, W, n) bytes, 8-byte aligned, uninitialised
int vsr_key_launch(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride, const uint8_t* cmask, int n, int H, int W,
                   int y0, int rows, int c0, int c1, int T, void* workspace, void* stream);
// the three per-call launches of --glyph-hold K, 1 <= K <= 8 (checked by vsr_key_apply_hold): the strong and the weak seeds, the seeds
// held over the K frames to either side, the same mix; workspace: vsr_key_hold_workspace_bytes(H, W, n) bytes, 8-byte aligned, uninitialised
int vsr_key_hold_launch(uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride, const uint8_t* cmask, int n, int H,
                        int W, int y0, int rows, int c0, int c1, int T, int K, void* workspace, void* stream);
// the seed launch of vsr_key_launch alone (--borrow, borrow_kernels.hip): [sa, sb) are the bitmap's rows as rows of the frames (the
// rows [c0 - 1, c1 + 1) of the picture that the frames hold, not empty); bitmap: n * (sb - sa) * ceil(W / 64) words, every one written
int vsr_key_seeds_launch(const uint8_t* frames, int64_t frame_stride, const uint8_t* src, int64_t src_frame_stride, const uint8_t* cmask, int n,
                         int W, int y0, int rows, int sa, int sb, int T, void* bitmap, void* stream);
}
