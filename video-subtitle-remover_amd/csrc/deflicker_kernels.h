// Launchers of the deflicker kernels (deflicker_kernels.hip): the per-pair sums of how much the source moved in the ring around the
// mask, and the gated temporal blend of the fill inside it.  All pointers are device pointers; all return 0 or -1 (launch error).  The
// arguments are checked by the C-ABI entry points (vsr_deflicker_pairs / vsr_deflicker_apply), not here.  The frames hold `rows` rows
// of the picture from its row y0; [c0, c1) are the rows of the picture that hold a non-zero of the mask; map is vsr_regrain_sets'.
#pragma once
#include <stdint.h>

extern "C" {
// pairs [n][R]: pairs[t][k-1] = sum over E and the channels of |src_t - src_{t+k}|, 0 where t + k >= n (zeroed here, on the stream)
int vsr_deflicker_launch_pairs(const uint8_t* src, int64_t src_frame_stride, const uint8_t* map, int n, int W, int y0, int rows, int c0,
                               int c1, int R, uint64_t* pairs, void* stream);
// in place on the frames, from counts (vsr_regrain_sets), stats (vsr_regrain_measure) and pairs as the launches before left them on the
// same stream; snap: the frames' local rows [max(c0 - y0, 0), min(c1 - y0, rows)) as they were, frame f at snap + f * snap_stride
int vsr_deflicker_launch_apply(uint8_t* frames, int64_t frame_stride, const uint8_t* snap, int64_t snap_stride, const uint8_t* map,
                               const uint64_t* counts, const uint64_t* stats, const uint64_t* pairs, int n, int W, int y0, int rows, int c0,
                               int c1, int R, void* stream);
}
