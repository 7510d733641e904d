// Launchers of the stroke-text kernels (stroke_kernels.hip): the per-cell stroke counts of --text-detect strokes over the frames of a call,
// and the text map made from them.  All pointers are device pointers; both return 0 or the hipError_t of the launch
// (hipErrorInvalidValue for F outside 1..8).  The arguments are checked by the C-ABI entry points (vsr_strokes_cells, vsr_strokes_text),
// not here.
#pragma once
#include <stdint.h>

extern "C" {
// one launch over the n frames frames + k * frame_stride: cv / ch uint8 [n][hc][wc], hc = ceil((H / F) / 4), wc = ceil((W / F) / 4)
int vsr_strokes_cells_launch(const uint8_t* frames, int64_t frame_stride, int n, int H, int W, int F, int S, int C, uint8_t* cv, uint8_t* ch,
                             void* stream);
// one launch: text float [n][hc][wc] (1.0 where both window sums reach their thresholds, else 0.0)
int vsr_strokes_text_launch(const uint8_t* cv, const uint8_t* ch, int n, int hc, int wc, int WX, int WY, int NV, int NH, float* text, void* stream);
}
