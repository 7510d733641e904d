// Launchers of the --opencv-fill exemplar kernels (exemplar_kernels.hip).  All pointers are device pointers; every launcher
// returns 0 or -1 (launch error).  The statement is tests/_exemplar_statement.py.
#pragma once
#include <stdint.h>

extern "C" {

// one level of one call: what every kernel but k_ex_down needs
struct vsr_ex_level {
    uint8_t* img;              // uint8 [n][H][W][3], frame f at img + f * img_stride bytes (level 0: the caller's frames)
    int64_t img_stride;
    int32_t H, W, level;
    const uint8_t* cls;        // [H][W] EX_* bits (exemplar_plan.h)
    const int16_t* src;        // [ns][2] valid sources
    uint32_t ns;
    uint32_t* fa;              // match fields uint32 [n][bh][bw]: y in the low half, x in the high half, 0xFFFFFFFF = no target
    uint32_t* fb;
    int32_t by0, bx0, bh, bw;  // the box the fields cover
};

// k_ex_down: dst level = 2 x 2 mean of src level (sizes (Hs+1)/2 x (Ws+1)/2), all n frames
int vsr_ex_launch_down(const uint8_t* src, int64_t src_stride, int Hs, int Ws, uint8_t* dst, int64_t dst_stride, int n, void* stream);
// k_ex_init: the coarsest level's hole pixels interpolated from the known pixels; table int32 [nh][6]
int vsr_ex_launch_init(const vsr_ex_level* lv, const int32_t* table, int64_t nh, int n, void* stream);
// k_ex_up: the level's initial field into fa AND fb, from the coarser level's fa (coarse == nullptr: the "any source" draw)
int vsr_ex_launch_up(const vsr_ex_level* lv, const vsr_ex_level* coarse, int n, void* stream);
// k_ex_search: one synchronous pass over the listed tiles; reads fb if from_b else fa, writes the other
int vsr_ex_launch_search(const vsr_ex_level* lv, const int32_t* tiles, int ntiles, int it, int ps, int from_b, int n, void* stream);
// k_ex_vote: every hole pixel from the field (fb if from_b else fa), in place
int vsr_ex_launch_vote(const vsr_ex_level* lv, int from_b, int n, void* stream);
}
