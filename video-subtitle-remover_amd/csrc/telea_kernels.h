// Launcher of the Telea level-replay kernel (telea_kernels.hip).  All pointers but the tap tables are device pointers;
// returns 0 or -1 (launch error).
#pragma once
#include <stdint.h>

extern "C" {
// frames: uint8 [n][H][W][3], frame f at frames + f * frame_stride bytes, filled in place.  One workgroup per frame.
// level_off [L+1], yx [P][2], w / flags [NT][P]: the arrays of vsr::TeleaPlan; tap_dk / tap_dl [NT] are host arrays.
int vsr_telea_launch_fill(uint8_t* frames, int64_t frame_stride, int n, int H, int W, int L, int64_t P, int NT, const int8_t* tap_dk,
                          const int8_t* tap_dl, const int32_t* level_off, const int32_t* yx, const float* w, const uint8_t* flags,
                          void* stream);
}
