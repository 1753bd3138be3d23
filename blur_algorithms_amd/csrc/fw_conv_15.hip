// fused matrix-core kernel with one channel per workgroup, 15 window blocks of 16 positions (pad <= 104): 1 and 4 channels, and
// 3 channels for pad 89 .. 104
#include "fw_kernels.hpp"
BLUR_FW(15)
BLUR_FW_C3(15)
