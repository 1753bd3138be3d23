// fused matrix-core kernel with one channel per workgroup, 19 window blocks of 16 positions (pad <= 136): 1 and 4 channels, and
// 3 channels for pad 121 .. 136
#include "fw_kernels.hpp"
BLUR_FW(19)
BLUR_FW_C3(19)
