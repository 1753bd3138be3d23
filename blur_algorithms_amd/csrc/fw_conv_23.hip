// fused matrix-core kernel with one channel per workgroup, 23 window blocks of 16 positions (pad <= 168): 1 and 4 channels, and
// 3 channels for pad 153 .. 168
#include "fw_kernels.hpp"
BLUR_FW(23)
BLUR_FW_C3(23)
