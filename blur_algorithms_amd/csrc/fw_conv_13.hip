// fused matrix-core kernel with one channel per workgroup, 13 window blocks of 16 positions (pad <= 88): 1 and 4 channels, and
// 3 channels for pad 73 .. 88
#include "fw_kernels.hpp"
BLUR_FW(13)
BLUR_FW_C3(13)
