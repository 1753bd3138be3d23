// fused matrix-core kernel with one channel per workgroup, 21 window blocks of 16 positions (pad <= 152): 1 and 4 channels, and
// 3 channels for pad 137 .. 152
#include "fw_kernels.hpp"
BLUR_FW(21)
BLUR_FW_C3(21)
