// fused matrix-core kernel with one channel per workgroup, 7 window blocks of 16 positions (pad <= 40): 1 and 4 channels, and
// 3 channels for the launches over a subset of them (one sigma per channel)
#include "fw_kernels.hpp"
BLUR_FW(7)
