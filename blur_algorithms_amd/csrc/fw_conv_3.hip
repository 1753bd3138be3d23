// fused matrix-core kernel with one channel per workgroup, 3 window blocks of 16 positions (pad <= 8): 1 and 4 channels, and
// 3 channels for the launches over a subset of them (one sigma per channel)
#include "fw_kernels.hpp"
BLUR_FW(3)
