// fused matrix-core kernel with one channel per workgroup, 7 window blocks of 16 positions (pad <= 40): 1 and 4 channels
#include "fw_kernels.hpp"
BLUR_FW(7)
