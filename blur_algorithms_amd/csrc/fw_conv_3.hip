// fused matrix-core kernel with one channel per workgroup, 3 window blocks of 16 positions (pad <= 8): 1 and 4 channels
#include "fw_kernels.hpp"
BLUR_FW(3)
