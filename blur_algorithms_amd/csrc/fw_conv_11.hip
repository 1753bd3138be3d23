// fused matrix-core kernel with one channel per workgroup, 11 window blocks of 16 positions (pad <= 72): 1 and 4 channels
#include "fw_kernels.hpp"
BLUR_FW(11)
