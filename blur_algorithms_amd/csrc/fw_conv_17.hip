// fused matrix-core kernel with one channel per workgroup, 17 window blocks of 16 positions (pad <= 120): 1 and 4 channels, and
// 3 channels for pad 105 .. 120
#include "fw_kernels.hpp"
BLUR_FW(17)
BLUR_FW_C3(17)
