// fused matrix-core kernel for bfloat16 images of 1, 3 or 4 channels, 15 window blocks of 16 positions: pad <= 104; one channel per workgroup
#include "ff_kernels.hpp"
BLUR_FF_BF16(15)
