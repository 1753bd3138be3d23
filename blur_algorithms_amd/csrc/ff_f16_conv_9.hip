// fused matrix-core kernel for float16 images of 1, 3 or 4 channels, 9 window blocks of 16 positions: pad <= 56; one channel per workgroup
#include "ff_kernels.hpp"
BLUR_FF_F16(9)
