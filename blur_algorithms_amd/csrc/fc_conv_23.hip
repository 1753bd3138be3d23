// fused matrix-core kernel for 1- and 4-channel images, 23 window blocks of 16 positions: pad <= 168; one channel per workgroup
#include "fc_kernels.hpp"
BLUR_FC(23)
