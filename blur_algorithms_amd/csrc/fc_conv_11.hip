// fused matrix-core kernel for 1- and 4-channel images, 11 window blocks of 16 positions: pad <= 72; one channel per workgroup
#include "fc_kernels.hpp"
BLUR_FC(11)
