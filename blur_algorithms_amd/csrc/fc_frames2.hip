// fc_prepass_frames<2, G> (fw_kernels.hpp): the pre-pass of a two-channel launch over frames with their own sigmas -- the chroma plane
// of an NV12 clip, blur_gaussian_nv12_frame_sigmas_batch_dev.  A unit of its own, not engine.hip's like the one- and four-channel
// instantiations: next to fc_prepass<2, G> there, these changed that kernel's register allocation (the same instructions, two
// registers swapped), and the scalar NV12 entry's kernels stay byte for byte what they were.
#include "fw_kernels.hpp"
namespace blur_amd {
hipError_t fc_prepass_frames2_launch(int G, unsigned nblocks, hipStream_t st, const uint8_t* src, int* srow, int* cpart, long long* zsum, uint8_t* strips, int rows, int cols,
                                     int pada, int nbands, int nbatches, int cpitch, int n_alt, int chunks, int nright, int strip_blocks, int band_rows, unsigned chmask,
                                     uint32_t spitch, size_t sframe, const FwFrame* ft)
{
    auto kern = G == 1 ? fc_prepass_frames<2, 1> : (G == 2 ? fc_prepass_frames<2, 2> : fc_prepass_frames<2, 4>);
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(256), 0, st, src, srow, cpart, zsum, strips, rows, cols, pada, nbands, nbatches, cpitch, n_alt, chunks, nright, strip_blocks,
                       band_rows, chmask, spitch, sframe, ft);
    return hipGetLastError();
}
}  // namespace blur_amd
