// The fused matrix-core kernel for float32, u16, float16 and bfloat16 images of 1, 3 or 4 channels (ff_kernels.hpp; one channel per
// workgroup), one window class and pixel type per compilation: -DBLUR_INST_NKB=<NKB> -DBLUR_INST_T=float | uint16_t | ff_f16 | ff_bf16
// -> build/ff_conv_<NKB>.o, ff_u16_conv_<NKB>.o, ff_f16_conv_<NKB>.o, ff_bf16_conv_<NKB>.o.  Which channel counts a class has is
// ff_class_ok_t's rule (ff_launch); uint16_t has two channels as well, in every class (the chroma plane of a P016 surface).
#include "ff_kernels.hpp"
#include "fx_registry.hpp"
namespace blur_amd {
static_assert(fx_is_class(BLUR_INST_NKB), "ff_conv.hip: NKB is a class of BLUR_FX_CLASSES");
template <> const FfEntryT<BLUR_INST_T>* fx_entry<FfEntryT<BLUR_INST_T>, BLUR_INST_NKB>()
{
    static const FfEntryT<BLUR_INST_T> e = { BLUR_INST_NKB, ff_launch<BLUR_INST_T, BLUR_INST_NKB> };
    return &e;
}
}  // namespace blur_amd
