// The fused matrix-core kernel with three channels per workgroup (fx_kernels.hpp), one window class per compilation:
// -DBLUR_INST_NKB=<NKB> -> build/fx_conv_<NKB>.o, NKB <= 11 (the wider classes' three-channel entry is fw_conv.hip's)
#include "fx_kernels.hpp"
#include "fx_registry.hpp"
namespace blur_amd {
static_assert(fx_is_class(BLUR_INST_NKB) && BLUR_INST_NKB <= 11, "fx_conv.hip: NKB is a class of BLUR_FX_CLASSES up to 11");
template <> const FxEntry* fx_entry<FxEntry, BLUR_INST_NKB>()
{
    static const FxEntry e = { BLUR_INST_NKB, fx_launch_u8<BLUR_INST_NKB> };
    return &e;
}
}  // namespace blur_amd
