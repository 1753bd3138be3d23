// The two-kernel matrix-core engine (mx_kernels.hpp), one window class per compilation: -DBLUR_INST_NKB=<NKB> -> build/mx_conv_<NKB>.o
#include "mx_kernels.hpp"
#include "fx_registry.hpp"
namespace blur_amd {
static_assert(fx_is_class(BLUR_INST_NKB), "mx_conv.hip: NKB is a class of BLUR_FX_CLASSES");
template <> const MxEntry* fx_entry<MxEntry, BLUR_INST_NKB>()
{
    static const MxEntry e = { BLUR_INST_NKB, mx_launch_row_u8<BLUR_INST_NKB>, mx_launch_col_u8<BLUR_INST_NKB> };
    return &e;
}
}  // namespace blur_amd
