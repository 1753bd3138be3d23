// The fused matrix-core kernel with one channel per workgroup (fw_kernels.hpp), one window class per compilation:
// -DBLUR_INST_NKB=<NKB> -> build/fw_conv_<NKB>.o.  Every class: one, two and four channels (FcEntry; two: the chroma plane of an NV12
// surface), and three channels for the launches over a subset of them (Fw3Entry: one sigma per channel), each with and without a
// frame list.  NKB >= 13 as well: whole BGR frames (FxEntry, pad 73 .. 168).
#include "fw_kernels.hpp"
#include "fx_registry.hpp"
namespace blur_amd {
static_assert(fx_is_class(BLUR_INST_NKB), "fw_conv.hip: NKB is a class of BLUR_FX_CLASSES");
template <> const FcEntry* fx_entry<FcEntry, BLUR_INST_NKB>()
{
    static const FcEntry e = { BLUR_INST_NKB, fw_launch_u8c14<BLUR_INST_NKB> };
    return &e;
}
template <> const Fw3Entry* fx_entry<Fw3Entry, BLUR_INST_NKB>()
{
    static const Fw3Entry e = { BLUR_INST_NKB, fw_launch_u8c3_sel<BLUR_INST_NKB> };
    return &e;
}
#if BLUR_INST_NKB >= 13
template <> const FxEntry* fx_entry<FxEntry, BLUR_INST_NKB>()
{
    static const FxEntry e = { BLUR_INST_NKB, fw_launch_u8c3<BLUR_INST_NKB> };
    return &e;
}
#endif
}  // namespace blur_amd
