// fc_registry.hpp -- the window sizes (NKB blocks of 16 positions) the fused kernels for 1- and 4-channel images are instantiated
// for, one translation unit each (fc_conv_<NKB>.hip): the same classes as fx_registry.hpp.  A kernel serves every pad <= 8 (NKB - 2).
#pragma once
#include "fc_kernels.hpp"
namespace blur_amd {
#define BLUR_FC_DECL(NKB_) const FcEntry* fc_entry_##NKB_();
BLUR_FC_DECL(3) BLUR_FC_DECL(5) BLUR_FC_DECL(7) BLUR_FC_DECL(9) BLUR_FC_DECL(11)
BLUR_FC_DECL(13) BLUR_FC_DECL(15) BLUR_FC_DECL(17) BLUR_FC_DECL(19) BLUR_FC_DECL(21) BLUR_FC_DECL(23)
#undef BLUR_FC_DECL
inline const FcEntry* find_fc_entry(int nkb)
{
    static const FcEntry* const list[] = { fc_entry_3(), fc_entry_5(), fc_entry_7(), fc_entry_9(), fc_entry_11(),
                                           fc_entry_13(), fc_entry_15(), fc_entry_17(), fc_entry_19(), fc_entry_21(), fc_entry_23() };
    for (const FcEntry* e : list)
        if (e->nkb == nkb) return e;
    return nullptr;
}
}  // namespace blur_amd
