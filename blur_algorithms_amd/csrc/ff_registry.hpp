// ff_registry.hpp -- the window sizes (NKB blocks of 16 positions) the fused kernels for float32 images are instantiated for, one
// translation unit each (ff_conv_<NKB>.hip): the same classes as fc_registry.hpp.  A kernel serves every pad <= 8 (NKB - 2).
#pragma once
#include "ff_kernels.hpp"
namespace blur_amd {
#define BLUR_FF_DECL(NKB_) const FfEntry* ff_entry_##NKB_();
BLUR_FF_DECL(3) BLUR_FF_DECL(5) BLUR_FF_DECL(7) BLUR_FF_DECL(9) BLUR_FF_DECL(11)
BLUR_FF_DECL(13) BLUR_FF_DECL(15) BLUR_FF_DECL(17) BLUR_FF_DECL(19) BLUR_FF_DECL(21) BLUR_FF_DECL(23)
#undef BLUR_FF_DECL
inline const FfEntry* find_ff_entry(int nkb)
{
    static const FfEntry* const list[] = { ff_entry_3(), ff_entry_5(), ff_entry_7(), ff_entry_9(), ff_entry_11(),
                                           ff_entry_13(), ff_entry_15(), ff_entry_17(), ff_entry_19(), ff_entry_21(), ff_entry_23() };
    for (const FfEntry* e : list)
        if (e->nkb == nkb) return e;
    return nullptr;
}
}  // namespace blur_amd
